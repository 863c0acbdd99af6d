"""numpy f64 restatement of ops.gae_advnorm (csrc/mappo_ops.hip k_gae_scan .. k_gae_norm): GAE, the value targets and the advantage
normalisation as oracle/model_oracle.py `gae` writes them (reference DHGN/mappo_parallel.py:643-658).

r, active (N, T, P); v (N, T + 1, P).  Every operation in f64, nothing rounded on the way."""
import numpy as np


def gae(r, v, active, gamma, lamda, use_adv_norm=True):
    """-> (adv, v_target), f64"""
    r, v, active = (np.asarray(x, np.float64) for x in (r, v, active))
    T = r.shape[1]
    deltas = (r + gamma * v[:, 1:] - v[:, :-1]) * active            # model_oracle.py: deltas = (r + gamma * v[:, 1:] - v[:, :-1]) * active
    adv = np.zeros_like(r)
    g = np.zeros_like(r[:, 0])
    for t in range(T - 1, -1, -1):
        g = deltas[:, t] + gamma * lamda * g                        # g = deltas[:, t] + gamma * lamda * g
        adv[:, t] = g
    v_target = adv + v[:, :-1]                                      # v_target = adv + v[:, :-1]
    if use_adv_norm:
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-5) * active   # (adv - adv.mean()) / (adv.std() + 1e-5) * active; torch.std is unbiased
    return adv, v_target
