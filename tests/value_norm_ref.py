"""numpy restatement of algo.use_value_norm (csrc/value_norm.hpp, ops.gae_advnorm_vn / value_norm_update / value_norm_targets):
the PopArt-style normaliser of the value targets of the env_3d / env_n2n trainers.  The reference project has no such class; this
file is the specification, every operation in f64.

State: np.float64 (3,) = (m, q, d), the running mean, the running mean of squares and the debiasing term, all 0 at the start."""
import numpy as np

VAR_MIN = 1e-2


def new_state():
    return np.zeros(3, np.float64)


def stats(state):
    """-> (mean, std): (0, 1) before the first update, else m / d and sqrt(max(q / d - mean^2, 1e-2))"""
    m, q, d = (np.float64(x) for x in state)
    if d == 0.0:
        return np.float64(0.0), np.float64(1.0)
    mean = m / d
    return mean, np.sqrt(np.maximum(q / d - mean * mean, VAR_MIN))


def sums(v_target, active):
    """(S1, S2, c) over the live rows (active != 0) of the value targets, f64"""
    y = np.asarray(v_target, np.float64)[np.asarray(active) != 0]
    return np.array([y.sum(), (y * y).sum(), float(y.size)], np.float64)


def update(state, s, beta):
    """the moving-average step from s = (S1, S2, c), possibly summed over ranks, in place; c == 0 changes nothing"""
    S1, S2, c = (np.float64(x) for x in s)
    if not c > 0.0:
        return state
    beta = np.float64(beta)
    w = np.float64(1.0) - beta
    state[0] = beta * state[0] + w * (S1 / c)
    state[1] = beta * state[1] + w * (S2 / c)
    state[2] = beta * state[2] + w
    return state


def denormalise(state, v, mask):
    """v std + mean where mask != 0, exactly 0 elsewhere (f64)"""
    mean, sd = stats(state)
    return np.where(np.asarray(mask) != 0, np.asarray(v, np.float64) * sd + mean, 0.0)


def value_masks(active, vmask):
    """the mask of v (N, T + 1, P): active[:, t] for t < T, the rollout's bootstrap mask vmask (N, P) for t = T"""
    return np.concatenate([np.asarray(active), np.asarray(vmask)[:, None]], 1)


def gae(state, r, v, active, vmask, gamma, lamda, use_adv_norm=True):
    """GAE on the denormalised values -> (adv, v_target) f64: delta = (r + gamma v' - v) active, gae_t = delta_t + gamma lamda
    gae_{t+1}, v_target = gae + v; with use_adv_norm adv = (gae - mean) / (std_unbiased + 1e-5) active over all elements"""
    r, active = np.asarray(r, np.float64), np.asarray(active, np.float64)
    vd = denormalise(state, v, value_masks(active, vmask))
    N, T, P = r.shape
    adv = np.zeros((N, T, P))
    g = np.zeros((N, P))
    for t in range(T - 1, -1, -1):
        delta = (r[:, t] + gamma * vd[:, t + 1] - vd[:, t]) * active[:, t]
        g = delta + gamma * lamda * g
        adv[:, t] = g
    v_target = adv + vd[:, :-1]
    if use_adv_norm:
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-5) * active
    return adv, v_target


def targets(state, v_target, active):
    """(v_target - mean) / std on live rows, 0 elsewhere (f64)"""
    mean, sd = stats(state)
    return np.where(np.asarray(active) != 0, (np.asarray(v_target, np.float64) - mean) / sd, 0.0)
