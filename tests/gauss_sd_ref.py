"""Host reference of the state-dependent log-std / tanh-squashed Gaussian policy (csrc/gauss_policy.hpp: k_gauss_head_ex,
k_ppo_loss_gauss_ex), numpy f64 after the u grid of tests/gauss_ref.py.

ls_raw = feat W_ls^T + b_ls (state mode) or the log_std vector (param mode); ls = clamp(ls_raw, lo, hi); u = mu + exp(ls) z with the
noise of gauss_ref.normals.  The environment gets clamp(u, -1, 1) (clip) or tanh(u) (tanh); the log-probability is the Normal one minus
sum_a c(u_a) in tanh mode, c(u) = log(1 - tanh(u)^2) = 2 (ln 2 - u - softplus(-2 u)).  The entropy is the base Gaussian's.
"""
import numpy as np

from tests.gauss_ref import HALF_LN_2PI, normals


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def tanh_log_jac(u):
    """c(u) = log(1 - tanh(u)^2), written so that it stays finite for large |u|"""
    u = np.asarray(u, np.float64)
    return 2.0 * (np.log(2.0) - u - softplus(-2.0 * u))


def head_sample(feat, W, b, log_std, seed, counter, greedy=False, lo=-np.inf, hi=np.inf, squash="clip"):
    """-> (mu, ls_raw, z, u, env_action, logp) in f64; log_std is the (A,) vector or a pair (W_ls, b_ls)"""
    feat, W, b = (np.asarray(x, np.float64) for x in (feat, W, b))
    R, A = feat.shape[0], W.shape[0]
    mu = feat @ W.T + b
    if isinstance(log_std, (tuple, list)):
        W_ls, b_ls = (np.asarray(x, np.float64) for x in log_std)
        ls_raw = feat @ W_ls.T + b_ls
    else:
        ls_raw = np.broadcast_to(np.asarray(log_std, np.float64), (R, A))
    ls = np.clip(ls_raw, lo, hi)
    z = np.zeros((R, A)) if greedy else normals(np.uint64(counter) + np.arange(R, dtype=np.uint64), seed, A)
    u = mu + np.exp(ls) * z
    logp = (-0.5 * z * z - ls - HALF_LN_2PI).sum(-1)
    if squash == "tanh":
        logp = logp - tanh_log_jac(u).sum(-1)
        env = np.tanh(u)
    else:
        env = np.clip(u, -1.0, 1.0)
    return mu, ls_raw, z, u, env, logp


def _ppo(lp, ent, vn, lo_old, ad, act, vo, vt, eps, ent_coef, use_value_clip, ratio=None):
    """ppo_elem over all rows -> (actor_loss, critic_loss, g_lp, g_ent, g_v): tie rules of autograd for min / max / clamp.
    ratio: None, or the rows' ratios as data in place of exp(lp - lo_old) (tests/ppo_edges_cases.py: the bits the device's expf gave,
    so that a row built on a clip edge is on it in f64 too; g_lp is then the gradient that reaches lp through that ratio)"""
    ratio = np.exp(lp - lo_old) if ratio is None else np.asarray(ratio, np.float64)
    s1, s2 = ratio * ad, np.clip(ratio, 1 - eps, 1 + eps) * ad
    la = -np.minimum(s1, s2) - ent_coef * ent
    asum = act.sum()
    up = act / asum
    tie = s1 == s2
    w1, w2 = (s1 < s2) + 0.5 * tie, (s2 < s1) + 0.5 * tie
    inside = (ratio >= 1 - eps) & (ratio <= 1 + eps)
    g_lp = -up * (w1 + inside * w2) * ad * ratio
    g_ent = -up * ent_coef
    eo = vn - vt
    if use_value_clip:
        dv = vn - vo
        ec = np.clip(dv, -eps, eps) + vo - vt
        qa, qb = ec * ec, eo * eo
        lc = np.maximum(qa, qb)
        wa, wb = (qa > qb) + 0.5 * (qa == qb), (qb > qa) + 0.5 * (qa == qb)
        gv = wa * 2 * ec * ((dv >= -eps) & (dv <= eps)) + wb * 2 * eo
    else:
        lc = eo * eo
        gv = 2 * eo
    return (la * act).sum() / asum, (lc * act).sum() / asum, g_lp, g_ent, up * gv


def ppo_loss(mu, ls_raw, u, values_now, logp_old, adv, active, values_old, v_target, eps, ent_coef, use_value_clip=True,
             lo=-np.inf, hi=np.inf, squash="clip"):
    """-> (actor_loss, critic_loss, grad_mu, grad_ls_raw, grad_values).  mu, u (.., A); ls_raw (A,) (param mode: its gradient summed
    over the rows) or (.., A) (state mode: per row); the rest (..).  The clamp's gradient passes on the closed range [lo, hi]."""
    mu, u = np.asarray(mu, np.float64), np.asarray(u, np.float64)
    lr = np.asarray(ls_raw, np.float64)
    vn, lo_old, ad, act, vt = (np.asarray(x, np.float64) for x in (values_now, logp_old, adv, active, v_target))
    vo = None if values_old is None else np.asarray(values_old, np.float64)
    ls = np.clip(np.broadcast_to(lr, mu.shape), lo, hi)
    var = np.exp(2 * ls)
    d = u - mu
    lp = (-d * d / (2 * var) - ls - HALF_LN_2PI).sum(-1)
    if squash == "tanh":
        lp = lp - tanh_log_jac(u).sum(-1)
    ent = (0.5 + HALF_LN_2PI + ls).sum(-1)
    la, lc, g_lp, g_ent, g_v = _ppo(lp, ent, vn, lo_old, ad, act, vo, vt, eps, ent_coef, use_value_clip)
    g_mu = g_lp[..., None] * d / var
    pas = (np.broadcast_to(lr, mu.shape) >= lo) & (np.broadcast_to(lr, mu.shape) <= hi)
    g_ls = (g_lp[..., None] * (d * d / var - 1) + g_ent[..., None]) * pas
    if lr.ndim == 1:
        g_ls = g_ls.reshape(-1, mu.shape[-1]).sum(0)
    return la, lc, g_mu, g_ls, g_v


def torch_ppo_loss(mu, ls_raw, u, values_now, logp_old, adv, active, values_old, v_target, eps, ent_coef, use_value_clip=True,
                   lo=-float("inf"), hi=float("inf"), squash="clip"):
    """the same losses on torch.distributions.Normal with an explicit clamp of ls_raw and, in tanh mode, minus log(1 - tanh(u)^2)
    (a constant of the parameters): the yardstick of the numpy reference above and of the GPU loss"""
    import torch
    ls = torch.clamp(ls_raw, lo, hi)
    dist = torch.distributions.Normal(mu, torch.exp(ls))
    lp, ent = dist.log_prob(u).sum(-1), dist.entropy().sum(-1)
    if squash == "tanh":
        lp = lp - torch.log1p(-torch.tanh(u.detach()) ** 2).sum(-1)
    return torch_ppo_rows(torch.exp(lp - logp_old), ent, values_now, adv, active, values_old, v_target, eps, ent_coef, use_value_clip)


def torch_ppo_rows(ratios, ent, values_now, adv, active, values_old, v_target, eps, ent_coef, use_value_clip=True):
    """the op-by-op graph behind the policy: torch.min / torch.max / torch.clamp on the rows' ratios and entropies.  Its autograd
    gradients are the specification of ppo_elem's tie and closed-range rules (tests/test_ppo_edges_cases_cpu.py)"""
    import torch
    surr1 = ratios * adv
    surr2 = torch.clamp(ratios, 1 - eps, 1 + eps) * adv
    actor_loss = -torch.min(surr1, surr2) - ent_coef * ent
    actor_loss = (actor_loss * active).sum() / active.sum()
    if use_value_clip:
        values_error_clip = torch.clamp(values_now - values_old, -eps, eps) + values_old - v_target
        values_error_original = values_now - v_target
        critic_loss = torch.max(values_error_clip ** 2, values_error_original ** 2)
    else:
        critic_loss = (values_now - v_target) ** 2
    critic_loss = (critic_loss * active).sum() / active.sum()
    return actor_loss, critic_loss
