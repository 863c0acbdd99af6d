"""numpy restatement -- and the specification -- of the imitation warm start's launches (csrc/imitation.hpp: bc_loss_gauss_fwd_bwd,
bc_loss_cat_fwd_bwd, e3d_bc_select, n2n_bc_select; algo.bc_iterations), in f64.

Rows are the leading dimensions flattened; `active` is the 0 / 1 mask of live rows and every mean is sum_i active_i x_i / sum active.
Gradients are those of actor_loss + critic_loss with autograd's rules: clamp passes the gradient on its closed range, max sends half of
it to each side of an exact tie."""
import numpy as np

P_EPS = float(np.finfo(np.float32).eps)   # torch.distributions' clamp_probs bound for fp32 probabilities


def critic(values_now, values_old, v_target, eps, use_value_clip):
    """-> (lc, d lc / d values_now) per row: the squared error of ppo_elem, with the PPO value clip when use_value_clip"""
    v, vt = np.asarray(values_now, np.float64), np.asarray(v_target, np.float64)
    eo = v - vt
    if not use_value_clip:
        return eo * eo, 2.0 * eo
    vo = np.asarray(values_old, np.float64)
    d = v - vo
    ec = (np.clip(d, -eps, eps) + vo) - vt
    qa, qb = ec * ec, eo * eo
    wa = np.where(qa > qb, 1.0, np.where(qa == qb, 0.5, 0.0))
    wb = np.where(qb > qa, 1.0, np.where(qa == qb, 0.5, 0.0))
    din = (d >= -eps) & (d <= eps)
    return np.maximum(qa, qb), wa * 2.0 * ec * din + wb * 2.0 * eo


def wrap_residual(d):
    """d -> d - 2 floor((d + 1) / 2), in [-1, 1): the residual of a quantity whose values +-1 are the same heading"""
    d = np.asarray(d, np.float64)
    return d - 2.0 * np.floor((d + 1.0) / 2.0)


def bc_loss_gauss(mu, ls_raw, target, values_now, active, values_old, v_target, eps, use_value_clip, lo=-np.inf, hi=np.inf, fit_std=False,
                  wrap0=False):
    """mu, target (..., A); ls_raw (A,) (param mode) or (..., A) (state mode); the rest (...).  -> dict: actor_loss, critic_loss, g_mu
    (..., A), g_ls (ls_raw's shape), g_v (...), sq_sum = sum_i active_i sum_a d_a^2 and rows = sum active"""
    mu, target, ls_raw = (np.asarray(x, np.float64) for x in (mu, target, ls_raw))
    act = np.asarray(active, np.float64)
    rows = act.sum()
    up = act / rows
    ls = np.clip(ls_raw, lo, hi)
    iv = np.exp(-2.0 * ls)
    d = target - mu
    if wrap0:
        d = d.copy()
        d[..., 0] = wrap_residual(d[..., 0])
    la = (0.5 * d * d * iv + (ls if fit_std else 0.0) * np.ones_like(d)).sum(-1)
    lc, dlc = critic(values_now, values_old, v_target, eps, use_value_clip)
    g_ls = up[..., None] * (1.0 - d * d * iv) * ((ls_raw >= lo) & (ls_raw <= hi)) if fit_std else np.zeros_like(d)
    if ls_raw.ndim == 1:
        g_ls = g_ls.reshape(-1, ls_raw.shape[0]).sum(0)
    return dict(actor_loss=(la * act).sum() / rows, critic_loss=(lc * act).sum() / rows, g_mu=-up[..., None] * d * iv, g_ls=g_ls, g_v=up * dlc,
                sq_sum=((d * d).sum(-1) * act).sum(), rows=rows)


def bc_loss_cat(prob, label, values_now, active, values_old, v_target, eps, use_value_clip):
    """prob (..., A), label (...) integers; -> dict: actor_loss, critic_loss, g_prob (..., A), g_v (...), hits = the number of live rows
    whose argmax over the row as given (lowest index on ties) is the label, and rows = sum active"""
    prob = np.asarray(prob, np.float64)
    label = np.asarray(label).astype(np.int64)
    act = np.asarray(active, np.float64)
    rows = act.sum()
    up = act / rows
    s = prob.sum(-1, keepdims=True)
    p = prob / s
    onehot = np.arange(prob.shape[-1]) == label[..., None]
    psel = (p * onehot).sum(-1)
    c = np.clip(psel, P_EPS, 1.0 - P_EPS)
    la = -np.log(c)
    gsel = np.where((psel >= P_EPS) & (psel <= 1.0 - P_EPS), -up / c, 0.0)   # d / d probs[label]; the clamp's pass rule
    g_prob = (onehot * gsel[..., None] - (gsel * psel)[..., None]) / s     # through probs = prob / prob.sum(-1)
    lc, dlc = critic(values_now, values_old, v_target, eps, use_value_clip)
    hits = ((prob.argmax(-1) == label) * (act != 0)).sum()                 # numpy's argmax: the first maximum
    return dict(actor_loss=(la * act).sum() / rows, critic_loss=(lc * act).sum() / rows, g_prob=g_prob, g_v=up * dlc, hits=float(hits), rows=rows)


def tanh_label(g, bound):
    """the pre-squash label of a teacher action under tanh squashing: atanh(clamp(g, -bound, bound)), finite for g = +-1"""
    return np.arctanh(np.clip(np.asarray(g, np.float64), -bound, bound))


def e3d_select(guide, follow, env_action, squash="clip", bound=0.999):
    """guide, env_action (N, P, 3) f64, follow (N,) -> (labels (N, P, 3) fp32, the executed actions (N, P, 3) f64)"""
    guide = np.asarray(guide, np.float64)
    labels = (tanh_label(guide, bound) if squash == "tanh" else guide).astype(np.float32)
    return labels, np.where(np.asarray(follow).astype(bool)[:, None, None], guide, np.asarray(env_action, np.float64))


def n2n_select(guide, follow, a_n):
    """guide, a_n (N, P) int32, follow (N,) -> (labels (N, P) fp32, the executed actions (N, P) int32)"""
    guide = np.asarray(guide, np.int32)
    return guide.astype(np.float32), np.where(np.asarray(follow).astype(bool)[:, None], guide, np.asarray(a_n, np.int32)).astype(np.int32)
