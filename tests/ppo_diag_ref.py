"""f64 numpy restatement of the update diagnostics (csrc/ppo_diag.hpp): the eight per-row terms, their sums over
the live rows, the derived values, the early-stop rule, and the log-probability / entropy of the three policies in f64 for the
kernels that form them in fp32."""
import math

import numpy as np

NSUM = 8
HALF_LN_2PI = 0.5 * math.log(2.0 * math.pi)
F32_EPS = float(np.finfo(np.float32).eps)


def row_terms(lr, ratio, ent, v_now, v_tgt, active, eps):
    """(n, 8) f64: the terms of every row, 0 for an inactive one.  lr, ratio: the fp32 lp_now - lp_old and expf(lr) (or f64 stand-ins);
    eps: the clip range; 1 - eps and 1 + eps are formed in fp32 as the loss does when ratio is fp32.  expm1 is libm's, element by
    element (numpy's vectorised expm1 may be another implementation)."""
    lr, ent, v_now, v_tgt = (np.asarray(x).reshape(-1) for x in (lr, ent, v_now, v_tgt))
    ratio, live = np.asarray(ratio).reshape(-1), np.asarray(active).reshape(-1) != 0
    x, y = lr.astype(np.float64), v_tgt.astype(np.float64)
    if ratio.dtype == np.float32:
        lo, hi = np.float32(1) - np.float32(eps), np.float32(1) + np.float32(eps)
    else:
        lo, hi = 1.0 - float(eps), 1.0 + float(eps)
    t = np.zeros((len(x), NSUM))        # only live rows are evaluated: what an inactive row holds is never looked at
    x, y, vn = x[live], y[live], v_now.astype(np.float64)[live]
    t[live, 0] = 1.0
    t[live, 1] = np.array([math.expm1(v) for v in x]) - x
    t[live, 2] = (ratio[live] < lo) | (ratio[live] > hi)
    t[live, 3] = ent.astype(np.float64)[live]
    t[live, 4] = y
    t[live, 5] = y * y
    t[live, 6] = (y - vn) * (y - vn)
    t[live, 7] = ratio.astype(np.float64)[live]
    return t


def sums(terms):
    return terms.sum(0)


def derive(s):
    c = float(s[0])
    if c == 0:
        return dict(approx_kl=math.nan, clip_fraction=math.nan, entropy=math.nan, explained_variance=math.nan, ratio_mean=math.nan)
    mean = s[4] / c
    var = s[5] / c - mean * mean
    return dict(approx_kl=s[1] / c, clip_fraction=s[2] / c, entropy=s[3] / c, explained_variance=1.0 - (s[6] / c) / var if var > 0 else math.nan,
                ratio_mean=s[7] / c)


def stop_epoch(kls, target):
    """index of the first epoch whose KL exceeds the target (its gradient is discarded: also the number of optimizer steps), else None"""
    for e, kl in enumerate(kls):
        if target is not None and kl > target:
            return e
    return None


# ---- the log-probability and entropy the kernels form in fp32, in f64 -----------------------------------------------------------------
def categorical(prob, action):
    """torch.distributions.Categorical(prob): renormalisation, probs_to_logits' clamp to [eps32, 1 - eps32], gather, entropy"""
    p = prob.astype(np.float64)
    p = p / p.sum(-1, keepdims=True)
    l = np.log(np.clip(p, F32_EPS, 1.0 - F32_EPS))
    lp = np.take_along_axis(l, action.astype(np.int64)[..., None], -1)[..., 0]
    return lp, -(l * p).sum(-1)


def gaussian(mu, ls_raw, action, lo=-math.inf, hi=math.inf, tanh=False):
    """Normal(mu, exp(ls)).log_prob(u).sum(-1) [- sum log(1 - tanh(u)^2)] and the entropy, ls = clamp(ls_raw, lo, hi)"""
    mu, u = mu.astype(np.float64), action.astype(np.float64)
    ls = np.clip(np.broadcast_to(ls_raw.astype(np.float64), mu.shape), lo, hi)
    lp = (-((u - mu) ** 2) / (2.0 * np.exp(2.0 * ls)) - ls - HALF_LN_2PI).sum(-1)
    if tanh:
        x = -2.0 * u
        lp = lp - (2.0 * (math.log(2.0) - u - (np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))))).sum(-1)
    return lp, (0.5 + HALF_LN_2PI + ls).sum(-1)
