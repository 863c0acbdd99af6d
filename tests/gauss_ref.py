"""Host reference of the diagonal-Gaussian policy (csrc/gauss_policy.hpp: k_gauss_head, k_ppo_loss_gauss), numpy only.

Noise: row r of a launch calls Philox4x32-10 at counter (ctr = *counter + r: c0 = low, c1 = high word), c2 = j for the dims 4 j .. 4 j + 3,
c3 = 0, key = seed; every output word becomes u = ((o >> 8) + 1/2) 2^-24, evaluated here in fp32 bit for bit as the kernel does (the top
of the grid rounds to 1, ties to even), and Box-Muller turns (u0, u1) into (sqrt(-2 ln u0) cos 2 pi u1, sqrt(-2 ln u0) sin 2 pi u1) and
(u2, u3) likewise.  Everything after the u grid is f64.
The loss follows ppo_elem (csrc/mappo_ops.hip) and DHGN/mappo_parallel.py:692-706 with autograd's tie rules for min / max / clamp.
"""
import numpy as np

from tests.sampling_ref import philox4x32_10_words

HALF_LN_2PI = 0.5 * np.log(2.0 * np.pi)
_LO = np.uint64(0xFFFFFFFF)


def uniforms(ctr, seed, j):
    """(R, 4) fp32 u of noise block j for the 64-bit counters ctr (R,)"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    seed = int(seed)
    words = philox4x32_10_words(ctr & _LO, ctr >> np.uint64(32), j, 0, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack([((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24) for w in words], -1)


def normals(ctr, seed, A):
    """(R, A) f64 standard normal draws of the rows at counters ctr"""
    blocks = []
    for j in range((A + 3) // 4):
        u = uniforms(ctr, seed, j).astype(np.float64)
        ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
        blocks.append(np.stack([ra * np.cos(2 * np.pi * u[:, 1]), ra * np.sin(2 * np.pi * u[:, 1]),
                                rb * np.cos(2 * np.pi * u[:, 3]), rb * np.sin(2 * np.pi * u[:, 3])], -1))
    return np.concatenate(blocks, -1)[:, :A]


def head_sample(feat, W, b, log_std, seed, counter, greedy=False):
    """-> (mu, z, action, env_action, logp) in f64 for the rows of feat (R, H) drawn at counters counter + r"""
    feat, W, b, ls = (np.asarray(x, np.float64) for x in (feat, W, b, log_std))
    R, A = feat.shape[0], W.shape[0]
    mu = feat @ W.T + b
    z = np.zeros((R, A)) if greedy else normals(np.uint64(counter) + np.arange(R, dtype=np.uint64), seed, A)
    a = mu + np.exp(ls) * z
    logp = (-0.5 * z * z - ls - HALF_LN_2PI).sum(-1)
    return mu, z, a, np.clip(a, -1.0, 1.0), logp


def ppo_loss_gauss(mu, log_std, action, values_now, logp_old, adv, active, values_old, v_target, eps, ent_coef, use_value_clip=True):
    """-> (actor_loss, critic_loss, grad_mu, grad_log_std, grad_values): the masked-mean PPO losses of Normal(mu, exp(log_std)) and their
    gradients (grad_mu / grad_log_std of the actor loss, grad_values of the critic loss).  mu, action (.., A); the rest (..)."""
    mu, ls, a = (np.asarray(x, np.float64) for x in (mu, log_std, action))
    vn, lo, ad, act, vt = (np.asarray(x, np.float64) for x in (values_now, logp_old, adv, active, v_target))
    var = np.exp(2 * ls)
    d = a - mu
    lp = (-d * d / (2 * var) - ls - HALF_LN_2PI).sum(-1)
    ent = (0.5 + HALF_LN_2PI + ls).sum()
    ratio = np.exp(lp - lo)
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
        vo = np.asarray(values_old, np.float64)
        dv = vn - vo
        ec = np.clip(dv, -eps, eps) + vo - vt
        qa, qb = ec * ec, eo * eo
        lc = np.maximum(qa, qb)
        wa, wb = (qa > qb) + 0.5 * (qa == qb), (qb > qa) + 0.5 * (qa == qb)
        gv = wa * 2 * ec * ((dv >= -eps) & (dv <= eps)) + wb * 2 * eo
    else:
        lc = eo * eo
        gv = 2 * eo
    g_mu = g_lp[..., None] * d / var
    g_ls = (g_lp[..., None] * (d * d / var - 1) + g_ent[..., None]).reshape(-1, mu.shape[-1]).sum(0)
    return (la * act).sum() / asum, (lc * act).sum() / asum, g_mu, g_ls, up * gv


def torch_ppo_loss_gauss(mu, log_std, action, values_now, logp_old, adv, active, values_old, v_target, eps, ent_coef, use_value_clip=True):
    """the same losses written as the reference writes PPO (DHGN/mappo_parallel.py:692-706) on torch.distributions.Normal: the
    yardstick of the numpy reference above and of the f64 re-evaluations in the GPU tests"""
    import torch
    dist = torch.distributions.Normal(mu, torch.exp(log_std))
    lp, ent = dist.log_prob(action).sum(-1), dist.entropy().sum(-1)
    ratios = torch.exp(lp - logp_old)
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
