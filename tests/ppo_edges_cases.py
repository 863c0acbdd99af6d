"""Shared inputs of tests/test_ppo_edges_cases_cpu.py and tests/test_ppo_loss_edges_gpu.py (numpy only, no GPU): the rows that sit
exactly on the decisions of the four PPO loss kernels (csrc/mappo_ops.hip ppo_elem, k_ppo_loss_prob; csrc/gauss_policy.hpp
k_ppo_loss_gauss_ex), the random bulk cases with their preconditions, the row counts and the references of both.

A case is a dict of fp32 numpy arrays in the logical (batch-major) shape: kind ("plain", "prob", "gauss", "gauss_ex"), shape
(d0, d1, d2), adv / active / v_now / v_old / v_tgt / lp_old of that shape, eps, ent_coef, and the policy's operands: lp_now and ent
(plain); prob (.., A) and action (prob); mu, action (.., A) and ls ((A,), or (.., A) with state) plus lo, hi, squash (gauss, gauss_ex).
reference() evaluates the existing f64 restatements on it: gauss_sd_ref._ppo / ppo_loss, gauss_ref.ppo_loss_gauss,
kickstart_ref.ppo_loss_cat.  A case is built once and shared: nobody writes into it.

How the edge rows are exact in fp32 and in f64:
  policy clip    the loss takes lp_now and lp_old, and ratio = expf(lp_now - lp_old) is the device's.  A launch fixes one d, reads
                 r = expf(d) from the device (ops.ppo_ratio) and sets eps = r - 1 (d > 0) or 1 - r (d < 0) in fp32: the subtraction is
                 exact, 1.f + eps == r (1.f - eps == r) exactly, and the reference takes r and eps as data, so the row is on the edge in
                 both precisions whatever expf returns.  One fp32 step of d moves exp(d) by about a seventh of a step of the ratio, so
                 the neighbours are 1, 2, 4 .. 64 steps of d away on both sides and the ratio's own bits say which side each is on.
  value clip     v_old = 0 and eps = 0.25: every difference is exact, and the targets keep v_now - v_tgt representable.
  categorical    rows whose fp32 sum is exactly 1 (the renormalisation is the identity) with entries on finfo(float32).eps and
                 1 - eps32, and half of that beyond them.
  log-std        ls_raw on lo = -0.5 and hi = 0.5 and one fp32 step on either side of each.
"""
import functools
import math
import zlib

import numpy as np

from tests import gauss_ref
from tests import gauss_sd_ref as gs
from tests import kickstart_ref as kr
from tests import ppo_diag_ref as pd

F32 = np.float32
ENT = 0.01              # entropy coefficient of every case but the categorical edge batch
BULK_EPS = 0.2
INF = math.inf

# rows = d0 d1 d2: one row, one short of a workgroup, a long d2, d1 == 1, three odd dimensions, exactly the 256 x 256 cap of the
# launch, and one row into the second pass of its grid-stride loop
SHAPES = [(1, 1, 1), (1, 255, 1), (1, 1, 257), (257, 1, 1), (3, 17, 5), (1, 65536, 1), (1, 65537, 1)]
VIEW_SHAPES = [(3, 17, 5), (257, 1, 1)]
A_SHAPES = [(3, 17, 5), (1, 257, 1)]
VIEWS = ("time_major", "batch_major", "column_block", "value_slice", "mixed")

# the launches of the bulk tests: name -> (kind, A, state, squash)
VARIANTS = {
    "plain": ("plain", 0, False, "clip"),
    "prob": ("prob", 9, False, "clip"),
    "gauss": ("gauss", 3, False, "clip"),
    "ex_param_clip": ("gauss_ex", 16, False, "clip"),
    "ex_param_tanh": ("gauss_ex", 5, False, "tanh"),
    "ex_state_clip": ("gauss_ex", 8, True, "clip"),
    "ex_state_tanh": ("gauss_ex", 3, True, "tanh"),
}
# every compiled action count: name -> (kind, state, squash), A = 1 .. 16 each
A_VARIANTS = {
    "prob": ("prob", False, "clip"),
    "gauss": ("gauss", False, "clip"),
    "ex_param_clip": ("gauss_ex", False, "clip"),
    "ex_param_tanh": ("gauss_ex", False, "tanh"),
    "ex_state_clip": ("gauss_ex", True, "clip"),
    "ex_state_tanh": ("gauss_ex", True, "tanh"),
}
SHARP = 40.0            # logits of the sharp categorical case: probabilities below eps32 and at 1


def steps_out(x, k):
    """the fp32 value(s) k steps from x away from zero (k < 0: towards zero)"""
    return (np.asarray(x, F32).view(np.int32) + np.asarray(k, np.int32)).view(F32)


def _f64(c, *keys):
    return [None if c.get(k) is None else np.asarray(c[k], np.float64) for k in keys]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def log_prob64(c):
    """the f64 (log-probability, entropy) of the case's policy on its fp32 inputs"""
    if c["kind"] == "plain":
        return c["lp_now"].astype(np.float64), c["ent"].astype(np.float64)
    if c["kind"] == "prob":
        return pd.categorical(c["prob"], c["action"])
    return pd.gaussian(c["mu"], c["ls"], c["action"], c["lo"], c["hi"], c["squash"] == "tanh")


def reference(c, value_clip):
    """-> dict: la, lc and grads, the list of f64 gradients in the order of the call's differentiable operands ((lp_now, ent, v) /
    (prob, v) / (mu, ls, v)), from the existing restatements.  A case with "ratio" hands its rows' ratios to _ppo as data."""
    v_now, lp_old, adv, active, v_old, v_tgt = _f64(c, "v_now", "lp_old", "adv", "active", "v_old", "v_tgt")
    eps, ent_coef = float(c["eps"]), float(c["ent_coef"])
    vo = v_old if value_clip else None
    if c["kind"] == "plain":
        lp, ent = log_prob64(c)
        la, lc, g_lp, g_ent, g_v = gs._ppo(lp, ent, v_now, lp_old, adv, active, vo, v_tgt, eps, ent_coef, value_clip, ratio=c.get("ratio"))
        return dict(la=la, lc=lc, grads=[g_lp, g_ent, g_v])
    if c["kind"] == "prob":
        la, lc, g_prob, g_v = kr.ppo_loss_cat(c["prob"], c["action"], v_now, lp_old, adv, active, vo, v_tgt, eps, ent_coef, value_clip)
        return dict(la=la, lc=lc, grads=[g_prob, g_v])
    if c["kind"] == "gauss":
        la, lc, g_mu, g_ls, g_v = gauss_ref.ppo_loss_gauss(c["mu"], c["ls"], c["action"], v_now, lp_old, adv, active, vo, v_tgt, eps, ent_coef,
                                                           value_clip)
    else:
        la, lc, g_mu, g_ls, g_v = gs.ppo_loss(c["mu"], c["ls"], c["action"], v_now, lp_old, adv, active, vo, v_tgt, eps, ent_coef, value_clip,
                                              c["lo"], c["hi"], c["squash"])
    return dict(la=la, lc=lc, grads=[g_mu, g_ls, g_v])


# ---- edge batch 1: the policy clip ------------------------------------------------------------------------------------------------------
POLICY_EDGES = (0.171875, -0.21875)     # d of the edge row: the upper edge (ratio about 1.19) and the lower one (about 0.80)
POLICY_STEPS = (1, 2, 4, 8, 16, 32, 64)
POLICY_ADVS = (1.5, -0.75, 0.0)


def policy_clip_lrs(d):
    """the fp32 log-ratios of the launch of edge d: row 0 the edge, then 1 .. 64 fp32 steps inside and outside it, ratio 1, far out"""
    ks = [0] + [s * k for k in POLICY_STEPS for s in (-1, 1)]
    return np.concatenate([steps_out(F32(d), ks), np.array([0.0, 2 * d], F32)])


def policy_clip_batch(d, ratios):
    """the plain case of edge d; ratios: expf of policy_clip_lrs(d) as the device gives it (fp32; row 0 defines eps).  Every log-ratio
    meets both signs of the advantage and adv == 0, live and inactive (the inactive rows hold finite garbage).  v_now == v_old, so the
    critic row is an exact tie inside the value clip.  side: -1 inside the clip range, 0 on the edge, +1 outside, by the ratio's bits;
    factor: the share of -up adv ratio that is the gradient with respect to lp_now (nan where adv == 0: the gradient is 0)."""
    lrs, ratios = policy_clip_lrs(d), np.asarray(ratios, F32)
    assert ratios.shape == lrs.shape and ratios.dtype == F32
    r0 = ratios[0]
    eps = r0 - F32(1) if d > 0 else F32(1) - r0
    assert eps.dtype == F32 and 0.1 < eps < 0.3
    assert (F32(1) + eps if d > 0 else F32(1) - eps) == r0                    # exact in fp32: the kernel's edge is r0
    assert (1.0 + float(eps) if d > 0 else 1.0 - float(eps)) == float(r0)     # and in f64: the reference's edge is r0
    n_l, n_a = len(lrs), len(POLICY_ADVS)
    lr, ratio = np.repeat(lrs, n_a * 2), np.repeat(ratios, n_a * 2)
    adv = np.tile(np.repeat(np.array(POLICY_ADVS, F32), 2), n_l)
    active = np.tile(np.array([1.0, 0.0], F32), n_l * n_a)
    dead = active == 0
    adv = np.where(dead, adv * F32(32) + F32(3), adv).astype(F32)
    n = len(lr)
    side = (np.sign(ratio.astype(np.float64) - float(r0)) * np.sign(d)).astype(np.int64)
    picks_clipped = (adv > 0) == (d > 0)            # above 1 + eps the minimum takes the clipped term for adv > 0, below 1 - eps for adv < 0
    factor = np.where(side <= 0, 1.0, np.where(picks_clipped, 0.0, 1.0))
    factor = np.where(adv == 0, np.nan, factor)
    shape = (1, n, 1)
    r = lambda x: np.ascontiguousarray(x, F32).reshape(shape)
    return dict(kind="plain", shape=shape, A=0, lp_now=r(lr), lp_old=r(np.zeros(n)), ratio=r(ratio), ent=r(np.full(n, 1.25)), adv=r(adv),
                active=r(active), v_now=r(np.where(dead, 3.0, 0.5)), v_old=r(np.where(dead, -1.0, 0.5)), v_tgt=r(np.where(dead, -7.0, 0.25)),
                eps=float(eps), ent_coef=ENT, side=side, factor=factor, d=d)


# ---- edge batch 2: the value clip ---------------------------------------------------------------------------------------------------------
V_EPS = 0.25


def value_clip_rows():
    """(v_now, v_tgt, tag) with v_old = 0: on both edges, one fp32 step inside and outside each, the outside tie qa == qb and its
    mirror, far outside with either branch of the maximum, and v_now == v_old"""
    e, rows = F32(V_EPS), []
    for s in (1.0, -1.0):
        for tag, vn in (("on", F32(s) * e), ("inside", steps_out(F32(s) * e, -1)), ("outside", steps_out(F32(s) * e, 1))):
            rows += [(vn, 0.625 * s, tag), (vn, 0.0, tag)]
        rows += [(s * 1.0, s * 0.625, "tie"), (s * 2.0, s * 0.625, "far_unclipped"), (s * 2.0, s * 3.0, "far_clipped")]
    return rows + [(0.0, 0.375, "centre")]


def value_clip_case(kind, A=0, state=False, squash="clip", seed=5):
    """the value-clip rows, live and inactive, under a policy whose ratio is 1 to rounding (lp_old is the row's own log-probability):
    the critic half of every kernel is independent of it"""
    rows = value_clip_rows()
    n = 2 * len(rows)
    shape = (1, n, 1)
    active = np.tile(np.array([1.0, 0.0], F32), len(rows))
    v_now = np.repeat(np.array([r[0] for r in rows], F32), 2)
    v_tgt = np.repeat(np.array([r[1] for r in rows], F32), 2)        # (an inactive row sits on the same decision, with another advantage)
    c = _policy(kind, shape, A, state, squash, np.random.default_rng(seed))
    r = lambda x: np.ascontiguousarray(x, F32).reshape(shape)
    c.update(shape=shape, eps=V_EPS, ent_coef=ENT, active=r(active), v_now=r(v_now), v_old=r(np.zeros(n)), v_tgt=r(v_tgt),
             adv=r(np.where(active == 0, 37.0, 0.5)), tags=[t for _, _, t in rows for _ in range(2)])
    c["lp_old"] = log_prob64(c)[0].astype(F32)
    return c


def value_decisions(c, dtype):
    """(din, sign(qa - qb)) of every row in the given precision, in ppo_elem's order of operations: what has to agree between fp32 and
    f64 for a value-clip row to be exact"""
    vn, vo, vt = (c[k].astype(dtype).reshape(-1) for k in ("v_now", "v_old", "v_tgt"))
    eps = dtype(c["eps"])
    d = vn - vo
    ec, eo = (np.clip(d, -eps, eps) + vo) - vt, vn - vt
    return (d >= -eps) & (d <= eps), np.sign(ec * ec - eo * eo)


# ---- edge batch 3: the categorical clamp ----------------------------------------------------------------------------------------------------
CAT_EPS = 0.2
CAT_ENT = 2.0 ** -18
CAT_SMALL_ADV = 2.0 ** -18
CAT_PAIRS = ((2.0 ** -23, 1.0 - 2.0 ** -23, "on"), (2.0 ** -24, 1.0 - 2.0 ** -24, "outside"))


def categorical_case(A, ent_coef):
    """rows (p_small, p_large) on / beyond probs_to_logits' clamp edges, in slots (0, 1) of A = 2 or (3, 11) of A = 16 (the rest exact
    zeros), either order, either entry the taken action, live and inactive.  The fp32 sum of a row is exactly 1.

    The gradient through prob / prob.sum() is g_k = gp_k - sum_j gp_j p_j.  Where the taken action is the entry next to 1, g of that
    entry is the difference of two numbers that agree to 2^-23: fp32 (the kernel's or torch's) cannot form it to a relative 1e-5.  Those
    rows therefore carry a small dyadic advantage (2^-18), and the entropy coefficient of the batch is 2^-18 as well, which puts the one
    ill-conditioned element below the comparison's floor of 1e-12 while the other elements of the row, which are what an open clamp would change
    (0 in place of -g_lp), stay eight orders of magnitude above it."""
    assert A in (2, 16)
    i, j = (0, 1) if A == 2 else (3, 11)
    big = (1.5, 0.0, -0.75, 0.0)                            # (the rows that take the small entry: k is even)
    prob, action, adv, active, tags = [], [], [], [], []
    k = 0
    for ps, pl, tag in CAT_PAIRS:
        for si, li in ((i, j), (j, i)):
            for a in (si, li):
                row = np.zeros(A, F32)
                row[si], row[li] = F32(ps), F32(pl)
                assert row.sum(dtype=F32) == F32(1) and row.astype(np.float64).sum() == 1.0
                a_row = (CAT_SMALL_ADV if k % 4 < 2 else -CAT_SMALL_ADV) if a == li else big[k % 4]
                for act in (1.0, 0.0):
                    prob.append(row)
                    action.append(float(a))
                    active.append(act)
                    adv.append(a_row if act else a_row * 64.0 + 9.0)
                    tags.append((tag, "small" if a == si else "large"))
                k += 1
    n = len(prob)
    shape = (1, n, 1)
    r = lambda x: np.ascontiguousarray(x, F32).reshape(shape)
    c = dict(kind="prob", shape=shape, A=A, prob=np.stack(prob).reshape(shape + (A,)), action=r(action), adv=r(adv), active=r(active),
             v_now=r(np.linspace(-1, 1, n)), v_old=r(np.linspace(-1, 1, n) + 0.0625), v_tgt=r(np.full(n, 0.5)), eps=CAT_EPS, ent_coef=ent_coef,
             tags=tags)
    c["lp_old"] = (log_prob64(c)[0] + 0.01).astype(F32)       # ratio about 0.99: inside the clip range whatever the last bit of logf is
    return c


# ---- edge batch 4: the log-std bounds -------------------------------------------------------------------------------------------------------
LS_LO, LS_HI, LS_EPS = -0.5, 0.5, 0.2
LS_VALUES = np.array([F32(LS_LO), F32(LS_HI), steps_out(F32(LS_LO), 1), steps_out(F32(LS_HI), 1), steps_out(F32(LS_LO), -1),
                      steps_out(F32(LS_HI), -1)], F32)     # on lo, on hi, one step beyond each, one step inside each
LS_PASS = np.array([True, True, False, False, True, True])
LS_D = np.array([0.5, -1.25, 2.0, -0.25, 1.5, -2.5], F32)  # u - mu: dyadic, and d^2 / sigma^2 stays clear of 1


def log_std_case(state, squash):
    """A = 6: the six values above as the log_std vector (param mode), or rolled through the dimensions row by row (state mode)"""
    A, n = 6, 12
    shape = (1, n, 1)
    active = np.tile(np.array([1.0, 0.0], F32), n // 2)
    mu = (np.arange(n * A).reshape(n, A) % 5 - 2).astype(F32) * F32(0.25)
    action = mu + np.stack([np.roll(LS_D, k // 2) for k in range(n)])
    ls = np.stack([np.roll(LS_VALUES, k // 2) for k in range(n)]) if state else LS_VALUES.copy()
    passes = np.stack([np.roll(LS_PASS, k // 2) for k in range(n)]) if state else LS_PASS.copy()
    r = lambda x: np.ascontiguousarray(x, F32).reshape(shape)
    adv = np.where(active == 0, 41.0, np.tile(np.array([1.5, 1.5, 0.75, 0.75], F32), n // 4))
    c = dict(kind="gauss_ex", shape=shape, A=A, state=state, squash=squash, lo=LS_LO, hi=LS_HI, mu=mu.reshape(shape + (A,)),
             action=action.astype(F32).reshape(shape + (A,)), ls=ls.reshape(shape + (A,)) if state else ls, passes=passes, adv=r(adv),
             active=r(active), v_now=r(np.linspace(-1, 1, n)), v_old=r(np.linspace(-1, 1, n) - 0.0625), v_tgt=r(np.full(n, 0.5)), eps=LS_EPS,
             ent_coef=ENT)
    sign = np.where(np.arange(n) % 4 < 2, 1.0, -1.0)
    c["lp_old"] = (log_prob64(c)[0] + 0.01 * sign.reshape(shape)).astype(F32)   # ratios about 0.99 and 1.01: inside the clip range
    return c


def log_std_condition(c):
    """sum |terms| / |sum of terms| of every g_ls entry whose clamp passes: the factor by which fp32's relative rounding is magnified"""
    ls = np.clip(np.broadcast_to(c["ls"], c["mu"].shape).astype(np.float64), c["lo"], c["hi"])
    d = c["action"].astype(np.float64) - c["mu"].astype(np.float64)
    ref = reference(c, True)
    act = c["active"].astype(np.float64)
    up = act / act.sum()
    g_lp = (ref["grads"][0] * np.exp(2 * ls) / np.where(d == 0, 1, d))[..., :1]          # g_mu = g_lp d / sigma^2
    mag = np.abs(g_lp) * (d * d / np.exp(2 * ls) + 1) + (up * c["ent_coef"])[..., None]
    g_ls = ref["grads"][1]
    if not c["state"]:
        mag = mag.reshape(-1, c["A"]).sum(0)
    keep = c["passes"].reshape(g_ls.shape) & (g_ls != 0)
    return (mag / np.where(keep, np.abs(g_ls), 1))[keep]


# ---- bulk ------------------------------------------------------------------------------------------------------------------------------------
def _policy(kind, shape, A, state, squash, rng, sharp=2.0):
    """random operands of one policy (no PPO inputs yet)"""
    f = lambda *s: rng.standard_normal(s).astype(F32)
    c = dict(kind=kind, shape=tuple(shape), A=A, state=state, squash=squash)
    if kind == "plain":
        c["lp_now"], c["ent"] = (f(*shape) * 2 - 3).astype(F32), (f(*shape) * F32(0.3) + 2).astype(F32)
    elif kind == "prob":
        logits = f(*shape, A).astype(np.float64) * sharp
        e = np.exp(logits - logits.max(-1, keepdims=True))
        c["prob"] = (e / e.sum(-1, keepdims=True)).astype(F32) * F32(1.25)        # unnormalised: the kernel renormalises
        c["action"] = rng.integers(0, A, shape).astype(F32)
    else:
        c["mu"] = f(*shape, A)
        c["lo"], c["hi"] = (-1.0, 0.5) if kind == "gauss_ex" else (-INF, INF)
        c["ls"] = (f(*shape, A) * F32(0.8) - F32(0.3)).astype(F32) if state else (f(A) * F32(0.8) - F32(0.3)).astype(F32)   # some beyond the bounds
        # the action is a sample of the policy, as in the rollout and in the generators whose tolerances these tests take over
        # (tests/test_gauss_gpu.py, tests/test_gauss_sd_gpu.py): (u - mu) / sigma is of order 1 and the log-probability of order A.  An
        # action drawn without regard to sigma puts it at a thousand, where its fp32 rounding alone moves the ratio by more than 1e-5.
        sigma = np.exp(np.clip(c["ls"].astype(np.float64), c["lo"], c["hi"]))
        c["action"] = (c["mu"] + sigma * rng.standard_normal(shape + (A,))).astype(F32)
    return c


def violations(c):
    """the rows of a case that break a precondition of the bulk comparison, in f64: (ratio within 1e-3 relative of 1 -+ eps,
    | |v_now - v_old| - eps | < 1e-3, outside the value clip with |qa - qb| <= 1e-5 max(qa, qb)).  Beyond them fp32 and f64 take the
    same side of every decision, so the two differ by rounding alone."""
    eps = float(c["eps"])
    v_now, lp_old, v_old, v_tgt = _f64(c, "v_now", "lp_old", "v_old", "v_tgt")
    ratio = np.exp(log_prob64(c)[0] - lp_old)
    near_ratio = (np.abs(ratio / (1 - eps) - 1) < 1e-3) | (np.abs(ratio / (1 + eps) - 1) < 1e-3)
    dv = v_now - v_old
    near_dv = np.abs(np.abs(dv) - eps) < 1e-3
    ec, eo = np.clip(dv, -eps, eps) + v_old - v_tgt, v_now - v_tgt
    qa, qb = ec * ec, eo * eo
    near_tie = (np.abs(dv) > eps) & (np.abs(qa - qb) <= 1e-5 * np.maximum(qa, qb))
    return near_ratio, near_dv, near_tie


def case_seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def bulk_case(kind, shape, A=0, state=False, squash="clip", sharp=2.0):
    """random rows of one loss call, about a third of them inactive and holding finite garbage.  Rows that break a precondition are
    nudged (lp_old by -0.01, v_old by +0.01, v_tgt by +0.01), none is dropped; c["passes"] counts the passes that nudged something and
    the preconditions are asserted before the case is handed out, hence before any launch."""
    rng = np.random.default_rng(case_seed(kind, shape, A, state, squash, sharp))
    f = lambda *s: rng.standard_normal(s).astype(F32)
    c = _policy(kind, shape, A, state, squash, rng, sharp)
    c["eps"], c["ent_coef"], c["sharp"] = BULK_EPS, ENT, sharp
    active = (rng.random(shape) > 1 / 3).astype(F32)
    active.reshape(-1)[0] = 1.0                              # (the one-row case stays live)
    dead = active == 0
    c["active"] = active
    # both signs, around 1/2: with a mean of 0 the actor loss is what is left of terms of order 1 that cancel, and fp32's rounding of
    # those terms would be measured against a loss of almost nothing
    c["adv"] = np.where(dead, f(*shape) * F32(30), f(*shape) + F32(0.5)).astype(F32)
    c["v_old"] = f(*shape)
    c["v_tgt"] = np.where(dead, f(*shape) * F32(30), f(*shape) * 2 + 1).astype(F32)
    c["v_now"] = (c["v_tgt"] + f(*shape) * F32(0.7)).astype(F32)
    c["v_old"] = np.where(rng.random(shape) < 0.5, c["v_now"] + f(*shape) * F32(0.15), c["v_old"]).astype(F32)    # half inside the value clip
    lp64 = log_prob64(c)[0]
    c["lp_old"] = (lp64 + rng.standard_normal(shape) * np.where(dead, 3.0, 0.15)).astype(F32)
    c["passes"] = 0
    for _ in range(3):
        near_ratio, near_dv, near_tie = violations(c)
        if not (near_ratio.any() or near_dv.any() or near_tie.any()):
            break
        c["passes"] += 1
        c["lp_old"] = np.where(near_ratio, c["lp_old"] - F32(0.01), c["lp_old"]).astype(F32)
        c["v_old"] = np.where(near_dv, c["v_old"] + F32(0.01), c["v_old"]).astype(F32)
        c["v_tgt"] = np.where(near_tie & ~near_dv, c["v_tgt"] + F32(0.01), c["v_tgt"]).astype(F32)
    assert_preconditions(c)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def assert_preconditions(c):
    near_ratio, near_dv, near_tie = violations(c)
    assert not near_ratio.any() and not near_dv.any() and not near_tie.any(), (c["kind"], c["shape"], c["A"], int(near_ratio.sum()),
                                                                                 int(near_dv.sum()), int(near_tie.sum()))


@functools.lru_cache(maxsize=None)
def bulk_reference(value_clip, *key):
    """reference(bulk_case(*key), value_clip), computed once per session"""
    return reference(bulk_case(*key), value_clip)


def bulk_keys():
    """the key of every bulk case the GPU tests launch (the arguments of bulk_case)"""
    keys = []
    for kind, A, state, squash in VARIANTS.values():
        keys += [(kind, shape, A, state, squash) for shape in SHAPES]
    for kind, state, squash in A_VARIANTS.values():
        keys += [(kind, shape, A, state, squash) for shape in A_SHAPES for A in range(1, 17)]
    keys += [("gauss_ex", shape, 4, state, "direction") for shape in A_SHAPES for state in (False, True)]
    keys += [("prob", shape, 9, False, "clip", SHARP) for shape in VIEW_SHAPES]
    return list(dict.fromkeys(keys))
