"""Host reference of the action samplers (k_categorical / k_head in csrc/mappo_ops.hip), numpy only.

Row r of a launch draws from Philox4x32-10 (Random123) at counter `offset + r` with key `seed`: the 64-bit counter is the two low
counter words (c0 = low, c1 = high, c2 = c3 = 0), the 64-bit seed the two key words (k0 = low, k1 = high).  The kernels use word 0 of
the output: u = ((o0 >> 8) + 1/2) / 2^24 of the row's total probability, and the action is the first bin whose upper edge lies above u.
Here everything after the generator is exact (f64): where the kernels' fp32 arithmetic can decide an edge the other way, the row is
flagged ambiguous instead of guessed.
"""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
U24 = 2.0 ** -24   # fp32 unit roundoff, also the spacing of the u grid

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10_words(c0, c1, c2, c3, k0, k1):
    """the four output words of Philox4x32-10 for counter (c0, c1, c2, c3) and key (k0, k1); arrays of uint32 values (broadcast),
    returned as uint64 arrays"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _LO for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2   # 32 x 32 -> 64-bit products, exact in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def philox4x32_10(ctr, seed):
    """output word 0 for 64-bit counters `ctr` and a 64-bit `seed`, as the samplers call the generator"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    seed = int(seed)
    return philox4x32_10_words(ctr & _LO, ctr >> _32, 0, 0, seed & 0xFFFFFFFF, seed >> 32)[0]


def uniform(ctr, seed):
    """the exact point u / tot of each draw, in (0, 1)"""
    return ((philox4x32_10(ctr, seed) >> np.uint64(8)).astype(np.float64) + 0.5) * U24


def fp32_band(p, x):
    """half-width of the band around each bin edge inside which k_categorical's fp32 arithmetic may decide the other way: its
    running sums (sequential, so edge k carries at most U24 * sum_{j<=k} cum_j of rounding) against its draw (the u grid rounds
    ties to even above 2^23, half a step; the product with its own fp32 total, one rounding plus the total's error).  First order,
    with a 1 % margin for the second."""
    p = np.asarray(p, np.float64)
    cum = np.cumsum(p, axis=-1)
    err = np.cumsum(cum, axis=-1) - cum[..., :1]   # sum_{j=1..k} cum_j: the first addition 0 + p_0 is exact
    tot = cum[..., -1:]
    return 1.01 * U24 * (err + x[..., None] * err[..., -1:] + 1.5 * tot) + 1e-44


def inverse_cdf(p, ctr, seed, delta):
    """(action, ambiguous) of Categorical(p) at the draws of counters `ctr` (one per row of p, shape (R, A)).

    action: the first k with u * tot < cum_k in exact arithmetic on the fp32 probabilities; if no bin is hit (only when every
    probability is 0), the last k with p_k > 0, else A - 1.  A zero-probability bin is never hit: its upper edge equals the edge
    below it.  ambiguous: u * tot lies within `delta` of a bin edge.  `delta` is absolute, a number or an array that broadcasts
    against p (one width per edge), or a function of (p, x) returning one, x being the draw in (0, 1)."""
    p = np.asarray(p, np.float64)
    R, A = p.shape
    x = uniform(ctr, seed)
    cum = np.cumsum(p, axis=1)
    t = x * cum[:, -1]
    hit = t[:, None] < cum
    pos = p > 0
    last_pos = np.where(pos.any(1), A - 1 - np.argmax(pos[:, ::-1], axis=1), A - 1)
    action = np.where(hit.any(1), np.argmax(hit, axis=1), last_pos)
    d = delta(p, x) if callable(delta) else delta
    ambiguous = (np.abs(t[:, None] - cum) <= d).any(1)
    return action, ambiguous


def logp_ref(p, a):
    """Categorical(probs=p).log_prob(a) in f64: log(clamp(p_a / sum p, eps, 1 - eps)) (probs_to_logits clamps, no renormalising)"""
    p = np.asarray(p, np.float64)
    pa = np.take_along_axis(p, np.asarray(a, np.int64)[:, None], 1)[:, 0]
    return np.log(np.clip(pa / p.sum(1), FLT_EPSILON, 1.0 - FLT_EPSILON))


def logp_tol(p):
    """bound on |kernel - logp_ref| from k_categorical's fp32 total (sequential sum) and its division, beyond logf's own ulp"""
    p = np.asarray(p, np.float64)
    cum = np.cumsum(p, axis=1)
    return 1.01 * U24 * ((cum.sum(1) - cum[:, 0]) / np.maximum(cum[:, -1], 1e-300) + 1.0)
