"""The two action samplers against the exact host reference (tests/sampling_ref.py): categorical_sample (k_categorical) and the rollout
action head head_sample / head_linear (k_head, every instantiation), draw by draw on the Philox stream, including the top draw of the
u grid, which lands exactly on the row's total."""
import numpy as np
import pytest
import torch

from tests.helpers import no_gc_during_capture

from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu

# (seed, counter) pairs whose draw is the top of the u grid (o0 >> 8 == 0xFFFFFF): rank 0, rank 1 (r << 40), and one with both the
# counter's high word and the seed's high word non-zero
TOP_DRAWS = [(3, 2350790), (77, 3895978), (3, 0x10000634706), (0xDEADBEEF12345678, 0x500FCD3FEFA)]
HEAD_DELTA = 4e-6   # band around the bin edges for k_head: its fp32 logits, softmax and running sums against the f64 ones
HEAD_LOGP_ATOL = 2e-6


def _ops():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops


def _counter(v):
    return torch.full((1,), int(v), dtype=torch.int64, device="cuda")


def _probs(R, A, s, rng):
    """softmax(randn * s) rows in fp32, with every eighth-row pattern: zeros at the front, in the middle, at the end, a single
    positive entry, scaled by 1e-3 and 1e3, and an exact tie of the maximum (for greedy)"""
    z = rng.standard_normal((R, A)) * s
    e = np.exp(z - z.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(np.float32)
    kind = np.arange(R) % 8
    if A > 1:
        nz = max(1, A // 3)
        p[kind == 1, :nz] = 0
        if A > 2:
            m0 = max(1, (A - nz) // 2)
            p[kind == 2, m0:min(m0 + nz, A - 1)] = 0
        p[kind == 3, A - nz:] = 0
        one = np.nonzero(kind == 4)[0]
        keep = rng.integers(0, A, one.size)
        v = rng.uniform(0.1, 2.0, one.size).astype(np.float32)
        p[one] = 0
        p[one, keep] = v
        tie = np.nonzero(kind == 7)[0]
        j = np.sort(np.stack([rng.choice(A, 2, replace=False) for _ in tie]), 1) if tie.size else np.zeros((0, 2), int)
        mx = p[tie].max(1)
        p[tie, j[:, 0]] = mx
        p[tie, j[:, 1]] = mx
    p[kind == 5] *= np.float32(1e-3)
    p[kind == 6] *= np.float32(1e3)
    # s = 40 can leave nothing but subnormals after the zeroing (all-zero rows are out of the samplers' contract)
    p[p.sum(1) < 1e-30] = 1.0
    return p


def _check_draws(p, seed, offset, action, logp):
    """k_categorical's actions against the exact reference off the rounding band, no zero-probability action, and logp against
    Categorical(p).log_prob at the action; returns the number of ambiguous rows"""
    R, A = p.shape
    ctr = np.uint64(offset) + np.arange(R, dtype=np.uint64)
    ref, amb = sr.inverse_cdf(p, ctr, seed, sr.fp32_band)
    bad = np.nonzero(~amb & (action != ref))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}: kernel {action[bad[:5]]} ref {ref[bad[:5]]}"
    tot = p.astype(np.float64).sum(1)
    pa = p[np.arange(R), action]
    zero = np.nonzero((tot > 0) & (pa == 0))[0]
    assert zero.size == 0, f"zero-probability actions at rows {zero[:5]}: {action[zero[:5]]}"
    lr = sr.logp_ref(p, action)
    tol = 1e-6 * np.abs(lr) + 1e-7 + sr.logp_tol(p)
    worst = np.argmax(np.abs(logp - lr) - tol)
    assert np.abs(logp[worst] - lr[worst]) <= tol[worst], (worst, logp[worst], lr[worst])
    return int(amb.sum())


def _sample(p_dev, seed, offset, greedy=False):
    a, lp = _ops().categorical_sample(p_dev, seed, offset, greedy=greedy)
    return a.cpu().numpy(), lp.cpu().numpy()


@pytest.mark.parametrize("R", [1, 255, 256, 257, 65539])
@pytest.mark.parametrize("A", [1, 2, 3, 8, 9, 16, 17, 33, 100])
def test_categorical_sample_matches_the_exact_reference(A, R):
    ops = _ops()
    rng = np.random.default_rng(1000 * A + R)
    # offsets: rank 0; a carry into the counter's high word inside the launch; rank 1 / rank 5 streams (r << 40); seeds with a
    # non-zero high word (one with nothing but the high word)
    streams = [(3, 0), (0xDEADBEEF12345678, 2 ** 32 - R // 2), (77, (1 << 40) + 12345), (1 << 32, (5 << 40) + 2 ** 32 - R // 2)]
    n_amb = n = 0
    for s in (1, 8, 40):
        p = _probs(R, A, s, rng)
        p_dev = torch.from_numpy(p).cuda()
        for seed, offset in streams:
            a, lp = _sample(p_dev, seed, offset)
            n_amb += _check_draws(p, seed, offset, a, lp)
            n += R
            # the device-counter form: the same draws, the counter advanced by exactly R
            c = _counter(offset)
            ac, lpc = ops.categorical_sample(p_dev, seed, 0, counter=c)
            assert np.array_equal(ac.cpu().numpy(), a) and np.array_equal(lpc.cpu().numpy(), lp)
            assert int(c.item()) == offset + R
        # greedy: the first maximal index (torch.argmax / np.argmax on the exact ties of every eighth row), the counter still
        # advanced by R
        ref = np.argmax(p, 1)
        a, lp = _sample(p_dev, 3, 0, greedy=True)
        assert np.array_equal(a, ref)
        lr = sr.logp_ref(p, ref)
        assert np.all(np.abs(lp - lr) <= 1e-6 * np.abs(lr) + 1e-7 + sr.logp_tol(p))
        c = _counter(1 << 40)
        ac, _ = ops.categorical_sample(p_dev, 3, 0, greedy=True, counter=c)
        assert np.array_equal(ac.cpu().numpy(), ref) and int(c.item()) == (1 << 40) + R
    assert n_amb <= max(1, 1e-3 * n), (n_amb, n)


@pytest.mark.parametrize("nz", [1, 2])
@pytest.mark.parametrize("A", [3, 9, 33])
@pytest.mark.parametrize("seed,top", TOP_DRAWS)
def test_categorical_top_draw_skips_trailing_zeros(seed, top, A, nz):
    """u == tot exactly at the top of the u grid: no bin's upper edge lies above it, and the action must be the last category with
    positive probability, not A - 1 (probability 0 here)."""
    ops = _ops()
    assert int(sr.philox4x32_10(np.array([top], np.uint64), seed)[0]) >> 8 == 0xFFFFFF
    R, row = 300, 257
    rng = np.random.default_rng(A + nz)
    p = _probs(R, A, 1, rng)
    p[:, A - nz:] = 0
    p[p.sum(1) == 0, 0] = 1.0
    p[row] = rng.uniform(0.1, 1.0, A)   # a plain row: its zeros are the trailing ones
    p[row, A - nz:] = 0
    offset = top - row
    p_dev = torch.from_numpy(p).cuda()
    a, lp = _sample(p_dev, seed, offset)
    c = _counter(offset)
    ac, lpc = ops.categorical_sample(p_dev, seed, 0, counter=c)
    for act, logp in ((a, lp), (ac.cpu().numpy(), lpc.cpu().numpy())):
        assert act[row] == A - 1 - nz, act[row]
        assert abs(logp[row] - sr.logp_ref(p[row:row + 1], [A - 1 - nz])[0]) <= 1e-6
        _check_draws(p, seed, offset, act, logp)


def _head_weights(A, rng):
    W = (rng.standard_normal((A, 128)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(A) * 0.5).astype(np.float32)
    return W, b


def _softmax64(feat, W, b):
    y = feat.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    e = np.exp(y - y.max(1, keepdims=True))
    return y, e / e.sum(1, keepdims=True)


def _head_sample(feat_d, W_d, b_d, seed, c0, greedy=False):
    ops = _ops()
    R = feat_d.shape[0]
    counter, ticket = _counter(c0), torch.zeros(1, dtype=torch.int32, device="cuda")
    a = torch.empty(R, dtype=torch.int32, device="cuda")
    lp = torch.empty(R, device="cuda")
    with torch.no_grad():
        ops.head_sample(feat_d, W_d, b_d, seed, counter, ticket, (a, lp), greedy=greedy)
    assert int(counter.item()) == c0 + R and int(ticket.item()) == 0
    return a.cpu().numpy(), lp.cpu().numpy()


def _check_head_draws(p64, seed, c0, a, lp):
    R = p64.shape[0]
    ref, amb = sr.inverse_cdf(p64, np.uint64(c0) + np.arange(R, dtype=np.uint64), seed, HEAD_DELTA)
    bad = np.nonzero(~amb & (a != ref))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}: kernel {a[bad[:5]]} ref {ref[bad[:5]]}"
    err = np.abs(lp - sr.logp_ref(p64, a))
    assert err.max() <= HEAD_LOGP_ATOL, (int(np.argmax(err)), err.max())
    return int(amb.sum())


@pytest.fixture(scope="module")
def head_feat():
    """one feature matrix for every head test (the largest R is 2 * 262144 + 37 rows: past one sweep of the capped grid)"""
    f = np.random.default_rng(7).standard_normal((2 * 262144 + 37, 128), dtype=np.float32)
    return f, torch.from_numpy(f).cuda()


@pytest.mark.parametrize("R", [1, 63, 64, 65, 32768, 2 * 262144 + 37])
@pytest.mark.parametrize("A", list(range(1, 17)))
def test_head_matches_f64_reference(A, R, head_feat):
    """head_linear within the fp32 dot-product bound of the f64 logits; head_sample's actions against the exact inverse CDF of the f64
    softmax off the rounding band, its log-probabilities within 2e-6, the counter and the ticket; greedy = the f64 argmax off
    near-ties.  R = 2 * 262144 + 37 runs the grid-stride loop (1024 workgroups x 256 rows per sweep)."""
    ops = _ops()
    rng = np.random.default_rng(17 * A + R)
    feat, feat_d = head_feat[0][:R], head_feat[1][:R]
    W, b = _head_weights(A, rng)
    W_d, b_d = torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda()
    y64, p64 = _softmax64(feat, W, b)
    with torch.no_grad():
        assert ops._head_ok(feat_d, W_d, b_d)   # the kernel, not the F.linear fallback
        y = ops.head_linear(feat_d, W_d, b_d).cpu().numpy()
    bound = 130 * sr.U24 * (np.abs(feat) @ np.abs(W.astype(np.float64)).T + np.abs(b))
    assert np.all(np.abs(y - y64) <= bound), float(np.max(np.abs(y - y64) / bound))

    seed, c0 = 0xDEADBEEF12345678 ^ A, (3 << 40) + 2 ** 32 - R // 2   # the counter's high word carries inside the launch
    a, lp = _head_sample(feat_d, W_d, b_d, seed, c0)
    n_amb = _check_head_draws(p64, seed, c0, a, lp)
    assert n_amb <= max(1, 1e-3 * R), n_amb

    a, lp = _head_sample(feat_d, W_d, b_d, seed, c0, greedy=True)
    top2 = np.sort(y64, 1)[:, -2:] if A > 1 else np.concatenate([y64 - 1, y64], 1)
    clear = top2[:, 1] - top2[:, 0] > 1e-5
    assert np.array_equal(a[clear], np.argmax(y64, 1)[clear])
    assert np.abs(lp - sr.logp_ref(p64, a)).max() <= HEAD_LOGP_ATOL


@pytest.mark.parametrize("nz", [1, 2])
@pytest.mark.parametrize("A", [3, 9, 16])
@pytest.mark.parametrize("seed,top", TOP_DRAWS)
def test_head_top_draw_skips_trailing_zeros(seed, top, A, nz):
    """the fused head at the top draw: a bias of -300 makes the trailing probabilities exactly 0 in the kernel's fp32 softmax"""
    R, row = 300, 257
    rng = np.random.default_rng(A + nz)
    feat = rng.standard_normal((R, 128), dtype=np.float32)
    W, b = _head_weights(A, rng)
    b[A - nz:] = -300.0
    _, p64 = _softmax64(feat, W, b)
    c0 = top - row
    a, lp = _head_sample(torch.from_numpy(feat).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(), seed, c0)
    assert a[row] == A - 1 - nz, a[row]
    assert abs(lp[row] - np.log(p64[row, A - 1 - nz])) <= HEAD_LOGP_ATOL
    assert np.all(a < A - nz)
    _check_head_draws(p64, seed, c0, a, lp)


def test_samplers_replay_in_a_captured_graph():
    """head_sample and categorical_sample(counter=) captured in one graph on one stream and replayed three times: capturing runs
    nothing, every replay advances each counter by R and draws what the reference draws at the counter it found."""
    ops = _ops()
    R, A = 4099, 9
    rng = np.random.default_rng(11)
    feat = rng.standard_normal((R, 128), dtype=np.float32)
    W, b = _head_weights(A, rng)
    _, p64 = _softmax64(feat, W, b)
    p = _probs(R, A, 2, rng)
    feat_d, W_d, b_d, p_d = (torch.from_numpy(v).cuda() for v in (feat, W, b, p))
    (sh, ch), (sc, cc) = (0xDEADBEEF12345678, (1 << 40) + 2 ** 32 - 100), (5, (2 << 40) + 77)
    c_head, c_cat = _counter(ch), _counter(cc)
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    a_h, lp_h = torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, device="cuda")
    a_c, lp_c = torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with no_gc_during_capture(), torch.no_grad(), torch.cuda.graph(graph):
        ops.head_sample(feat_d, W_d, b_d, sh, c_head, ticket, (a_h, lp_h))
        ops.categorical_sample(p_d, sc, 0, counter=c_cat, out=(a_c, lp_c))
    torch.cuda.synchronize()
    assert int(c_head.item()) == ch and int(c_cat.item()) == cc
    for k in range(1, 4):
        graph.replay()
        torch.cuda.synchronize()
        assert int(c_head.item()) == ch + k * R and int(c_cat.item()) == cc + k * R and int(ticket.item()) == 0
        _check_head_draws(p64, sh, ch + (k - 1) * R, a_h.cpu().numpy(), lp_h.cpu().numpy())
        _check_draws(p, sc, cc + (k - 1) * R, a_c.cpu().numpy(), lp_c.cpu().numpy())
