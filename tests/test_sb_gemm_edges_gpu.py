"""Every instantiation of k_sb_gemm_n128 (csrc/sb_gemm.hpp; 21 behind sb_gemm, sb_gemm_signs, sb_gemm_masked, sb_gemm_masked_bits) and
k_sb_colsum_reduce at the edges of the launch arithmetic, through the C entry points: the tile edges (1 .. 33 rows), grids of 1, 2, 3
and 129 workgroups, a full grid with one, two (one workgroup only), three and four trips, and -- 128 <- 128 only -- both sides of the
two row-count thresholds (tests/sb_edges_cases.py; each case first asserts that the device at hand puts it into its class).

Operands are column blocks of wider matrices with 32 guard rows behind row R: NaN behind X and the mask, 0xFF behind the mask bits, a
canary in the outputs, the sign bytes and the addend.  Guard rows, neighbouring columns and neighbouring bytes must come back
untouched (as bits) and nothing of a guard row may reach a column sum.

Bound (tests/test_split_bf16_gpu.py, tests/test_sb_wgrad_pc_gpu.py `_check`): with e = max |y - ref| / scale against the f64
act(x W^T + b + C), scale = |x| |W|^T + |b| + |C| per element, e_kernel <= 2 e_lib + 2^-23 where e_lib is torch's fp32 evaluation of
the same expression, and e_kernel <= K 2^-24, the textbook bound of a K-term fp32 dot product.  A column sum over R rows uses the sum
of the kept elements' scales; its textbook bound is (K + R) 2^-24: K 2^-24 per element and R - 1 fp32 additions of at most 2^-24 of
the running sum of magnitudes each.

Row independence: row r of every launch equals, bit for bit, the same epilogue applied in fp32 to row r of one anchor launch (plain
form, 4 127 rows) -- whatever R, grid and OPT.  sb_encoder_tail's contract rests on this."""
import time

import pytest
import torch

from tests import sb_edges_cases as cases

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
GUARD = 32
CANARY = -725003.0
CHUNK = 65536
SLOW = {}
WORST = {}


def _lib():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops, ops.load_library()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if SLOW:
        k = max(SLOW, key=SLOW.get)
        print(f"\nslowest case {k}: {SLOW[k]:.2f} s; {len(SLOW)} cases, {sum(SLOW.values()):.1f} s in all")
    for what, (ratio, tag) in sorted(WORST.items()):
        print(f"worst e_kernel / (2 e_lib + 2^-23), {what}: {ratio:.3f} at {tag}")
    _MASTER.clear()
    _ANCHOR.clear()


# ---- operands -------------------------------------------------------------------------------------------------------------------------
_MASTER, _ANCHOR = {}, {}


def _master(N, K, rows):
    """x (rows, K), W (N, K), b (N), addend (rows, N), mask (rows, N) of the shape; the first rows are the same whatever `rows` (a longer
    request appends).  W ~ 0.1 sqrt(128 / K) randn and b ~ N(0.55, 0.6): x W^T + b ~ N(0.55, 1.28), a third negative
    (tests/test_encoder_tail_gpu.py make_operands); the mask carries exact 0, -0 and 1e-42 (test_input_gradient_with_the_relu_..)"""
    m = _MASTER.get((N, K))
    have = m["x"].shape[0] if m else 0
    if have >= rows:
        return m
    if m is None:
        _MASTER.clear()                                  # one shape's operands at a time, and the anchor launch that belongs to them
        _ANCHOR.clear()
        g = torch.Generator(device="cuda").manual_seed(1000 * N + K)
        m = dict(W=(torch.randn(N, K + 4, device="cuda", generator=g) * (0.1 * (128.0 / K) ** 0.5))[:, 4:],
                 b=torch.randn(N, device="cuda", generator=g) * 0.6 + 0.55,
                 x=torch.empty(0, K, device="cuda"), add=torch.empty(0, N, device="cuda"), mask=torch.empty(0, N, device="cuda"))
        _MASTER[(N, K)] = m
    masked = "masked" in cases.FORMS[(N, K)]
    while have < rows:                                   # the anchor's rows first, on their own: the same numbers whatever comes later
        n = cases.ANCHOR_ROWS if have == 0 else rows - have
        g = torch.Generator(device="cuda").manual_seed(1000 * N + K + 7 * have + 1)
        m["x"] = torch.cat([m["x"], torch.randn(n, K, device="cuda", generator=g)])
        m["add"] = torch.cat([m["add"], torch.randn(n, N, device="cuda", generator=g) * 0.5])
        m["mask"] = torch.cat([m["mask"], torch.randn(n if masked else 0, N, device="cuda", generator=g)])
        have += n
    if masked:
        y = m["mask"]
        y[::3, ::5] = 0.0
        y[1::7, 1::4] = -0.0
        y[2::11, 2::3] = 1e-42
    return m


def _wide(R, cols, lead, ld, fill, body=None, dtype=torch.float32):
    """an (R + GUARD, ld) matrix of `fill` and its (R, cols) block at column `lead`, set to `body`"""
    assert lead + cols <= ld and (dtype != torch.float32 or (lead % 4 == 0 and ld % 4 == 0 and ld > cols))
    w = torch.full((R + GUARD, ld), fill, dtype=dtype, device="cuda")
    blk = w[:R, lead:lead + cols]
    if body is not None:
        blk.copy_(body[:R])
    assert blk.data_ptr() % (16 if dtype == torch.float32 else 1) == 0
    return w, blk


def _i32(t):
    return t.view(torch.int32)


def _untouched(w, R, lead, cols, fill):
    """everything of the wide matrix outside the (R, cols) block still holds `fill`, as bits"""
    if w.dtype == torch.uint8:
        same = lambda t: bool((t == fill).all())
    else:
        bits = int(torch.tensor([fill], dtype=torch.float32).view(torch.int32))
        same = lambda t: bool((_i32(t) == bits).all())
    return same(w[R:]) and same(w[:R, :lead]) and same(w[:R, lead + cols:])


def _epilogue(p, b, a, relu):
    """the kernel's epilogue on a raw product in fp32: (p + b) + a, then max(., 0)"""
    v = p if b is None else p + b
    v = v if a is None else v + a
    return torch.relu(v) if relu else v


def _forward(N, K, R, m, bias, relu, addend, signs, xw):
    """one sb_gemm / sb_gemm_signs launch into a fresh canary matrix.  addend: None, "separate" or "inplace".  Returns the result
    block, the sign bytes block (or None); asserts the return code and everything that must stay untouched."""
    ops, L = _lib()
    x = xw[1]
    W, b = m["W"], (m["b"] if bias else None)
    ldy, lead = N + 128 + 4, 128
    yw, y = _wide(R, N, lead, ldy, CANARY, m["add"] if addend == "inplace" else None)
    aw = a = None
    if addend == "separate":
        aw, a = _wide(R, N, 8, N + 12, CANARY, m["add"])
        assert a.stride(0) != y.stride(0)
    elif addend == "inplace":
        a = y
    bw = by = None
    args = [R, N, K, ops._ptr(x), x.stride(0), ops._ptr(W), W.stride(0), ops._ptr(b), int(relu), ops._ptr(a), a.stride(0) if a is not None else 0,
            ops._ptr(y), y.stride(0)]
    if signs:
        bw, by = _wide(R, N // 8, 16, N // 8 + 21, 0x5A, dtype=torch.uint8)
        rc = L.sb_gemm_signs(*args, ops._ptr(by), by.stride(0), ops._stream())
    else:
        rc = L.sb_gemm(*args, ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _untouched(yw, R, lead, N, CANARY), "the result's guard rows or neighbouring columns changed"
    if aw is not None:
        assert _untouched(aw, R, 8, N, CANARY) and torch.equal(_i32(a), _i32(m["add"][:R])), "the addend changed"
    if signs:
        assert _untouched(bw, R, 16, N // 8, 0x5A), "the sign bytes' guard rows or neighbouring bytes changed"
    return y, by


def _xw(R, K, m):
    return _wide(R, K, 4, K + 8, float("nan"), m["x"])


def _anchor(N, K):
    """the raw product of the first 4 127 rows by the plain form (no bias, no ReLU)"""
    if (N, K) not in _ANCHOR:
        _ANCHOR.clear()
        m = _master(N, K, cases.ANCHOR_ROWS)
        _ANCHOR[(N, K)] = _forward(N, K, cases.ANCHOR_ROWS, m, False, False, None, False, _xw(cases.ANCHOR_ROWS, K, m))[0].clone()
    return _ANCHOR[(N, K)]


# ---- the f64 reference, in row chunks -----------------------------------------------------------------------------------------------------------
def _chunks(R):
    return [(r0, min(R, r0 + CHUNK)) for r0 in range(0, R, CHUNK)]


def _pre64(m, r0, r1, bias, addend):
    """f64 pre-activation x W^T + b + C of rows r0 .. r1 - 1, its scale |x| |W|^T + |b| + |C|, and torch's fp32 evaluation"""
    x, W = m["x"][r0:r1], m["W"]
    x64, W64 = x.double(), W.double()
    pre, scale = x64 @ W64.t(), x64.abs() @ W64.abs().t()
    base = None
    if bias:
        pre += m["b"].double()
        scale += m["b"].double().abs()
        base = m["b"]
    if addend:
        a = m["add"][r0:r1]
        pre += a.double()
        scale += a.double().abs()
        base = a if base is None else a + base
    lib = x @ W.t() if base is None else torch.addmm(base, x, W.t())
    return pre, scale, lib


def _check_forward(tag, what, y, by, R, K, m, bias, relu, addend):
    """the bound on y; the sign bytes against ref64 > 0 wherever |ref64| exceeds the bound; the share of negative pre-activations"""
    e = e_lib = 0.0
    neg = 0
    for r0, r1 in _chunks(R):
        pre, scale, lib = _pre64(m, r0, r1, bias, addend)
        ref = torch.relu(pre) if relu else pre
        lib = torch.relu(lib) if relu else lib
        den = scale.clamp_min(1e-300)
        e = max(e, float(((y[r0:r1].double() - ref).abs() / den).max()))
        e_lib = max(e_lib, float(((lib.double() - ref).abs() / den).max()))
        neg += int((pre < 0).sum())
    bound = 2.0 * e_lib + ULP
    print(f"{tag} {what}: e_kernel {e:.3e} e_lib {e_lib:.3e} ratio {e / bound:.3f}")
    WORST["elements"] = max(WORST.get("elements", (0.0, "")), (e / bound, f"{tag} {what}"))
    assert torch.isfinite(y).all(), (tag, what)
    assert e <= bound, (tag, what, e, e_lib)
    assert e <= K * 2.0 ** -24, (tag, what, e)
    if by is not None:
        tol = min(bound, K * 2.0 ** -24)
        wrong = 0
        for r0, r1 in _chunks(R):
            pre, scale, _ = _pre64(m, r0, r1, bias, addend)
            sure = pre.abs() > tol * scale
            wrong += int(((cases.unpack_signs(by[r0:r1]) != (pre > 0)) & sure).sum())
        assert wrong == 0, (tag, what, wrong)
    if bias and R >= 64:
        frac = neg / float(R * y.shape[1])
        assert 0.2 < frac < 0.45, (tag, what, frac)         # about a third of the pre-activations are negative


def _check_rows(tag, what, y, R, N, K, m, bias, relu, addend):
    """row r of this launch == the same epilogue on row r of the anchor launch"""
    n = min(R, cases.ANCHOR_ROWS)
    want = _epilogue(_anchor(N, K)[:n], m["b"] if bias else None, m["add"][:n] if addend else None, relu)
    assert torch.equal(y[:n], want), (tag, what, "rows differ from the anchor launch's")


def _assert_class(N, K, form, key, R, cus):
    """the case sits in the class it was chosen for on THIS device"""
    KC, NT, OPT = cases.form_variant(N, K, form, R)
    la = cases.sb_gemm_launch(R, KC, NT, cus, form.startswith("masked"))
    if key in cases.SMALL:
        grid = {1: 1, 15: 1, 16: 1, 17: 1, 31: 1, 32: 1, 33: 2, 95: 3, 4127: 129}[key]
        assert la.grid == grid and la.grid_mod4 == grid % 4 != 0 and la.trips == {1} and la.last_rows == (key - 1) % 32 + 1, (key, la)
    elif key == "32c-1":
        assert (la.grid, la.trips, la.last_rows, la.prologue_fetch) == (cus, {1}, 31, {False}), la
    elif key == "32c+1":
        assert (la.grid, la.trips, la.last_rows, la.second_trip_wgs, la.prologue_fetch) == (cus, {1, 2}, 1, 1, {True, False}), la
    elif key == "64c+17":
        assert (la.grid, la.trips, la.last_rows, la.two_ahead_fetch) == (cus, {2, 3}, 17, {True, False}), la
    elif key == "96c+45":
        assert (la.grid, la.trips, la.last_rows) == (cus, {3, 4}, 13), la
    else:
        assert key in cases.THRESHOLDS and (N, K) == (128, 128)
        assert la.wpc == (2 if R >= 131072 else 1) and la.grid == cus * la.wpc and min(la.trips) > 3 and la.two_ahead_fetch == {True, False}, la
        assert (OPT & 2 == 2) == (R >= 786432 and form != "addend"), (form, R, OPT)
    return KC, NT, OPT, la


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def _forward_case(tag, N, K, form, R, m):
    addend, signs = form in ("addend", "addend_signs"), form in ("signs", "addend_signs")
    xw = _xw(R, K, m)
    for bias, relu in ((True, True), (False, False)):
        for how in (("separate", "inplace") if addend else (None,)):
            what = f"bias {int(bias)} relu {int(relu)} addend {how}"
            y, by = _forward(N, K, R, m, bias, relu, how, signs, xw)
            _check_forward(tag, what, y, by, R, K, m, bias, relu, addend)
            _check_rows(tag, what, y, R, N, K, m, bias, relu, addend)
            if signs:
                y0, _ = _forward(N, K, R, m, bias, relu, how, False, xw)
                assert torch.equal(_i32(y), _i32(y0)), (tag, what, "the result differs from the launch without sign bits")
                assert torch.equal(by, cases.pack_signs(y)), (tag, what, "sign bytes != packed (Y > 0)")
    assert bool(torch.isnan(xw[0][R:]).all()) and torch.equal(_i32(xw[1]), _i32(m["x"][:R]))         # X is read only


def _masked_launch(N, K, R, m, xw, mask_cols, bits):
    ops, L = _lib()
    x, W = xw[1], m["W"]
    yw, y = _wide(R, N, 128, N + 128 + 4, CANARY)
    csw = torch.full((N + 8,), CANARY, device="cuda")
    cs = csw[4:4 + N]
    ws = torch.full((L.sb_gemm_masked_workspace(N),), 0xFF, dtype=torch.uint8, device="cuda")     # partial rows nobody wrote are NaN
    if bits:
        mw, mk = _wide(R, N // 8, 3, N // 8 + 5, 0xFF, cases.pack_signs(m["mask"][:R]), dtype=torch.uint8)
        rc = L.sb_gemm_masked_bits(R, N, K, ops._ptr(x), x.stride(0), ops._ptr(W), W.stride(0), ops._ptr(mk), mk.stride(0), mask_cols, ops._ptr(y),
                                   y.stride(0), ops._ptr(cs), ops._ptr(ws), ops._stream())
    else:
        mw, mk = _wide(R, N, 8, N + 12, float("nan"), m["mask"])
        rc = L.sb_gemm_masked(R, N, K, ops._ptr(x), x.stride(0), ops._ptr(W), W.stride(0), ops._ptr(mk), mk.stride(0), mask_cols, ops._ptr(y),
                              y.stride(0), ops._ptr(cs), ops._ptr(ws), ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _untouched(yw, R, 128, N, CANARY), "the result's guard rows or neighbouring columns changed"
    bitsc = int(torch.tensor([CANARY]).view(torch.int32))
    assert bool((_i32(csw[:4]) == bitsc).all()) and bool((_i32(csw[4 + N:]) == bitsc).all())
    return y, cs


def _masked_case(tag, N, K, form, R, m):
    assert R <= CHUNK
    xw = _xw(R, K, m)
    plain, _ = _forward(N, K, R, m, False, False, None, False, xw)
    _check_rows(tag, "plain launch", plain, R, N, K, m, False, False, False)
    pre, scale, lib = _pre64(m, 0, R, False, False)
    zero = torch.zeros_like(plain)
    for mask_cols in cases.mask_cols_of(N):
        what = f"mask_cols {mask_cols}"
        keep = torch.ones(R, N, dtype=torch.bool, device="cuda")
        keep[:, :mask_cols] = m["mask"][:R, :mask_cols] > 0
        runs = [_masked_launch(N, K, R, m, xw, mask_cols, form == "masked_bits") for _ in range(2)]
        (y, cs), (y2, cs2) = runs
        assert torch.isfinite(cs).all(), (tag, what, "a column sum is not finite")
        assert torch.equal(_i32(y), _i32(y2)) and torch.equal(_i32(cs), _i32(cs2)), (tag, what, "two runs differ")
        assert torch.equal(_i32(y), _i32(torch.where(keep, plain, zero))), (tag, what, "Y != where(keep, plain launch, 0)")
        other = _masked_launch(N, K, R, m, xw, mask_cols, form != "masked_bits")
        assert torch.equal(_i32(y), _i32(other[0])) and torch.equal(_i32(cs), _i32(other[1])), (tag, what, "float-mask and bit-mask forms differ")
        ref = pre * keep
        e = float(((y.double() - ref).abs() / scale.clamp_min(1e-300)).max())
        e_lib = float(((torch.where(keep, lib, zero).double() - ref).abs() / scale.clamp_min(1e-300)).max())
        print(f"{tag} {what} Y: e_kernel {e:.3e} e_lib {e_lib:.3e} ratio {e / (2.0 * e_lib + ULP):.3f}")
        WORST["elements"] = max(WORST.get("elements", (0.0, "")), (e / (2.0 * e_lib + ULP), f"{tag} {what}"))
        assert e <= 2.0 * e_lib + ULP and e <= K * 2.0 ** -24, (tag, what, e, e_lib)
        ref_cs, den_cs = ref.sum(0), (scale * keep).sum(0).clamp_min(1e-300)
        lib_cs = torch.where(keep, lib, zero).sum(0)
        ec, ec_lib = float(((cs.double() - ref_cs).abs() / den_cs).max()), float(((lib_cs.double() - ref_cs).abs() / den_cs).max())
        print(f"{tag} {what} column sums: e_kernel {ec:.3e} e_lib {ec_lib:.3e} ratio {ec / (2.0 * ec_lib + ULP):.3f}")
        WORST["column sums"] = max(WORST.get("column sums", (0.0, "")), (ec / (2.0 * ec_lib + ULP), f"{tag} {what}"))
        assert ec <= 2.0 * ec_lib + ULP, (tag, what, ec, ec_lib)
        assert ec <= (K + R) * 2.0 ** -24, (tag, what, ec)
    assert bool(torch.isnan(xw[0][R:]).all()) and torch.equal(_i32(xw[1]), _i32(m["x"][:R]))


@pytest.mark.parametrize("N,K,form,key", cases.gemm_cases(), ids=[f"{N}x{K}-{form}-{key}" for N, K, form, key in cases.gemm_cases()])
def test_split_gemm_variant_at_a_grid_edge(N, K, form, key):
    cus = _cus()
    R = cases.rows_of(key, cus)
    KC, NT, OPT, la = _assert_class(N, K, form, key, R, cus)
    tag = f"<{KC},{NT},{OPT}> {N}<-{K} {form} R {R} grid {la.grid}"
    t0 = time.perf_counter()
    with torch.no_grad():
        m = _master(N, K, max(R, cases.ANCHOR_ROWS))
        if form.startswith("masked"):
            _masked_case(tag, N, K, form, R, m)
        else:
            _forward_case(tag, N, K, form, R, m)
    torch.cuda.synchronize()
    SLOW[tag] = time.perf_counter() - t0
