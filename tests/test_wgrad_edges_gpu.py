"""Both weight-gradient kernel families at the edges of their split-K arithmetic, through the C entry points (ops.wgrad sends fewer
than 4 096 rows to the BLAS library): the five instantiations of k_sb_wgrad (csrc/sb_wgrad.hpp) behind wgrad_split_tn /
wgrad_split_tn2 and the three of k_wgrad with k_wgrad_reduce (csrc/mappo_ops.hip) behind wgrad_tn.  tests/wgrad_edges_cases.py has
the row counts and the launch arithmetic; every case first asserts which class it is in.

Split kernel: 0 .. 9 chunks per workgroup (fewer than the loader's DEPTH, DEPTH, the second and third trip of its `c += D` loop), the
mixed counts {0,1} .. {8,9}, a K % 16 tail after every count (the tail overwrites image 0: after an odd and after an even count), for
all three loader layouts.  fp32 kernel: 0, 1, 7, 8, 9, 15, 16, 17 and 24 steps per workgroup (0 .. 3 pairs of stages, 0, 1 and 7
left-over steps), every K % 4, grids with y or z above 1, and S = 256, 128, 64, 51, 42, 28, 25 and 4 partials for k_wgrad_reduce.

Operands are column blocks of wider matrices (lead column and stride multiples of 4) with 32 guard rows behind row K; guard rows and
neighbouring columns are NaN, so a row behind K or a column beside an operand that reaches the result makes it NaN.  C lies between
two canaries; the workspace is exactly wgrad_*_workspace(M, N) bytes between two canaries, pre-filled with 0xFF (a partial nobody
wrote is NaN).  With accumulate = 0, C is pre-filled with NaN.  Every launch runs twice for identical bits.

Bound (tests/test_sb_wgrad_pc_gpu.py `_check`): with e = max |c - ref| / scale against the f64 a^T b (+ C0), scale = |a|^T |b| (+ |C0|),
e_kernel <= 2 e_lib + 2^-23 where e_lib is torch's fp32 a.T @ b (+ C0), and e_kernel <= K 2^-24, the textbook bound of a K-term fp32
dot product."""
import time

import pytest
import torch

from tests import wgrad_edges_cases as cases

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
GUARD = 32
PAD = 64                  # canary floats before and after C
WS_PAD = 256              # canary bytes before and after the workspace
CANARY = -725003.0
BAD_ARG = 20001           # include/mappo_ops.h MO_ERR_BAD_ARG
SLOW = {}
WORST = {}
_MASTER = {}
_WS = {}


def _lib():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops, ops.load_library()


@pytest.fixture(scope="module", autouse=True)
def _report():
    _lib()                                               # the library and the device context are up before the first case is timed
    torch.zeros(1, device="cuda").sum().item()
    yield
    if SLOW:
        k = max(SLOW, key=SLOW.get)
        print(f"\nslowest case {k}: {SLOW[k]:.2f} s; {len(SLOW)} cases, {sum(SLOW.values()):.1f} s in all")
    for what, (ratio, tag) in sorted(WORST.items()):
        print(f"worst e_kernel / (2 e_lib + 2^-23), {what}: {ratio:.3f} at {tag}")
    _MASTER.clear()
    _WS.clear()


def _i32(t):
    return t.view(torch.int32)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def _master(fam, M, N, rows):
    """a (rows, M), b (rows, N) of a family and shape: one pair at a time, generated once at the most rows any of its cases needs"""
    key = (fam, M, N)
    if key not in _MASTER or _MASTER[key][0].shape[0] < rows:
        _MASTER.clear()
        g = torch.Generator(device="cuda").manual_seed(1000 * M + N + (7 if fam == "fp32" else 0))
        _MASTER[key] = (torch.randn(rows, M, device="cuda", generator=g), torch.randn(rows, N, device="cuda", generator=g))
    return _MASTER[key]


def _max_rows(fam, M, N):
    return 36877 if fam == "split" else 4 * cases.WG_S[(M, N)] * 24 + 3


def _wide(K, cols, lead, ld, body):
    """a (K + GUARD, ld) matrix of NaN and its (K, cols) block at column `lead`, set to the first K rows of `body`"""
    assert lead % 4 == 0 and ld % 4 == 0 and lead + cols <= ld and ld > cols
    w = torch.full((K + GUARD, ld), float("nan"), device="cuda")
    blk = w[:K, lead:lead + cols]
    blk.copy_(body[:K])
    assert blk.data_ptr() % 16 == 0 and blk.stride(0) == ld
    return blk


def _operands(fam, M, N, K):
    ma, mb = _master(fam, M, N, _max_rows(fam, M, N))
    return _wide(K, M, 4, M + 8, ma), _wide(K, N, 8, N + 12, mb)


def _workspace(nbytes):
    """exactly nbytes of 0xFF between two canaries"""
    if nbytes not in _WS:
        _WS.clear()
        _WS[nbytes] = torch.empty(nbytes + 2 * WS_PAD, dtype=torch.uint8, device="cuda")
    buf = _WS[nbytes]
    buf[:WS_PAD] = 0xA5
    buf[WS_PAD:WS_PAD + nbytes] = 0xFF
    buf[WS_PAD + nbytes:] = 0xA5
    ws = buf[WS_PAD:WS_PAD + nbytes]
    assert ws.data_ptr() % 16 == 0
    return buf, ws


def _launch(fam, a, b, c0=None, a2=None):
    """one launch into a fresh C between canaries (NaN, or c0 with accumulate = 1) -> a copy of C; asserts the return code, the
    workspace size and every canary.  a2: the second column block of A (wgrad_split_tn2)"""
    ops, L = _lib()
    K, N = a.shape[0], b.shape[1]
    M = a.shape[1] + (a2.shape[1] if a2 is not None else 0)
    if fam == "split":
        nbytes, want = L.wgrad_split_workspace(M, N), cases.SB_WGS * M * N * 4
    else:
        nbytes, want = L.wgrad_tn_workspace(M, N), cases.wgrad_split(M, N)[0] * M * N * 4
    assert nbytes == want, (nbytes, want)
    buf, ws = _workspace(nbytes)
    cw = torch.full((PAD + M * N + PAD,), CANARY, device="cuda")
    c = cw[PAD:PAD + M * N].view(M, N)
    if c0 is None:
        c.fill_(float("nan"))
    else:
        c.copy_(c0)
    acc = int(c0 is not None)
    if a2 is not None:
        assert fam == "split"
        rc = L.wgrad_split_tn2(K, a.shape[1], a2.shape[1], N, ops._ptr(a), a.stride(0), ops._ptr(a2), a2.stride(0), ops._ptr(b), b.stride(0),
                               ops._ptr(c), acc, ops._ptr(ws), ops._stream())
    else:
        fn = L.wgrad_split_tn if fam == "split" else L.wgrad_tn
        rc = fn(K, M, N, ops._ptr(a), a.stride(0), ops._ptr(b), b.stride(0), ops._ptr(c), acc, ops._ptr(ws), ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    bits = int(torch.tensor([CANARY]).view(torch.int32))
    assert bool((_i32(cw[:PAD]) == bits).all()) and bool((_i32(cw[PAD + M * N:]) == bits).all()), "the floats around C changed"
    assert bool((buf[:WS_PAD] == 0xA5).all()) and bool((buf[WS_PAD + nbytes:] == 0xA5).all()), "the bytes around the workspace changed"
    return c.clone()


def _twice(fam, a, b, c0=None, a2=None):
    c1, c2 = _launch(fam, a, b, c0, a2), _launch(fam, a, b, c0, a2)
    assert torch.equal(_i32(c1), _i32(c2)), "two runs differ"
    return c1


def _check(tag, fam, c, a, b, c0=None):
    """c = (c0 +) a^T b: finite, within 2 x the fp32 library's error + 1 ulp and within K 2^-24 of the f64 product"""
    K = a.shape[0]
    a64, b64 = a.double(), b.double()
    ref, scale, lib = a64.t() @ b64, a64.abs().t() @ b64.abs(), a.t() @ b
    if c0 is not None:
        ref, scale, lib = ref + c0.double(), scale + c0.double().abs(), lib + c0
    den = scale.clamp_min(1e-300)
    e, e_lib = float(((c.double() - ref).abs() / den).max()), float(((lib.double() - ref).abs() / den).max())
    bound = 2.0 * e_lib + ULP
    print(f"{tag}: e_kernel {e:.3e} e_lib {e_lib:.3e} ratio {e / bound:.3f} e_kernel / (K 2^-24) {e / (K * 2.0 ** -24):.3f}")
    WORST[fam] = max(WORST.get(fam, (0.0, "")), (e / bound, tag))
    assert torch.isfinite(c).all(), tag
    assert e <= bound, (tag, e, e_lib)
    assert e <= K * 2.0 ** -24, (tag, e)


# ---- k_sb_wgrad ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", cases.sb_cases(), ids=[f"{M}x{N}-{K}" for M, N, K in cases.sb_cases()])
def test_split_wgrad_at_a_chunk_edge(M, N, K):
    """K = 1 and 15 are a tail alone, which k_sb_wgrad multiplies in fp32 itself: with the tail as piece products on the bf16 matrix
    instruction (truncated accumulation) K = 1 measured e_kernel 1.19e-07 .. 1.36e-07 on the five shapes, 2.0
    to 2.3 times the textbook bound 1 x 2^-24, with e_lib 5.9e-08"""
    lay, cnt = cases.sb_wgrad_layout(M, N), cases.sb_wgrad_counts(K)
    assert (cnt.counts, cnt.tail) == cases.sb_expected(K), cnt
    tag = f"split {M}x{N} K {K} chunks {sorted(cnt.counts)} tail {cnt.tail} DEPTH {lay.DEPTH} off {lay.off_waves}"
    t0 = time.perf_counter()
    a, b = _operands("split", M, N, K)
    _check(tag, "split", _twice("split", a, b), a, b)
    SLOW[tag] = time.perf_counter() - t0


@pytest.mark.parametrize("M,N", cases.SB_SHAPES)
@pytest.mark.parametrize("K", cases.SB_ACC_ROWS)
def test_split_wgrad_accumulates_onto_c(M, N, K):
    tag = f"split {M}x{N} K {K} accumulate"
    t0 = time.perf_counter()
    a, b = _operands("split", M, N, K)
    c0 = torch.randn(M, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(K + M)) * float(K) ** 0.5
    _check(tag, "split", _twice("split", a, b, c0), a, b, c0)
    SLOW[tag] = time.perf_counter() - t0


@pytest.mark.parametrize("M,N", cases.SB_SHAPES)
@pytest.mark.parametrize("n", cases.SB_ZERO_TAIL_N)
def test_split_wgrad_zero_tail_changes_no_bit(M, N, n):
    """K = 4096 n: every workgroup owns n chunks.  The same rows with 13 zero rows appended run the same chunks and then the tail path,
    which contributes zeros: the same bits"""
    K = 4096 * n
    assert cases.sb_wgrad_counts(K) == cases.sb_wgrad_counts(K + 13)._replace(tail=0) and cases.sb_wgrad_counts(K + 13).tail == 13
    tag = f"split {M}x{N} K {K} against K + 13 with zero rows"
    t0 = time.perf_counter()
    ma, mb = _master("split", M, N, _max_rows("split", M, N))
    zeros = torch.zeros(13, max(M, N), device="cuda")
    a, b = _wide(K, M, 4, M + 8, ma), _wide(K, N, 8, N + 12, mb)
    az, bz = _wide(K + 13, M, 4, M + 8, torch.cat([ma[:K], zeros[:, :M]])), _wide(K + 13, N, 8, N + 12, torch.cat([mb[:K], zeros[:, :N]]))
    assert torch.equal(_i32(_twice("split", a, b)), _i32(_twice("split", az, bz))), tag
    SLOW[tag] = time.perf_counter() - t0


@pytest.mark.parametrize("M,N,M1,K", cases.tn2_cases(), ids=[f"{M}x{N}-M1_{M1}-{K}" for M, N, M1, K in cases.tn2_cases()])
def test_split_wgrad_two_column_blocks(M, N, M1, K):
    """wgrad_split_tn2 with A's columns changing tensors at M1: the bits of wgrad_split_tn on the contiguous concatenation.  A1 is a
    column slice of a wider matrix, A2 has a row stride of its own"""
    cnt = cases.sb_wgrad_counts(K)
    assert cnt.tail and 4 <= M1 <= M - 4 and M1 % 4 == 0
    tag = f"split {M}x{N} M1 {M1} K {K} chunks {sorted(cnt.counts)} tail {cnt.tail}"
    t0 = time.perf_counter()
    ma, mb = _master("split", M, N, _max_rows("split", M, N))
    a1, a2 = _wide(K, M1, 8, M1 + 16, ma[:, :M1]), _wide(K, M - M1, 4, M - M1 + 28, ma[:, M1:])
    b = _wide(K, N, 8, N + 12, mb)
    assert a1.stride(0) != a2.stride(0)
    c = _twice("split", a1, b, a2=a2)
    whole = torch.full((K + GUARD, M), float("nan"), device="cuda")[:K]                          # contiguous rows, guard rows behind them
    whole.copy_(ma[:K])
    assert whole.is_contiguous()
    assert torch.equal(_i32(c), _i32(_launch("split", whole, b))), (tag, "differs from wgrad_split_tn on the concatenation")
    _check(tag, "split tn2", c, whole, b)
    if K == cases.TN2_ROWS[-1]:
        c0 = torch.randn(M, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(M1)) * float(K) ** 0.5
        ca = _twice("split", a1, b, c0, a2=a2)
        assert torch.equal(_i32(ca), _i32(_launch("split", whole, b, c0))), (tag, "accumulate differs from wgrad_split_tn's")
        _check(tag + " accumulate", "split tn2", ca, whole, b, c0)
    SLOW[tag] = time.perf_counter() - t0


# ---- k_wgrad / k_wgrad_reduce -------------------------------------------------------------------------------------------------------------
def _key_id(key):
    return str(key) if isinstance(key, int) else "-".join(str(k) for k in key)


@pytest.mark.parametrize("M,N,key", cases.wg_cases(), ids=[f"{M}x{N}-{_key_id(k)}" for M, N, k in cases.wg_cases()])
def test_fp32_wgrad_at_a_step_edge(M, N, key):
    S, am, bn, gy, gz = cases.wgrad_split(M, N)
    assert S == cases.WG_S[(M, N)]
    K = cases.wg_rows_of(key, S)
    cnt = cases.wgrad_counts(K, S)
    assert (cnt.counts, cnt.tail) == cases.wg_expected(key, S), cnt
    tag = (f"fp32 <{am},{bn}> {M}x{N} grid ({S},{gy},{gz}) K {K} steps {sorted(cnt.counts)} pairs {sorted(cnt.pairs)} "
           f"leftover {sorted(cnt.leftover)} tail {cnt.tail}")
    t0 = time.perf_counter()
    a, b = _operands("fp32", M, N, K)
    _check(tag, "fp32", _twice("fp32", a, b), a, b)
    SLOW[tag] = time.perf_counter() - t0


@pytest.mark.parametrize("M,N", cases.WG_SHAPES)
@pytest.mark.parametrize("key", cases.wg_acc_keys(), ids=_key_id)
def test_fp32_wgrad_accumulates_onto_c(M, N, key):
    K = cases.wg_rows_of(key, cases.WG_S[(M, N)])
    tag = f"fp32 {M}x{N} K {K} accumulate"
    t0 = time.perf_counter()
    a, b = _operands("fp32", M, N, K)
    c0 = torch.randn(M, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(K + M)) * float(K) ** 0.5
    _check(tag, "fp32", _twice("fp32", a, b, c0), a, b, c0)
    SLOW[tag] = time.perf_counter() - t0


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    """every refusal leaves C and the workspace as they were"""
    ops, L = _lib()
    p, st = ops._ptr, ops._stream()
    K = 64
    wa = torch.randn(K, 1160, device="cuda")
    wb = torch.randn(K, 392, device="cuda")
    a, b = wa[:, :384], wb[:, :128]
    c = torch.full((1152 * 128,), CANARY, device="cuda")
    ws = torch.full((L.wgrad_tn_workspace(384, 128),), 0x5A, dtype=torch.uint8, device="cuda")
    assert L.wgrad_split_workspace(384, 128) <= ws.numel() and L.wgrad_split_workspace(256, 256) == -1
    assert L.wgrad_split_workspace(384, 256) == -1 and L.wgrad_split_workspace(512, 128) == -1 and L.wgrad_tn_workspace(100, 128) == -1
    lda, ldb = a.stride(0), b.stride(0)

    def tn(fn, K=K, M=384, N=128, a=a, lda=lda, b=b, ldb=ldb):
        return fn(K, M, N, p(a), lda, p(b), ldb, p(c), 0, p(ws), st)

    def tn2(K=K, M1=256, M2=128, N=128, a1=a, lda1=lda, a2=wa[:, 256:384], lda2=lda, b=b, ldb=ldb):
        return L.wgrad_split_tn2(K, M1, M2, N, p(a1), lda1, p(a2), lda2, p(b), ldb, p(c), 0, p(ws), st)

    for fn in (L.wgrad_split_tn, L.wgrad_tn):
        assert tn(fn, K=0) == BAD_ARG and tn(fn, K=-4) == BAD_ARG
        assert tn(fn, lda=380) == BAD_ARG and tn(fn, ldb=124) == BAD_ARG                       # lda < M, ldb < N
        assert tn(fn, lda=lda + 2) == BAD_ARG and tn(fn, ldb=ldb + 1) == BAD_ARG               # strides that are no multiple of 4
        assert tn(fn, a=wa[:, 1:385]) == BAD_ARG and tn(fn, b=wb[:, 2:130]) == BAD_ARG         # misaligned pointers
        assert tn(fn, M=100) == BAD_ARG and tn(fn, N=0) == BAD_ARG
    for M, N in ((256, 256), (384, 256), (384, 384), (512, 128), (128, 512)):                  # outside sb_wgrad_shape_ok
        assert not cases.sb_wgrad_shape_ok(M, N) and tn(L.wgrad_split_tn, M=M, N=N, lda=1160, ldb=1160) == BAD_ARG
    assert tn(L.wgrad_tn, M=1152, lda=1160) == BAD_ARG and tn(L.wgrad_tn, N=1152, ldb=1160) == BAD_ARG
    assert tn2(K=0) == BAD_ARG
    assert tn2(M1=0, M2=384) == BAD_ARG and tn2(M1=384, M2=0) == BAD_ARG
    assert tn2(M1=254, M2=130) == BAD_ARG and tn2(M1=2, M2=382) == BAD_ARG                    # M1 % 4 != 0
    assert tn2(M1=256, M2=256) == BAD_ARG and tn2(M1=128, M2=128, N=256) == BAD_ARG            # M1 + M2, N outside sb_wgrad_shape_ok
    assert tn2(lda1=252) == BAD_ARG and tn2(lda2=124) == BAD_ARG and tn2(ldb=124) == BAD_ARG
    assert tn2(lda1=lda + 2) == BAD_ARG and tn2(lda2=lda + 2) == BAD_ARG and tn2(ldb=ldb + 2) == BAD_ARG
    assert tn2(a1=wa[:, 1:257]) == BAD_ARG and tn2(a2=wa[:, 257:385]) == BAD_ARG and tn2(b=wb[:, 3:131]) == BAD_ARG
    torch.cuda.synchronize()
    bits = int(torch.tensor([CANARY]).view(torch.int32))
    assert bool((_i32(c) == bits).all()) and bool((ws == 0x5A).all()), "a refused call wrote something"
    assert tn2() == 0 and tn(L.wgrad_split_tn) == 0 and tn(L.wgrad_tn) == 0                   # and the same calls with good arguments run
    torch.cuda.synchronize()


# ---- ops.wgrad on both sides of its two switches -----------------------------------------------------------------------------------------
def test_ops_wgrad_outside_the_split_shapes_and_below_its_row_threshold(monkeypatch):
    """split_bf16 mode: (256, 256) is outside SPLIT_WGRAD_SHAPES and takes k_wgrad -- wgrad_tn's bits; 4 095 rows are below
    WGRAD_MIN_ROWS and go to the BLAS library -- a.T @ b's bits"""
    ops, L = _lib()
    monkeypatch.setattr(ops, "WGRAD_MODE", "split_bf16")
    assert (256, 256) not in ops.SPLIT_WGRAD_SHAPES and ops.WGRAD_MIN_ROWS == 4096
    g = torch.Generator(device="cuda").manual_seed(4099)
    a, b = torch.randn(4099, 256, device="cuda", generator=g), torch.randn(4099, 256, device="cuda", generator=g)
    got = ops.wgrad(a, b)
    assert torch.equal(_i32(got), _i32(_launch("fp32", a, b)))
    _check("ops.wgrad 256x256 K 4099", "fp32", got, a, b)
    lo = ops.wgrad(a[:4095], b[:4095])
    assert torch.equal(_i32(lo), _i32(a[:4095].t() @ b[:4095]))
