"""relu_bwd_colsum (csrc/mappo_ops.hip k_relu_bwd_colsum, k_colsum_reduce) and wgrad_skinny (k_wgrad_skinny, k_skinny_reduce) through
their C entry points, which take any row count (ops.relu_bwd_colsum / ops.wgrad_skinny route fewer than 4 096 rows to torch).

k_relu_bwd_colsum: F / 4 float4 columns, cpb = 256 / (F / 4) rows per workgroup step, four steps in flight (`r + 3 * cpb < r1`) and
a remainder loop, at most 2 048 workgroups with a contiguous slice of rows each.  Up to 2 048 cpb rows no slice is longer than cpb
and only the remainder loop runs (1, cpb - 1, cpb, 4 cpb, 4 cpb + 1, 2 048 cpb + 3 rows); the four-in-flight loop needs a full grid
with more than 3 cpb rows per slice, so R = 2 048 x {3 cpb, 3 cpb + 1, 4 cpb, 4 cpb + 1, 7 cpb + 1} puts the slice on both sides of
the hand-over between the loops, and one row count leaves the last workgroup short (`_relu_rows`, checked by `_relu_trips`).
k_wgrad_skinny: min(R, 2 048) workgroups, eight rows in flight and a remainder loop: 1, 7, 8, 9 rows, 2 047 .. 2 049, and
8 * 2 048 + 5 (nine rows per workgroup: one full step and one remainder row).

Bound (tests/test_sb_wgrad_pc_gpu.py `_check`): each sum's error against f64 is at most twice that of the same sum by torch in fp32,
plus one fp32 ulp, in units of that sum's own sum of magnitudes (|S|^T |X| for a product element, sum |.| for a column sum).  gin is a
selection of gout: bit-equal to aten::threshold_backward.  Every case runs twice for identical bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


def _lib():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops, ops.load_library()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(what, got, lib, ref, scale):
    """got, lib fp32; ref, scale f64 (device tensors)"""
    den = scale.clamp_min(1e-300)
    e, e_lib = float(((got.double() - ref).abs() / den).max()), float(((lib.double() - ref).abs() / den).max())
    bound = 2.0 * e_lib + ULP
    print(f"{what}: e_kernel {e:.3e} e_lib {e_lib:.3e} ratio {e / bound:.3f}")
    assert torch.isfinite(got).all()
    assert e <= bound, (what, e, e_lib)


def _block(rows, cols, gen, lead, ld):
    """a (rows, cols) column block of a dense (rows, ld) matrix, starting at column `lead`"""
    assert lead + cols <= ld
    return torch.randn(rows, ld, device="cuda", generator=gen)[:, lead:lead + cols]


# ---- relu_bwd_colsum --------------------------------------------------------------------------------------------------------------------------
def _relu_rows(F):
    """Workgroup b owns the rows b rpb .. (b + 1) rpb - 1, rpb = ceil(R / grid), grid = min(ceil(R / cpb), 2 048); lane row rr of it
    takes the four-in-flight loop while rr + 3 cpb < rpb.
    - up to 2 048 cpb rows every workgroup has at most cpb rows: one trip of the remainder loop (1, cpb - 1, cpb, 4 cpb, 4 cpb + 1:
      one to five workgroups); at 2 048 cpb + 3, rpb = cpb + 1: a second remainder trip for lane row 0;
    - R = 2 048 rpb fills the grid with rpb rows each: rpb = 3 cpb is the last size with the remainder loop alone (three trips),
      3 cpb + 1 sends lane row 0 alone through the four-in-flight loop, 4 cpb every lane row once with nothing left over,
      4 cpb + 1 hands lane row 0 over to the remainder loop for one row, 7 cpb + 1 gives lane row 0 two four-in-flight trips and the
      others one trip and three remainder rows;
    - 2 048 (4 cpb + 1) - (2 cpb + 1): the last workgroup is short (2 cpb rows, remainder loop) beside 2 047 full ones."""
    cpb = 256 // (F // 4)
    small = {1, cpb - 1, cpb, 4 * cpb, 4 * cpb + 1, 2048 * cpb + 3} - {0}
    full = {2048 * rpb for rpb in (3 * cpb, 3 * cpb + 1, 4 * cpb, 4 * cpb + 1, 7 * cpb + 1)}
    return sorted(small | full | {2048 * (4 * cpb + 1) - (2 * cpb + 1)})


def _relu_trips(F, R):
    """the launch arithmetic of relu_bwd_colsum restated: the set of (four-in-flight trips, remainder trips) over all lane rows of all
    workgroups, so that the claims above are checked and not only made"""
    cpb = 256 // (F // 4)
    grid = min(-(-R // cpb), 2048)
    rpb = -(-R // grid)
    seen = set()
    for rows in {min(rpb, R - b * rpb) for b in (0, (R - 1) // rpb)}:               # the first workgroup and the last one that has rows
        for rr in range(cpb):
            r, four, rest = rr, 0, 0
            while r + 3 * cpb < rows:
                r, four = r + 4 * cpb, four + 1
            while r < rows:
                r, rest = r + cpb, rest + 1
            seen.add((four, rest))
    return seen


for _F in (4, 8, 512, 1024, 128):
    _c = 256 // (_F // 4)
    assert all(four == 0 for R in _relu_rows(_F) if R <= 2048 * _c + 3 for four, _ in _relu_trips(_F, R))
    assert _relu_trips(_F, 2048 * 3 * _c) == {(0, 3)}
    assert _relu_trips(_F, 2048 * (3 * _c + 1)) == ({(1, 0), (0, 3)} if _c > 1 else {(1, 0)})
    assert _relu_trips(_F, 2048 * 4 * _c) == {(1, 0)}
    assert _relu_trips(_F, 2048 * (4 * _c + 1)) == ({(1, 1), (1, 0)} if _c > 1 else {(1, 1)})
    assert _relu_trips(_F, 2048 * (7 * _c + 1)) == ({(2, 0), (1, 3)} if _c > 1 else {(2, 0)})
    assert (0, 2) in _relu_trips(_F, 2048 * (4 * _c + 1) - (2 * _c + 1))


def _relu_bwd(gout, y, gin, cs):
    ops, L = _lib()
    F = gout.shape[1]
    ws = torch.empty(L.relu_bwd_colsum_workspace(F), dtype=torch.uint8, device="cuda")
    return L.relu_bwd_colsum(gout.shape[0], F, ops._ptr(gout), gout.stride(0), ops._ptr(y), y.stride(0), ops._ptr(gin), ops._ptr(cs), ops._ptr(ws),
                             ops._stream())


@pytest.mark.parametrize("F,R", [(F, R) for F in (4, 8, 512, 1024, 128) for R in _relu_rows(F)])
def test_relu_backward_with_column_sums(F, R):
    gen = torch.Generator(device="cuda").manual_seed(F * 7 + R)
    gout = _block(R, F, gen, 4, F + 8)                     # row strides above F; both blocks start on 16 bytes
    y = _block(R, F, gen, 0, F + 4).relu_()                # a saved ReLU output: exact +0 for half the elements ...
    y[torch.rand(R, F, device="cuda", generator=gen) < 0.1] = -0.0                                         # ... and -0 for some
    assert y.stride(0) == F + 4 and gout.stride(0) == F + 8
    if R * F >= 256:
        assert bool(((y == 0) & ~torch.signbit(y)).any()) and bool(torch.signbit(y).any())
    outs = []
    for _ in range(2):
        gin = torch.full((R, F), float("nan"), device="cuda")
        cs = torch.full((F,), float("nan"), device="cuda")
        assert _relu_bwd(gout, y, gin, cs) == 0
        torch.cuda.synchronize()
        outs.append((gin, cs))
    (gin, cs), (gin2, cs2) = outs
    assert torch.equal(_bits(gin), _bits(gin2)) and torch.equal(_bits(cs), _bits(cs2))
    want = torch.ops.aten.threshold_backward(gout, y, 0.0)
    assert torch.equal(_bits(gin), _bits(want))
    want64 = want.double()
    _check(f"F {F} R {R} colsum", cs, want.sum(0), want64.sum(0), want64.abs().sum(0))


def test_relu_backward_refuses_what_it_cannot_tile():
    """F = 36 (9 float4 columns do not divide 256 lanes), F = 2 and a pointer off the 16-byte boundary: an error code, nothing written"""
    ops, L = _lib()
    gen = torch.Generator(device="cuda").manual_seed(1)
    R = 64

    def refused(F, shift=0):
        gout = torch.randn(R * F + 4, device="cuda", generator=gen)[shift:shift + R * F].view(R, F)
        y = torch.randn(R, F, device="cuda", generator=gen)
        gin, cs = torch.full((R, F), 3.0, device="cuda"), torch.full((F,), 3.0, device="cuda")
        rc = _relu_bwd(gout, y, gin, cs)
        torch.cuda.synchronize()
        return rc != 0 and bool((gin == 3.0).all()) and bool((cs == 3.0).all())

    assert refused(36) and refused(2) and refused(128, shift=1)
    assert not refused(128)                                # the same call on the boundary runs


# ---- wgrad_skinny ---------------------------------------------------------------------------------------------------------------------------
SK_NS, SK_F, SK_R = (1, 2, 9, 16), (64, 128, 1024), (1, 7, 8, 9, 2_047, 2_048, 2_049, 8 * 2_048 + 5)
# (R, NS, F, transposed, colsum_x, colsum_s): four (NS, F) pairs per row count, walking the three lists at different rates
SK_CASES = [(R, SK_NS[(i + j) % 4], SK_F[(i + 2 * j) % 3], (i + j) % 2, j % 2, (j // 2 + i) % 2) for i, R in enumerate(SK_R) for j in range(4)]
assert all({c[k] for c in SK_CASES} == set(vals) for k, vals in ((1, SK_NS), (2, SK_F), (3, (0, 1)), (4, (0, 1)), (5, (0, 1))))
assert all(len({c[1:3] for c in SK_CASES if c[0] == R}) >= 2 for R in SK_R)
assert (16, 1024) in {c[1:3] for c in SK_CASES}


@pytest.mark.parametrize("R,NS,F,transposed,colsum_x,colsum_s", SK_CASES)
def test_skinny_weight_gradient(R, NS, F, transposed, colsum_x, colsum_s):
    ops, L = _lib()
    gen = torch.Generator(device="cuda").manual_seed(R * 31 + NS * 7 + F)
    S = _block(R, NS, gen, 1, NS + 3)                      # lds > NS, ldx > F
    X = _block(R, F, gen, 1, F + 2)
    ws = torch.empty(L.wgrad_skinny_workspace(NS, F), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        C = torch.full((F, NS) if transposed else (NS, F), float("nan"), device="cuda")
        cx = torch.full((F,), float("nan"), device="cuda") if colsum_x else None
        cs = torch.full((NS,), float("nan"), device="cuda") if colsum_s else None
        rc = L.wgrad_skinny(R, NS, F, ops._ptr(S), S.stride(0), ops._ptr(X), X.stride(0), transposed, ops._ptr(C), ops._ptr(cx), ops._ptr(cs),
                            ops._ptr(ws), ops._stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.append((C, cx, cs))
    for a, b in zip(*outs):
        assert (a is None and b is None) or torch.equal(_bits(a), _bits(b))
    C, cx, cs = outs[0]
    tag = f"R {R} NS {NS} F {F} t {transposed}"
    S64, X64 = S.double(), X.double()
    _check(tag + " C", C.t() if transposed else C, S.t() @ X, S64.t() @ X64, S64.abs().t() @ X64.abs())
    if colsum_x:
        _check(tag + " colsum_x", cx, X.sum(0), X64.sum(0), X64.abs().sum(0))
    if colsum_s:
        _check(tag + " colsum_s", cs, S.sum(0), S64.sum(0), S64.abs().sum(0))
