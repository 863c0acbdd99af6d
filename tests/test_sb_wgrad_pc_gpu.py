"""k_sb_wgrad (csrc/sb_wgrad.hpp) at the row counts of the update: loader waves feeding MFMA waves.

wgrad_split_tn / wgrad_split_tn2 against an f64 product, held to the bound tests/test_split_bf16_gpu.py holds the split kernels to
(at most twice the fp32 library's error plus one fp32 ulp, in units of each dot product's own scale), and run twice for identical bits.
Covers every loader layout (M + N = 256: one unit per loader lane; 512: two; 384: two, the second switched off in two of the four
loader waves), the A2 column-block form of dW_hh, a K % 16 tail, row strides wider than the operands and accumulate=1.  The chunk
counts between these row counts and the few-row ones are in tests/test_wgrad_edges_gpu.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


def _norm_err(y, ref, scale):
    return float(((y.double() - ref).abs() / scale.clamp_min(1e-300)).max())


def _lib():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops, ops.load_library()


def _operands(rows, cols, gen, ld=None):
    """a (rows, cols) view with row stride ld (>= cols, a multiple of 4: the kernel's 16-byte loads)"""
    ld = ld or cols
    base = torch.randn(rows, ld, device="cuda", generator=gen)
    return base[:, :cols]


def _tn(a, b, out, accumulate):
    ops, L = _lib()
    M, N = a.shape[1], b.shape[1]
    ws = torch.empty(L.wgrad_split_workspace(M, N), dtype=torch.uint8, device="cuda")
    rc = L.wgrad_split_tn(a.shape[0], M, N, ops._ptr(a), a.stride(0), ops._ptr(b), b.stride(0), ops._ptr(out), int(accumulate), ops._ptr(ws),
                          ops._stream())
    assert rc == 0, rc
    return out


def _tn2(a1, a2, b, out, accumulate):
    ops, L = _lib()
    M1, M2, N = a1.shape[1], a2.shape[1], b.shape[1]
    ws = torch.empty(L.wgrad_split_workspace(M1 + M2, N), dtype=torch.uint8, device="cuda")
    rc = L.wgrad_split_tn2(a1.shape[0], M1, M2, N, ops._ptr(a1), a1.stride(0), ops._ptr(a2), a2.stride(0), ops._ptr(b), b.stride(0), ops._ptr(out),
                           int(accumulate), ops._ptr(ws), ops._stream())
    assert rc == 0, rc
    return out


def _check(c, a, b, c0=None):
    """c = (c0 +) a^T b within 2 x the fp32 library's error + 1 ulp of the f64 product"""
    ref = a.double().t() @ b.double()
    scale = a.double().abs().t() @ b.double().abs()
    lib = a.t() @ b
    if c0 is not None:
        ref = ref + c0.double()
        scale = scale + c0.double().abs()
        lib = lib + c0
    e, e_lib = _norm_err(c, ref, scale), _norm_err(lib, ref, scale)
    assert torch.isfinite(c).all()
    assert e <= 2.0 * e_lib + ULP, (e, e_lib)


@pytest.mark.parametrize("M,N,rows", [(128, 128, 492_000), (128, 384, 492_000), (384, 128, 492_000), (128, 128, 1_476_000)])
def test_sb_wgrad_update_shapes(M, N, rows):
    gen = torch.Generator(device="cuda").manual_seed(M + 7 * N + rows)
    a, b = _operands(rows, M, gen), _operands(rows, N, gen)
    c1 = _tn(a, b, torch.empty(M, N, device="cuda"), False)
    c2 = _tn(a, b, torch.empty(M, N, device="cuda"), False)
    torch.cuda.synchronize()
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32))
    _check(c1, a, b)


def test_sb_wgrad_two_column_blocks():
    """dW_hh's form: columns 0 .. 255 of A from one tensor, 256 .. 383 from another (wgrad_split_tn2, M1 = 256)"""
    rows = 492_000
    gen = torch.Generator(device="cuda").manual_seed(11)
    a1, a2, b = _operands(rows, 256, gen, ld=384), _operands(rows, 128, gen), _operands(rows, 128, gen)
    c1 = _tn2(a1, a2, b, torch.empty(384, 128, device="cuda"), False)
    c2 = _tn2(a1, a2, b, torch.empty(384, 128, device="cuda"), False)
    torch.cuda.synchronize()
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32))
    _check(c1, torch.cat([a1, a2], dim=1), b)
    # the same product from one contiguous A: the same bits (the column blocks only change where the loader reads)
    c3 = _tn(torch.cat([a1, a2], dim=1).contiguous(), b, torch.empty(384, 128, device="cuda"), False)
    assert torch.equal(c1.view(torch.int32), c3.view(torch.int32))


@pytest.mark.parametrize("M,N", [(128, 128), (128, 256), (256, 128), (128, 384), (384, 128)])
def test_sb_wgrad_tail_strides_accumulate(M, N):
    """K % 16 != 0 (the last workgroup's tail), row strides wider than the operands, accumulate=1 onto a non-zero C"""
    rows = 492_000 + 13
    gen = torch.Generator(device="cuda").manual_seed(3 * M + N)
    a, b = _operands(rows, M, gen, ld=M + 4), _operands(rows, N, gen, ld=N + 12)
    c0 = torch.randn(M, N, device="cuda", generator=gen)
    c = _tn(a, b, c0.clone(), True)
    torch.cuda.synchronize()
    _check(c, a, b, c0)


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 4095, 4096 + 16 * 3 + 5])
def test_sb_wgrad_few_rows(rows):
    """fewer chunks than workgroups: empty row ranges, a tail alone, one chunk"""
    gen = torch.Generator(device="cuda").manual_seed(rows)
    a, b = _operands(rows, 384, gen), _operands(rows, 128, gen)
    c = _tn(a, b, torch.empty(384, 128, device="cuda"), False)
    torch.cuda.synchronize()
    _check(c, a, b)
