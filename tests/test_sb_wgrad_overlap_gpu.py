"""k_sb_wgrad (csrc/sb_wgrad.hpp) at the smallest row counts at which its loader / MFMA pipeline can go wrong.

A workgroup takes 16-row chunks, 256 workgroups share the rows, and a loader lane keeps DEPTH chunks in flight (3 at M + N = 384 and
512, 4 at 256) in a loop unrolled DEPTH times over a double-buffered LDS image.  So the row counts are 16 * 256 * c + r with c chunks
per workgroup around both depths -- 1, 2, DEPTH - 1, DEPTH, DEPTH + 1, 2 DEPTH + 1 -- and r = 0 or 13 (the K % 16 tail of the last
workgroup): at most 36 877 rows.  Every instantiation (128 x 128, 128 x 256, 256 x 128, 128 x 384, 384 x 128) and the two-block form
of dW_hh (wgrad_split_tn2) run every row count.

Each case: operands with row strides wider than their columns; two launches give identical bits, and the bits of the same product from
contiguous operands; the result meets the bound of tests/test_sb_wgrad_pc_gpu.py::_check (at most twice the fp32 library's error plus
one fp32 ulp of each dot product's scale, against the f64 product); a third launch accumulates onto a non-zero C within the same
bound; canary floats behind C and behind the workspace are untouched; a captured-graph replay is bit-equal to the eager launch.
"""
import pytest
import torch

from tests.helpers import no_gc_during_capture

from tests.test_sb_wgrad_pc_gpu import _check, _lib, _operands

pytestmark = pytest.mark.gpu

WGS, CR = 256, 16                                        # SB_WGRAD_WGS, SbWgCfg::CR
CHUNKS = sorted({c for depth in (3, 4) for c in (1, 2, depth - 1, depth, depth + 1, 2 * depth + 1)})   # 1 2 3 4 5 7 9
FORMS = [("tn", 128, 128), ("tn", 128, 256), ("tn", 256, 128), ("tn", 128, 384), ("tn", 384, 128), ("tn2", 384, 128)]
CANARY, PAD = -1234.5, 64


class _Launch:
    """one product with its C and its workspace carved out of canary-filled buffers"""

    def __init__(self, form, a, b):
        self.ops, self.L = _lib()
        self.form, self.a, self.b = form, a, b
        self.M, self.N = a.shape[1], b.shape[1]
        self.a1, self.a2 = (a[:, :256], a[:, 256:]) if form == "tn2" else (None, None)
        self.c_buf = torch.full((self.M * self.N + PAD,), CANARY, device="cuda")
        ws_bytes = self.L.wgrad_split_workspace(self.M, self.N)
        assert ws_bytes > 0 and ws_bytes % 4 == 0
        self.ws_buf = torch.full((ws_bytes // 4 + PAD,), CANARY, device="cuda")
        self.c = self.c_buf[:self.M * self.N].view(self.M, self.N)

    def __call__(self, accumulate=False):
        ops, L, a, b = self.ops, self.L, self.a, self.b
        if self.form == "tn2":
            a1, a2 = self.a1, self.a2
            rc = L.wgrad_split_tn2(a.shape[0], 256, self.M - 256, self.N, ops._ptr(a1), a1.stride(0), ops._ptr(a2), a2.stride(0), ops._ptr(b),
                                   b.stride(0), ops._ptr(self.c), int(accumulate), ops._ptr(self.ws_buf), ops._stream())
        else:
            rc = L.wgrad_split_tn(a.shape[0], self.M, self.N, ops._ptr(a), a.stride(0), ops._ptr(b), b.stride(0), ops._ptr(self.c), int(accumulate),
                                  ops._ptr(self.ws_buf), ops._stream())
        assert rc == 0, rc
        return self.c

    def canaries_intact(self):
        return bool((self.c_buf[self.M * self.N:] == CANARY).all()) and bool((self.ws_buf[-PAD:] == CANARY).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("r", [0, 13])
@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("form,M,N", FORMS)
def test_sb_wgrad_pipeline_edges(form, M, N, chunks, r):
    rows = CR * WGS * chunks + r
    gen = torch.Generator(device="cuda").manual_seed(1000 * M + 10 * N + 100_000 * chunks + r + (7 if form == "tn2" else 0))
    a, b = _operands(rows, M, gen, ld=M + 4), _operands(rows, N, gen, ld=N + 12)
    run = _Launch(form, a, b)
    c1 = run().clone()
    c2 = run().clone()
    torch.cuda.synchronize()
    assert torch.equal(_bits(c1), _bits(c2))
    _check(c1, a, b)
    # the same product from contiguous operands (and, for the two-block form, from one A): the same bits
    dense = _Launch("tn", a.contiguous(), b.contiguous())
    assert torch.equal(_bits(dense()), _bits(c1))
    # accumulate=1 onto a non-zero C
    c0 = torch.randn(M, N, device="cuda", generator=gen)
    run.c.copy_(c0)
    c3 = run(accumulate=True).clone()
    _check(c3, a, b, c0)
    # captured-graph replay against the eager launch (the launch's one-time attribute call has happened above)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with no_gc_during_capture(), torch.cuda.graph(g):
        run()
    run.c.fill_(CANARY)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(run.c), _bits(c1))
    assert run.canaries_intact() and dense.canaries_intact()
