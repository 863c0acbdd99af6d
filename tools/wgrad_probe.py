"""Weight-gradient GEMM (a^T b over ~5e5 rows): split-K MFMA kernel vs the BLAS library.

  python tools/wgrad_probe.py            times, library against ops.wgrad
  python tools/wgrad_probe.py --hashes   SHA-256 of C for a fixed list of (form, M, N, rows, seed, accumulate) cases of the split-bf16
                                         kernel (wgrad_split_tn / wgrad_split_tn2): two builds that add the same numbers in the same
                                         order print the same list (profiles/r20_sb_wgrad_hashes_*.txt)
"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_multi_agent_reinforcement_learning_amd import ops, trainer

# (form, M, N, rows, seed, accumulate): the update's shapes and row counts, a K % 16 tail, few chunks per workgroup, an empty-range grid
HASH_CASES = [
    ("tn", 384, 128, 492_000, 1, 0), ("tn", 128, 384, 492_000, 2, 0), ("tn", 128, 128, 1_476_000, 3, 0), ("tn", 256, 128, 492_000, 4, 0),
    ("tn", 128, 256, 492_000, 5, 0), ("tn2", 384, 128, 492_000, 6, 1), ("tn", 384, 128, 492_013, 7, 1), ("tn", 128, 128, 492_013, 8, 0),
    ("tn", 128, 384, 16 * 256 * 3 + 13, 9, 0), ("tn", 384, 128, 16 * 256 * 4, 10, 1), ("tn", 128, 128, 16 * 256 * 5 + 13, 11, 0),
    ("tn", 256, 128, 16 * 256 * 2, 12, 0), ("tn2", 384, 128, 16 * 256 * 7 + 13, 13, 0), ("tn", 128, 256, 4095, 14, 1), ("tn", 384, 128, 17, 15, 0),
]


def hashes():
    L = ops.load_library()
    for form, M, N, rows, seed, acc in HASH_CASES:
        gen = torch.Generator(device="cuda").manual_seed(seed)
        a = torch.randn(rows, M + 4, device="cuda", generator=gen)[:, :M]      # row strides wider than the operands
        b = torch.randn(rows, N + 12, device="cuda", generator=gen)[:, :N]
        c = torch.randn(M, N, device="cuda", generator=gen)
        ws = torch.empty(L.wgrad_split_workspace(M, N), dtype=torch.uint8, device="cuda")
        if form == "tn2":
            a1, a2 = a[:, :256], a[:, 256:]
            rc = L.wgrad_split_tn2(rows, 256, M - 256, N, ops._ptr(a1), a1.stride(0), ops._ptr(a2), a2.stride(0), ops._ptr(b), b.stride(0), ops._ptr(c), acc,
                                   ops._ptr(ws), ops._stream())
        else:
            rc = L.wgrad_split_tn(rows, M, N, ops._ptr(a), a.stride(0), ops._ptr(b), b.stride(0), ops._ptr(c), acc, ops._ptr(ws), ops._stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        print(f"{form:3s} M={M} N={N} rows={rows} seed={seed} accumulate={acc}: {hashlib.sha256(c.cpu().numpy().tobytes()).hexdigest()}")


def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def times():
    trainer.enable_tuned_gemms()
    for K, M, N in ((492000, 384, 128), (492000, 128, 384), (492000, 128, 128), (1476000, 128, 128), (492000, 256, 128), (492000, 128, 256)):
        a = torch.randn((K, M), device="cuda"); b = torch.randn((K, N), device="cuda")
        t_lib = timeit(lambda: torch.mm(a.t(), b)); t_own = timeit(lambda: ops.wgrad(a, b))
        fl = 2.0 * K * M * N
        print(f"K={K} M={M} N={N}: library {t_lib:8.1f} us ({fl/t_lib/1e6:6.1f} TFLOP/s)   wgrad {t_own:8.1f} us ({fl/t_own/1e6:6.1f} TFLOP/s, {(M+N)*K*4/t_own/1e6:5.2f} TB/s)")


if __name__ == "__main__":
    hashes() if "--hashes" in sys.argv[1:] else times()
