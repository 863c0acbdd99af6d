"""The launch arithmetic of the two weight-gradient kernel families restated in plain Python: k_sb_wgrad<MT, NT> (csrc/sb_wgrad.hpp,
launch_sb_wgrad; behind wgrad_split_tn / wgrad_split_tn2) and k_wgrad<AM, BN> with k_wgrad_reduce (csrc/mappo_ops.hip, wgrad_split;
behind wgrad_tn), and the row counts that sit on the edges of that arithmetic.  Both grids depend on the shape only (the split
kernel's is the constant 256), so a row count reaches the same class on every device.  Shared by
tests/test_wgrad_edges_cases_cpu.py, which checks that the row counts reach every class they are chosen for, and by
tests/test_wgrad_edges_gpu.py, which asserts at the top of every case which class the case is in."""
from collections import namedtuple

# ---- k_sb_wgrad ---------------------------------------------------------------------------------------------------------------------------
SB_WGS = 256              # SB_WGRAD_WGS: the grid, whatever the device
SB_CR = 16                # SbWgCfg::CR: rows per chunk
SB_LOAD_WAVES = 4         # SB_WG_LOAD_WAVES
SB_SHAPES = [(128, 128), (128, 256), (256, 128), (128, 384), (384, 128)]       # (M, N) of the five instantiations

SbCounts = namedtuple("SbCounts", "chunks counts last tail")
SbLayout = namedtuple("SbLayout", "UL DEPTH off_waves")


def sb_wgrad_shape_ok(M, N):
    return M in (128, 256, 384) and N in (128, 256, 384) and M + N <= 512 and M * N < 256 * 256


def sb_wgrad_counts(K):
    """workgroup b owns the chunks chunks b / 256 .. chunks (b + 1) / 256 - 1 of the K / 16 full ones; the K % 16 rows behind them are
    the last workgroup's tail -> (chunks, the set of chunk counts, the last workgroup's count, K % 16)"""
    assert K >= 1
    chunks = K // SB_CR
    counts = [chunks * (b + 1) // SB_WGS - chunks * b // SB_WGS for b in range(SB_WGS)]
    assert sum(counts) == chunks
    return SbCounts(chunks, set(counts), counts[-1], K % SB_CR)


def sb_wgrad_layout(M, N):
    """SbWgCfg<M / 128, N / 128>: load units per loader lane and chunk, chunks in flight per loader lane, and how many of the four
    loader waves have their second unit switched off (on[1] false)"""
    assert sb_wgrad_shape_ok(M, N)
    units = 2 * 2 * ((M + N) // 4)
    lt = 64 * SB_LOAD_WAVES
    UL = -(-units // lt)
    off = sum(1 for u in range(UL) for lw in range(SB_LOAD_WAVES) if not ((u + 1) * lt <= units or 64 * lw + lt * u < units))
    return SbLayout(UL, 4 if UL == 1 else 3, off)


def sb_classes(K, depth):
    """what a launch of K rows decides of the loader's ring of `depth` chunks: the classes of its workgroups' chunk counts, and the
    image the tail overwrites after the last workgroup's count (parity) -- as a set of names"""
    c = sb_wgrad_counts(K)
    out = set()
    for n in c.counts:
        out.add("none" if n == 0 else "below depth" if n < depth else "depth" if n == depth else "second trip" if n <= 2 * depth
                else "third trip")
    if c.tail:
        out.add(f"tail after {'an even' if c.last % 2 == 0 else 'an odd'} count")
    return out


SB_SMALL = [1, 15, 16, 17, 4095, 4096, 4097]


def sb_uniform_rows(n, tail):
    """every workgroup owns exactly n chunks; with `tail`, 13 rows follow an odd n and 5 an even one"""
    return 4096 * n + ((13 if n % 2 else 5) if tail else 0)


SB_UNIFORM = [sb_uniform_rows(n, tail) for n in range(1, 10) for tail in (False, True)]
SB_MIXED = {4080: {0, 1}, 8211: {2, 3}, 14352: {3, 4}, 20479: {4, 5}, 20496: {5, 6}, 34839: {8, 9}}
SB_ROWS = SB_SMALL + [K for K in SB_UNIFORM if K not in SB_SMALL] + list(SB_MIXED)      # 4096 is in both lists
SB_ACC_ROWS = [4096 * 4 + 5, 20479, 4096 * 9 + 13]     # accumulate = 1 onto a non-zero C
SB_ZERO_TAIL_N = (4, 9)                                 # 4096 n rows against the same rows with 13 zero rows appended: n even, n odd

# wgrad_split_tn2: (M, N) -> the M1 at which A's columns change tensors
TN2_SPLITS = {(384, 128): [4, 128, 252, 256, 380], (128, 128): [4, 64, 124], (128, 256): [4, 64, 124], (128, 384): [4, 64, 124],
              (256, 128): [128, 252]}
TN2_ROWS = [17, 12301, 16389, 20479, 36877]


def sb_expected(K):
    """(the set of chunk counts, K % 16) the row count K of SB_ROWS is chosen for"""
    if K in SB_MIXED:
        return SB_MIXED[K], K % 16
    if K >= 4096:
        n = K // 4096
        assert K in (4097, sb_uniform_rows(n, False), sb_uniform_rows(n, True))
        return {n}, K - 4096 * n
    return {1: {0}, 15: {0}, 16: {0, 1}, 17: {0, 1}, 4095: {0, 1}}[K], K % 16


def sb_cases():
    return [(M, N, K) for (M, N) in SB_SHAPES for K in SB_ROWS]


def tn2_cases():
    return [(M, N, M1, K) for (M, N), m1s in TN2_SPLITS.items() for M1 in m1s for K in TN2_ROWS]


# ---- k_wgrad / k_wgrad_reduce -------------------------------------------------------------------------------------------------------------
WG_U = 4                  # k-steps per pipeline stage; a pair of stages is 2 U = 8 steps
WgCounts = namedtuple("WgCounts", "steps counts pairs leftover last tail")


def wgrad_split(M, N):
    """wgrad_split + wgrad_tn's grid -> (S, am, bn, grid_y, grid_z): k_wgrad<am, bn> on dim3(S, grid_y, grid_z)"""
    assert M >= 128 and N >= 128 and M % 128 == 0 and N % 128 == 0 and M <= 1024 and N <= 1024
    am = 3 if (M, N) == (384, 128) else 1
    bn = 3 if (M, N) == (128, 384) else 1
    gy, gz = M // (128 * am), N // (128 * bn)
    return max(1, 256 // (gy * gz)), am, bn, gy, gz


def wgrad_counts(K, S):
    """workgroup x of S owns the 4-row steps steps x / S .. steps (x + 1) / S - 1 of the K / 4 full ones: n_s / 8 pairs of U-step
    stages, then n_s % 8 single steps; the K % 4 rows behind them are the last workgroup's tail"""
    assert K >= 1 and S >= 1
    steps = K // 4
    counts = [steps * (x + 1) // S - steps * x // S for x in range(S)]
    assert sum(counts) == steps
    return WgCounts(steps, set(counts), {n // (2 * WG_U) for n in counts}, {n % (2 * WG_U) for n in counts}, counts[-1], K % 4)


WG_SMALL = [1, 3, 4, 5]
WG_EVEN = [(1, 0), (7, 1), (8, 0), (8, 2), (9, 3), (15, 0), (16, 1), (17, 2), (24, 3)]            # (n, t): 4 S n + t rows
WG_UNEVEN = [(0, "S-1", 0), (7, 1, 2), (8, "S-1", 0), (15, "S/2+1", 1), (16, 1, 3)]            # (n, k, t): 4 (S n + k) + t rows
WG_SHAPES = [(128, 128), (384, 128), (128, 384), (256, 128), (128, 256), (256, 256), (384, 256), (640, 128), (640, 256), (384, 384),
             (1024, 1024)]
WG_S = {(128, 128): 256, (384, 128): 256, (128, 384): 256, (256, 128): 128, (128, 256): 128, (256, 256): 64, (384, 256): 42,
        (640, 128): 51, (640, 256): 25, (384, 384): 28, (1024, 1024): 4}
WG_INSTANTIATIONS = {(1, 1), (3, 1), (1, 3)}


def _k_of(k, S):
    return {"S-1": S - 1, "S/2+1": S // 2 + 1}.get(k, k)


def wg_row_keys():
    """the row counts of the fp32 route as keys that do not depend on S"""
    return WG_SMALL + [("even", n, t) for n, t in WG_EVEN] + [("uneven", n, k, t) for n, k, t in WG_UNEVEN]


def wg_rows_of(key, S):
    if isinstance(key, int):
        return key
    if key[0] == "even":
        return 4 * S * key[1] + key[2]
    return 4 * (S * key[1] + _k_of(key[2], S)) + key[3]


def wg_expected(key, S):
    """the set of steps per workgroup and K % 4 the key is chosen for"""
    if isinstance(key, int):
        return ({0, 1} if key >= 4 and S > 1 else {key // 4}), key % 4
    if key[0] == "even":
        return {key[1]}, key[2]
    return {key[1], key[1] + 1}, key[3]


def wg_acc_keys():
    """accumulate = 1 onto a non-zero C: three row counts per shape"""
    return [("even", 8, 2), ("uneven", 15, "S/2+1", 1), ("even", 24, 3)]


def wg_cases():
    return [(M, N, key) for (M, N) in WG_SHAPES for key in wg_row_keys()]
