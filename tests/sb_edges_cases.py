"""The launch arithmetic of the split-bf16 GEMM family (csrc/sb_gemm.hpp k_sb_gemm_n128, launch_sb_gemm, launch_sb_gemm_best;
csrc/mappo_split.hip sb_gemm_masked / sb_gemm_masked_bits) and of the two fused rollout cells (csrc/mappo_ops.hip k_gru_cell,
k_gru_cell_sb and their entry points) restated in plain Python, the row counts that sit on the edges of that arithmetic, and the
sign-bit packing of sb_gemm_signs.  Shared by tests/test_sb_edges_cases_cpu.py, which checks that the row counts reach every class
they are chosen for, and by tests/test_sb_gemm_edges_gpu.py / tests/test_gru_cell_edges_gpu.py, which assert at the top of every case
that the device at hand puts the case into its class."""
from collections import namedtuple

import torch

TILE_ROWS = 32            # rows per iteration of k_sb_gemm_n128
CELL_ROWS = 16            # GRU_RB: rows per tile of both cells
WPC2_MIN_ROWS = 131072    # launch_sb_gemm: two workgroups per CU from here up (KC * NT == 4 only)
PHASE_MIN_ROWS = 786432   # launch_sb_gemm_best<4, 1>: the phase-shifted OPT 2 / 10 from here up

Launch = namedtuple("Launch", "n_it wpc grid trips prologue_fetch two_ahead_fetch last_rows grid_mod4 second_trip_wgs")


def _persistent(n_it, grid):
    """workgroup b of `grid` takes tiles b, b + grid, ..: the set of trip counts, the outcomes of the prologue's second fetch
    (b + grid < n_it), the outcomes of the loop's two-ahead fetch (it + 2 grid < n_it over every tile it), and how many workgroups
    take more than one trip"""
    trips, prologue, ahead, second = set(), set(), set(), 0
    for b in range(grid):
        its = range(b, n_it, grid)
        trips.add(len(its))
        prologue.add(b + grid < n_it)
        second += len(its) > 1
        for it in its:
            ahead.add(it + 2 * grid < n_it)
    return trips, prologue, ahead, second


def sb_gemm_launch(R, KC, NT, cus, masked):
    """launch_sb_gemm<KC, NT, .> for R rows on a device with `cus` compute units"""
    assert R >= 1
    n_it = -(-R // TILE_ROWS)
    wpc = 2 if KC * NT == 4 and R >= WPC2_MIN_ROWS and not masked else 1
    grid = min(n_it, cus * wpc)
    trips, prologue, ahead, second = _persistent(n_it, grid)
    return Launch(n_it, wpc, grid, trips, prologue, ahead, R - (n_it - 1) * TILE_ROWS, grid % 4, second)


MASK_OPT = {(4, 2): 6, (4, 3): 4, (12, 1): 6}     # SBG_MASK_OPT_256, _384, _K384


def sb_gemm_variant(N, K, addend, signs, R, masked=None):
    """(KC, NT, OPT) of the k_sb_gemm_n128 instantiation behind sb_gemm / sb_gemm_signs (launch_sb_gemm_best) or, with
    masked = "float" / "bits", behind sb_gemm_masked / sb_gemm_masked_bits"""
    KC, NT = K // 32, N // 128
    assert (KC, NT) in ((4, 1), (8, 1), (12, 1), (4, 2), (4, 3)) and K % 32 == 0 and N % 128 == 0
    if masked:
        assert masked in ("float", "bits") and not addend and not signs and (KC, NT) in MASK_OPT
        return KC, NT, MASK_OPT[(KC, NT)] | (16 if masked == "bits" else 0)
    plain = 0 if (KC, NT) == (4, 1) else 2
    add = 2 if KC == 12 else (3 if KC == 8 else (0 if NT == 3 else 1))
    phase = (KC, NT) == (4, 1) and R >= PHASE_MIN_ROWS
    if signs:
        assert NT == 1 and KC <= 8
        return KC, NT, (add | 8) if addend else (10 if phase else plain | 8)
    if addend:
        return KC, NT, add
    return KC, NT, 2 if phase else plain


ALL_VARIANTS = {(4, 1, 0), (4, 1, 1), (4, 1, 2), (4, 1, 8), (4, 1, 9), (4, 1, 10), (8, 1, 2), (8, 1, 3), (8, 1, 10), (8, 1, 11), (12, 1, 2),
                (4, 2, 2), (4, 2, 1), (4, 3, 2), (4, 3, 0), (4, 2, 6), (4, 3, 4), (12, 1, 6), (4, 2, 22), (4, 3, 20), (12, 1, 22)}
assert len(ALL_VARIANTS) == 21

# ---- the row counts ---------------------------------------------------------------------------------------------------------------------
SMALL = [1, 15, 16, 17, 31, 32, 33, 95, 4127]          # grids of 1, 1, 1, 1, 1, 1, 2, 3 and 129 workgroups (cus >= 129)
EDGE_KEYS = ["32c-1", "32c+1", "64c+17", "96c+45"]
THRESHOLDS = [131071, 131072, 131073, 786431, 786432, 786433]
ANCHOR_ROWS = 4127                                      # the plain launch every other launch's rows are compared with


def rows_of(key, c):
    """a row count of a case: an int, or one of EDGE_KEYS evaluated at c compute units"""
    if isinstance(key, int):
        return key
    return {"32c-1": 32 * c - 1, "32c+1": 32 * c + 1, "64c+17": 64 * c + 17, "96c+45": 96 * c + 45}[key]


def EDGE(c):
    return [rows_of(k, c) for k in EDGE_KEYS]


# (N, K) -> the forms the GPU test runs; "plain" / "addend" = sb_gemm, "signs" / "addend_signs" = sb_gemm_signs, "masked" / "masked_bits"
SHAPES = [(128, 128), (128, 256), (128, 384), (256, 128), (384, 128)]
FORMS = {(128, 128): ("plain", "addend", "signs", "addend_signs"), (128, 256): ("plain", "addend", "signs", "addend_signs"),
         (128, 384): ("plain", "addend", "masked", "masked_bits"), (256, 128): ("plain", "addend", "masked", "masked_bits"),
         (384, 128): ("plain", "addend", "masked", "masked_bits")}
THRESHOLD_FORMS = ("plain", "signs", "addend")          # of (128, 128)


def form_variant(N, K, form, R):
    return sb_gemm_variant(N, K, form in ("addend", "addend_signs"), form in ("signs", "addend_signs"), R,
                           {"masked": "float", "masked_bits": "bits"}.get(form))


def gemm_cases():
    """(N, K, form, row key) of every case of tests/test_sb_gemm_edges_gpu.py"""
    out = [(N, K, form, key) for (N, K) in SHAPES for form in FORMS[(N, K)] for key in SMALL + EDGE_KEYS]
    return out + [(128, 128, form, R) for form in THRESHOLD_FORMS for R in THRESHOLDS]


def mask_cols_of(N):
    return list(range(0, N + 1, 128))


# ---- the cells --------------------------------------------------------------------------------------------------------------------------
CellLaunch = namedtuple("CellLaunch", "nblk slots trips prologue_fetch two_ahead_fetch last_rows second_trip_slots")
CELL_NETS = [1, 2, 3, 4]                                # MO_GRU_CELL_MAX_NETS = 4
CELL_SMALL = [1, 15, 16, 17]
CELL_EDGE_KEYS = ["16S-1", "16S+1", "32S+1", "48S+21"]


def cell_slots(n_nets, cus, split):
    """persistent workgroups (fp32 cell) or workgroup pairs (split cell) per cell before the clamp to the number of tiles"""
    return max(1, cus // n_nets // 2) if split else max(1, cus // n_nets)


def cell_rows_of(key, n_nets, cus, split):
    if isinstance(key, int):
        return key
    S = cell_slots(n_nets, cus, split)
    return {"16S-1": 16 * S - 1, "16S+1": 16 * S + 1, "32S+1": 32 * S + 1, "48S+21": 48 * S + 21}[key]


def cell_launch(B, n_nets, cus, split):
    """gru_cell_split_fwd_multi (split) / gru_cell_fwd_multi: slot s takes tiles s, s + slots, ..  The split cell fetches a second
    tile in its prologue and two tiles ahead in its loop; the fp32 cell fetches one tile ahead in its loop only (blk + slots < nblk:
    reported as prologue_fetch, its two_ahead_fetch is empty)."""
    assert B >= 1
    nblk = -(-B // CELL_ROWS)
    slots = min(cell_slots(n_nets, cus, split), nblk)
    trips, prologue, ahead, second = _persistent(nblk, slots)
    if not split:
        prologue, ahead = {blk + slots < nblk for blk in range(nblk)}, set()
    return CellLaunch(nblk, slots, trips, prologue, ahead, B - (nblk - 1) * CELL_ROWS, second)


def cell_cases():
    """(split, n_nets, row key) of every case of tests/test_gru_cell_edges_gpu.py"""
    return [(split, n, key) for split in (True, False) for n in CELL_NETS for key in CELL_SMALL + CELL_EDGE_KEYS]


# ---- sign bits ----------------------------------------------------------------------------------------------------------------------------
def pack_signs(y):
    """(rows, N) -> (rows, N / 8) uint8: bit k of byte j of a row = (y[row][8 j + k] > 0)"""
    R, N = y.shape
    assert N % 8 == 0
    w = 1 << torch.arange(8, device=y.device, dtype=torch.int32)
    return ((y > 0).reshape(R, N // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def unpack_signs(b):
    """(rows, N / 8) uint8 -> (rows, N) bool"""
    R, nb = b.shape
    sh = torch.arange(8, device=b.device, dtype=torch.int32)
    return ((b.to(torch.int32).unsqueeze(-1) >> sh) & 1).bool().reshape(R, nb * 8)
