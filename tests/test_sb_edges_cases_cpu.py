"""tests/sb_edges_cases.py claims that its row counts put the split-bf16 GEMM family and the two fused cells on every edge of their
launch arithmetic.  Here the claims are checked, without a GPU, for devices of 64, 256 and 304 compute units; the GPU tests assert the
same per case for the device they run on.  The sign-bit packing is held to a per-element loop."""
import pytest
import torch

from tests import sb_edges_cases as cases

CUS = [64, 256, 304]


def _kcnt(N, K):
    return K // 32, N // 128


@pytest.mark.parametrize("c", CUS)
def test_edge_rows_are_what_they_are_named_for(c):
    """32c - 1: a full grid, one trip; 32c + 1: exactly one workgroup takes a second trip, over a 1-row tile, and the prologue's second
    fetch is true for it alone; 64c + 17: the two-ahead fetch is true for the first time; 96c + 45: 3 and 4 trips, 13-row tail"""
    for KC, NT, masked in ((4, 1, False), (8, 1, False), (12, 1, True), (4, 2, True), (4, 3, False)):
        a, b, d, e = (cases.sb_gemm_launch(R, KC, NT, c, masked) for R in cases.EDGE(c))
        assert (a.grid, a.trips, a.prologue_fetch, a.two_ahead_fetch, a.last_rows) == (c, {1}, {False}, {False}, 31)
        assert (b.grid, b.trips, b.prologue_fetch, b.two_ahead_fetch, b.last_rows, b.second_trip_wgs) == (c, {1, 2}, {True, False}, {False}, 1, 1)
        assert cases.sb_gemm_launch(64 * c, KC, NT, c, masked).two_ahead_fetch == {False}          # not before 64c + 1
        assert (d.grid, d.trips, d.two_ahead_fetch, d.last_rows) == (c, {2, 3}, {True, False}, 17)
        assert (e.grid, e.trips, e.last_rows) == (c, {3, 4}, 13)
        assert {x.wpc for x in (a, b, d, e)} == {1}


@pytest.mark.parametrize("c", CUS)
def test_row_lists_reach_every_class(c):
    rows = cases.SMALL + cases.EDGE(c)
    for KC, NT, masked in ((4, 1, False), (8, 1, False), (12, 1, False), (4, 2, False), (4, 3, False), (12, 1, True), (4, 2, True), (4, 3, True)):
        ls = [cases.sb_gemm_launch(R, KC, NT, c, masked) for R in rows]
        assert {x.grid_mod4 for x in ls} == {0, 1, 2, 3}
        assert {x.grid for x in ls} >= {1, 2, 3, c}
        assert set().union(*(x.prologue_fetch for x in ls)) == {True, False}
        assert set().union(*(x.two_ahead_fetch for x in ls)) == {True, False}
        trips = set().union(*(x.trips for x in ls))
        assert trips >= {1, 2, 3} and max(trips) > 3
        assert {x.last_rows for x in ls} >= {1, 13, 15, 16, 17, 31, 32}
        if masked:      # the column-sum reduction's remainder loop: grids that are no multiple of 4, among them one above 4
            assert {x.grid for x in ls if x.grid_mod4} >= {1, 2, 3} and (c < 129 or 129 in {x.grid for x in ls})
    if c >= 129:
        assert [cases.sb_gemm_launch(R, 4, 1, c, False).grid for R in cases.SMALL] == [1, 1, 1, 1, 1, 1, 2, 3, 129]


@pytest.mark.parametrize("c", CUS)
def test_thresholds_switch_the_workgroups_per_cu_and_the_phase_shift(c):
    ls = {R: cases.sb_gemm_launch(R, 4, 1, c, False) for R in cases.THRESHOLDS}
    assert [ls[R].wpc for R in cases.THRESHOLDS] == [1, 2, 2, 2, 2, 2]
    assert ls[131071].grid == c and ls[131072].grid == 2 * c
    assert {R: cases.sb_gemm_launch(R, 8, 1, c, False).wpc for R in cases.THRESHOLDS} == dict.fromkeys(cases.THRESHOLDS, 1)
    assert cases.sb_gemm_launch(131072, 4, 1, c, True).wpc == 1
    for form, below, above in (("plain", 0, 2), ("signs", 8, 10), ("addend", 1, 1)):
        opts = [cases.form_variant(128, 128, form, R)[2] for R in cases.THRESHOLDS]
        assert opts == [below] * 4 + [above] * 2, (form, opts)
    for R in cases.THRESHOLDS:
        assert True in ls[R].two_ahead_fetch and False in ls[R].two_ahead_fetch and min(ls[R].trips) > 3
    if c == 256:
        assert ls[131073].grid == 512 and ls[131073].trips == {8, 9} and ls[131073].last_rows == 1
        assert sum(1 for b in range(512) if len(range(b, ls[131073].n_it, 512)) == 9) == 1
        assert ls[786433].trips == {48, 49} and ls[786432].trips == {48} and ls[786431].last_rows == 31


def test_the_cases_enumerate_all_21_instantiations():
    for c in CUS:
        seen = {cases.form_variant(N, K, form, cases.rows_of(key, c)) for N, K, form, key in cases.gemm_cases()}
        assert seen == cases.ALL_VARIANTS
    # and without the threshold rows exactly the two phase-shifted ones are missing
    seen = {cases.form_variant(N, K, form, cases.rows_of(key, 256)) for N, K, form, key in cases.gemm_cases() if key not in cases.THRESHOLDS}
    assert cases.ALL_VARIANTS - seen == {(4, 1, 2), (4, 1, 10)}
    assert len(cases.gemm_cases()) == 20 * 13 + 18 and len(set(cases.gemm_cases())) == len(cases.gemm_cases())
    assert cases.mask_cols_of(384) == [0, 128, 256, 384] and cases.mask_cols_of(128) == [0, 128]


def test_variant_selection_restates_launch_sb_gemm_best():
    v = cases.sb_gemm_variant
    assert v(128, 128, False, False, 1) == (4, 1, 0) and v(128, 128, True, False, 10 ** 6) == (4, 1, 1)
    assert v(128, 128, False, False, 786432) == (4, 1, 2) and v(128, 128, False, True, 786432) == (4, 1, 10)
    assert v(128, 128, True, True, 786432) == (4, 1, 9) and v(128, 128, False, True, 786431) == (4, 1, 8)
    assert v(128, 256, False, False, 10 ** 6) == (8, 1, 2) and v(128, 256, True, False, 5) == (8, 1, 3)
    assert v(128, 256, False, True, 10 ** 6) == (8, 1, 10) and v(128, 256, True, True, 5) == (8, 1, 11)
    assert v(128, 384, False, False, 5) == v(128, 384, True, False, 5) == (12, 1, 2)
    assert v(256, 128, False, False, 5) == (4, 2, 2) and v(256, 128, True, False, 5) == (4, 2, 1)
    assert v(384, 128, False, False, 5) == (4, 3, 2) and v(384, 128, True, False, 5) == (4, 3, 0)
    assert v(256, 128, False, False, 5, "float") == (4, 2, 6) and v(256, 128, False, False, 5, "bits") == (4, 2, 22)
    assert v(384, 128, False, False, 5, "float") == (4, 3, 4) and v(384, 128, False, False, 5, "bits") == (4, 3, 20)
    assert v(128, 384, False, False, 5, "float") == (12, 1, 6) and v(128, 384, False, False, 5, "bits") == (12, 1, 22)
    with pytest.raises(AssertionError):
        v(256, 128, False, True, 5)          # sign bits: 128 outputs from 128 / 256 inputs only
    with pytest.raises(AssertionError):
        v(128, 128, False, False, 5, "float")


@pytest.mark.parametrize("c", CUS)
@pytest.mark.parametrize("split", [True, False])
def test_cell_rows_reach_every_class(c, split):
    for n in cases.CELL_NETS:
        S = cases.cell_slots(n, c, split)
        assert S == (c // n // 2 if split else c // n) and S > 1
        ls = {key: cases.cell_launch(cases.cell_rows_of(key, n, c, split), n, c, split) for key in cases.CELL_SMALL + cases.CELL_EDGE_KEYS}
        assert [ls[k].slots for k in cases.CELL_SMALL] == [1, 1, 1, 2] and [ls[k].last_rows for k in cases.CELL_SMALL] == [1, 15, 16, 1]
        a, b, d, e = (ls[k] for k in cases.CELL_EDGE_KEYS)
        assert (a.slots, a.trips, a.last_rows, a.second_trip_slots) == (S, {1}, 15, 0)
        assert (b.slots, b.trips, b.last_rows, b.second_trip_slots) == (S, {1, 2}, 1, 1)        # exactly one slot takes a second trip
        assert cases.cell_launch(32 * S, n, c, split).trips == {2}                               # no third trip before 32 S + 1
        assert (d.slots, d.trips, d.last_rows) == (S, {2, 3}, 1)
        assert (e.slots, e.trips, e.last_rows) == (S, {3, 4}, 5)
        assert a.prologue_fetch == {False} and b.prologue_fetch == {True, False}
        if split:
            assert b.two_ahead_fetch == {False} and d.two_ahead_fetch == {True, False}
        else:
            assert all(x.two_ahead_fetch == set() for x in ls.values())
    assert len(cases.cell_cases()) == 2 * 4 * 8


def test_sign_bits_pack_and_unpack_against_a_loop():
    g = torch.Generator().manual_seed(3)
    y = torch.randn(5, 24, generator=g)
    y[0, 0], y[1, 7], y[2, 8], y[3, 23], y[4, 15] = 0.0, -0.0, 1e-42, float("nan"), float("inf")
    b = cases.pack_signs(y)
    assert b.dtype == torch.uint8 and b.shape == (5, 3)
    for r in range(5):
        for j in range(3):
            want = 0
            for k in range(8):
                if float(y[r, 8 * j + k]) > 0:
                    want |= 1 << k
            assert int(b[r, j]) == want, (r, j)
    bits = cases.unpack_signs(b)
    assert bits.dtype == torch.bool and torch.equal(bits, y > 0)
    assert bool(bits[2, 8]) and not bool(bits[0, 0]) and not bool(bits[1, 7]) and not bool(bits[3, 23]) and bool(bits[4, 15])
    every = torch.arange(256, dtype=torch.int32).to(torch.uint8).reshape(32, 8)
    assert torch.equal(cases.pack_signs(cases.unpack_signs(every).float()), every)
