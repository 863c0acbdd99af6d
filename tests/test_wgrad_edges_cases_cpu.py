"""tests/wgrad_edges_cases.py claims that its row counts put k_sb_wgrad and k_wgrad / k_wgrad_reduce on every edge of their launch
arithmetic.  Here the claims are checked without a GPU; tests/test_wgrad_edges_gpu.py asserts the same per case."""
import pytest

from tests import wgrad_edges_cases as cases


def test_split_layouts_are_the_three_the_loader_has():
    assert [cases.sb_wgrad_layout(M, N) for M, N in cases.SB_SHAPES] == [(1, 4, 0), (2, 3, 2), (2, 3, 2), (2, 3, 0), (2, 3, 0)]
    assert len(cases.SB_SHAPES) == len(set(cases.SB_SHAPES)) == 5 and all(cases.sb_wgrad_shape_ok(M, N) for M, N in cases.SB_SHAPES)
    every = [(M, N) for M in range(128, 1025, 128) for N in range(128, 1025, 128) if cases.sb_wgrad_shape_ok(M, N)]
    assert sorted(every) == sorted(cases.SB_SHAPES)                    # the instantiation set is complete
    assert {cases.sb_wgrad_layout(M, N).DEPTH for M, N in cases.SB_SHAPES} == {3, 4}
    assert {cases.sb_wgrad_layout(M, N).off_waves for M, N in cases.SB_SHAPES} == {0, 2}


def test_split_rows_reach_every_chunk_count_and_a_tail_after_each():
    cs = {K: cases.sb_wgrad_counts(K) for K in cases.SB_ROWS}
    assert len(cases.SB_ROWS) == len(set(cases.SB_ROWS)) == 7 + 18 + 6 - 1        # 4096 is small and uniform
    reached = set().union(*(c.counts for c in cs.values()))
    assert reached == set(range(10))
    assert {c.last for c in cs.values() if c.tail} == set(range(10))             # a tail after each count 0 .. 9
    assert {c.last for c in cs.values() if not c.tail} >= set(range(1, 10))      # and each count without one
    for n in range(1, 10):
        a, b = cs[cases.sb_uniform_rows(n, False)], cs[cases.sb_uniform_rows(n, True)]
        assert (a.counts, a.last, a.tail) == ({n}, n, 0) and (b.counts, b.last, b.tail) == ({n}, n, 13 if n % 2 else 5)
    for K, pair in cases.SB_MIXED.items():
        assert cs[K].counts == pair, (K, cs[K])
    assert [(cs[K].counts, cs[K].last, cs[K].tail) for K in cases.SB_SMALL] == [
        ({0}, 0, 1), ({0}, 0, 15), ({0, 1}, 1, 0), ({0, 1}, 1, 1), ({0, 1}, 1, 15), ({1}, 1, 0), ({1}, 1, 1)]
    assert max(cases.SB_ROWS + cases.TN2_ROWS + cases.SB_ACC_ROWS) == 36877


@pytest.mark.parametrize("depth", [3, 4])
def test_split_rows_reach_every_class_of_the_prefetch_ring(depth):
    """fewer chunks than DEPTH, exactly DEPTH, the second trip of the `c += D` loop, 2 DEPTH + 1, and the tail into image 0 after an odd
    and after an even count -- in each of these classes"""
    per = {K: cases.sb_classes(K, depth) for K in cases.SB_ROWS}
    assert set().union(*per.values()) == {"none", "below depth", "depth", "second trip", "third trip", "tail after an even count",
                                           "tail after an odd count"}
    uniform = {n: cases.sb_classes(cases.sb_uniform_rows(n, True), depth) for n in range(1, 10)}
    for n, cl in uniform.items():
        ring = "below depth" if n < depth else "depth" if n == depth else "second trip" if n <= 2 * depth else "third trip"
        assert cl == {ring, f"tail after {'an odd' if n % 2 else 'an even'} count"}, (n, cl)
    for ring in ("below depth", "depth", "second trip", "third trip"):
        tails = set().union(*(cl - {ring} for cl in uniform.values() if ring in cl))
        want = {"tail after an even count", "tail after an odd count"}
        ns = [n for n, cl in uniform.items() if ring in cl]
        assert tails == want or (len(ns) == 1 and len(tails) == 1), (ring, tails)        # a class of one count (DEPTH; 9 = 2 * 4 + 1) has one parity
    assert 2 * depth + 1 in set().union(*(cases.sb_wgrad_counts(K).counts for K in cases.SB_ROWS))
    # the rows of the accumulate and tn2 cases: a tail after both parities too
    for rows in (cases.SB_ACC_ROWS, cases.TN2_ROWS):
        assert {cases.sb_wgrad_counts(K).last % 2 for K in rows if cases.sb_wgrad_counts(K).tail} == {0, 1}
    for n in cases.SB_ZERO_TAIL_N:
        assert cases.sb_wgrad_counts(4096 * n + 13).counts == {n} == cases.sb_wgrad_counts(4096 * n).counts
    assert {n % 2 for n in cases.SB_ZERO_TAIL_N} == {0, 1}


def test_tn2_splits():
    assert set(cases.TN2_SPLITS) == set(cases.SB_SHAPES)
    for (M, N), m1s in cases.TN2_SPLITS.items():
        assert all(4 <= m1 <= M - 4 and m1 % 4 == 0 for m1 in m1s)
    assert {4, 380} <= set(cases.TN2_SPLITS[(384, 128)])                 # the first and the last column quad
    assert len(cases.tn2_cases()) == (5 + 3 * 3 + 2) * 5
    cs = [cases.sb_wgrad_counts(K) for K in cases.TN2_ROWS]
    assert [c.counts for c in cs] == [{0, 1}, {3}, {4}, {4, 5}, {9}] and all(c.tail for c in cs)


def test_fp32_split_restates_wgrad_split():
    for (M, N), S in cases.WG_S.items():
        s, am, bn, gy, gz = cases.wgrad_split(M, N)
        assert s == S and gy * 128 * am == M and gz * 128 * bn == N and s * gy * gz <= 256, (M, N)
    assert list(cases.WG_S) == cases.WG_SHAPES
    assert {cases.wgrad_split(M, N)[1:3] for M, N in cases.WG_SHAPES} == cases.WG_INSTANTIATIONS and len(cases.WG_INSTANTIATIONS) == 3
    assert {cases.wgrad_split(M, N)[1:3] for M in range(128, 1025, 128) for N in range(128, 1025, 128)} == cases.WG_INSTANTIATIONS
    assert {S % 4 for S in cases.WG_S.values()} == {0, 1, 2, 3}          # k_wgrad_reduce: the four waves' strided sums, unequal lengths
    assert {cases.wgrad_split(M, N)[3] > 1 for M, N in cases.WG_SHAPES} == {True, False}
    assert {cases.wgrad_split(M, N)[4] > 1 for M, N in cases.WG_SHAPES} == {True, False}
    assert max(cases.wg_rows_of(k, 4) for k in cases.wg_row_keys()) == 387


@pytest.mark.parametrize("S", sorted(set(cases.WG_S.values())))
def test_fp32_rows_reach_every_class(S):
    keys = cases.wg_row_keys()
    assert len(keys) == 4 + 9 + 5
    cs = {}
    for key in keys:
        K = cases.wg_rows_of(key, S)
        c = cs[key] = cases.wgrad_counts(K, S)
        counts, tail = cases.wg_expected(key, S)
        assert (c.counts, c.tail) == (counts, tail), (key, S, c)
    assert len({cases.wg_rows_of(k, S) for k in keys}) == len(keys)
    assert set().union(*(c.counts for c in cs.values())) == {0, 1, 7, 8, 9, 15, 16, 17, 24}
    assert set().union(*(c.pairs for c in cs.values())) == {0, 1, 2, 3}
    assert set().union(*(c.leftover for c in cs.values())) == {0, 1, 7}
    assert {c.tail for c in cs.values()} == {0, 1, 2, 3}
    # a tail behind a last workgroup with no step, with leftover steps only, and with pairs only
    assert {(c.last // 8 > 0, c.last % 8 > 0) for c in cs.values() if c.tail} >= {(False, False), (False, True), (True, False), (True, True)}
    for key in cases.wg_acc_keys():
        assert key in keys
