"""CPU checks of tests/msg_ref.py (the float64 reference of the DHGN relation message) and of the inputs of tests/test_msg_variants_gpu.py:
the reference against the materialised torch formula and torch autograd in float64, its edge cases, the conditions every GPU case's
inputs must satisfy for the gradient bound to be strict, the selector mirror against the launchers' source text, and the coverage of
the launchers' switch table by the cases."""
import os

import numpy as np
import pytest
import torch

from tests import msg_ref as mr
from tests import test_msg_variants_gpu as gv
from tests.test_ops_gpu import _ref_msg_agg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small(seed, R, P, K, E, din, q_div, weighted):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(R, P, 4, generator=g) * 10 + 20).double()
    q = torch.zeros(R // q_div, K, 4).double()
    q[:, :, :2] = torch.randint(0, 40, (R // q_div, K, 2), generator=g).double()
    e = (torch.randn(R, 4, generator=g) * 10 + 20).double() if din == 8 else None
    adj = gv._adjacency(g, R, P, K, 0.5, weighted).double()
    kv = torch.randint(0, K + 1, (R // q_div,), generator=g)
    kv[0] = 0
    W = (torch.randn(E, din, generator=g) * 0.3).double().requires_grad_(True)
    b = (torch.randn(E, generator=g) * 0.1).double().requires_grad_(True)
    gout = torch.randn(R, P, E, generator=g).double()
    return p, q, e, adj, kv, W, b, gout


@pytest.mark.parametrize("source,weighted", [("tensor", False), ("tensor", True), ("ones", False), ("valid", False)])
@pytest.mark.parametrize("R,P,K,E,din,q_div", [(6, 5, 7, 8, 4, 3), (4, 3, 3, 16, 8, 1)])
def test_reference_equals_the_materialised_formula_and_autograd(source, weighted, R, P, K, E, din, q_div):
    p, q, e, adj, kv, W, b, gout = _small(R * 100 + K, R, P, K, E, din, q_div, weighted)
    qf = q.repeat_interleave(q_div, 0)
    if source == "tensor":
        a = adj
    elif source == "ones":
        a = torch.ones_like(adj)
    else:
        a = (torch.arange(K)[None, None, :] < kv.repeat_interleave(q_div)[:, None, None]).double().expand(R, P, K)
    want = _ref_msg_agg(p, qf, e.unsqueeze(-2) if e is not None else None, a, W, b, din == 8)
    want.backward(gout)
    got = mr.msg_agg(p, q, e, W, b, source, adj, kv, q_div, gout)
    # chunking must not matter: the same with one row per chunk
    one = mr.relation(p, q, e, W, b, [mr.abar(source, R, P, K, adj, kv, q_div)], [[(0, gout)]], q_div, chunk_entries=1)
    for mine in (got, dict(out=one["out"][0], **one["grads"][0])):
        assert np.allclose(mine["out"], want.detach().numpy(), rtol=1e-12, atol=1e-12)
        assert np.allclose(mine["dW"], W.grad.numpy(), rtol=1e-11, atol=1e-11)
        assert np.allclose(mine["db"], b.grad.numpy(), rtol=1e-11, atol=1e-11)


def test_pair_job_is_the_sum_of_both_networks():
    p, q, e, adj, kv, W, b, ga = _small(5, 6, 4, 5, 8, 8, 1, True)
    gc = torch.randn(6, 4, 8, generator=torch.Generator().manual_seed(9)).double()
    both = mr.msg_agg(p, q, e, W, b, "tensor", adj, gout=ga, gout_ones=gc)
    a = mr.msg_agg(p, q, e, W, b, "tensor", adj, gout=ga)
    c = mr.msg_agg(p, q, e, W, b, "ones", gout=gc)
    assert np.allclose(both["dW"], a["dW"] + c["dW"], rtol=1e-12, atol=1e-12) and np.allclose(both["db"], a["db"] + c["db"], rtol=1e-12, atol=1e-12)


def test_empty_relation_is_exactly_zero():
    p = torch.randn(3, 4, 4)
    for source in ("tensor", "ones", "valid"):
        r = mr.msg_agg(p, torch.zeros(3, 0, 4), None, torch.randn(8, 4), torch.randn(8), source, torch.zeros(3, 4, 0), torch.zeros(3, dtype=torch.int32),
                       gout=torch.randn(3, 4, 8))
        assert r["out"].shape == (3, 4, 8)
        for k in ("out", "dW", "db", "amb_W", "amb_b"):
            assert not r[k].any()


def test_adjacency_is_normalised_by_its_l1_norm():
    a = mr.abar("tensor", 1, 1, 2, torch.tensor([[[1.0, -1.0]]]))
    assert a.tolist() == [[[0.5, -0.5]]]
    assert mr.abar("tensor", 1, 1, 2, torch.zeros(1, 1, 2)).tolist() == [[[0.0, 0.0]]]
    p, q = torch.tensor([[[3.0, 0, 0, 0]]]), torch.tensor([[[1.0, 0, 0, 0], [2.0, 0, 0, 0]]])
    W, b = torch.tensor([[1.0, 0, 0, 0]]), torch.zeros(1)
    assert mr.msg_agg(p, q, None, W, b, "tensor", torch.tensor([[[1.0, -1.0]]]))["out"].item() == 0.5 * 2 - 0.5 * 1


def test_ambiguity_budget_marks_decisions_near_zero():
    """z = w (p - q) with p - q = 2^-20 of the magnitudes: inside the guard band; its budget is |g| |x|"""
    p, q = torch.tensor([[[8.0 + 2.0 ** -17, 0, 0, 0]]]), torch.tensor([[[8.0, 0, 0, 0]]])
    W, b = torch.tensor([[1.0, 0, 0, 0]]), torch.zeros(1)
    r = mr.msg_agg(p, q, None, W, b, "ones", gout=torch.full((1, 1, 1), 3.0))
    assert r["amb_b"].item() == 3.0 and r["amb_W"][0, 0] == 3.0 * 2.0 ** -17 and r["db"].item() == 3.0
    far = mr.msg_agg(p + 1, q, None, W, b, "ones", gout=torch.full((1, 1, 1), 3.0))
    assert not far["amb_b"].any() and not far["amb_W"].any() and not far["fwd_amb"].any()


# ---- conditions on the inputs of the GPU cases ---------------------------------------------------------------------------------------
AMB_SHARE_CAP = 0.02
FWD_AMB_CAP = 0.1     # of the forward bound: the forward verdict cannot hinge on how a kernel decides an ambiguous entry


def _conditions(grads, fwd):
    """grads: [dict(amb_W, amb_b)]; fwd: [(out, fwd_amb)] -> (share of gradient elements with a budget, largest fwd_amb in units of the bound)"""
    amb = np.concatenate([np.concatenate((g["amb_W"].ravel(), g["amb_b"].ravel())) for g in grads])
    share = float((amb > 0).mean())
    dep = max(float((fa / (mr.FWD_ATOL + mr.FWD_RTOL * np.abs(out))).max()) if out.size else 0.0 for out, fa in fwd)
    return share, dep


def single_conditions(name, E):
    ref = gv.single_reference(name, E)
    return _conditions(list(ref.values()), [(r["out"], r["fwd_amb"]) for r in ref.values()])


def three_conditions(name):
    ref = gv.three_reference(name)
    fwd = [(r[k], r["fwd_amb"][i]) for r in ref for i, k in enumerate(("actor", "ones", "valid")) if r[k] is not None]
    return _conditions([r["grads"] for r in ref], fwd)


def sorted_conditions(name):
    ref = gv.sorted_reference(name)
    return _conditions([ref], [(ref["out"], ref["fwd_amb"])])


def _assert_conditions(share, dep):
    assert share <= AMB_SHARE_CAP, f"{share:.4f} of the gradient elements carry an ambiguity budget: take another seed (SEED_BUMP)"
    assert dep <= FWD_AMB_CAP, f"a forward value depends on an ambiguous decision ({dep:.3f} of its bound): take another seed (SEED_BUMP)"


@pytest.mark.parametrize("name,E", gv.SINGLE_PARAMS, ids=[f"{n}-E{E}" for n, E in gv.SINGLE_PARAMS])
def test_inputs_of_the_single_relation_cases(name, E):
    _assert_conditions(*single_conditions(name, E))


@pytest.mark.parametrize("name", [c.name for c in gv.THREE])
def test_inputs_of_the_three_relation_cases(name):
    _assert_conditions(*three_conditions(name))


@pytest.mark.parametrize("name", [c.name for c in gv.SORTED])
def test_inputs_of_the_sorted_cases(name):
    _assert_conditions(*sorted_conditions(name))


def test_inputs_hold_the_edges_the_cases_are_named_for():
    w = gv.single_inputs("weighted-4x16", 64)["adj"]
    assert set(w.unique().tolist()) == {-1.5, 0.0, 0.25, 1.0, 2.0}
    assert w[1, 0].sum() == 0 and w[1, 0].abs().sum() == 3 and not w[0, 0].any()
    for name in ("rel2-P8", "qs-K16", "as-5x13"):
        c = gv.SINGLE_BY_NAME[name]
        assert {0, 1, c.K} <= set(gv.single_inputs(name, 64)["kvalid"].tolist())
    assert {0, 1, 6} <= set(gv.three_inputs("R12-P5")["kvalid"].tolist())
    o = gv.sorted_inputs("K255-E64-P1-q1")["o"]
    assert len(o[0].unique(dim=0)) == 3 and (o[1].abs().sum(-1) > 0).sum() == 2 and (o[0].abs().sum(-1) > 0).all()
    big = gv.single_inputs("bwd-tail", 64)
    assert torch.equal(big["p"][0], big["p"][gv.PERIOD]) and not torch.equal(big["adj"][1], big["adj"][1 + gv.PERIOD])


# ---- the selector mirror ------------------------------------------------------------------------------------------------------------
def test_selector_mirror_matches_the_launchers_source():
    """the thresholds the mirror copies, as they stand in csrc/mappo_ops.hip: a change there must be carried over to the mirror (and the
    cases re-derived), not pass unnoticed"""
    src = open(os.path.join(ROOT, "distributed_multi_agent_reinforcement_learning_amd", "csrc", "mappo_ops.hip")).read()
    for line in ("bool msg_q_small(int K) { return 4 * K <= 64; }",
                 "if (adj_mode == MO_ADJ_TENSOR) return P * K <= 64;",
                 "if (adj_mode == MO_ADJ_BITS) return P * MO_ADJ_ROW_WORDS(K) <= 128;",
                 "constexpr int BWD_BLOCKS = 2048, FWD_BLOCKS = 8192;",
                 "const bool halves = R <= 2048 && P > 4;",
                 "const int pt = halves ? (P <= 8 ? 4 : 8) : (P <= 8 ? 8 : 16), gy = (P + pt - 1) / pt;",
                 "if (P <= 8) MSGW_FWD_PT(8) else MSGW_FWD_PT(16)",
                 "if (P <= 8) MSGW_BWD_PT(8) else MSGW_BWD_PT(16)",
                 "const bool qs = msg_q_small(K), as = msg_adj_small(P, K, adj_mode), ev2 = (E % 128) == 0;",
                 "const int g0 = R < max_blocks ? (R > 0 ? R : 1) : max_blocks;"):
        assert line in src, line
    hdr = open(os.path.join(ROOT, "include", "mappo_ops.h")).read()
    assert "#define MO_ADJ_ROW_WORDS(K) (((((K) + 31) >> 5) + 3) & ~3)" in hdr
    assert [gv.adj_row_words(K) for K in (1, 32, 33, 128, 129, 256, 257)] == [4, 4, 4, 4, 8, 8, 12]
    assert gv.row_split(2049, gv.BWD_BLOCKS) == (2, 1025, 1) and gv.row_split(8193, gv.FWD_BLOCKS) == (2, 4097, 1) and gv.row_split(12, 8192) == (1, 12, 1)


def test_cases_cover_the_switch_table():
    """every value of every switch of the launchers -- and every (PT, QS, AS, EV) instantiation of the single-relation kernels that a
    shape can select -- is selected by at least one case that is compared with f64"""
    fwd, bwd = set(), set()
    for name, E in gv.SINGLE_PARAMS:
        c = gv.SINGLE_BY_NAME[name]
        for s in c.sources:
            a, b = gv.select_single(c.R, c.P, c.K, E, s), gv.select_single(c.R, c.P, c.K, E, s, bwd=True)
            fwd.add((a["PT"], a["QS"], a["AS"], a["EV"]))
            bwd.add((b["PT"], b["QS"], b["AS"], b["EV"], False, b["rpb"] > 1 and b["tail"] < b["rpb"]))
    # reachable: AS off needs P K > 64 (float) or P RWK > 128 (packed); every (PT, QS, AS) combination has such a shape
    every = {(pt, qs, as_, ev) for pt in (8, 16) for qs in (False, True) for as_ in (False, True) for ev in (1, 2)}
    assert fwd == every
    assert {t[:4] for t in bwd} == every and any(t[5] for t in bwd)
    three, pair = set(), set()
    for c in gv.THREE:
        for mode_o in ("tensor", "bits"):
            s = gv.select_msg3(c.R, c.P, c.E, c.P, c.Ke, c.Ko, mode_o)
            three.add((s["PT"], s["halves"]))
            three.add(("S01", s["S01"])); three.add(("AS2", s["AS2"])); three.add(("EV", s["EV"])); three.add(("tail", s["rpb"] > 1 and s["tail"] < s["rpb"]))
            three.add(("short wave", s["halves"] and s["last"] < s["PT"]))
        for K in (c.P, c.Ke):
            b = gv.select_single(c.R, c.P, K, c.E, "tensor", bwd=True, pair=True)
            pair.add((b["PT"], b["AS"], b["EV"]))
            pair.add(("tail", b["rpb"] > 1 and b["tail"] < b["rpb"]))
    assert {(4, True), (8, True), (8, False), (16, False)} <= three
    assert {(k, v) for k in ("S01", "AS2", "tail", "short wave") for v in (False, True)} | {("EV", 1), ("EV", 2)} <= three
    assert {(8, True, 1), (8, True, 2), (16, False, 1), (16, False, 2), (16, True, 1), ("tail", True), ("tail", False)} <= pair
    assert {c.E for c in gv.THREE} == {64, 128, 192} and any(c.Ko == 0 for c in gv.THREE) and any(c.Ke > 1 and c.Ko for c in gv.THREE)
    # weighted adjacency in both AS forms, forward and backward
    for name, as_ in (("weighted-4x16", True), ("weighted-8x40", False)):
        c = gv.SINGLE_BY_NAME[name]
        assert c.weighted and gv.select_single(c.R, c.P, c.K, 64, "tensor")["AS"] is as_
    assert {(c.K, c.E, c.P, c.q_div) for c in gv.SORTED} == {(K, E, P, q) for K in (2, 255) for E in (64, 192) for P in (1, 16) for q in (1, 7)}
