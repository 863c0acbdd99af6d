"""`algo.semantic_level_aggregator: att` on the CPU: what it adds to the `mean` model (one zero parameter, last) and what it refuses."""
import pytest
import torch

from distributed_multi_agent_reinforcement_learning_amd.model import DHGN
from tests.helpers import product_cfg


def _net(seed=3, E=128, depth=1, **algo):
    torch.manual_seed(seed)
    return DHGN(4, E, False, product_cfg(3, 20, 20, depth=depth, **{f"algo.{k}": v for k, v in algo.items()}).algo)


@pytest.mark.parametrize("other", [{}, {"vertex_level_aggregator": "att", "fcra_aggregator": "att"}], ids=["mean", "att-everywhere"])
def test_att_is_the_base_model_plus_one_zero_parameter(other):
    """last of all where it is the only alpha; behind the vertex and FCRA alphas, which keep their places, where those exist"""
    base, att, new = _net(**other), _net(semantic_level_aggregator="att", **other), "alpha.AGG_semantic"
    for names, plain in ((list(att.state_dict()), list(base.state_dict())), *[[[n for n, _ in m.named_parameters()] for m in (att, base)]]):
        assert [n for n in names if n != new] == plain
        assert names[-1] == new if not other else names[names.index(new) - 1] == "alpha.AGG_fcra_0"
    assert all(torch.equal(v, att.state_dict()[k]) for k, v in base.state_dict().items()), "an initial parameter differs from the mean model's"
    assert tuple(att.alpha["AGG_semantic"].shape) == (128, 1) and (att.alpha["AGG_semantic"] == 0).all()


def test_alpha_zero_is_the_mean_forward_in_f64():
    """(the vertex level on att and no FCRA hop: the mean message and the hops have no CPU path)"""
    base, att = [_net(depth=0, vertex_level_aggregator="att", **kw).double() for kw in ({}, {"semantic_level_aggregator": "att"})]
    g = torch.manual_seed(0)
    R, P, O = 4, 3, 5
    p, e, o = [torch.rand(R, k, 4, generator=g, dtype=torch.float64) * 20 for k in (P, 1, O)]
    adj = [(torch.rand(R, P, k, generator=g) < 0.5).double() for k in (P, 1, O)]
    hist = []
    for critic in (False, True):
        torch.testing.assert_close(att(p, e, o, *adj, hist, critic), base(p, e, o, *adj, hist, critic), rtol=1e-12, atol=1e-12)


def test_refusals():
    with pytest.raises(NotImplementedError):
        _net(semantic_level_aggregator="pool")
    with pytest.raises(ValueError):
        _net(E=64, semantic_level_aggregator="att")
