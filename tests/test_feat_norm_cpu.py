"""`algo.use_layer_norm` without a GPU: the key's parsing and refusals, the on-model's parameters, the CPU formula."""
import pytest
import torch
import torch.nn.functional as F

from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config

KEY = "algo.use_layer_norm"


def _options(name, **ov):
    from distributed_multi_agent_reinforcement_learning_amd import e3d_agent, imitation, kickstart, n2n_agent
    cfg = baseline_config(name, **ov)
    cls = n2n_agent.N2nMAPPO if name == "cfg4_n2n" else e3d_agent.E3dMAPPO
    agent = cls.__new__(cls)
    agent.imitation, agent.kick = imitation.imitation_options(cfg), kickstart.kickstart_options(cfg)   # (ParticleMAPPO.__init__ sets them first)
    cls._options(agent, cfg)
    return agent.use_layer_norm


@pytest.mark.parametrize("name", ["cfg4_n2n", "cfg5"])
def test_the_key_parses_defaults_to_false_and_is_refused_at_another_width(name):
    assert _options(name) is False and _options(name, **{KEY: False}) is False and _options(name, **{KEY: True}) is True
    assert _options(name, **{KEY: "false"}) is False and _options(name, **{KEY: "true"}) is True   # (a command line's strings)
    assert _options(name, **{"algo.rnn_hidden_dim": 64}) is False                                 # off: any width, as before
    with pytest.raises(ValueError, match=KEY):
        _options(name, **{KEY: "yes"})
    with pytest.raises(ValueError, match="algo.use_layer_norm.*algo.rnn_hidden_dim"):
        _options(name, **{KEY: True, "algo.rnn_hidden_dim": 64})
    from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
    with pytest.raises(ValueError, match=KEY):                                                    # the pursuit learner refuses the key
        MAPPO(baseline_config("cfg2", **{KEY: True}), 8, 2, "defender")


def test_on_model_is_the_off_model_plus_four_keys_last():
    from distributed_multi_agent_reinforcement_learning_amd.model import build_actor_critic
    nets = {}
    for on in (False, True):
        torch.manual_seed(3)
        nets[on] = build_actor_critic(baseline_config("cfg4_n2n", **({KEY: True} if on else {})), "cpu")
    for off, on in zip(nets[False], nets[True]):
        sd_off, sd_on = off.state_dict(), on.state_dict()
        assert list(sd_on) == list(sd_off) + ["feat_norm.weight", "feat_norm.bias"]
        assert all(torch.equal(sd_on[k], v) for k, v in sd_off.items())
        assert [n for n, _ in on.named_parameters()][-2:] == ["feat_norm.weight", "feat_norm.bias"]
        assert torch.equal(sd_on["feat_norm.weight"], torch.ones(128)) and torch.equal(sd_on["feat_norm.bias"], torch.zeros(128))


def test_cpu_f64_takes_the_torch_formula():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(0)
    xs = [torch.randn(3, 5, 128, dtype=torch.float64, requires_grad=True) for _ in range(2)]
    ws, bs = [[torch.randn(128, dtype=torch.float64, requires_grad=True) for _ in range(2)] for _ in range(2)]
    ys = ops.feat_norm_train(xs, ws, bs, 1e-5)
    refs = [F.layer_norm(x, (128,), w, b, 1e-5) for x, w, b in zip(xs, ws, bs)]
    assert all(torch.equal(y, r) for y, r in zip(ys, refs))
    g, g_ref = [torch.autograd.grad(sum(v.square().sum() for v in out), xs + ws + bs) for out in (ys, refs)]
    assert all(torch.equal(a, b) for a, b in zip(g, g_ref))
