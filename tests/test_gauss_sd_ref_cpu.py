"""CPU checks of the state-dependent log-std / tanh-squash options of the env_3d policy: the host reference (tests/gauss_sd_ref.py)
against f64 torch autograd, the config validation of E3dMAPPO and the parameters of GaussianActor in both modes."""
import numpy as np
import pytest
import torch

from tests import gauss_sd_ref
from tests.gauss_ref import HALF_LN_2PI

LO, HI = -1.0, 0.5


def _case(state, A, seed):
    rng = np.random.default_rng(seed)
    shape = (5, 6, 4)
    mu = rng.standard_normal(shape + (A,)) * 0.5
    if state:
        ls_raw = rng.standard_normal(shape + (A,)) * 0.8
        ls_raw.reshape(-1, A)[:4, 0] = [LO, HI, LO - 0.3, HI + 0.2]   # rows exactly on and beyond each bound
    else:
        ls_raw = np.array([LO, HI, HI + 0.4, LO - 0.2, 0.1][:A])
    ls = np.clip(np.broadcast_to(ls_raw, mu.shape), LO, HI)
    u = mu + np.exp(ls) * rng.standard_normal(shape + (A,))
    lp = (-0.5 * ((u - mu) / np.exp(ls)) ** 2 - ls - HALF_LN_2PI).sum(-1)
    lp_old = lp + rng.standard_normal(shape) * 0.1
    adv, vo, vt = (rng.standard_normal(shape) for _ in range(3))
    vn = vo + rng.standard_normal(shape) * 0.1
    active = (rng.random(shape) < 0.7).astype(np.float64)
    return mu, ls_raw, u, vn, lp_old, adv, active, vo, vt


@pytest.mark.parametrize("squash", ["clip", "tanh"])
@pytest.mark.parametrize("state", [False, True])
@pytest.mark.parametrize("use_value_clip", [True, False])
def test_loss_reference_matches_torch_autograd(squash, state, use_value_clip):
    A = 3 if state else 5
    mu, ls_raw, u, vn, lp_old, adv, active, vo, vt = _case(state, A, 3 + state + 2 * use_value_clip)
    eps, ent = 0.05, 0.05
    la, lc, g_mu, g_ls, g_v = gauss_sd_ref.ppo_loss(mu, ls_raw, u, vn, lp_old, adv, active, vo, vt, eps, ent, use_value_clip, LO, HI, squash)
    t = lambda x, g=False: torch.tensor(x, dtype=torch.float64, requires_grad=g)
    tmu, tls, tvn = t(mu, True), t(ls_raw, True), t(vn, True)
    ra, rc = gauss_sd_ref.torch_ppo_loss(tmu, tls, t(u), tvn, t(lp_old), t(adv), t(active), t(vo), t(vt), eps, ent, use_value_clip, LO, HI, squash)
    ga = torch.autograd.grad(ra, (tmu, tls))
    gc = torch.autograd.grad(rc, (tvn,))
    np.testing.assert_allclose(la, ra.item(), rtol=1e-12)
    np.testing.assert_allclose(lc, rc.item(), rtol=1e-12)
    np.testing.assert_allclose(g_mu, ga[0].numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(g_ls, ga[1].numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(g_v, gc[0].numpy(), rtol=1e-10, atol=1e-14)
    # the bounds themselves pass the gradient, values beyond them do not
    flat = np.broadcast_to(ls_raw, mu.shape).reshape(-1, A)
    if state:
        gl = g_ls.reshape(-1, A)
        assert np.all(gl[(flat < LO) | (flat > HI)] == 0)
        on = (flat == LO) | (flat == HI)
        assert on.any() and np.all(gl[on] != 0)
    else:
        assert g_ls[2] == 0 and g_ls[3] == 0 and g_ls[0] != 0 and g_ls[1] != 0


def test_tanh_log_prob_is_the_change_of_variables():
    # the squashed density of y = tanh(u): log N(u) - log(1 - tanh(u)^2), checked through the explicit Jacobian 1 - y^2
    u = np.linspace(-6, 6, 101)
    y = np.tanh(u)
    np.testing.assert_allclose(gauss_sd_ref.tanh_log_jac(u), np.log1p(-y * y), rtol=1e-9, atol=1e-12)
    assert np.isfinite(gauss_sd_ref.tanh_log_jac(np.array([-400.0, 400.0]))).all()


def test_head_reference_modes():
    rng = np.random.default_rng(1)
    feat, W, b = rng.standard_normal((9, 128)), rng.standard_normal((3, 128)) * 0.1, rng.standard_normal(3)
    W_ls, b_ls = rng.standard_normal((3, 128)) * 0.2, rng.standard_normal(3)
    mu, ls_raw, z, u, env, lp = gauss_sd_ref.head_sample(feat, W, b, (W_ls, b_ls), 3, 100, lo=LO, hi=HI, squash="tanh")
    ls = np.clip(feat @ W_ls.T + b_ls, LO, HI)
    np.testing.assert_allclose(u, mu + np.exp(ls) * z)
    np.testing.assert_array_equal(env, np.tanh(u))
    ref = torch.distributions.Normal(torch.tensor(mu), torch.tensor(np.exp(ls))).log_prob(torch.tensor(u)).sum(-1).numpy()
    np.testing.assert_allclose(lp, ref - np.log1p(-np.tanh(u) ** 2).sum(-1), rtol=1e-10, atol=1e-10)
    # param mode with infinite bounds and clip is gauss_ref.head_sample
    from tests import gauss_ref
    ls_v = rng.standard_normal(3) * 0.3
    a = gauss_sd_ref.head_sample(feat, W, b, ls_v, 3, 100)
    r = gauss_ref.head_sample(feat, W, b, ls_v, 3, 100)
    for x, y in zip((a[0], a[2], a[3], a[4], a[5]), r):
        np.testing.assert_array_equal(x, y)


def _cfg(**ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config("cfg5", **ov)


@pytest.mark.parametrize("ov,key", [({"algo.gauss_std": "learned"}, "algo.gauss_std"), ({"algo.gauss_squash": "sigmoid"}, "algo.gauss_squash"),
                                    ({"algo.log_std_min": 1.0, "algo.log_std_max": 1.0}, "algo.log_std_min"),
                                    ({"algo.log_std_min": 2.5}, "algo.log_std_min"),
                                    ({"algo.gauss_std": "state", "env.action_dim": 9}, "algo.gauss_std")])
def test_config_validation(ov, key):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        E3dMAPPO(_cfg(**ov), 8, 1)


def test_config_defaults_and_accepted_values():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import gauss_policy_options
    assert gauss_policy_options(_cfg()) == ("param", "clip", -5.0, 2.0)
    assert gauss_policy_options(_cfg(**{"algo.gauss_std": "state", "algo.gauss_squash": "tanh", "env.action_dim": 8})) == ("state", "tanh", -5.0, 2.0)
    assert gauss_policy_options(_cfg(**{"algo.gauss_squash": "tanh", "env.action_dim": 16}))[1] == "tanh"   # param mode has no A <= 8 limit
    with pytest.raises(ValueError, match="use_reward_norm"):   # the existing rejection comes first, unchanged
        from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
        E3dMAPPO(_cfg(**{"algo.use_reward_norm": True, "algo.gauss_std": "bad"}), 8, 1)


def test_parse_overrides_reads_literals():
    from distributed_multi_agent_reinforcement_learning_amd.config import parse_overrides
    assert parse_overrides(["algo.gauss_std=state", "algo.log_std_min=-4", "runtime.num_envs=64"]) == \
        {"algo.gauss_std": "state", "algo.log_std_min": -4, "runtime.num_envs": 64}


def test_bench_e3d_passes_dotted_overrides_into_its_config():
    import importlib.util
    import os
    from tests.conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_e3d", os.path.join(ROOT, "tools", "bench_e3d.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    args, ov, cfg = bench.parse_args(["--num-envs", "64", "--steps", "3", "algo.gauss_std=state", "algo.gauss_squash=tanh", "algo.log_std_min=-3"])
    assert (args.num_envs, args.steps) == (64, 3)
    assert ov == {"algo.gauss_std": "state", "algo.gauss_squash": "tanh", "algo.log_std_min": -3}
    assert (cfg.runtime.num_envs, cfg.runtime.env, cfg.algo.gauss_std, cfg.algo.gauss_squash, cfg.algo.log_std_min) == (64, "e3d", "state", "tanh", -3)
    _, ov, cfg = bench.parse_args([])
    assert ov == {} and cfg.runtime.num_envs == 2048 and "gauss_std" not in cfg.algo      # no override: cfg5 as it was


def test_check_policy_meta_names_the_mismatched_key():
    from types import SimpleNamespace
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    check = E3dMAPPO.check_policy_meta
    meta = dict(gauss_std="state", gauss_squash="tanh", log_std_min=-5.0, log_std_max=2.0)
    agent = lambda std, sq, lo=-5.0, hi=2.0: SimpleNamespace(gauss_std=std, gauss_squash=sq, log_std_min=lo, log_std_max=hi,
                                                               policy_ex=(std, sq) != ("param", "clip"))
    check(agent("state", "tanh"), meta, "f")                      # the same policy loads
    check(agent("param", "clip", -1.0, 1.0), None, "f")           # default files carry no entry; the default mode has no bounds
    for a, key in ((agent("param", "clip"), "algo.gauss_std"), (agent("state", "clip"), "algo.gauss_squash"),
                   (agent("state", "tanh", -4.0), "algo.log_std_min"), (agent("state", "tanh", hi=1.5), "algo.log_std_max")):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            check(a, meta, "f")
    with pytest.raises(ValueError, match=r"algo\.gauss_std"):
        check(agent("state", "tanh"), None, "f")


def test_gaussian_actor_parameters():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import GaussianActor
    torch.manual_seed(0)
    p = GaussianActor(16, 128, 3, 2, 128, -0.5)
    names = [k for k, _ in p.named_parameters()]
    trunk = ["shared_net.fc1.weight", "shared_net.fc1.bias", "shared_net.fc2.weight", "shared_net.fc2.bias"] + \
        [f"GRU.{w}_l{k}" for k in range(2) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + ["Mean.weight", "Mean.bias"]
    assert names == ["log_std"] + trunk and list(p.state_dict()) == names
    torch.manual_seed(0)
    q = GaussianActor(16, 128, 3, 2, 128, -0.5, gauss_std="param")
    assert list(q.state_dict()) == list(p.state_dict())
    for k, v in q.state_dict().items():
        assert torch.equal(v, p.state_dict()[k]), k
    torch.manual_seed(0)
    s = GaussianActor(16, 128, 3, 2, 128, -0.5, gauss_std="state")
    sn = [k for k, _ in s.named_parameters()]
    assert sn == trunk + ["LogStd.weight", "LogStd.bias"] and list(s.state_dict()) == sn
    assert torch.all(s.LogStd.weight == 0) and torch.all(s.LogStd.bias == -0.5)
    feat = torch.randn(7, 128)
    sigma = torch.exp(torch.nn.functional.linear(feat, s.LogStd.weight, s.LogStd.bias))
    assert torch.allclose(sigma, torch.exp(p.log_std.detach()).expand(7, 3))
    for k in trunk:        # the layers before LogStd draw the same numbers as in param mode
        assert torch.equal(dict(s.named_parameters())[k], dict(p.named_parameters())[k]), k
