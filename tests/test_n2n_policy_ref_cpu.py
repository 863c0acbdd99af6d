"""CPU checks of the env_n2n policy-kernel reference (tests/n2n_policy_ref.py) and of the cfg4_n2n wiring (config, `main --config
cfg4_n2n`, the learner's argument checks)."""
import numpy as np
import pytest

from tests import n2n_policy_ref as ref


@pytest.mark.parametrize("P,E", [(4, 1), (8, 2), (16, 4)])
def test_policy_inputs_reference_is_self_consistent(P, E):
    rng = np.random.default_rng(P * 10 + E)
    N = 64
    p, e, target, pp_in, pe_in = ref.random_records(rng, N, P, E)
    db = (rng.random(N) < 0.2).astype(np.uint8)
    out = ref.policy_inputs(p, e, pp_in, pe_in, db)
    live = out["live"].astype(bool)
    assert np.array_equal(live, (p[:, 4] != 0) & (db[:, None] == 0))
    assert not live[db == 1].any()
    assert np.all(out["p4"][~live] == 0) and np.all(out["e4"][e[:, 4] == 0] == 0)
    # rows of live pursuers: positions and velocity components, |(vx, vy)| = v
    np.testing.assert_allclose(out["p4"][..., 0][live], p[:, 0][live], rtol=1e-6)
    np.testing.assert_allclose(np.hypot(out["p4"][..., 2], out["p4"][..., 3])[live], p[:, 3][live], atol=1e-6)
    # e_ref: the first active evader, zeros when there is none
    for n in range(N):
        on = np.flatnonzero(e[n, 4] != 0)
        assert np.array_equal(out["e_ref"][n], out["e4"][n, on[0]] if on.size else np.zeros(4, np.float32))
    # adjacencies: the input where both ends are live / active, else zero
    assert np.all(out["pp_adj"] <= pp_in) and np.all(out["pe_adj"] <= pe_in)
    assert np.all(out["pp_adj"][~live] == 0) and np.all(out["pp_adj"].transpose(0, 2, 1)[~live] == 0)
    assert np.all(out["pe_adj"].transpose(0, 2, 1)[e[:, 4] == 0] == 0)


def test_policy_record_reference_is_self_consistent():
    rng = np.random.default_rng(3)
    N, P, E = 50, 8, 2
    acc = ref.new_accumulators(N)
    ret = np.zeros(N)
    for step in range(4):
        p, e, target, pp_in, pe_in = ref.random_records(rng, N, P, E)
        live = ref.policy_inputs(p, e, pp_in, pe_in, acc["done_before"])["live"]
        reward = rng.integers(-2, 3, (N, P)).astype(np.float32)
        done = (rng.random(N) < 0.1).astype(np.uint8)
        value = rng.standard_normal((N, P)).astype(np.float32)
        r, active, v, vz, new = ref.policy_record(p, e, target, reward, done, live, value, acc, 0.5)
        assert np.array_equal(active, live) and np.all(r[live == 0] == 0) and np.all(v[live == 0] == 0)
        ret += r.astype(np.float64).sum(-1)
        assert np.all(new["length"] == acc["length"] + (acc["done_before"] == 0))
        assert np.all(new["done_before"] >= acc["done_before"]) and np.all(new["ended"] >= acc["ended"])
        assert np.all(new["captured"] <= new["ended"])       # every evader captured is a reason to end
        assert np.all(vz[new["ended"] == 1]) and np.all(vz[p[:, 4] == 0])
        # an environment done before this step takes no further reward, length, capture or end
        old = acc["done_before"] == 1
        assert np.all(new["ret"][old] == acc["ret"][old]) and np.all(new["length"][old] == acc["length"][old])
        acc = new
    np.testing.assert_allclose(acc["ret"], ret, rtol=1e-6, atol=1e-5)


def test_cfg4_n2n_loads():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    cfg = baseline_config("cfg4_n2n")
    assert cfg.runtime.env == "n2n" and cfg.runtime.n2n_evader == "slsqp" and cfg.runtime.num_envs == 1024
    assert cfg.env.num_defender == 16 and cfg.env.num_evader == 1 and cfg.env.max_steps == 100
    assert cfg.algo.depth == 3 and cfg.algo.use_reward_norm is False
    assert cfg.env.state_dim == 4 and cfg.env.action_dim == 9 and cfg.algo.num_relation == 3
    cfg4 = baseline_config("cfg4")                                  # the pursuit stand-in is unchanged
    assert cfg4.runtime.get("env", "pursuit") == "pursuit" and cfg4.map.map_size == [64, 64] and cfg4.algo.use_reward_norm is True


def test_main_cfg4_n2n_routes_to_the_n2n_trainer(monkeypatch):
    from distributed_multi_agent_reinforcement_learning_amd import main as m
    calls = []
    monkeypatch.setattr(m, "train_n2n", lambda cfg, **kw: calls.append(("n2n", cfg, kw)))
    monkeypatch.setattr(m, "train_e3d", lambda cfg, **kw: calls.append(("e3d", cfg, kw)))
    monkeypatch.setattr(m, "train_agent_multiprocessing", lambda cfg, **kw: calls.append(("pursuit", cfg, kw)))
    m.main(["--config", "cfg4_n2n", "--iterations", "5", "runtime.num_envs=64"])
    assert len(calls) == 1 and calls[0][0] == "n2n"
    assert calls[0][1].runtime.num_envs == 64 and calls[0][2]["max_iterations"] == 5
    m.main(["--config", "cfg4", "--iterations", "1"])
    assert calls[-1][0] == "pursuit"
    m.main(["--config", "cfg5", "--iterations", "1"])
    assert calls[-1][0] == "e3d"


@pytest.mark.parametrize("ov,match", [({"algo.use_reward_norm": True}, "use_reward_norm"), ({"env.num_defender": 17}, "num_defender")])
def test_n2n_agent_rejects_unsupported_settings(ov, match):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO
    with pytest.raises(ValueError, match=match):
        N2nMAPPO(baseline_config("cfg4_n2n", **ov), 8, 1, device="cpu")
