"""CPU checks of algo.use_reward_scaling: tests/reward_scale_ref.py reproduces the reference's RewardScaling fixture bit for bit,
masked lockstep ticks leave the state untouched, and the option is parsed / refused where it should be."""
import os

import numpy as np
import pytest

from tests import reward_scale_ref as ref
from tests.conftest import GOLDEN

KINDS = ("n2n", "e3d", "syn")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "reward_scaling.npz"))


def test_fixture_is_what_the_issue_describes(gold):
    assert float(gold["gamma"]) == 0.99
    assert gold["n2n_x"].shape[1] == 16 and gold["e3d_x"].shape[1] == 8 and gold["syn_x"].shape == (240, 8)
    assert int(gold["syn_start"].sum()) == 6 and gold["syn_x"][0].min() < 0     # the first-sample quirk is in the fixture
    for k in KINDS:
        assert np.isfinite(gold[k + "_y"]).all() and np.any(gold[k + "_y"] != 0) and gold[k + "_start"][0] == 1
    # the quirk itself: at n == 1 the std is R = x, so a first reward of -1 comes out positive
    first = gold["syn_x"][0]
    assert np.all(gold["syn_y"][0][first < 0] > 0)


@pytest.mark.parametrize("kind", KINDS)
def test_reference_restatement_is_bit_exact(gold, kind):
    s = ref.Stream(gold, kind)
    state = ref.new_state(1, s.P)
    live = np.ones((1, s.P), np.float32)
    for a, b in s.episodes:
        ref.reset(state, s.P)
        for t in range(a, b):
            r = ref.step(state, s.x[t][None], live, np.zeros(1, bool), float(gold["gamma"]))
            assert np.array_equal(r[0].view(np.uint32), s.y[t].astype(np.float32).view(np.uint32)), (kind, t)
    assert np.array_equal(state[0].view(np.uint64), s.final.view(np.uint64))


def test_masked_ticks_leave_the_state_untouched(gold):
    """three environments in lockstep on the syn stream: 0 runs every episode to its end, 1 is done after 7 steps of each, 2 is done
    from the start; inactive pursuers (live 0) still feed their reward to the state and get r = 0"""
    s = ref.Stream(gold, "syn")
    g, P = float(gold["gamma"]), s.P
    state, solo = ref.new_state(3, P), ref.new_state(1, P)
    live = np.ones((3, P), np.float32)
    live[:, 5] = 0
    for a, b in s.episodes:
        ref.reset(state, P); ref.reset(solo, P)
        for t in range(a, b):
            db = np.array([False, t - a >= 7, True])
            before = state.copy()
            x = np.repeat(s.x[t][None], 3, 0)
            r = ref.step(state, x, live, db, g)
            assert np.array_equal(state[db], before[db])
            assert np.all(r[:, 5] == 0)
            assert np.array_equal(r[0, :5], s.y[t].astype(np.float32)[:5])
            if t - a < 7:
                want = ref.step(solo, s.x[t][None], live[:1], np.zeros(1, bool), g)
                assert np.array_equal(r[1], want[0])
            else:
                assert np.array_equal(r[1], x[1].astype(np.float32) * live[1])
    assert np.array_equal(state[0], s.final) and np.array_equal(state[1], solo[0]) and not state[2].any()
    assert state[1, 0] == 7 * len(s.episodes)


def test_rollout_helper_matches_stepwise(gold):
    s = ref.Stream(gold, "syn")
    a, b = s.episodes[0]
    raw = np.stack([s.x[a:b], s.x[a:b][::-1]])
    live = np.ones_like(raw, dtype=np.float32)
    st = ref.new_state(2, s.P)
    out = ref.rollout(st, raw, live, np.array([b - a, 5]), 0.99)
    assert np.array_equal(out[0], s.y[a:b].astype(np.float32)) and st[1, 0] == 5 and np.all(out[1, 5:] == raw[1, 5:].astype(np.float32))


def test_option_parses_and_defaults_to_off():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config, load_config, parse_overrides
    assert "use_reward_scaling" not in load_config().algo          # config.yaml and its schema stay as they are
    for name in ("cfg5", "cfg4_n2n"):
        assert bool(baseline_config(name).algo.get("use_reward_scaling", False)) is False
        ov = parse_overrides(["algo.use_reward_scaling=True"])
        assert ov == {"algo.use_reward_scaling": True}
        assert baseline_config(name, **ov).algo.use_reward_scaling is True


def test_pursuit_refuses_the_option():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
    with pytest.raises(ValueError, match="algo.use_reward_scaling"):
        MAPPO(baseline_config("cfg1", **{"algo.use_reward_scaling": True}), 4, 2, "Learner")


@pytest.mark.parametrize("scaling", [False, True])
def test_reward_norm_still_raises_on_both_agents(scaling):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO
    ov = {"algo.use_reward_norm": True, "algo.use_reward_scaling": scaling}
    with pytest.raises(ValueError, match="use_reward_norm"):
        E3dMAPPO(baseline_config("cfg5", **ov), 8, 1)
    with pytest.raises(ValueError, match="use_reward_norm"):
        N2nMAPPO(baseline_config("cfg4_n2n", **ov), 8, 1)
