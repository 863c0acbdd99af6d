"""CPU checks of algo.reward_shaping: tests/shaping_ref.py over the recorded env_3d / env_n2n traces and a synthetic episode -- the
telescoping identity that makes the shaping policy-invariant and the terminal rule -- and the parsing of the options."""
import os

import numpy as np
import pytest

from tests import evader_cases as ec
from tests import shaping_ref as ref

GAMMA, COEF = 0.99, 0.1
TRACES = ec.e3d_trace_files() + ec.n2n_trace_files()


def _trace(path):
    """a recorded episode as shaping_ref.episode takes it (N = 1): the states every step starts from plus the final one"""
    d = np.load(path)
    T, limit = len(d["done"]), int(d["meta"][3])
    p = np.concatenate([d["p"], d["p_end"][None]]).transpose(0, 2, 1)[None]       # (1, T + 1, C, P)
    e = np.concatenate([d["e"], d["e_end"][None]]).transpose(0, 2, 1)[None]
    assert np.array_equal(d["p"][0], d["p0"]) and np.array_equal(p[0, 1:, -1, :] != 0, d["active"] != 0)
    kill = float(d["cfg"][4])
    ended = np.array([ref.ended_after(p[:, t + 1], e[:, t + 1], d["target"][None], kill)[0] for t in range(T)])
    ended = np.logical_or.accumulate(ended)[None]
    done = (d["done"] != 0)[None]
    assert done[0, -1] and not done[0, :-1].any() and np.array_equal(ended[0], done[0] & (ended[0] | (T < limit)))
    return dict(p=p, e=e, raw=d["reward"].astype(np.float32)[None], done=done, ended=ended, T=T, limit=limit)


def _synthetic():
    """two env_n2n-shaped environments (P = 3, E = 2, limit 12).  0: pursuer 1 dies in step 4, evader 0 is captured in step 6, evader 1
    in step 9: the episode ends by capture after 10 steps.  1: pursuer 2 dies in step 3, the episode runs into the time limit."""
    rng = np.random.RandomState(5)
    N, T, P, E = 2, 12, 3, 2
    p, e = np.zeros((N, T + 1, 5, P)), np.zeros((N, T + 1, 5, E))
    p[:, 0, :2], e[:, 0, :2] = rng.uniform(0, 20, (N, 2, P)), rng.uniform(0, 20, (N, 2, E))
    p[:, :, 4], e[:, :, 4] = 1.0, 1.0
    for t in range(T):
        p[:, t + 1, :2] = p[:, t, :2] + rng.uniform(-0.3, 0.3, (N, 2, P))
        e[:, t + 1, :2] = e[:, t, :2] + rng.uniform(-0.5, 0.5, (N, 2, E))
    def park(a, n, t, k):          # inactive from the state after step t on: parked at (1000, 1000) as the environments do
        a[n, t + 1:, :, k] = 0.0
        a[n, t + 1:, :2, k] = 1000.0
    park(p, 0, 4, 1); park(e, 0, 6, 0); park(e, 0, 9, 1); park(p, 1, 3, 2)
    raw = np.zeros((N, T, P), np.float32)
    raw[0, 6, 0] = raw[0, 9, 2] = 1.0
    raw[0, 4, 1] = raw[1, 3, 2] = -1.0
    done, ended = np.zeros((N, T), bool), np.zeros((N, T), bool)
    done[0, 9:] = ended[0, 9:] = True
    done[1, T - 1] = True
    return dict(p=p, e=e, raw=raw, done=done, ended=ended, T=T, limit=T)


def test_traces_are_the_recorded_ones():
    assert len(ec.e3d_trace_files()) >= 6 and len(ec.n2n_trace_files()) >= 7
    kinds = [(_trace(f)["ended"][0, -1], _trace(f)["p"].shape[2]) for f in TRACES]
    assert {c for _, c in kinds} == {5, 7} and any(k for k, _ in kinds)


@pytest.mark.parametrize("coef", [COEF, 1.0])
@pytest.mark.parametrize("path", TRACES + ["synthetic"], ids=lambda p: os.path.basename(p)[:-4] if p.endswith(".npz") else p)
def test_shaping_telescopes_over_every_live_span(path, coef):
    """policy invariance: sum_t gamma^t F_t over a pursuer's live span of L steps == gamma^L Phi_next(last) - Phi(s_0).  At most 200
    f64 terms of magnitude <= coef * 35 round to about 1e-12; 1e-9 absolute leaves three orders of margin."""
    s = _synthetic() if path == "synthetic" else _trace(path)
    ep = ref.episode(s["p"], s["e"], s["raw"], s["done"], s["ended"], coef, GAMMA)
    lhs, rhs, L = ref.telescoped(ep, GAMMA)
    assert L.max() > 0 and np.abs(ep["F"]).max() > 0
    assert np.abs(ep["phi0"]).max() <= coef * 35
    err = np.abs(lhs - rhs).max()
    print(f"{os.path.basename(path)} coef {coef}: live spans {L.min()}..{L.max()}, max |sum - closed form| {err:.2e}")
    assert err <= 1e-9
    # the shaped reward is the raw one plus F on live rows, the raw one elsewhere
    live = ep["live"].astype(np.float64)
    assert np.array_equal(ep["x"], s["raw"].astype(np.float64) + ep["F"] * live)
    assert np.array_equal(ref.buffer_reward(ep["x"], ep["live"])[ep["live"] == 0], np.zeros(int((ep["live"] == 0).sum()), np.float32))


@pytest.mark.parametrize("path", TRACES + ["synthetic"], ids=lambda p: os.path.basename(p)[:-4] if p.endswith(".npz") else p)
def test_terminal_rule(path):
    """Phi_next is exactly 0 where the pursuer is inactive after the step and where the episode ended for a reason other than the
    time limit; a time-limit ending keeps it"""
    s = _synthetic() if path == "synthetic" else _trace(path)
    ep = ref.episode(s["p"], s["e"], s["raw"], s["done"], s["ended"], COEF, GAMMA)
    T = s["T"]
    p_on_after = s["p"][:, 1:, -1, :] != 0
    assert np.all(ep["phi_next"][~p_on_after] == 0.0)
    assert np.all(ep["phi_next"][s["ended"]] == 0.0)
    for n in range(len(s["p"])):
        t = int(np.argmax(s["done"][n]))                       # the episode's last step
        if s["ended"][n, t]:
            assert np.all(ep["phi_next"][n, t] == 0.0)
            continue
        assert t == s["limit"] - 1                             # done without an ending: the time limit
        want = ref.potential(s["p"][n:n + 1, t + 1], s["e"][n:n + 1, t + 1], COEF)[0]
        assert np.array_equal(ep["phi_next"][n, t], want) and np.any(want[p_on_after[n, t]] < 0)
    # before the end every live pursuer that stays active carries the potential of the next state
    keep = p_on_after & ~s["ended"][:, :, None] & ~ep["done_before"][:, :, None]
    nxt = np.stack([ref.potential(s["p"][:, t + 1], s["e"][:, t + 1], COEF) for t in range(T)], 1)
    assert np.array_equal(ep["phi_next"][keep], nxt[keep])


def test_synthetic_episode_has_the_three_cases():
    s = _synthetic()
    ep = ref.episode(s["p"], s["e"], s["raw"], s["done"], s["ended"], COEF, GAMMA)
    L = ref.telescoped(ep, GAMMA)[2]
    assert L.tolist() == [[10, 5, 10], [12, 12, 4]]
    assert s["ended"][0, 9] and not s["ended"][1].any() and s["done"][1, 11]          # a capture ending, a time-limit ending
    assert np.all(ep["phi_next"][0, 9] == 0) and np.all(ep["phi_next"][1, 11, :2] < 0)
    assert ep["phi_next"][0, 4, 1] == 0 and ep["F"][0, 4, 1] == -ep["phi_next"][0, 3, 1]  # a death pays back the carried potential
    # with evader 0 parked at (1000, 1000) the nearest ACTIVE evader is evader 1
    d1 = np.sqrt(((s["p"][0, 8, :2, 0] - s["e"][0, 8, :2, 1]) ** 2).sum())
    assert abs(ref.potential(s["p"][:1, 8], s["e"][:1, 8], COEF)[0, 0] + COEF * d1) <= 1e-15
    # environments done before a step are not touched
    assert np.all(ep["F"][0, 10:] * ep["live"][0, 10:] == 0) and np.array_equal(ep["x"][0, 10:], s["raw"][0, 10:].astype(np.float64))


def test_potential_edge_cases():
    p = np.zeros((1, 7, 2)); e = np.zeros((1, 7))
    p[0, :3, 0], p[0, :3, 1], p[0, 6] = (1, 2, 2), (1000, 1000, 1000), (1, 0)
    e[0, 6] = 1
    assert ref.potential(p, e, 0.5).tolist() == [[-1.5, 0.0]]
    e[0, 6] = 0
    assert ref.potential(p, e, 0.5).tolist() == [[0.0, 0.0]]


# ---- options ------------------------------------------------------------------------------------------------------------------------
def test_options_parse_and_default_to_off():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config, load_config, parse_overrides
    from distributed_multi_agent_reinforcement_learning_amd.reward_shaping import reward_shaping_options
    assert "reward_shaping" not in load_config().algo and "shaping_coef" not in load_config().algo     # config.yaml stays as it is
    for name in ("cfg5", "cfg4_n2n"):
        assert reward_shaping_options(baseline_config(name)) == ("none", 0.1)
        ov = parse_overrides(["algo.reward_shaping=distance", "algo.shaping_coef=0.25"])
        assert ov == {"algo.reward_shaping": "distance", "algo.shaping_coef": 0.25}
        assert reward_shaping_options(baseline_config(name, **ov)) == ("distance", 0.25)
        assert reward_shaping_options(baseline_config(name, **parse_overrides(["algo.reward_shaping=none"]))) == ("none", 0.1)


def _agents():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO
    return (("cfg5", E3dMAPPO), ("cfg4_n2n", N2nMAPPO))


@pytest.mark.parametrize("mode", ["dist", "potential", "True", ""])
def test_unknown_mode_raises_on_both_agents(mode):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    for name, Agent in _agents():
        with pytest.raises(ValueError, match="algo.reward_shaping"):
            Agent(baseline_config(name, **{"algo.reward_shaping": mode}), 8, 1, device="cpu")   # raised before the device check


@pytest.mark.parametrize("coef", [0.0, -0.1, float("inf"), float("nan")])
@pytest.mark.parametrize("mode", ["none", "distance"])
def test_bad_coefficient_raises_on_both_agents(coef, mode):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    for name, Agent in _agents():
        with pytest.raises(ValueError, match="algo.shaping_coef"):
            Agent(baseline_config(name, **{"algo.reward_shaping": mode, "algo.shaping_coef": coef}), 8, 1, device="cpu")


def test_pursuit_refuses_the_option():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
    with pytest.raises(ValueError, match="algo.reward_shaping"):
        MAPPO(baseline_config("cfg1", **{"algo.reward_shaping": "distance"}), 4, 2, "Learner")
