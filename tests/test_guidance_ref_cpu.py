"""CPU checks of the scripted lead-pursuit pursuers: tests/guidance_ref.py -- the specification the kernels are held to in
tests/test_guidance_gpu.py -- against properties that need no device, a closed loop on the committed oracles, the shared GPU inputs,
and the parsing of the options."""
import numpy as np
import pytest

from tests import guidance_cases as gc
from tests import guidance_ref as ref

PI = np.pi


def _e3d(p_rows, e_row):
    """one environment from rows (x, y, z, phi, gamma, v, active) -> records p (1, 7, P), e (1, 7)"""
    return np.array(p_rows, np.float64).T[None], np.array(e_row, np.float64)[None]


def _n2n(p_rows, e_rows):
    """one environment from rows (x, y, phi, v, active) -> records p (1, 5, P), e (1, 5, E)"""
    return np.array(p_rows, np.float64).T[None], np.array(e_rows, np.float64).T[None]


# ---- the law ------------------------------------------------------------------------------------------------------------------------
def test_pure_pursuit_points_at_the_evader_3_4_5():
    """lead = 0 and no team-mate in range: the command is the line of sight.  r = (3, 4, 0), d = 5; r = (3, 0, 4) for the pitch."""
    p, e = _e3d([[1, 1, 1, 0.3, 0.2, 0.5, 1]], [4, 5, 1, 2.0, 0.5, 1.0, 1])
    a = ref.e3d_actions(p, e, 0.7, 0.0, 2.0, 1.0)[0, 0]
    assert abs(a[0] - 0.2951672353008665) <= 1e-15 and a[1] == 0.0 and a[2] == 1.0   # atan(4 / 3) / pi; g = (0.6, 0.8, 0) is rounded
    p, e = _e3d([[1, 1, 1, 0.3, 0.2, 0.5, 1]], [4, 1, 5, 2.0, 0.5, 1.0, 1])
    a = ref.e3d_actions(p, e, 0.7, 0.0, 2.0, 1.0)[0, 0]
    assert a[0] == 0.0 and abs(a[1] - 2 * 0.2951672353008665) <= 1e-15 and a[2] == 1.0
    g, on = ref.e3d_direction(p, e, 0.7, 0.0, 2.0, 1.0)
    assert on.all() and np.array_equal(g[0, :, 0], [0.6, 0.0, 0.8])
    # the plane: bearing atan2(4, 3) = 0.927 rad = 1.18 octants -> action 1 (heading pi / 4)
    p, e = _n2n([[1, 1, 0.0, 0.3, 1]], [[4, 5, 2.0, 1.0, 1]])
    a, b = ref.n2n_actions(p, e, 0.3, 0.0, 2.0, 1.0, with_bearing=True)
    assert a.dtype == np.int32 and a.tolist() == [[1]] and abs(b[0, 0] - np.arctan2(4.0, 3.0)) <= 1e-15


@pytest.mark.parametrize("lead", [0.0, 0.5, 1.0, 7.0])
def test_stationary_evader_gives_the_same_command_for_any_lead(lead):
    p, e = gc.records(*gc.e3d_case(8)[:2])
    e = e.copy(); e[:, 5] = 0.0
    assert np.array_equal(ref.e3d_actions(p, e, 0.7, lead, 2.0, 1.0), ref.e3d_actions(p, e, 0.7, 0.0, 2.0, 1.0))
    p, e = gc.records(*gc.n2n_case(16, 8)[:2])
    e = e.copy(); e[:, 3] = 0.0
    assert np.array_equal(ref.n2n_actions(p, e, 0.3, lead, 2.0, 1.0), ref.n2n_actions(p, e, 0.3, 0.0, 2.0, 1.0))


def test_lead_time_is_capped_by_distance_and_by_the_parameter():
    """t = min(d / p_vmax, lead): evader at distance 5 flying along +y at speed 1.  p_vmax 0.5: d / p_vmax = 10 > lead = 2, aim = r + 2 e_vel;
    p_vmax 10: d / p_vmax = 0.5 < lead, aim = r + 0.5 e_vel."""
    assert ref.lead_time(np.array([5.0, 5.0, 0.0]), np.array([0.5, 10.0, 0.0]), 2.0).tolist() == [2.0, 0.5, 2.0]   # (0 / 0 takes the cap)
    p, e = _e3d([[0, 0, 0, 0, 0, 0, 1]], [5, 0, 0, PI / 2, 0.0, 1.0, 1])
    for p_vmax, t in ((0.5, 2.0), (10.0, 0.5)):
        a = ref.e3d_actions(p, e, p_vmax, 2.0, 2.0, 1.0)[0, 0]
        assert abs(a[0] - np.arctan2(t, 5.0) / PI) <= 1e-15 and abs(a[1]) <= 1e-15 and a[2] == 1.0
    p, e = _n2n([[0, 0, 0, 0.3, 1]], [[5, 0, PI / 2, 1.0, 1]])
    for p_vmax, t in ((0.5, 2.0), (10.0, 0.5)):
        b = ref.n2n_actions(p, e, p_vmax, 2.0, 2.0, 1.0, with_bearing=True)[1][0, 0]
        assert abs(b - np.arctan2(t, 5.0)) <= 1e-15


def test_two_close_pursuers_repel_each_other_mirrored():
    pos = np.array([[[0.0, 1.0, 9.0], [0.0, 0.5, 9.0], [0.0, 0.25, 9.0]]])      # (1, 3, P = 3): 0 and 1 are 1.1456 apart, 2 is far
    on = np.ones((1, 3), bool)
    t0, u0 = ref.separation_from(pos, on, 0, 2.0, 1.5)                           # what pursuer 0 adds to the others
    t1, u1 = ref.separation_from(pos, on, 1, 2.0, 1.5)
    assert u0.tolist() == [[False, True, False]] and u1.tolist() == [[True, False, False]]
    assert np.array_equal(t0[0, :, 1], -t1[0, :, 0]) and np.abs(t0[0, :, 1]).max() > 0
    d = np.sqrt(1.0 + 0.25 + 0.0625)
    want = 1.5 * np.array([1.0, 0.5, 0.25]) / d * (2.0 - d) / 2.0                # pushes 1 away from 0, weight falling to 0 at sep_range
    assert np.allclose(t0[0, :, 1], want, rtol=0, atol=1e-15)
    # and through the whole law: with the evader straight ahead of both, the commands are mirror images about the line of sight
    p, e = _e3d([[0, -0.5, 0, 0, 0, 0, 1], [0, 0.5, 0, 0, 0, 0, 1]], [10, 0, 0, 0, 0, 0, 1])
    a = ref.e3d_actions(p, e, 0.7, 0.0, 2.0, 1.0)[0]
    assert a[0, 0] == -a[1, 0] and a[0, 0] < 0 < a[1, 0] and a[0, 1] == a[1, 1] == 0.0
    los = ref.e3d_actions(p, e, 0.7, 0.0, 2.0, 0.0)[0, :, 0]                     # gain 0: the line of sight
    assert np.abs(los - np.arctan2([0.5, -0.5], 10.0) / PI).max() <= 1e-15 and np.all(np.abs(a[:, 0]) > np.abs(los))


def test_team_mates_at_distance_zero_or_beyond_the_range_add_nothing():
    pos = np.array([[[0.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0]]])   # 1 on top of 0, 2 at exactly sep_range, 3 inside
    on = np.array([[True, True, True, False]])
    term, use = ref.separation_from(pos, on, 0, 2.0, 1.0)
    assert use.tolist() == [[False, False, False, True]] and np.all(term[0, :, :3] == 0.0) and np.isfinite(term).all()
    for j in (1, 2):                       # distance 0 and distance == sep_range: nobody is pushed by them ... except 3 (inside of 1)
        assert not ref.separation_from(pos, on, j, 2.0, 1.0)[1][0, :3].any()
    assert not ref.separation_from(pos, on, 3, 2.0, 1.0)[1].any()          # an inactive team-mate pushes nobody
    # sep_range 0 switches the term off without dividing by it
    p, e = gc.records(*gc.e3d_case(9)[:2])
    with np.errstate(all="raise"):
        a = ref.e3d_actions(p, e, 0.7, 1.0, 0.0, 1.0)
    assert np.array_equal(a, ref.e3d_actions(p, e, 0.7, 1.0, 2.0, 0.0)) and not np.array_equal(a, ref.e3d_actions(p, e, 0.7, 1.0, 2.0, 1.0))


def test_inactive_pursuer_and_inactive_evader_hold():
    p, e = _e3d([[1, 1, 1, 0.3, -0.2, 0.5, 1], [1000, 1000, 1000, 0, 0, 0, 0], [3, 3, 3, -2.0, 1.0, 0.7, 1]], [4, 5, 1, 2.0, 0.5, 1.0, 1])
    a = ref.e3d_actions(p, e, 0.7, 1.0, 2.0, 1.0)[0]
    assert a[1].tolist() == [0.0, 0.0, -1.0] and a[0, 2] == a[2, 2] == 1.0
    e[0, 6] = 0.0
    a = ref.e3d_actions(p, e, 0.7, 1.0, 2.0, 1.0)[0]
    assert np.array_equal(a, [[0.3 / PI, -0.2 / (PI / 2), -1.0], [0.0, 0.0, -1.0], [-2.0 / PI, 1.0 / (PI / 2), -1.0]])
    assert ref.hold_rows_e3d(p, e, 0.7, 1.0, 2.0, 1.0).all()
    # g exactly 0 (the pursuer sits on a stationary evader): hold as well
    p, e = _e3d([[4, 5, 1, 0.3, -0.2, 0.5, 1]], [4, 5, 1, 2.0, 0.5, 0.0, 1])
    assert ref.e3d_actions(p, e, 0.7, 1.0, 2.0, 1.0)[0, 0].tolist() == [0.3 / PI, -0.2 / (PI / 2), -1.0]
    p, e = _n2n([[1, 1, 0.5, 0.3, 1], [1000, 1000, 0, 0, 0]], [[4, 5, 2.0, 1.0, 1], [7, 7, 1.0, 1.0, 0]])
    assert ref.n2n_actions(p, e, 0.3, 1.0, 2.0, 1.0).tolist() == [[1, 0]]
    e[0, 4, 0] = 0.0                                                    # no evader left
    assert ref.n2n_actions(p, e, 0.3, 1.0, 2.0, 1.0).tolist() == [[0, 0]]


def test_a_parked_evader_is_never_chosen_while_an_active_one_exists():
    p, e = _n2n([[999, 999, 0, 0.3, 1], [1, 1, 0, 0.3, 1]], [[1000, 1000, 0, 0, 0], [4, 5, 0, 0.0, 1], [1000, 1000, 0, 0, 0]])
    g, on, k = ref.n2n_direction(p, e, 0.3, 0.0, 2.0, 1.0)
    assert on.all() and k.tolist() == [[1, 1]]                          # even for the pursuer a step away from the parked ones
    assert ref.n2n_actions(p, e, 0.3, 0.0, 2.0, 1.0).tolist() == [[ref.octant(np.arctan2(5.0 - 999, 4.0 - 999)), 1]]
    # ties go to the lowest index
    p, e = _n2n([[0, 0, 0, 0.3, 1]], [[0, 3, 0, 0, 1], [3, 0, 0, 0, 1], [0, -3, 0, 0, 1]])
    assert ref.n2n_direction(p, e, 0.3, 0.0, 2.0, 1.0)[2].tolist() == [[0]]
    for P, E in gc.N2N_PE:                                              # ... and on the GPU inputs
        p, e = gc.records(*gc.n2n_case(P, E)[:2])
        g, on, k = ref.n2n_direction(p, e, 0.3, 1.0, 2.0, 1.0)
        chosen_on = np.take_along_axis(e[:, 4], k, -1) != 0
        assert np.array_equal(chosen_on, np.broadcast_to((e[:, 4] != 0).any(-1)[:, None], k.shape))


def test_octant_mapping():
    k = np.arange(1, 9)
    centres = ref.action_heading(k)                                     # pi/4, pi/2, 3pi/4, pi, -3pi/4, -pi/2, -pi/4, 0
    assert np.array_equal(centres[:4], k[:4] * PI / 4) and np.array_equal(centres[4:], k[4:] * PI / 4 - 2 * PI)
    assert ref.octant(centres).tolist() == k.tolist()
    for eps in (-0.3, 0.3):                                             # anywhere inside the octant
        assert ref.octant(np.arctan2(np.sin(centres + eps), np.cos(centres + eps))).tolist() == k.tolist()
    assert ref.octant(PI) == 4 and ref.octant(-PI) == 4                 # both signs of pi are the same heading
    assert ref.octant(0.0) == 8 and ref.octant(-0.0) == 8 and ref.octant(-2 * PI) == 8 and ref.octant(2 * PI) == 8   # k = 0, -8, 8 -> 8
    assert ref.octant(-PI / 4) == 7 and ref.octant(-3 * PI / 4) == 5
    assert ref.octant(np.linspace(-PI, PI, 1001)).min() == 1 and ref.octant(np.linspace(-PI, PI, 1001)).max() == 8
    b = np.array([PI / 8, PI / 8 + 5e-10, PI / 8 + 2e-9, -3 * PI / 8 - 5e-10, 0.1, np.nan])
    assert ref.near_octant_boundary(b).tolist() == [True, True, False, True, False, False]


# ---- closed loop on the committed oracles ---------------------------------------------------------------------------------------------
def test_a_lone_faster_pursuer_closes_in_on_env_3d():
    """the oracle's env_3d stepped with the reference's actions for 30 steps: a lone pursuer (p_vmax 0.7) against an evader (e_vmax 0.3)
    on a fixed straight command never loses ground"""
    from oracle import e3d_oracle as eo
    cfg = eo.make_cfg(1, 200, e_vmax=0.3)
    p0 = np.array([[5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.0]])
    e0 = np.array([14.0, 9.0, 8.0, 0.3, 0.1, 0.0, 1.0])
    r = e0[:3] - p0[0, :3]
    p0[0, 3], p0[0, 4] = np.arctan2(r[1], r[0]), np.arctan2(r[2], np.hypot(r[0], r[1]))
    oe = eo.OracleE3d(cfg, p0, e0, np.array([100.0, 100.0, 100.0]))
    cmd = np.array([0.3 / PI, 0.1 / (PI / 2), 1.0])
    dist = [np.linalg.norm(oe.e[0, :3] - oe.p[0, :3])]
    for _ in range(30):
        a = ref.e3d_actions(oe.p.T[None], oe.e, cfg.p_vmax, *ref.default_params(cfg.kill_radius))[0]
        assert a.shape == (1, 3) and a[0, 2] == 1.0
        oe.evader_step(cmd)
        oe.step(a)
        assert oe.e[0, 6] == 1.0 and oe.p[0, 6] == 1.0
        dist.append(np.linalg.norm(oe.e[0, :3] - oe.p[0, :3]))
    assert np.all(np.diff(dist) <= 0.0) and dist[-1] < dist[0] - 4.0, dist


def test_a_lone_faster_pursuer_closes_in_on_env_n2n():
    """the same on the oracle's env_n2n (p_vmax 0.3, evader speed 0.2, headings in octants)"""
    from oracle import n2n_oracle as no
    cfg = no.make_cfg(1, 1, 100, e_vmax=0.2)
    p0 = np.array([[5.0, 5.0, PI / 4, 0.0, 1.0]])
    e0 = np.array([[12.0, 11.0, 0.4, 0.2, 1.0]])
    oe = no.OracleN2n(cfg, p0, e0, np.array([100.0, 100.0]))
    cmd = np.array([0.4 / PI])
    dist = [np.linalg.norm(oe.e[0, :2] - oe.p[0, :2])]
    for _ in range(30):
        a = ref.n2n_actions(oe.p.T[None], oe.e.T[None], cfg.p_vmax, *ref.default_params(cfg.kill_radius))[0]
        assert a.dtype == np.int32 and 1 <= a[0] <= 8
        oe.evader_step(cmd)
        oe.step(a)
        assert oe.e[0, 4] == 1.0 and oe.p[0, 4] == 1.0
        dist.append(np.linalg.norm(oe.e[0, :2] - oe.p[0, :2]))
    assert np.all(np.diff(dist) <= 0.0) and dist[-1] < dist[0] - 1.0, dist


# ---- the inputs of the GPU test -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", gc.E3D_P)
def test_e3d_gpu_inputs_hold_the_forced_cases(P):
    p, e = gc.records(*gc.e3d_case(P)[:2])
    for lead, sr, gain in gc.PARAMS:
        a = ref.e3d_actions(p, e, gc.E3D_P_VMAX, lead, sr, gain)
        hold = ref.hold_rows_e3d(p, e, gc.E3D_P_VMAX, lead, sr, gain)
        assert a.shape == (gc.N, P, 3) and np.abs(a).max() <= 1.0
        assert hold[2].all() and hold[1, 0] and hold[3, P - 1] and hold[4, P - 1] and hold.sum() == P + 3
        assert np.all(a[hold][:, 2] == -1.0) and np.all(a[~hold][:, 2] == 1.0)
    pos, on = p[:, :3], p[:, 6] != 0
    used = [ref.separation_from(pos, on, j, 2.0, 1.0)[1] for j in range(P)]
    assert used[0][0, 1] and used[1][0, 0] and used[0][4, 1] and not used[P - 1][4].any()   # the close pairs push, the inactive one does not
    assert not np.array_equal(ref.e3d_actions(p, e, gc.E3D_P_VMAX, 1.0, 2.0, 1.0), ref.e3d_actions(p, e, gc.E3D_P_VMAX, 0.0, 2.0, 1.0))


@pytest.mark.parametrize("P,E", gc.N2N_PE)
def test_n2n_gpu_inputs_hold_the_forced_cases_and_touch_no_octant_boundary(P, E):
    p, e = gc.records(*gc.n2n_case(P, E)[:2])
    for lead, sr, gain in gc.PARAMS:
        a, b = ref.n2n_actions(p, e, gc.N2N_P_VMAX, lead, sr, gain, with_bearing=True)
        assert a.shape == (gc.N, P) and a.dtype == np.int32 and a.min() == 0 and a.max() <= 8
        assert np.all(a[2] == 0) and a[1, 0] == 0 and a[3, P - 1] == 0 and a[4, P - 1] == 0 and (a == 0).sum() == P + 3
        assert not ref.near_octant_boundary(b).any()                    # the reference alone leaves no row out of the GPU comparison
    assert len(np.unique(ref.n2n_actions(p, e, gc.N2N_P_VMAX, 1.0, 2.0, 1.0))) >= (5 if P > 3 else 3)


# ---- options --------------------------------------------------------------------------------------------------------------------------
def _agents():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO
    return (("cfg5", E3dMAPPO), ("cfg4_n2n", N2nMAPPO))


def test_options_parse_and_default():
    from distributed_multi_agent_reinforcement_learning_amd import guidance as gd
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config, load_config, parse_overrides
    assert not any(k.startswith("guidance") or k == "eval_baseline" for k in load_config().runtime)   # config.yaml stays as it is
    for name in ("cfg5", "cfg4_n2n"):
        assert gd.guidance_options(baseline_config(name)) == (1.0, None, 1.0) and gd.eval_baseline_options(baseline_config(name)) is None
        ov = parse_overrides(["runtime.guidance_lead=0", "runtime.guidance_sep_range=3", "runtime.guidance_sep_gain=0.5", "runtime.eval_baseline=guidance"])
        assert gd.guidance_options(baseline_config(name, **ov)) == (0.0, 3.0, 0.5)
        assert gd.eval_baseline_options(baseline_config(name, **ov)) == "guidance"
    assert ref.default_params(0.5) == (gd.DEFAULT_LEAD, gd.DEFAULT_SEP_KILL_RADII * 0.5, gd.DEFAULT_SEP_GAIN) == (1.0, 2.0, 1.0)


@pytest.mark.parametrize("key", ["guidance_lead", "guidance_sep_range", "guidance_sep_gain"])
@pytest.mark.parametrize("value", [-0.1, float("inf"), float("nan"), "far"])
def test_bad_parameters_raise_on_both_agents_naming_the_key(key, value):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    for name, Agent in _agents():
        with pytest.raises(ValueError, match="runtime." + key):
            Agent(baseline_config(name, **{"runtime." + key: value}), 8, 1, device="cpu")   # raised before the device check


def test_bad_baseline_and_policy_raise():
    from distributed_multi_agent_reinforcement_learning_amd import guidance as gd
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    for name in ("cfg5", "cfg4_n2n"):
        with pytest.raises(ValueError, match="runtime.eval_baseline"):
            gd.eval_baseline_options(baseline_config(name, **{"runtime.eval_baseline": "pso"}))
    gd.check_policy("network", {}), gd.check_policy("network", None), gd.check_policy("guidance", None)
    with pytest.raises(ValueError, match="guidance"):
        gd.check_policy("guidance", {"r": None})
    with pytest.raises(ValueError, match="policy"):
        gd.check_policy("pso", None)


def test_baseline_flag_is_refused_on_the_pursuit_configs(capsys):
    from distributed_multi_agent_reinforcement_learning_amd import main as cli
    for name in ("cfg1", "cfg3"):
        with pytest.raises(SystemExit):
            cli.main(["--config", name, "--baseline", "guidance"])
        assert "--baseline" in capsys.readouterr().err
