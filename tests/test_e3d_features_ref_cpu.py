"""CPU checks of env_3d's line-of-sight policy features: tests/e3d_features_ref.py -- the specification the kernel is held to in
tests/test_e3d_features_gpu.py -- on hand cases, its link to the scripted pursuers' law (tests/guidance_ref.py), the host entry
e3d_pursuit_features_host against it, the shared GPU inputs, and the parsing of the options."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import e3d_features_cases as fc
from tests import e3d_features_ref as ref
from tests import guidance_ref

CFG = fc.CFG
MODES = ref.EVADER_OBS


def _case(p_rows, e_row, target=(10, 10, 10), t=0, pp=None, pe=None):
    """one environment from rows (x, y, z, phi, gamma, v, active); pp defaults to all ones, pe to all ones"""
    p = np.array(p_rows, np.float64).T[None]
    P = p.shape[2]
    pp = np.ones((1, P, P), np.float32) if pp is None else np.array(pp, np.float32).reshape(1, P, P)
    pe = np.ones((1, P), np.float32) if pe is None else np.array(pe, np.float32).reshape(1, P)
    return dict(p=p, e=np.array(e_row, np.float64)[None], target=np.array(target, np.float64)[None], time_step=np.array([t], np.int32), pp_adj=pp, pe_adj=pe)


def _ref(c, mode="sensed", cfg=CFG):
    return ref.pursuit_features(cfg, c["p"], c["e"], c["target"], c["time_step"], c["pp_adj"], c["pe_adj"], mode)


# ---- the law, by hand ---------------------------------------------------------------------------------------------------------------
def test_line_of_sight_3_4_5():
    """r = (3, 4, 0), d = 5: columns 7-9 = (0.6, 0.8, 0) and column 10 = 5 / 20; r = (3, 0, 4) for the third component"""
    a, c = _ref(_case([[1, 1, 1, 0.3, 0.2, 0.5, 1]], [4, 5, 1, 2.0, 0.5, 1.0, 1]))
    want = np.array([0.6, 0.8, 0.0, 0.25], np.float64).astype(np.float32)
    assert np.array_equal(a[0, 0, 7:11], want) and np.array_equal(c[0, 0, 7:11], want)
    a, _ = _ref(_case([[1, 1, 1, 0.3, 0.2, 0.5, 1]], [4, 1, 5, 2.0, 0.5, 1.0, 1]))
    assert np.array_equal(a[0, 0, 7:11], np.array([0.6, 0.0, 0.8, 0.25], np.float64).astype(np.float32))


def test_own_columns_and_the_clock():
    a, c = _ref(_case([[5, 10, 20, 0.0, 0.0, 0.35, 1]], [4, 5, 1, 0, 0, 0, 1], t=50))
    assert np.array_equal(a[0, 0, :7], np.array([-0.5, 0.0, 1.0, 1.0, 0.0, 0.0, 0.5], np.float32))
    assert a[0, 0, 31] == np.float32(0.25) and a[0, 0, 30] == 0.0
    assert np.array_equal(a[0, 0, :7], c[0, 0, :7])
    a, _ = _ref(_case([[5, 10, 20, np.pi / 2, 0.0, 0.7, 1]], [4, 5, 1, 0, 0, 0, 1]))
    assert np.allclose(a[0, 0, 3:7], [0, 1, 0, 1], atol=1e-7)
    a, _ = _ref(_case([[5, 10, 20, 0.3, np.pi / 2, 0.7, 1]], [4, 5, 1, 0, 0, 0, 1]))
    assert np.allclose(a[0, 0, 3:6], [0, 0, 1], atol=1e-7)


def test_heading_straight_at_a_stationary_evader():
    """u_i = rh: column 15 = 1 and the closing speed is the pursuer's own, column 14 = v_i / (e_vmax + p_vmax)"""
    a, _ = _ref(_case([[2, 3, 4, 0.0, 0.0, 0.5, 1]], [9, 3, 4, 1.0, 0.3, 0.0, 1]))
    assert a[0, 0, 15] == 1.0 and a[0, 0, 14] == np.float32(0.5 / 1.7) and a[0, 0, 16] == 1.0
    assert np.array_equal(a[0, 0, 11:14], np.zeros(3, np.float32))                       # a stationary evader has no velocity
    # an evader fleeing along the line of sight at speed 1 from a pursuer at 0.5: the range opens at 0.5
    a, _ = _ref(_case([[2, 3, 4, 0.0, 0.0, 0.5, 1]], [9, 3, 4, 0.0, 0.0, 1.0, 1]))
    assert a[0, 0, 14] == np.float32(-0.5 / 1.7) and np.array_equal(a[0, 0, 11:14], np.array([1, 0, 0], np.float32))
    # heading away: column 15 = -1
    a, _ = _ref(_case([[2, 3, 4, np.pi, 0.0, 0.5, 1]], [9, 3, 4, 0.0, 0.0, 0.0, 1]))
    assert abs(a[0, 0, 15] + 1.0) <= 1e-7


def test_target_offset_of_the_evader():
    a, c = _ref(_case([[2, 3, 4, 0, 0, 0.5, 1]], [9, 3, 4, 0, 0, 0, 1], target=(19, 3, 0)))
    want = np.array([0.5, 0.0, -0.2], np.float64).astype(np.float32)
    assert np.array_equal(a[0, 0, 17:20], want) and np.array_equal(c[0, 0, 17:20], want)


def _k(c, mode):
    return _ref(c, mode)[0][0, :, ref.K_COL].tolist()


def test_chain_relays_a_sighting_in_team_mode():
    """A - B - C - D spaced 5 apart with a communication range of 6, only D senses the evader; E is isolated"""
    c = fc.chain_case(4)
    assert c["pe_adj"].tolist() == [[0, 0, 0, 1]] and c["pp_adj"][0, 0].tolist() == [1, 1, 0, 0]
    assert _k(c, "sensed") == [0, 0, 0, 1] and _k(c, "team") == [1, 1, 1, 1] and _k(c, "global") == [1, 1, 1, 1]
    assert _k(fc.chain_case(4, dead=2), "team") == [0, 0, 0, 1]         # C inactive: the relay is cut (C's own row is zero)
    assert _ref(fc.chain_case(4, dead=2), "team")[1][0, :, ref.K_COL].tolist() == [1, 1, 0, 1]   # the critic: every active row
    # an isolated fifth pursuer, 100 away from the chain, hears nothing
    p = np.concatenate((c["p"], np.array([[[100.0], [0], [0], [0], [0], [0], [1]]])), 2)
    pp = np.zeros((1, 5, 5), np.float32); pp[0, :4, :4] = c["pp_adj"][0]; pp[0, 4, 4] = 1
    c5 = dict(c, p=p, pp_adj=pp, pe_adj=np.array([[0, 0, 0, 1, 0]], np.float32))
    assert _k(c5, "team") == [1, 1, 1, 1, 0] and _k(c5, "sensed") == [0, 0, 0, 1, 0]
    # the evader block of a pursuer that knows is the same in every mode that lets it know
    assert np.array_equal(_ref(c, "team")[0][0, 0], _ref(c, "global")[0][0, 0])
    assert np.all(_ref(c, "sensed")[0][0, 0, ref.EVADER_COLS] == 0)


def test_one_direction_of_pp_adj_links_two_pursuers():
    rows = [[0, 0, 0, 0, 0, 0, 1], [5, 0, 0, 0, 0, 0, 1], [10, 0, 0, 0, 0, 0, 1]]
    for pp in ([[0, 1, 0], [0, 0, 0], [0, 0, 0]], [[0, 0, 0], [1, 0, 0], [0, 0, 0]]):      # 0 -> 1 only, 1 -> 0 only
        for sensor, want in ((0, [1, 1, 0]), (1, [1, 1, 0]), (2, [0, 0, 1])):
            pe = [int(i == sensor) for i in range(3)]
            assert _k(_case(rows, [1, 1, 1, 0, 0, 0, 1], pp=pp, pe=pe), "team") == want, (pp, sensor)
    # a link to an inactive pursuer that senses relays nothing
    rows[1][6] = 0
    assert _k(_case(rows, [1, 1, 1, 0, 0, 0, 1], pp=[[0, 1, 0], [1, 0, 1], [0, 1, 0]], pe=[0, 1, 0]), "team") == [0, 0, 0]


def test_nearest_neighbour_ties_pick_the_lowest_index():
    """mirrored, exactly representable positions: 1 and 2 are both at squared distance 4 from 0, 3 at 9"""
    rows = [[8, 8, 8, 0, 0, 0, 1], [10, 8, 8, 0, 0, 0, 1], [6, 8, 8, 0, 0, 0, 1], [8, 11, 8, 0, 0, 0, 1]]
    a, c = _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1]))
    for f in (a, c):
        assert np.array_equal(f[0, 0, 20:25], np.array([1, 0, 0, 0.1, 0.25], np.float32))     # pursuer 1: +x
        assert np.array_equal(f[0, 0, 25:30], np.array([-1, 0, 0, 0.1, 0.25], np.float32))    # pursuer 2: -x
        assert f[0, 0, 30] == 1.0
    # three-way tie: 1, 2 and 3 all at distance 2 -> 1 then 2
    rows[3][:3] = [8, 10, 8]
    a, _ = _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1]))
    assert a[0, 0, 20] == 1.0 and a[0, 0, 25] == -1.0
    # the actor sees only pp_adj[i][j] == 1: with 1 hidden the tie is between 2 and 3
    pp = np.ones((4, 4)); pp[0, 1] = 0
    a, c = _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1], pp=pp))
    assert a[0, 0, 20] == -1.0 and a[0, 0, 26] == 1.0 and a[0, 0, 30] == np.float32(2 / 3) and c[0, 0, 20] == 1.0 and c[0, 0, 30] == 1.0
    # a nearer later team-mate displaces both
    rows[3][:3] = [8, 9, 8]
    a, _ = _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1]))
    assert a[0, 0, 21] == 1.0 and a[0, 0, 23] == np.float32(0.05) and a[0, 0, 25] == 1.0


def test_no_and_one_visible_team_mate_leave_zero_blocks():
    rows = [[8, 8, 8, 0, 0, 0, 1], [10, 8, 8, 0, 0, 0, 1], [6, 8, 8, 0, 0, 0, 1]]
    a, c = _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1], pp=np.zeros((3, 3))))
    assert np.all(a[0, :, 20:31] == 0) and c[0, 0, 30] == 1.0 and np.any(c[0, 0, 25:30] != 0)
    pp = np.zeros((3, 3)); pp[0, 2] = 1
    a, _ = _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1], pp=pp))
    assert a[0, 0, 20] == -1.0 and np.all(a[0, 0, 25:30] == 0) and a[0, 0, 30] == 0.5
    # pp_adj pointing at an inactive pursuer shows nobody
    rows[2][6] = 0
    a, c = _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1], pp=pp))
    assert np.all(a[0, 0, 20:31] == 0) and c[0, 0, 30] == 0.5 and np.all(c[0, 0, 25:30] == 0)


def test_coincident_team_mates_have_no_direction_and_full_proximity():
    rows = [[8, 8, 8, 0, 0, 0, 1], [8, 8, 8, 0, 0, 0, 1]]
    a, _ = _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1]))
    assert np.array_equal(a[0, 0, 20:25], np.array([0, 0, 0, 0, 1], np.float32)) and np.isfinite(a).all()
    # inside the kill radius the proximity saturates at 1; at twice the radius it is 1 / 2
    rows[1][0] = 8.25
    assert _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1]))[0][0, 0, 24] == 1.0
    rows[1][0] = 9.0
    assert _ref(_case(rows, [1, 1, 1, 0, 0, 0, 1]))[0][0, 0, 24] == 0.5
    # a pursuer on top of the evader: direction 0, range 0, k still 1
    a, _ = _ref(_case([[8, 8, 8, 0, 0, 0.5, 1]], [8, 8, 8, 0, 0, 0, 1]))
    assert np.all(a[0, 0, 7:11] == 0) and a[0, 0, 16] == 1.0 and a[0, 0, 14] == 0.0 and np.isfinite(a).all()


def test_a_single_pursuer():
    a, c = _ref(_case([[1, 1, 1, 0.3, 0.2, 0.5, 1]], [4, 5, 1, 2.0, 0.5, 1.0, 1]), "team")
    assert a.shape == c.shape == (1, 1, 32) and np.array_equal(a, c) and np.all(a[0, 0, 20:31] == 0) and a[0, 0, 16] == 1.0
    a, _ = _ref(_case([[1, 1, 1, 0.3, 0.2, 0.5, 1]], [4, 5, 1, 2.0, 0.5, 1.0, 1], pe=[0]), "team")
    assert a[0, 0, 16] == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_inactive_rows_and_an_inactive_evader_are_exact_zeros(mode):
    c = fc.random_case(8)
    a, cr = _ref(c, mode)
    dead = c["p"][:, 6] == 0
    assert dead.any() and np.all(a[dead] == 0) and np.all(cr[dead] == 0)
    assert c["e"][2, 6] == 0 and np.all(a[2][:, ref.EVADER_COLS] == 0) and np.all(cr[2][:, ref.EVADER_COLS] == 0)
    live = ~dead
    assert np.all(cr[live][:, ref.K_COL] == (c["e"][:, 6] != 0)[:, None].repeat(8, 1)[live])


def test_the_critic_ignores_the_adjacencies():
    c = fc.random_case(9)
    _, c0 = _ref(c, "sensed")
    for mode in MODES:
        _, c1 = _ref(dict(c, pp_adj=1 - c["pp_adj"], pe_adj=1 - c["pe_adj"]), mode)
        assert np.array_equal(c0, c1)
    a0, _ = _ref(c, "sensed")
    a1, _ = _ref(dict(c, pe_adj=1 - c["pe_adj"]), "sensed")
    assert not np.array_equal(a0, a1)


def test_unknown_mode_raises():
    with pytest.raises(ValueError, match="evader_obs"):
        _ref(fc.chain_case(4), "nearest")


# ---- the link to the scripted pursuers -----------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 9])
def test_global_line_of_sight_is_the_pure_pursuit_direction(P):
    """columns 7-9 in global mode = the direction g of guidance_ref with lead = 0 and sep_gain = 0 (before the fp32 rounding)"""
    c = fc.random_case(P, seed=1)
    g, on = guidance_ref.e3d_direction(c["p"], c["e"], CFG["p_vmax"], 0.0, 2.0, 0.0)
    rows = 0
    for n in range(fc.N):
        pos = [[float(v) for v in c["p"][n, k]] for k in range(3)]
        for i in range(P):
            if not on[n, i]:
                continue
            f = ref._row(CFG, c["p"][n, :6, i], c["e"][n], c["target"][n], 0, 1, pos, i, [])
            assert np.abs(np.array(f[7:10]) - g[n, :, i]).max() <= 1e-15
            rows += 1
    assert rows >= P


# ---- the host entry against the specification -----------------------------------------------------------------------------------------
def _lib():
    from distributed_multi_agent_reinforcement_learning_amd import build
    path = build.build_lib("libe3d_env.so")
    assert path and os.path.exists(path)
    L = C.CDLL(path)
    L.e3d_pursuit_features_host.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_void_p]
    return L


def host_features(c, mode, cfg=CFG):
    """e3d_pursuit_features_host on a case dict -> (actor, critic), the outputs pre-filled with 7"""
    from distributed_multi_agent_reinforcement_learning_amd.e3d_env import E3dConfig
    N, _, P = c["p"].shape
    k = E3dConfig()
    k.P, k.max_step = P, cfg["max_step"]
    for name in ("p_vmax", "e_vmax", "kill_radius", "p_comm_range", "p_sen_range"):
        setattr(k, name, cfg[name])
    arr = {n: np.ascontiguousarray(c[n], dt) for n, dt in (("p", np.float64), ("e", np.float64), ("target", np.float64), ("time_step", np.int32),
                                                          ("pp_adj", np.float32), ("pe_adj", np.float32))}
    fa, fcr = np.full((N, P, 32), 7.0, np.float32), np.full((N, P, 32), 7.0, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib().e3d_pursuit_features_host(C.byref(k), N, ptr(arr["p"]), ptr(arr["e"]), ptr(arr["target"]), ptr(arr["time_step"]), ptr(arr["pp_adj"]),
                                          ptr(arr["pe_adj"]), MODES.index(mode), ptr(fa), ptr(fcr))
    assert rc == 0
    return fa, fcr


def check_against_ref(got, want, c):
    """rtol = atol = 1e-6 (the figures of test_policy_features_match_numpy); the k column, the rows of inactive pursuers and the
    evader block of an environment without an evader are exact"""
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=1e-6, atol=1e-6)
        assert np.array_equal(g[..., ref.K_COL], w[..., ref.K_COL])
        dead = c["p"][:, 6] == 0
        assert np.all(g[dead] == 0)
        gone = c["e"][:, 6] == 0
        assert np.all(g[gone][..., ref.EVADER_COLS] == 0)
        zero = w == 0
        assert np.all(g[zero] == 0)   # every column the law leaves at zero (missing team-mates, unknown evader)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", fc.P_CASES)
def test_host_entry_matches_the_specification(P, mode):
    c = fc.random_case(P)
    check_against_ref(host_features(c, mode), _ref(c, mode), c)


@pytest.mark.parametrize("P,dead", [(4, None), (4, 2), (9, None), (9, 4), (33, None), (33, 16)])
def test_host_entry_relays_along_chains(P, dead):
    c = fc.chain_case(P, dead)
    a, _ = host_features(c, "team")
    want = [1.0] * P if dead is None else [0.0] * (dead + 1) + [1.0] * (P - dead - 1)
    assert a[0, :, ref.K_COL].tolist() == want == _k(c, "team")
    assert host_features(c, "sensed")[0][0, :, ref.K_COL].tolist() == [0.0] * (P - 1) + [1.0]


def test_host_entry_hand_cases():
    rows = [[8, 8, 8, 0, 0, 0, 1], [10, 8, 8, 0, 0, 0, 1], [6, 8, 8, 0, 0, 0, 1], [8, 10, 8, 0, 0, 0, 1], [8, 8, 8, 0, 0, 0, 1]]
    c = _case(rows, [1, 1, 1, 0, 0, 0, 1])
    for mode in MODES:
        got, want = host_features(c, mode), _ref(c, mode)
        assert np.array_equal(got[0][..., 20:31], want[0][..., 20:31]) and np.array_equal(got[1][..., 20:31], want[1][..., 20:31])
    assert host_features(c, "sensed")[0][0, 0, 20:25].tolist() == [0, 0, 0, 0, 1]     # the coincident pursuer 4 is the nearest


@pytest.mark.parametrize("P", fc.P_CASES)
def test_the_shared_cases_have_no_near_ties(P):
    """what tests/test_e3d_features_gpu.py relies on: no two squared team-mate distances of a row closer than 1e-9 relative, in every
    row of the fixed seeds (none is left out)"""
    c = fc.random_case(P)
    gap, rows = ref.nearest_gap(c["p"])
    assert rows == int((c["p"][:, 6] != 0).sum()) and gap >= fc.MIN_GAP, (gap, rows)


# ---- the options -----------------------------------------------------------------------------------------------------------------------
def _cfg(**ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config("cfg5", **ov)


def test_option_defaults_and_values():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import e3d_feature_options
    assert e3d_feature_options(_cfg()) == ("basic", "sensed")
    for mode in MODES:
        assert e3d_feature_options(_cfg(**{"algo.e3d_features": "pursuit", "algo.e3d_evader_obs": mode})) == ("pursuit", mode)
    assert e3d_feature_options(_cfg(**{"algo.e3d_evader_obs": "sensed"})) == ("basic", "sensed")


@pytest.mark.parametrize("ov,key", [({"algo.e3d_features": "los"}, "algo.e3d_features"),
                                    ({"algo.e3d_features": "pursuit", "algo.e3d_evader_obs": "all"}, "algo.e3d_evader_obs"),
                                    ({"algo.e3d_evader_obs": "team"}, "algo.e3d_evader_obs"),
                                    ({"algo.e3d_evader_obs": "global"}, "algo.e3d_evader_obs")])
def test_bad_options_raise_naming_the_key(ov, key):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO, e3d_feature_options
    with pytest.raises(ValueError, match=key):
        e3d_feature_options(_cfg(**ov))
    with pytest.raises(ValueError, match=key):     # before the device check: the agent raises this on a machine without a GPU as well
        E3dMAPPO(_cfg(**ov), 4, 1, device="cpu")


def test_obs_norm_with_pursuit_raises_naming_both_keys():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    with pytest.raises(ValueError, match="algo.use_obs_norm.*algo.e3d_features"):
        E3dMAPPO(_cfg(**{"algo.e3d_features": "pursuit", "algo.use_obs_norm": True}), 4, 1, device="cpu")


def test_evader_obs_names_map_to_the_abi_codes():
    from distributed_multi_agent_reinforcement_learning_amd import e3d_env
    assert e3d_env.EVADER_OBS == MODES and [e3d_env.evader_obs_code(m) for m in MODES] == [0, 1, 2] and e3d_env.PURSUIT_FEAT == ref.FEAT
    with pytest.raises(ValueError, match="evader_obs"):
        e3d_env.evader_obs_code("nearest")
