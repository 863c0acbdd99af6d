"""CPU checks of env_3d's centralised critic input (algo.e3d_critic: central): tests/central_critic_ref.py -- the
specification the kernel is held to in tests/test_central_critic_gpu.py -- on hand cases, the host entry e3d_central_features_host
against it on the shared cases, the three identities that tie the wide row to the pursuit rows, and the parsing of the option."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import central_critic_cases as cc
from tests import central_critic_ref as cref
from tests import e3d_features_ref as ref

CFG = cc.CFG
MODES = ref.EVADER_OBS


def _ref(c, mode="sensed"):
    return cref.central_features(CFG, c["p"], c["e"], c["target"], c["time_step"], c["pp_adj"], c["pe_adj"], mode)


def _slot(f, i, s):
    return f[0, i, 32 + 8 * s:40 + 8 * s]


def _f32(*v):
    return np.array(v, np.float64).astype(np.float32)


# ---- the law, by hand -------------------------------------------------------------------------------------------------------------------
def test_team_mate_offset_3_4_5():
    """p_j - p_i = (3, 4, 0), d = 5: columns 0-3 of slot 0 = (0.6, 0.8, 0, 5 / 20); (3, 0, 4) for the third component"""
    _, c = _ref(cc.case([[1, 1, 1, 0, 0, 0, 1], [4, 5, 1, 0, 0, 0, 1]]))
    assert c.shape == (1, 2, 40) and np.array_equal(_slot(c, 0, 0)[:4], _f32(0.6, 0.8, 0.0, 0.25))
    assert np.array_equal(_slot(c, 1, 0)[:4], _f32(-0.6, -0.8, 0.0, 0.25))             # ... and seen from the other side
    _, c = _ref(cc.case([[1, 1, 1, 0, 0, 0, 1], [4, 1, 5, 0, 0, 0, 1]]))
    assert np.array_equal(_slot(c, 0, 0)[:4], _f32(0.6, 0.0, 0.8, 0.25))


def test_team_mate_heading_along_y_at_full_speed():
    _, c = _ref(cc.case([[1, 1, 1, 0, 0, 0, 1], [4, 5, 1, np.pi / 2, 0.0, CFG["p_vmax"], 1]]))
    s = _slot(c, 0, 0)
    assert np.allclose(s[4:7], [0, 1, 0], atol=1e-7) and s[5] == 1.0 and s[7] == 1.0
    assert np.array_equal(_slot(c, 1, 0)[4:8], _f32(1, 0, 0, 0))                        # pursuer 0 heads along +x at rest
    _, c = _ref(cc.case([[1, 1, 1, 0, 0, 0, 1], [4, 5, 1, 0.3, np.pi / 2, 0.35, 1]]))
    assert np.allclose(_slot(c, 0, 0)[4:7], [0, 0, 1], atol=1e-7) and _slot(c, 0, 0)[7] == 0.5


def test_three_team_mates_are_ordered_by_distance():
    """from pursuer 0: 3 at distance 1, 1 at 2, 2 at 4, whatever their indices; the speeds tell them apart"""
    rows = [[8, 8, 8, 0, 0, 0, 1], [8, 10, 8, 0, 0, 0.07, 1], [4, 8, 8, 0, 0, 0.14, 1], [8, 8, 9, 0, 0, 0.21, 1]]
    c = cc.case(rows)
    _, f = _ref(c)
    assert f.shape == (1, 4, 56)
    assert [float(_slot(f, 0, s)[7]) for s in range(3)] == [float(np.float32(v / 0.7)) for v in (0.21, 0.07, 0.14)]
    assert [float(_slot(f, 0, s)[3]) for s in range(3)] == [float(np.float32(d / 20)) for d in (1, 2, 4)]
    assert np.array_equal(_slot(f, 0, 0)[:3], _f32(0, 0, 1)) and np.array_equal(_slot(f, 0, 2)[:3], _f32(-1, 0, 0))
    assert cref.order(c["p"])[0].tolist() == [[3, 1, 2], [0, 3, 2], [0, 3, 1], [0, 1, 2]]


@pytest.mark.parametrize("swap", [False, True])
def test_an_exact_tie_puts_the_lowest_index_first(swap):
    c = cc.tie_case(swap)
    _, f = _ref(c)
    first, second = (_f32(-1, 0, 0, 0.15), _f32(1, 0, 0, 0.15)) if swap else (_f32(1, 0, 0, 0.15), _f32(-1, 0, 0, 0.15))
    assert np.array_equal(_slot(f, 0, 0)[:4], first) and np.array_equal(_slot(f, 0, 1)[:4], second)
    assert _slot(f, 0, 0)[7] == np.float32((0.35 if swap else 0.7) / 0.7) and _slot(f, 0, 1)[7] == np.float32((0.7 if swap else 0.35) / 0.7)
    assert cref.order(c["p"])[0, 0].tolist() == [1, 2, 3]


def test_a_dead_team_mate_closes_the_gap_and_leaves_the_last_slot_zero():
    rows = [[8, 8, 8, 0, 0, 0, 1], [8, 10, 8, 0, 0, 0.07, 1], [4, 8, 8, 0, 0, 0.14, 1], [8, 8, 9, 0, 0, 0.21, 1]]
    rows[1] = [1000.0, 1000.0, 1000.0, 0, 0, 0, 0]
    c = cc.case(rows)
    _, f = _ref(c)
    assert cref.order(c["p"])[0].tolist() == [[3, 2, -1], [-1, -1, -1], [0, 3, -1], [0, 2, -1]]
    assert _slot(f, 0, 0)[7] == np.float32(0.21 / 0.7) and _slot(f, 0, 1)[7] == np.float32(0.14 / 0.7)
    assert np.all(_slot(f, 0, 2) == 0) and np.all(f[0, 1] == 0) and f[0, 0, 30] == np.float32(2 / 3)


def test_a_single_pursuer_has_the_pursuit_critic_row():
    c = cc.case([[1, 1, 1, 0.3, 0.2, 0.5, 1]], [4, 5, 1, 2.0, 0.5, 1.0, 1])
    a, f = _ref(c, "team")
    pa, pc = ref.pursuit_features(CFG, c["p"], c["e"], c["target"], c["time_step"], c["pp_adj"], c["pe_adj"], "team")
    assert cref.feat(1) == 32 and f.shape == (1, 1, 32) and np.array_equal(f, pc) and np.array_equal(a, pa)


def test_widths():
    assert [cref.feat(P) for P in (1, 2, 8, 16)] == [32, 40, 88, 152] and all(cref.feat(P) * 4 % 32 == 0 for P in range(1, 17))
    with pytest.raises(ValueError):
        _ref(cc.all_active_case(17))


@pytest.mark.parametrize("P", cc.P_CASES)
def test_the_identities_hold_in_the_specification(P):
    for c in (cc.random_case(P), cc.all_active_case(P)):
        for mode in MODES:
            a, f = _ref(c, mode)
            pa, pc = ref.pursuit_features(CFG, c["p"], c["e"], c["target"], c["time_step"], c["pp_adj"], c["pe_adj"], mode)
            filled = cc.identities(a, f, pa, pc, c["p"])
    assert filled == cc.N * P * (P - 1)                                                  # the all-active case fills every slot


# ---- the host entry against the specification ---------------------------------------------------------------------------------------------
def _lib():
    from distributed_multi_agent_reinforcement_learning_amd import build
    path = build.build_lib("libe3d_env.so")
    assert path and os.path.exists(path)
    L = C.CDLL(path)
    L.e3d_central_features_host.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_void_p]
    return L


def host_features(c, mode, cfg=CFG):
    """e3d_central_features_host on a case dict -> (actor, critic), the outputs pre-filled with 7"""
    from distributed_multi_agent_reinforcement_learning_amd.e3d_env import E3dConfig
    N, _, P = c["p"].shape
    k = E3dConfig()
    k.P, k.max_step = P, cfg["max_step"]
    for name in ("p_vmax", "e_vmax", "kill_radius", "p_comm_range", "p_sen_range"):
        setattr(k, name, cfg[name])
    arr = {n: np.ascontiguousarray(c[n], dt) for n, dt in (("p", np.float64), ("e", np.float64), ("target", np.float64), ("time_step", np.int32),
                                                          ("pp_adj", np.float32), ("pe_adj", np.float32))}
    fa, fcr = np.full((N, P, 32), 7.0, np.float32), np.full((N, P, cref.feat(P)), 7.0, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib().e3d_central_features_host(C.byref(k), N, ptr(arr["p"]), ptr(arr["e"]), ptr(arr["target"]), ptr(arr["time_step"]), ptr(arr["pp_adj"]),
                                          ptr(arr["pe_adj"]), MODES.index(mode), ptr(fa), ptr(fcr))
    assert rc == 0
    return fa, fcr


@pytest.mark.parametrize("P", cc.P_CASES)
def test_the_shared_cases_have_no_near_ties(P):
    """what the comparisons rely on: no two squared team-mate distances of a row closer than MIN_GAP relative"""
    for c in (cc.random_case(P), cc.all_active_case(P)):
        assert cc.gap_of(c) >= cc.MIN_GAP


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", cc.P_CASES)
def test_host_entry_matches_the_specification(P, mode):
    for c in (cc.random_case(P), cc.all_active_case(P)):
        got = host_features(c, mode)
        cc.check_against_ref(got, _ref(c, mode), c)
        pa, pc = ref.pursuit_features(CFG, c["p"], c["e"], c["target"], c["time_step"], c["pp_adj"], c["pe_adj"], mode)
        np.testing.assert_allclose(got[0], pa, rtol=1e-6, atol=1e-6)
        cc.identities(got[0], got[1], got[0], got[1][..., :32], c["p"])                    # 2 and 3 on the host's own bytes


@pytest.mark.parametrize("swap", [False, True])
def test_host_entry_on_the_exact_tie(swap):
    c = cc.tie_case(swap)
    got, want = host_features(c, "global"), _ref(c, "global")
    assert np.array_equal(got[1][..., 32:], want[1][..., 32:])                          # exactly representable: equal to the bit


def test_host_entry_on_a_single_pursuer_and_a_dead_team_mate():
    c = cc.case([[1, 1, 1, 0.3, 0.2, 0.5, 1]], [4, 5, 1, 2.0, 0.5, 1.0, 1])
    cc.check_against_ref(host_features(c, "team"), _ref(c, "team"), c)
    rows = [[8, 8, 8, 0, 0, 0, 1], [1000.0, 1000.0, 1000.0, 0, 0, 0, 0], [4, 8, 8, 0, 0, 0.14, 1], [8, 8, 9, 0, 0, 0.21, 1]]
    c = cc.case(rows)
    got = host_features(c, "sensed")
    cc.check_against_ref(got, _ref(c, "sensed"), c)
    assert np.all(got[1][0, 0, 48:56] == 0) and np.all(got[1][0, 1] == 0)


# ---- the option ---------------------------------------------------------------------------------------------------------------------------
PURSUIT = {"algo.e3d_features": "pursuit"}


def _cfg(**ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config("cfg5", **ov)


def test_option_defaults_and_values():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3D_CRITIC, e3d_critic_options
    assert E3D_CRITIC == ("local", "central")
    assert e3d_critic_options(_cfg()) == "local" and e3d_critic_options(_cfg(**{"algo.e3d_critic": "local"})) == "local"
    assert e3d_critic_options(_cfg(**PURSUIT)) == "local"
    assert e3d_critic_options(_cfg(**PURSUIT, **{"algo.e3d_critic": "central"})) == "central"
    assert e3d_critic_options(_cfg(**PURSUIT, **{"algo.e3d_critic": "central", "env.num_defender": 16})) == "central"


@pytest.mark.parametrize("ov,keys", [({"algo.e3d_critic": "global"}, "algo.e3d_critic"),
                                     ({"algo.e3d_critic": "central"}, "algo.e3d_critic.*algo.e3d_features"),
                                     ({"algo.e3d_critic": "central", "algo.e3d_features": "basic"}, "algo.e3d_critic.*algo.e3d_features"),
                                     ({**PURSUIT, "algo.e3d_critic": "central", "env.num_defender": 17}, "algo.e3d_critic.*env.num_defender")])
def test_bad_options_raise_naming_the_keys(ov, keys):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO, e3d_critic_options
    with pytest.raises(ValueError, match=keys):
        e3d_critic_options(_cfg(**ov))
    with pytest.raises(ValueError, match=keys):     # before the device check: raised on a machine without a GPU as well
        E3dMAPPO(_cfg(**ov), 4, 1, device="cpu")


@pytest.mark.parametrize("ov", [{"algo.e3d_critic": "local"}, {**PURSUIT, "algo.e3d_critic": "local"}, {**PURSUIT, "algo.e3d_critic": "central"}])
def test_good_options_pass_through_to_the_device_check(ov):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    with pytest.raises(RuntimeError, match="GPU only"):
        E3dMAPPO(_cfg(**ov), 4, 1, device="cpu")


def test_python_constants_match_the_specification():
    from distributed_multi_agent_reinforcement_learning_amd import e3d_env
    assert e3d_env.CENTRAL_MATE == cref.MATE == 8 and e3d_env.CENTRAL_MAX_P == cref.MAX_P == 16
    assert [e3d_env.central_feat(P) for P in range(1, 17)] == [cref.feat(P) for P in range(1, 17)] and e3d_env.central_feat(8) == 88
