"""CPU checks of the direction-vector action head (algo.gauss_squash: direction): the specification
tests/direction_ref.py on its own (the edge table, the round trip through the label, the angle), the two host entries
gauss_direction_map_host / e3d_direction_label_host against it, and the parsing of the option and the policy entry of files."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import direction_ref as ref
from tests import gauss_sd_ref

E3D_ERR_BAD_CONFIG, E3D_ERR_NULL = 40001, 40002


def _lib():
    from distributed_multi_agent_reinforcement_learning_amd import build
    path = build.build_lib("libe3d_env.so")
    L = C.CDLL(path)
    L.gauss_direction_map_host.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    L.e3d_direction_label_host.argtypes = [C.c_int32, C.c_void_p, C.c_void_p]
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _draws(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.999, 0.999, n), rng.uniform(-0.999, 0.999, n), rng.choice([-1.0, 1.0], n) * rng.uniform(0, 1, n)], -1)


# ---- the specification ------------------------------------------------------------------------------------------------------------
def test_edge_table_is_exact():
    for u, want in ref.EDGES:
        got = ref.to_env(np.array(u, np.float32))
        assert np.array_equal(_bits(got), _bits(np.array(want))), (u, got, want)      # bit for bit: +0 where the table says 0
    assert np.signbit(np.float32(-0.0)) and ref.to_env(np.array([-1, -0.0, 0, 0], np.float32))[0] == -1.0


def test_round_trip_through_the_label():
    g = _draws(200_000, 0)
    back = ref.to_env(ref.label(g))
    err = np.abs(back - g).max(0)
    print("round trip: max error a0 %.3g, a1 %.3g, a2 %.3g" % tuple(err))
    # the label's fp32 rounding (measured 1.8e-8 / 3.0e-8); a formula error is at least 1e-3
    assert err[0] <= 2e-7 and err[1] <= 2e-7
    assert np.array_equal(back[:, 2], g[:, 2].astype(np.float32).astype(np.float64))   # the speed passes through: its fp32 value
    lab = ref.label(g)
    assert lab.dtype == np.float32 and np.abs(np.linalg.norm(lab[:, :3].astype(np.float64), axis=1) - 1.0).max() <= 2e-7


def test_label_of_a_hold_row():
    # the teacher holds: it commands the pursuer's own heading phi / pi and pitch gamma / (pi / 2) at speed -1 -- the same formula
    phi, gamma = 2.5, -0.4
    lab = ref.label(np.array([phi / np.pi, gamma / (np.pi / 2), -1.0]))
    want = np.array([np.cos(gamma) * np.cos(phi), np.cos(gamma) * np.sin(phi), np.sin(gamma), -1.0])
    assert np.abs(lab.astype(np.float64) - want).max() <= 6e-8 and lab[3] == -1.0
    env = ref.to_env(lab)
    assert abs(env[0] * np.pi - phi) <= 2e-7 * np.pi and abs(env[1] * np.pi / 2 - gamma) <= 2e-7 * np.pi and env[2] == -1.0


def test_angle():
    e = np.eye(3)
    assert ref.angle([2.0, 0, 0, 9.0], [0.5, 0, 0, -9.0]) == 0.0                      # the fourth dimension takes no part
    assert ref.angle(e[0], e[1]) == np.pi / 2 and ref.angle(e[2], 3 * e[0]) == np.pi / 2
    assert ref.angle(e[1], -e[1]) == np.pi
    assert ref.angle(np.zeros(3), e[0]) == np.pi / 2                                  # a mean that points nowhere
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=(1000, 3)), rng.normal(size=(1000, 3))
    cosang = (a * b).sum(-1) / np.linalg.norm(a, axis=-1) / np.linalg.norm(b, axis=-1)
    np.testing.assert_allclose(ref.angle(a, b), np.arccos(cosang), rtol=0, atol=1e-12)
    assert ref.angle(np.stack([np.zeros(3), e[0]]), np.stack([e[0], e[0]])).tolist() == [np.pi / 2, 0.0]


def test_ppo_reference_of_the_mode_is_clip_on_four_dimensions():
    rng = np.random.default_rng(2)
    n, A = 50, 4
    mu, u = rng.normal(size=(n, A)), rng.normal(size=(n, A))
    r = lambda: rng.normal(size=n)
    active = (rng.uniform(size=n) < 0.8).astype(np.float64)
    for ls in (rng.normal(size=A) * 0.3, rng.normal(size=(n, A)) * 0.3):
        args = (mu, ls, u, r(), r(), r(), active, r(), r(), 0.05, 0.01, True)
        a = ref.ppo_loss(*args, lo=-0.4, hi=0.3)
        b = gauss_sd_ref.ppo_loss(*args, lo=-0.4, hi=0.3, squash="clip")
        c = gauss_sd_ref.ppo_loss(*args, lo=-0.4, hi=0.3, squash="direction")
        t = gauss_sd_ref.ppo_loss(*args, lo=-0.4, hi=0.3, squash="tanh")
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        assert a[0] != t[0]                                                            # (the tanh mode does differ on these inputs)


# ---- the host entries -------------------------------------------------------------------------------------------------------------
def _map_host(u):
    u = np.ascontiguousarray(u, np.float32)
    out = np.full((u.shape[0], 3), 7.0)
    assert _lib().gauss_direction_map_host(u.shape[0], _ptr(u), _ptr(out)) == 0
    return out


def _label_host(g):
    g = np.ascontiguousarray(g, np.float64)
    out = np.full((g.shape[0], 4), 7.0, np.float32)
    assert _lib().e3d_direction_label_host(g.shape[0], _ptr(g), _ptr(out)) == 0
    return out


def test_map_host_edge_table_is_exact():
    u = np.array([e[0] for e in ref.EDGES], np.float32)
    want = np.array([e[1] for e in ref.EDGES])
    assert np.array_equal(_bits(_map_host(u)), _bits(want))


@pytest.mark.parametrize("R", [1, 7, 300])
def test_host_entries_match_the_specification(R):
    rng = np.random.default_rng(R)
    u = (rng.normal(size=(R, 4)) * np.array([1.0, 1.0, 1.0, 0.8])).astype(np.float32)
    u[::5, :2] *= 1e-3                                                                 # steep vectors: the pitch near its clamp
    got = _map_host(u)
    assert (got != 7.0).all() and np.abs(got).max() <= 1.0
    np.testing.assert_allclose(got, ref.to_env(u), rtol=0, atol=1e-12)                 # libm against numpy
    g = _draws(R, 100 + R)
    g[::3, 2] = -1.0
    lab, want = _label_host(g), ref.label(g)
    assert lab.dtype == np.float32 and (lab != 7.0).all()
    assert (np.abs(lab.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()   # one fp32 ulp
    assert np.array_equal(lab[:, 3], g[:, 2].astype(np.float32))


def test_host_entries_check_their_arguments():
    L = _lib()
    u, env = np.zeros((2, 4), np.float32), np.full((2, 3), 7.0)
    g, lab = np.zeros((2, 3)), np.full((2, 4), 7.0, np.float32)
    assert L.gauss_direction_map_host(2, None, _ptr(env)) == E3D_ERR_NULL and L.gauss_direction_map_host(2, _ptr(u), None) == E3D_ERR_NULL
    assert L.e3d_direction_label_host(2, None, _ptr(lab)) == E3D_ERR_NULL and L.e3d_direction_label_host(2, _ptr(g), None) == E3D_ERR_NULL
    assert L.gauss_direction_map_host(-1, _ptr(u), _ptr(env)) == E3D_ERR_BAD_CONFIG
    assert L.e3d_direction_label_host(-1, _ptr(g), _ptr(lab)) == E3D_ERR_BAD_CONFIG
    assert L.gauss_direction_map_host(0, _ptr(u), _ptr(env)) == 0 and L.e3d_direction_label_host(0, _ptr(g), _ptr(lab)) == 0
    assert (env == 7.0).all() and (lab == 7.0).all()                                   # nothing was written by any of these
    assert L.gauss_direction_map_host(1, _ptr(u), _ptr(env)) == 0 and (env[1] == 7.0).all() and (env[0] == 0.0).all()   # R rows, no more


# ---- options and files ------------------------------------------------------------------------------------------------------------
def _cfg(**ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config("cfg5", **ov)


def test_option_is_accepted_and_needs_three_actions():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO, gauss_policy_options, latent_dim
    assert gauss_policy_options(_cfg(**{"algo.gauss_squash": "direction"})) == ("param", "direction", -5.0, 2.0)
    assert gauss_policy_options(_cfg(**{"algo.gauss_squash": "direction", "algo.gauss_std": "state"}))[:2] == ("state", "direction")
    assert latent_dim("direction", 3) == 4 and latent_dim("clip", 3) == 3 and latent_dim("tanh", 5) == 5
    for dim in (2, 4):
        with pytest.raises(ValueError, match=r"algo\.gauss_squash"):
            gauss_policy_options(_cfg(**{"algo.gauss_squash": "direction", "env.action_dim": dim}))
        with pytest.raises(ValueError, match=r"algo\.gauss_squash"):
            E3dMAPPO(_cfg(**{"algo.gauss_squash": "direction", "env.action_dim": dim}), 8, 1)
    assert gauss_policy_options(_cfg()) == ("param", "clip", -5.0, 2.0)                # the key absent: as it was


def test_check_policy_meta_refuses_every_cross_mode_pair():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    agent = lambda sq: SimpleNamespace(gauss_std="param", gauss_squash=sq, log_std_min=-5.0, log_std_max=2.0, policy_ex=sq != "clip")
    meta = lambda sq: None if sq == "clip" else dict(gauss_std="param", gauss_squash=sq, log_std_min=-5.0, log_std_max=2.0)
    modes = ("clip", "tanh", "direction")
    for mine in modes:
        for theirs in modes:
            if mine == theirs:
                E3dMAPPO.check_policy_meta(agent(mine), meta(theirs), "f")
                continue
            with pytest.raises(ValueError, match=r"algo\.gauss_squash"):
                E3dMAPPO.check_policy_meta(agent(mine), meta(theirs), "f")
