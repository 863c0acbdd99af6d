"""Evader problems for the SLSQP evader tests (n2n_evader_slsqp / e3d_evader_slsqp) and the acceptance rules they are held to.

A problem group is a batch of environments with the same pursuer count, laid out as the device records
(n2n: p [M][5][P], e [M][5][E]; e3d: p [M][7][P], e [M][7]), with the reference's commands and the mask of the evaders the
reference actually called e_f on.  Sources: every step of the recorded traces (n2n_*.npz, e3d_*.npz) and every record of the
sampled problems (evader_n2n.npz, evader_e3d.npz; tests/golden/gen/make_goldens_evader.py).
"""
import ctypes as C
import glob
import os

import numpy as np

from tests.helpers import GOLDEN

N2N_KEYS = ("p_vmax", "e_vmax", "p_sen_range", "p_comm_range", "kill_radius", "ang_lmt", "step_size")
E3D_KEYS = ("p_vmax", "e_vmax", "p_sen_range", "p_comm_range", "kill_radius", "ang_lmt", "v_lmt", "step_size")


def n2n_config(cfg, P, E, episode_limit=100):
    from distributed_multi_agent_reinforcement_learning_amd.n2n_env import N2nConfig
    c = N2nConfig()
    c.P, c.E, c.episode_limit = P, E, episode_limit
    for k, v in zip(N2N_KEYS, cfg):
        setattr(c, k, float(v))
    return c


def e3d_config(cfg, P, max_step=200):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_env import E3dConfig
    c = E3dConfig()
    c.P, c.max_step = P, max_step
    for k, v in zip(E3D_KEYS, cfg):
        setattr(c, k, float(v))
    return c


def n2n_trace_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "n2n_*.npz")))


def e3d_trace_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "e3d_*.npz")))


def n2n_groups():
    out = []
    for f in n2n_trace_files():
        d = np.load(f)
        T = len(d["e_cmd"])
        out.append(dict(name=os.path.basename(f)[:-4], cfg=d["cfg"], P=d["p"].shape[1], E=d["e"].shape[1],
                        p=np.ascontiguousarray(d["p"].transpose(0, 2, 1)), e=np.ascontiguousarray(d["e"].transpose(0, 2, 1)),
                        target=np.ascontiguousarray(np.broadcast_to(d["target"], (T, 2))), ref=d["e_cmd"], called=d["e"][:, :, 4] > 0))
    d = np.load(os.path.join(GOLDEN, "evader_n2n.npz"))
    for P in (1, 8, 16):
        e = d[f"P{P}_e"]
        out.append(dict(name=f"evader_n2n_P{P}", cfg=d["cfg"], P=P, E=1, p=np.ascontiguousarray(d[f"P{P}_p"].transpose(0, 2, 1)),
                        e=np.ascontiguousarray(e[:, :, None]), target=d[f"P{P}_target"], ref=d[f"P{P}_cmd"][:, None],
                        called=(e[:, 4] > 0)[:, None]))
    return out


def e3d_groups():
    out = []
    for f in e3d_trace_files():
        d = np.load(f)
        T = len(d["e_cmd"])
        called = (d["e"][:, 0, 6] > 0) & (d["p"][:, :, 6] > 0).any(1)
        out.append(dict(name=os.path.basename(f)[:-4], cfg=d["cfg"], P=d["p"].shape[1], p=np.ascontiguousarray(d["p"].transpose(0, 2, 1)),
                        e=np.ascontiguousarray(d["e"][:, 0]), target=np.ascontiguousarray(np.broadcast_to(d["target"], (T, 3))),
                        ref=d["e_cmd"][:, 0], called=called))
    d = np.load(os.path.join(GOLDEN, "evader_e3d.npz"))
    for P in (1, 8, 16):
        p, e = d[f"P{P}_p"], d[f"P{P}_e"]
        out.append(dict(name=f"evader_e3d_P{P}", cfg=d["cfg"], P=P, p=np.ascontiguousarray(p.transpose(0, 2, 1)), e=e,
                        target=d[f"P{P}_target"], ref=d[f"P{P}_cmd"], called=(e[:, 6] > 0) & (p[:, :, 6] > 0).any(1)))
    return out


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def n2n_host(L, g):
    """the library's host path (the kernel's code compiled for the CPU)"""
    M = len(g["p"])
    cmd, nit = np.zeros((M, g["E"])), np.zeros((M, g["E"]), np.int32)
    rc = L.n2n_evader_slsqp_host(C.byref(n2n_config(g["cfg"], g["P"], g["E"])), M, _ptr(g["p"]), _ptr(g["e"]), _ptr(g["target"]),
                                 _ptr(cmd), _ptr(nit))
    assert rc == 0
    return cmd, nit


def e3d_host(L, g):
    M = len(g["p"])
    cmd, nit = np.zeros((M, 3)), np.zeros(M, np.int32)
    rc = L.e3d_evader_slsqp_host(C.byref(e3d_config(g["cfg"], g["P"])), M, _ptr(g["p"]), _ptr(g["e"]), _ptr(g["target"]),
                                 _ptr(cmd), _ptr(nit))
    assert rc == 0
    return cmd, nit


# ---- env_3d objective and bounds, restated from the reference's eva.py (:87-148, :212-240) ----

def e3d_bounds(e, ang_lmt, v_lmt):
    phi, ga, v = e[3], e[4], e[5]
    lb = np.array([np.clip((phi - ang_lmt) / np.pi, -1, 1), np.clip((ga - ang_lmt) / (np.pi / 2), -1, 1), np.clip((v - v_lmt) * 2 - 1, -1, 1)])
    ub = np.array([np.clip((phi + ang_lmt) / np.pi, -1, 1), np.clip((ga + ang_lmt) / (np.pi / 2), -1, 1), np.clip((v + v_lmt) * 2 - 1, -1, 1)])
    return lb, ub


def e3d_objective(a, p, e, target, v_max, kill_radius, step_size, e_sen_range=3.0):
    """p [7][P] (one record), e [7]; the evader's own step uses the literals pi/4, 0.4, 0.5 and the COMMANDED heading"""
    x, y, z, g0, v0 = e[0], e[1], e[2], e[4], e[5]
    phi, gamma, v = a[0] * np.pi, a[1] * np.pi / 2, (a[2] + 1) / 2 * v_max
    g = g0 + np.clip(gamma - g0, -np.pi / 4, np.pi / 4)
    vv = v0 + np.clip(v - v0, -0.4, 0.4)
    nx, ny, nz = x + vv * np.cos(g) * np.cos(phi) * 0.5, y + vv * np.cos(g) * np.sin(phi) * 0.5, z + vv * np.sin(g) * 0.5
    d = []
    for j in range(p.shape[1]):
        if p[6, j] == 0 or not np.sqrt((x - p[0, j]) ** 2 + (y - p[1, j]) ** 2 + (z - p[2, j]) ** 2) <= e_sen_range:
            continue
        qx = p[0, j] + p[5, j] * np.cos(p[3, j]) * np.cos(p[4, j]) * step_size
        qy = p[1, j] + p[5, j] * np.sin(p[3, j]) * np.cos(p[4, j]) * step_size
        qz = p[2, j] + p[5, j] * np.sin(p[4, j]) * step_size
        d.append(np.sqrt((nx - qx) ** 2 + (ny - qy) ** 2 + (nz - qz) ** 2))
    f = np.sqrt((nx - target[0]) ** 2 + (ny - target[1]) ** 2 + (nz - target[2]) ** 2)
    for di in sorted(d):
        f = f + 1 / (di / kill_radius) ** 5
    return f


# ---- acceptance rules ----

def n2n_check(groups, cmds):
    """-> (calls, hits within 1e-6, worst error); uncalled evaders must get exactly 0"""
    n = hit = 0
    worst = 0.0
    for g, c in zip(groups, cmds):
        assert np.all(c[~g["called"]] == 0.0), g["name"]
        err = np.abs(c - g["ref"])[g["called"]]
        n += err.size; hit += int((err <= 1e-6).sum()); worst = max(worst, float(err.max(initial=0.0)))
    return n, hit, worst


def e3d_misses(g, c, tol=1e-6):
    """indices of the called problems whose command is not within tol of the reference's"""
    err = np.abs(c - g["ref"]).max(1)
    return np.nonzero(g["called"] & (err > tol))[0]


def e3d_check(groups, cmds):
    """-> (calls, hits within 1e-6); asserts the rule for misses beyond 1e-3 (bound-respecting, objective not above the
    reference command's by more than 1e-6 max(1, |f|)) and zeros where the reference does not call e_f"""
    n = hit = 0
    for g, c in zip(groups, cmds):
        assert np.all(c[~g["called"]] == 0.0), g["name"]
        cfg = dict(zip(E3D_KEYS, g["cfg"]))
        err = np.abs(c - g["ref"]).max(1)
        n += int(g["called"].sum()); hit += int((g["called"] & (err <= 1e-6)).sum())
        for i in np.nonzero(g["called"] & (err > 1e-3))[0]:
            lb, ub = e3d_bounds(g["e"][i], cfg["ang_lmt"], cfg["v_lmt"])
            assert np.all(c[i] >= lb - 1e-12) and np.all(c[i] <= ub + 1e-12), (g["name"], i, c[i], lb, ub)
            args = (g["p"][i], g["e"][i], g["target"][i], cfg["e_vmax"], cfg["kill_radius"], cfg["step_size"])
            f_ref, f_dev = e3d_objective(g["ref"][i], *args), e3d_objective(c[i], *args)
            assert f_dev <= f_ref + 1e-6 * max(1.0, abs(f_ref)), (g["name"], i, f_dev, f_ref)
    return n, hit


# ---- above 16 pursuers: evader_n2n_wide.npz / evader_e3d_wide.npz (tests/golden/gen/make_goldens_evader_wide.py) ----

N2N_WIDE_P = (17, 32, 33, 64)                # PM 32, 32, 64, 64
E3D_WIDE_P = (17, 32, 33, 42, 43, 64)        # ... and 42 / 43: the last 64-lane launch (64 512 B of LDS) and the first 32-lane one


def n2n_wide_groups():
    """as n2n_groups(), one group per pursuer count, with `stable`: the mask the generator computed from the reference alone (its
    command moves by at most 1e-7 when every number of the problem moves by a relative 1e-12)"""
    d = np.load(os.path.join(GOLDEN, "evader_n2n_wide.npz"))
    out = []
    for P in N2N_WIDE_P:
        e = d[f"P{P}_e"]
        out.append(dict(name=f"evader_n2n_wide_P{P}", cfg=d["cfg"], P=P, E=1, p=np.ascontiguousarray(d[f"P{P}_p"].transpose(0, 2, 1)),
                        e=np.ascontiguousarray(e[:, :, None]), target=d[f"P{P}_target"], ref=d[f"P{P}_cmd"][:, None],
                        called=(e[:, 4] > 0)[:, None], stable=d[f"P{P}_stable"][:, None]))
    return out


def e3d_wide_groups():
    d = np.load(os.path.join(GOLDEN, "evader_e3d_wide.npz"))
    out = []
    for P in E3D_WIDE_P:
        p, e = d[f"P{P}_p"], d[f"P{P}_e"]
        out.append(dict(name=f"evader_e3d_wide_P{P}", cfg=d["cfg"], P=P, p=np.ascontiguousarray(p.transpose(0, 2, 1)), e=e,
                        target=d[f"P{P}_target"], ref=d[f"P{P}_cmd"], called=(e[:, 6] > 0) & (p[:, :, 6] > 0).any(1),
                        stable=d[f"P{P}_stable"]))
    return out


def check_nit(g, nit):
    """the iteration count is in 1..100 exactly where the reference calls e_f"""
    assert np.all((nit >= 1) == g["called"]) and nit.max() <= 100 and nit.min() >= 0, g["name"]


def n2n_wide_check(g, cmd, nit):
    """one wide env_n2n group: zeros and iteration counts on every problem; on the stable ones at least 97 % within 1e-6 of the
    reference and none beyond 1e-3.  -> (stable calls, hits)"""
    n2n_check([g], [cmd])                                                  # uncalled evaders get exactly 0
    check_nit(g, nit)
    err = np.abs(cmd - g["ref"])[g["called"] & g["stable"]]
    hit = int((err <= 1e-6).sum())
    print(f"{g['name']}: {hit} of {err.size} stable problems within 1e-6, worst {err.max(initial=0.0):.2e}; "
          f"{int((g['called'] & ~g['stable']).sum())} unstable")
    assert hit >= 0.97 * err.size, (g["name"], hit, err.size)
    assert err.max(initial=0.0) <= 1e-3, (g["name"], err.max())
    return err.size, hit


def e3d_wide_check(g, cmd, nit):
    """one wide env_3d group: zeros, iteration counts, bounds and the objective rule of e3d_check for misses beyond 1e-3 on every
    problem; on the stable ones at least 90 % within 1e-6.  -> (stable calls, hits)"""
    e3d_check([g], [cmd])
    check_nit(g, nit)
    cfg = dict(zip(E3D_KEYS, g["cfg"]))
    for i in np.nonzero(g["called"])[0]:
        lb, ub = e3d_bounds(g["e"][i], cfg["ang_lmt"], cfg["v_lmt"])
        assert np.all(cmd[i] >= lb - 1e-12) and np.all(cmd[i] <= ub + 1e-12), (g["name"], i, cmd[i], lb, ub)
    err = np.abs(cmd - g["ref"]).max(1)[g["called"] & g["stable"]]
    hit = int((err <= 1e-6).sum())
    print(f"{g['name']}: {hit} of {err.size} stable problems within 1e-6; {int((g['called'] & ~g['stable']).sum())} unstable")
    assert hit >= 0.90 * err.size, (g["name"], hit, err.size)
    return err.size, hit


def stable_share(g):
    """share of the problems the reference calls e_f on that are stable"""
    return float(g["stable"][g["called"]].mean())
