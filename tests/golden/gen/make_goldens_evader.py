"""Golden vectors for the on-device SLSQP evader of env_n2n and env_3d (csrc/slsqp_box.hpp, n2n_evader_slsqp / e3d_evader_slsqp).

Samples single evader problems -- one evader, its pursuers, the target -- and records the command of the reference's own
eva.e_f (environment/env_n2n/eva.py:36-80, environment/env_3d/eva.py:87-148; scipy SLSQP) for each, called as the reference's
evader_step calls it: with the ACTIVE pursuers only (get_team_state rules=True), the full pursuer speed list in env_n2n.
Commands for problems on which the reference never calls e_f are 0, as in make_goldens_n2n.py / make_goldens_e3d.py: an inactive
evader (both environments) or no active pursuer (env_3d).
The sample mixes generic states with the edge cases: no pursuer in sensing range, a pursuer near the kill radius, inactive
pursuers ahead of in-range ones (the p_v0[ne] speed-index quirk of env_n2n), env_3d evaders whose bounds clip at +-1, and
1, 8 and 16 pursuers.  Records are grouped by pursuer count: P{k}_p [M, k, 5|7], P{k}_e [M, 5|7], P{k}_target, P{k}_cmd.
Usage:  python tests/golden/gen/make_goldens_evader.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refload  # noqa: E402

refload.activate()
OUT = os.path.dirname(HERE)
PS = (1, 8, 16)
E_SR = 3.0  # e_sen_range of both reference environments


def _around(rng, c, P, kind, dim):
    """pursuer positions around the evader position c for one sampled case"""
    r = rng.uniform(0.0, 4.5, P)
    if kind == "none_in_range":
        r = rng.uniform(3.2, 8.0, P)
    elif kind == "kill":
        r[0] = rng.uniform(0.35, 0.75)
    if dim == 2:
        a = rng.uniform(-np.pi, np.pi, P)
        return np.stack((c[0] + r * np.cos(a), c[1] + r * np.sin(a)), 1)
    u = rng.normal(size=(P, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return c[None, :] + r[:, None] * u


def _active(rng, P, kind):
    act = (rng.random(P) < 0.85).astype(np.float64)
    if kind == "inactive_ahead" and P > 1:
        k = max(1, P // 3)
        act[:k] = 0.0  # the first pursuers are out: in-range indices no longer equal full-list indices
        act[k:] = 1.0
    return act


def _f32(a):
    """states are sampled on float32-representable values (the command is computed from them, so nothing is lost): the records
    compress to well under 1 MB"""
    return np.asarray(a, np.float32).astype(np.float64)


def _kinds(rng):
    return rng.choice(["generic", "none_in_range", "kill", "inactive_ahead", "generic"])


def n2n_problem(rng, P):
    """one sampled env_n2n problem: e [5], p [P, 5], target [2]"""
    kind = _kinds(rng)
    e = np.array([rng.uniform(2, 18), rng.uniform(2, 18), rng.uniform(-np.pi, np.pi), 1.0, 1.0])
    if rng.random() < 0.03:
        e = np.array([1000.0, 1000.0, 0.0, 1.0, 0.0])  # a captured evader: e_f is not called
    xy = _around(rng, e[:2], P, kind, 2)
    p = np.zeros((P, 5))
    p[:, :2] = xy
    p[:, 2] = rng.uniform(-np.pi, np.pi, P)
    p[:, 3] = np.where(rng.random(P) < 0.3, 0.0, rng.uniform(0.0, 0.3, P))  # distinct speeds expose p_v0[ne]
    p[:, 4] = _active(rng, P, kind)
    p[p[:, 4] == 0, :3] = (1000.0, 1000.0, 0.0)
    tg = rng.uniform(0, 20, 2)
    return _f32(e), _f32(p), _f32(tg)


def n2n_command(eva, e, p, tg):
    """the reference's command for one problem, 0 where evader_step does not call e_f"""
    if not e[4] > 0:
        return 0.0
    on = p[:, 4] > 0
    return float(eva.e_f(xy=np.array(e[:2]), e_ga=e[2], e_v=e[3], e_sr=E_SR, npx=list(p[on, 0]), npy=list(p[on, 1]),
                         bet=list(p[on, 2]), p_v=list(p[:, 3]), p_=10, d_=1, m_=5, tp=list(tg)))


N2N_CFG = np.asarray([0.3, 1.0, 3.0, 6.0, 0.5, np.pi / 4, 0.5])


def n2n(rng, per_p):
    from environment.env_n2n import eva
    out = {}
    for P in PS:
        ps, es, ts, cs = [], [], [], []
        for _ in range(per_p):
            e, p, tg = n2n_problem(rng, P)
            ps.append(p); es.append(e); ts.append(tg); cs.append(n2n_command(eva, e, p, tg))
        out[f"P{P}_p"], out[f"P{P}_e"], out[f"P{P}_target"], out[f"P{P}_cmd"] = map(np.asarray, (ps, es, ts, cs))
    # p_vmax, e_vmax, p_sen_range, p_comm_range, kill_radius, ang_lmt, step_size (particle_env.py:108-121,147)
    out["cfg"] = N2N_CFG
    return out


E3D_KILL, E3D_ANG, E3D_VL, E3D_H, E3D_VMAX = 0.5, np.pi / 4, 0.4, 0.5, 1.0
# p_vmax, e_vmax, p_sen_range, p_comm_range, kill_radius, ang_lmt, v_lmt, step_size (particle_env.py:78-121)
E3D_CFG = np.asarray([0.7, E3D_VMAX, 3.0, 6.0, E3D_KILL, E3D_ANG, E3D_VL, E3D_H])


def e3d_problem(rng, P):
    """one sampled env_3d problem: e [7], p [P, 7], target [3]"""
    kind = _kinds(rng)
    phi, gam, v = rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi / 2, np.pi / 2), rng.uniform(0, 1)
    if rng.random() < 0.25:  # bounds clipped at +-1: heading near +-pi, pitch near +-pi/2, speed near 0 or 1
        phi = np.sign(rng.random() - 0.5) * rng.uniform(0.8 * np.pi, np.pi)
        gam = np.sign(rng.random() - 0.5) * rng.uniform(0.35 * np.pi, 0.5 * np.pi)
        v = rng.choice([rng.uniform(0, 0.3), rng.uniform(0.7, 1.0)])
    e = np.array([*rng.uniform(2, 18, 3), phi, gam, v, 1.0])
    if rng.random() < 0.03:
        e[6] = 0.0
    p = np.zeros((P, 7))
    p[:, :3] = _around(rng, e[:3], P, kind, 3)
    p[:, 3] = rng.uniform(-np.pi, np.pi, P)
    p[:, 4] = rng.uniform(-np.pi / 2, np.pi / 2, P)
    p[:, 5] = rng.uniform(0, 0.7, P)
    p[:, 6] = _active(rng, P, kind)
    if rng.random() < 0.03:
        p[:, 6] = 0.0  # no pursuer left: evader_step is not called
    tg = rng.uniform(0, 20, 3)
    return _f32(e), _f32(p), _f32(tg)


def e3d_command(eva, e, p, tg):
    """the reference's command for one problem, zeros where evader_step does not call e_f"""
    on = p[:, 6] > 0
    if not (e[6] > 0 and on.any()):
        return np.zeros(3)
    return np.asarray(eva.e_f(xyz=np.array(e[:3]), e_phi=e[3], e_ga=e[4], e_v=e[5], e_v_max=E3D_VMAX, e_sr=E_SR,
                              npx=list(p[on, 0]), npy=list(p[on, 1]), npz=list(p[on, 2]), nphi=list(p[on, 3]),
                              ngamma=list(p[on, 4]), nv=list(p[on, 5]), tp=list(tg), time_step=E3D_H, ang_lmt=E3D_ANG, v_lmt=E3D_VL,
                              kill_radius=E3D_KILL), np.float64)


def e3d(rng, per_p):
    from environment.env_3d import eva
    out = {}
    for P in PS:
        ps, es, ts, cs = [], [], [], []
        for _ in range(per_p):
            e, p, tg = e3d_problem(rng, P)
            ps.append(p); es.append(e); ts.append(tg); cs.append(e3d_command(eva, e, p, tg))
        out[f"P{P}_p"], out[f"P{P}_e"], out[f"P{P}_target"], out[f"P{P}_cmd"] = map(np.asarray, (ps, es, ts, cs))
    out["cfg"] = E3D_CFG
    return out


def main():
    warnings.simplefilter("ignore")
    for name, fn, seed in (("evader_n2n", n2n, 11), ("evader_e3d", e3d, 13)):
        o = fn(np.random.default_rng(seed), 700)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **o)
        print(name, sum(len(o[f"P{P}_cmd"]) for P in PS), "records,", os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
