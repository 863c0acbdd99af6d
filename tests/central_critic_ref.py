"""numpy restatement -- and the specification -- of env_3d's centralised critic input (algo.e3d_critic: central;
csrc/central_critic.hpp, e3d_central_features, e3d_central_features_host), on top of tests/e3d_features_ref.py.

The actor's rows are pursuit_features' actor rows.  The critic's row of an active pursuer i has feat(P) = 32 + 8 (P - 1) columns:
    0-31           the critic row of pursuit_features
    32 + 8 s ...   slot s = 0 .. P - 2: the s-th team-mate j of V_i = the active j != i, by ascending squared distance, the lowest index
                   first on an exact tie (ref.visible) --
                   0-2 (p_j - p_i) / d_ij (0 when d_ij is 0)    3 d_ij / W    4-6 u_j = (cos gamma_j cos phi_j, cos gamma_j sin phi_j, sin gamma_j)
                   7 v_j / p_vmax
Slots s >= |V_i| are zero, the row of an inactive pursuer is zero.  Scalar f64 in the order written, rounded to fp32 at the end."""
import math

import numpy as np

from tests import e3d_features_ref as ref

MATE = 8       # E3D_CENTRAL_MATE
MAX_P = 16     # E3D_CENTRAL_MAX_P


def feat(P):
    """E3D_CENTRAL_FEAT(P)"""
    return ref.FEAT + MATE * (P - 1)


def _slot(cfg, pos, i, j, rec):
    """rec = (x, y, z, phi, gamma, v) of team-mate j"""
    dx, dy, dz = pos[0][j] - pos[0][i], pos[1][j] - pos[1][i], pos[2][j] - pos[2][i]
    d = math.sqrt(dx * dx + dy * dy + dz * dz)
    unit = (0.0, 0.0, 0.0) if d == 0.0 else (dx / d, dy / d, dz / d)
    phi, gamma, v = float(rec[3]), float(rec[4]), float(rec[5])
    cg = math.cos(gamma)
    return [*unit, d / ref.WORLD, cg * math.cos(phi), cg * math.sin(phi), math.sin(gamma), v / cfg["p_vmax"]]


def central_features(cfg, p, e, target, time_step, pp_adj, pe_adj, evader_obs):
    """-> (actor (N, P, 32), critic (N, P, feat(P))) fp32"""
    p = np.asarray(p, np.float64)
    N, _, P = p.shape
    if P > MAX_P:
        raise ValueError(f"P = {P} is above {MAX_P}")
    fa, fc32 = ref.pursuit_features(cfg, p, e, target, time_step, pp_adj, pe_adj, evader_obs)
    fc = np.zeros((N, P, feat(P)), np.float64)
    fc[..., :ref.FEAT] = fc32
    for n in range(N):
        pos = [[float(a) for a in p[n, c]] for c in range(3)]
        active = [bool(a != 0.0) for a in p[n, 6]]
        for i in range(P):
            if not active[i]:
                continue
            for s, j in enumerate(ref.visible(pos, i, [j for j in range(P) if j != i and active[j]])):
                fc[n, i, ref.FEAT + MATE * s:ref.FEAT + MATE * (s + 1)] = _slot(cfg, pos, i, j, p[n, :6, j])
    return fa, fc.astype(np.float32)


def order(p):
    """the team-mate index behind every slot, (N, P, P - 1) int, -1 for an empty slot or an inactive pursuer's row"""
    p = np.asarray(p, np.float64)
    N, _, P = p.shape
    out = np.full((N, P, max(P - 1, 0)), -1, np.int64)
    for n in range(N):
        pos = [[float(a) for a in p[n, c]] for c in range(3)]
        for i in range(P):
            if p[n, 6, i] == 0.0:
                continue
            for s, j in enumerate(ref.visible(pos, i, [j for j in range(P) if j != i and p[n, 6, j] != 0.0])):
                out[n, i, s] = j
    return out
