"""numpy restatement -- and the specification -- of env_3d's line-of-sight policy features (algo.e3d_features: pursuit;
csrc/pursuit_features.hpp, e3d_pursuit_features, e3d_pursuit_features_host).

Records are the device's: p (N, 7, P) and e (N, 7) f64 (x, y, z, phi, gamma, v, active), target (N, 3), time_step (N,), and the
observation's adjacencies pp_adj (N, P, P), pe_adj (N, P).  Every operation is scalar f64 in the order written (plain *, +, -, /, sqrt,
sin, cos; squares and dot products summed x, y, z, left to right), rounded to fp32 at the end, so the kernel differs from this only where
the device's cos / sin differ from libm's, by a few ulp.

A row (pursuer i) has 32 columns, the same for the actor and the critic:
    0-2   p_i / (W / 2) - 1            3-5  u_i = (cos gamma cos phi, cos gamma sin phi, sin gamma)           6  v_i / p_vmax
    7-9   k rh                         10   k d / W                  11-13 k e_vel / e_vmax
    14    k (-rh . (e_vel - v_i u_i)) / (e_vmax + p_vmax)            15    k (u_i . rh)         16  k         17-19 k (target - e_pos) / W
    20-24 nearest visible team-mate: (p_j - p_i) / d_ij (0 when d_ij is 0), d_ij / W, kill_radius / max(d_ij, kill_radius)
    25-29 the second nearest          30   |V_i| / max(P - 1, 1)     31    time_step / max_step
with r = e_pos - p_i, d = |r|, rh = r / d (0 when d is 0), W = 20.  The networks differ in k (who knows the evader: `knows`) and in V
(the visible team-mates: `visible`).  Rows of inactive pursuers are zero; with the evader inactive columns 7-19 are zero."""
import math

import numpy as np

WORLD = 20.0          # E3D_WORLD: the side of the reset cube
FEAT = 32             # E3D_FEAT2
EVADER_OBS = ("sensed", "team", "global")   # E3D_EVADER_OBS_SENSED / _TEAM / _GLOBAL = the index
K_COL, EVADER_COLS = 16, slice(7, 20)


def components(adj, active):
    """labels (P,) of the connected components of the graph over the ACTIVE pursuers with an edge i - j when j != i and adj[i][j] == 1
    or adj[j][i] == 1; an inactive pursuer is a component of its own"""
    P = len(active)
    label = list(range(P))
    link = [[j for j in range(P) if j != i and active[i] and active[j] and (adj[i][j] == 1 or adj[j][i] == 1)] for i in range(P)]
    seen = [False] * P
    for s in range(P):
        if seen[s]:
            continue
        stack, seen[s] = [s], True
        while stack:
            i = stack.pop()
            label[i] = s
            for j in link[i]:
                if not seen[j]:
                    seen[j] = True
                    stack.append(j)
    return label


def knows(evader_obs, pp_adj, pe_adj, active, active_e):
    """the actor's k (P,) of one environment, 0 or 1"""
    if evader_obs not in EVADER_OBS:
        raise ValueError(f"evader_obs: {evader_obs!r} is not one of {EVADER_OBS}")
    P = len(active)
    if not active_e:
        return [0] * P
    if evader_obs == "global":
        return [1] * P
    if evader_obs == "sensed":
        return [int(pe_adj[i] == 1) for i in range(P)]
    label = components(pp_adj, active)
    return [int(any(label[j] == label[i] and active[j] and pe_adj[j] == 1 for j in range(P))) for i in range(P)]


def sq_dist(pos, i, j):
    dx, dy, dz = pos[0][j] - pos[0][i], pos[1][j] - pos[1][i], pos[2][j] - pos[2][i]
    return dx * dx + dy * dy + dz * dz


def visible(pos, i, who):
    """`who` (the indices of V_i) sorted by squared distance to i, the lowest index first on ties"""
    return sorted(who, key=lambda j: (sq_dist(pos, i, j), j))


def _mate(pos, i, j, kill_radius):
    dx, dy, dz = pos[0][j] - pos[0][i], pos[1][j] - pos[1][i], pos[2][j] - pos[2][i]
    d = math.sqrt(dx * dx + dy * dy + dz * dz)
    unit = (0.0, 0.0, 0.0) if d == 0.0 else (dx / d, dy / d, dz / d)
    return [*unit, d / WORLD, kill_radius / max(d, kill_radius)]


def _row(cfg, s, ev, tg, t, k, pos, i, who):
    """s = (x, y, z, phi, gamma, v) of pursuer i, ev the evader's record, k in {0, 1}, who = V_i"""
    f = [0.0] * FEAT
    x, y, z, phi, gamma, v = (float(a) for a in s)
    half = WORLD / 2
    cg = math.cos(gamma)
    u = (cg * math.cos(phi), cg * math.sin(phi), math.sin(gamma))
    f[0:3] = x / half - 1, y / half - 1, z / half - 1
    f[3:6] = u
    f[6] = v / cfg["p_vmax"]
    if k:
        ex, ey, ez, ephi, egam, evel = (float(a) for a in ev[:6])
        r = (ex - x, ey - y, ez - z)
        d = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        rh = (0.0, 0.0, 0.0) if d == 0.0 else (r[0] / d, r[1] / d, r[2] / d)
        ecg = math.cos(egam)
        e_vel = (evel * ecg * math.cos(ephi), evel * ecg * math.sin(ephi), evel * math.sin(egam))
        w = (e_vel[0] - v * u[0], e_vel[1] - v * u[1], e_vel[2] - v * u[2])
        f[7:10] = rh
        f[10] = d / WORLD
        f[11:14] = e_vel[0] / cfg["e_vmax"], e_vel[1] / cfg["e_vmax"], e_vel[2] / cfg["e_vmax"]
        f[14] = (-rh[0] * w[0] + -rh[1] * w[1] + -rh[2] * w[2]) / (cfg["e_vmax"] + cfg["p_vmax"])
        f[15] = u[0] * rh[0] + u[1] * rh[1] + u[2] * rh[2]
        f[16] = 1.0
        f[17:20] = (float(tg[0]) - ex) / WORLD, (float(tg[1]) - ey) / WORLD, (float(tg[2]) - ez) / WORLD
    near = visible(pos, i, who)
    for b, j in enumerate(near[:2]):
        f[20 + 5 * b:25 + 5 * b] = _mate(pos, i, j, cfg["kill_radius"])
    P = len(pos[0])
    f[30] = len(near) / max(P - 1, 1)
    f[31] = int(t) / int(cfg["max_step"])
    return f


def pursuit_features(cfg, p, e, target, time_step, pp_adj, pe_adj, evader_obs):
    """cfg: a mapping with p_vmax, e_vmax, kill_radius, max_step.  -> (actor, critic), each (N, P, 32) fp32"""
    p, e = np.asarray(p, np.float64), np.asarray(e, np.float64).reshape(len(p), 7)
    target, time_step = np.asarray(target, np.float64), np.asarray(time_step)
    pp_adj, pe_adj = np.asarray(pp_adj), np.asarray(pe_adj).reshape(len(p), -1)
    N, _, P = p.shape
    fa, fc = np.zeros((N, P, FEAT), np.float64), np.zeros((N, P, FEAT), np.float64)
    for n in range(N):
        pos = [[float(a) for a in p[n, c]] for c in range(3)]
        active, active_e = [bool(a != 0.0) for a in p[n, 6]], bool(e[n, 6] != 0.0)
        ka = knows(evader_obs, pp_adj[n], pe_adj[n], active, active_e)
        for i in range(P):
            if not active[i]:
                continue
            mates = [j for j in range(P) if j != i and active[j]]
            fa[n, i] = _row(cfg, p[n, :6, i], e[n], target[n], time_step[n], ka[i], pos, i, [j for j in mates if pp_adj[n, i, j] == 1])
            fc[n, i] = _row(cfg, p[n, :6, i], e[n], target[n], time_step[n], int(active_e), pos, i, mates)
    return fa.astype(np.float32), fc.astype(np.float32)


def nearest_gap(p, pp_adj=None):
    """the smallest relative gap between the two smallest squared team-mate distances of any active pursuer (over all its active
    team-mates, which contain the actor's visible ones), and the number of rows it was taken over: below ~1e-9 a last-bit difference
    could swap the nearest two"""
    p = np.asarray(p, np.float64)
    N, _, P = p.shape
    gap, rows = np.inf, 0
    for n in range(N):
        pos = [[float(a) for a in p[n, c]] for c in range(3)]
        for i in range(P):
            if p[n, 6, i] == 0.0:
                continue
            rows += 1
            d = sorted(sq_dist(pos, i, j) for j in range(P) if j != i and p[n, 6, j] != 0.0)
            for a, b in zip(d, d[1:]):     # every adjacent pair: a subset's nearest two are adjacent in some subset, never closer than these
                gap = min(gap, (b - a) / max(b, 1e-300))
    return gap, rows


def policy_features(p, e, pp, pe):
    """the 16 basic features of e3d_policy_features (algo.e3d_features: basic), which the GPU tests hold to 1e-6 (rtol and atol):
    p (N, 7, P), e (N, 7) f64 records; pp (N, P, P), pe (N, P) -> actor, critic (N, P, 16) fp32"""
    N, _, P = p.shape
    fa, fc = np.zeros((N, P, 16), np.float32), np.zeros((N, P, 16), np.float32)
    for n in range(N):
        for i in range(P):
            if p[n, 6, i] == 0:
                continue
            s = p[n, :6, i]
            ae = e[n, 6]
            fa[n, i, :6] = fc[n, i, :6] = s
            fa[n, i, 6:12] = (e[n, :6] - s) * pe[n, i]
            fc[n, i, 6:12] = (e[n, :6] - s) * ae
            fa[n, i, 12], fc[n, i, 12] = pe[n, i], ae
            ja = [j for j in range(P) if j != i and pp[n, i, j] == 1]
            jc = [j for j in range(P) if j != i and p[n, 6, j] != 0]
            for js, f in ((ja, fa), (jc, fc)):
                if js:
                    f[n, i, 13:16] = np.mean([p[n, :3, j] - p[n, :3, i] for j in js], axis=0)
    return fa, fc
