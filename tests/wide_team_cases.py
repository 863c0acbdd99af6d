"""Episodes of env_3d and env_n2n with more than 16 pursuers: the lane groups of 32 and 64 lanes per environment (PT) of every kernel
in the tick's lane layout (csrc/e3d_env.hip, csrc/n2n_env.hip), which no narrower team reaches.

reset() cannot seat such teams (the reference's placement rejects points closer than 4 / 2 and gives up or, in the reference itself,
never returns), so every case is an initial state made here -- pursuers on a jittered grid, the evader(s) just outside it -- that the
tests inject through reset(init=...), a stream of pursuer actions and of evader commands for T ticks, and the ORACLE's trace of that
episode (oracle/e3d_oracle.py, oracle/n2n_oracle.py), computed once per case and shared.  About half of the team is steered at the
evader, so pursuers collide and evaders are caught; in the even environments the evaders fly into the team, in the odd ones they wander.

The environment counts are the smallest that put every kind of wave into one launch; launch() restates the launch arithmetic
(n2n_lanes / e3d_lanes: 4 waves per workgroup, 64 / PT environments per wave) and tests/test_wide_team_cases_cpu.py asserts the classes.
Shared by tests/test_wide_team_cases_cpu.py and tests/test_wide_teams_gpu.py."""
import functools
from collections import namedtuple

import numpy as np

from tests import guidance_ref

WAVE, WPB = 64, 4
T = 25
KILL_RADIUS, COMM_RANGE, SEN_RANGE = 0.5, 6.0, 3.0     # the defaults of both environments
E3D_CASES = ((17, 1, 19), (32, 1, 19), (33, 1, 11), (64, 1, 11))   # (P, E, N)
N2N_CASES = ((17, 1, 19), (32, 8, 19), (33, 2, 11), (64, 8, 11))
CASES = [("e3d",) + c for c in E3D_CASES] + [("n2n",) + c for c in N2N_CASES]
ONE_PER_PT = [("e3d", 32, 1, 19), ("e3d", 64, 1, 11), ("n2n", 32, 8, 19), ("n2n", 64, 8, 11)]
GUIDANCE_TICKS = (0, 8, 16)     # states the guidance, shaping and policy-input kernels are compared on: the start and two mid-episode
IDS = lambda c: f"{c[0]}-P{c[1]}-E{c[2]}-N{c[3]}"

Launch = namedtuple("Launch", "pt envs_per_block blocks full_waves mixed_waves dead_waves dead_waves_in_last_block")


def lanes(P, E=1):
    m = max(P, E)
    return 8 if m <= 8 else 16 if m <= 16 else 32 if m <= 32 else 64


def launch(P, E, N):
    """the grid of a launch in the tick's lane layout, and its waves by what they hold: only live groups, a live group beside one
    past N, only groups past N"""
    pt = lanes(P, E)
    G = WAVE // pt
    envs_per_block = G * WPB
    blocks = -(-N // envs_per_block)
    full = mixed = dead = dead_last = 0
    for w in range(blocks * WPB):
        live = sum(1 for g in range(G) if w * G + g < N)
        full += live == G
        mixed += 0 < live < G
        dead += live == 0
        dead_last += live == 0 and w // WPB == blocks - 1
    return Launch(pt, envs_per_block, blocks, full, mixed, dead, dead_last)


# ---- initial states -------------------------------------------------------------------------------------------------------------------
def _grid(rng, P, D, spacing, jitter):
    """P points of a jittered D-dimensional grid around (10, ..): neighbours are at least spacing - 2 jitter apart"""
    side = int(np.ceil(P ** (1.0 / D) - 1e-9))
    cells = np.stack(np.meshgrid(*[np.arange(side)] * D, indexing="ij"), -1).reshape(-1, D)
    cells = cells[rng.permutation(len(cells))[:P]]
    return 10.0 + (cells - (side - 1) / 2.0) * spacing + rng.uniform(-jitter, jitter, (P, D)), side * spacing / 2.0


def _outside(rng, D, radius):
    u = rng.normal(size=D)
    return 10.0 + u / np.linalg.norm(u) * radius


def upper_half_envs(N):
    """the environments whose team starts with the lower half of the lane group inactive: an odd one (at PT 32 the second group of its
    wave) and the last one"""
    return (1, N - 1)


def _park_lower_half(p, P, E, D):
    """pursuers 0 .. PT / 2 - 1 out from the start, parked as the tick parks them: whether a pursuer is left, and who hits the evader,
    is then decided by the upper lanes of the group alone, which is where a group mask built for the narrower width goes wrong"""
    for n in upper_half_envs(len(p)):
        p[n, :lanes(P, E) // 2] = 0.0
        p[n, :lanes(P, E) // 2, :D] = 1000.0


def e3d_init(P, N, seed=0):
    """-> p (N, P, 7), e (N, 7), target (N, 3) in the host order of reset(init=...): x, y, z, phi, gamma, v, active"""
    rng = np.random.RandomState(3000 + 10 * P + seed)
    p, e, tg = np.zeros((N, P, 7)), np.zeros((N, 7)), np.zeros((N, 3))
    for n in range(N):
        p[n, :, :3], half = _grid(rng, P, 3, 2.4, 0.5)
        p[n, :, 3], p[n, :, 4], p[n, :, 6] = rng.uniform(-np.pi, np.pi, P), rng.uniform(-1.2, 1.2, P), 1.0
        e[n, :3] = _outside(rng, 3, half * np.sqrt(3) + rng.uniform(0.5, 1.5))
        e[n, 3], e[n, 4], e[n, 5], e[n, 6] = rng.uniform(-np.pi, np.pi), rng.uniform(-1.2, 1.2), 0.5, 1.0
        tg[n] = _outside(rng, 3, 25.0)
    _park_lower_half(p, P, 1, 3)
    return p, e, tg


def n2n_init(P, E, N, seed=0):
    """-> p (N, P, 5), e (N, E, 5), target (N, 2): x, y, phi, v, active"""
    rng = np.random.RandomState(2000 + 10 * P + E + seed)
    p, e, tg = np.zeros((N, P, 5)), np.zeros((N, E, 5)), np.zeros((N, 2))
    for n in range(N):
        p[n, :, :2], half = _grid(rng, P, 2, 1.6, 0.4)
        p[n, :, 2], p[n, :, 4] = rng.uniform(-np.pi, np.pi, P), 1.0
        a0 = rng.uniform(-np.pi, np.pi)
        for k in range(E):   # around the team, at least 2 apart
            a, r = a0 + 2 * np.pi * k / E, half * np.sqrt(2) + rng.uniform(0.5, 1.5)
            e[n, k, :2] = 10.0 + r * np.cos(a), 10.0 + r * np.sin(a)
        e[n, :, 2], e[n, :, 3], e[n, :, 4] = rng.uniform(-np.pi, np.pi, E), 1.0, 1.0
        tg[n] = _outside(rng, 2, 30.0)
    _park_lower_half(p, P, E, 2)
    if N > 3:   # one environment ends because an evader reaches the target: two ticks straight ahead of evader 0
        tg[3] = e[3, 0, :2] + 1.0 * np.array([np.cos(e[3, 0, 2]), np.sin(e[3, 0, 2])])
    return p, e, tg


# ---- the oracle's episode -------------------------------------------------------------------------------------------------------------
def _bearing(dx, dy):
    return np.arctan2(dy, dx)


def _e3d_episode(P, N):
    from oracle import e3d_oracle as eo
    p0, e0, tg = e3d_init(P, N)
    cfg = eo.make_cfg(P, T)      # the last tick ends every episode still running on the time limit
    envs = [eo.OracleE3d(cfg, p0[n], e0[n], tg[n]) for n in range(N)]
    rng = np.random.RandomState(7000 + P)
    out = dict(kind="e3d", P=P, E=1, N=N, init=(p0, e0, tg), max_step=T,
               action=np.zeros((T, N, P, 3)), cmd=np.zeros((T, N, 3)), p=np.zeros((T + 1, N, 7, P)), e=np.zeros((T + 1, N, 7)),
               reward=np.zeros((T, N, P), np.float32), active=np.zeros((T, N, P), np.uint8), done=np.zeros((T, N), bool),
               p_state=np.zeros((T + 1, N, P, 6), np.float32), e_state=np.zeros((T + 1, N, 1, 6), np.float32),
               pp_adj=np.zeros((T + 1, N, P, P), np.float32), pe_adj=np.zeros((T + 1, N, P, 1), np.float32))

    def snap(t):
        for n, oe in enumerate(envs):
            out["p"][t, n], out["e"][t, n] = oe.p.T, oe.e[0]
            out["p_state"][t, n], out["e_state"][t, n], out["pp_adj"][t, n], out["pe_adj"][t, n] = oe.observe()

    snap(0)
    for t in range(T):
        for n, oe in enumerate(envs):
            act = rng.uniform(-1, 1, (P, 3))
            d = oe.e[0, :3] - oe.p[:, :3]
            chase = rng.random_sample(P) < 0.5
            act[:, 0] = np.where(chase, _bearing(d[:, 0], d[:, 1]) / np.pi, act[:, 0])
            act[:, 1] = np.where(chase, np.arctan2(d[:, 2], np.hypot(d[:, 0], d[:, 1])) / (np.pi / 2), act[:, 1])
            act[:, 2] = np.where(chase, 1.0, act[:, 2])
            cmd = rng.uniform(-1, 1, 3)
            if n % 2 == 0:   # into the team
                c = 10.0 - oe.e[0, :3]
                cmd = np.array([_bearing(c[0], c[1]) / np.pi, np.arctan2(c[2], np.hypot(c[0], c[1])) / (np.pi / 2), 1.0])
            out["action"][t, n], out["cmd"][t, n] = act, cmd
            if oe.e[0, 6] > 0 and oe.p[:, 6].sum() > 0:   # ParticleEnv.step: the evader moves only while the episode has both sides
                oe.evader_step(cmd)
            r, done, active = oe.step(act)
            out["reward"][t, n], out["done"][t, n], out["active"][t, n] = r.astype(np.float32), done, active
        snap(t + 1)
    return out


def _n2n_episode(P, E, N):
    from oracle import n2n_oracle as no
    p0, e0, tg = n2n_init(P, E, N)
    cfg = no.make_cfg(P, E, T)
    envs = [no.OracleN2n(cfg, p0[n], e0[n], tg[n]) for n in range(N)]
    rng = np.random.RandomState(8000 + 10 * P + E)
    out = dict(kind="n2n", P=P, E=E, N=N, init=(p0, e0, tg), max_step=T,
               action=np.zeros((T, N, P), np.int32), cmd=np.zeros((T, N, E)), p=np.zeros((T + 1, N, 5, P)), e=np.zeros((T + 1, N, 5, E)),
               reward=np.zeros((T, N, P), np.float32), active=np.zeros((T, N, P), np.uint8), done=np.zeros((T, N), bool),
               p_state=np.zeros((T + 1, N, P, 3), np.float32), e_state=np.zeros((T + 1, N, E, 3), np.float32),
               pp_adj=np.zeros((T + 1, N, P, P), np.float32), pe_adj=np.zeros((T + 1, N, P, E), np.float32))

    def snap(t):
        for n, oe in enumerate(envs):
            out["p"][t, n], out["e"][t, n] = oe.p.T, oe.e.T
            out["p_state"][t, n], out["e_state"][t, n], out["pp_adj"][t, n], out["pe_adj"][t, n] = oe.observe()

    snap(0)
    for t in range(T):
        for n, oe in enumerate(envs):
            act = rng.randint(0, 9, P).astype(np.int32)
            d = oe.e[None, :, :2] - oe.p[:, None, :2]                    # (P, E, 2)
            k = np.where(oe.e[None, :, 4] > 0, np.hypot(d[..., 0], d[..., 1]), np.inf).argmin(1)
            dk = d[np.arange(P), k]
            chase = rng.random_sample(P) < 0.5
            act = np.where(chase, guidance_ref.octant(_bearing(dk[:, 0], dk[:, 1])), act).astype(np.int32)
            cmd = rng.uniform(-1, 1, E)
            if n % 2 == 0 and not (n == 3):
                cmd = _bearing(10.0 - oe.e[:, 0], 10.0 - oe.e[:, 1]) / np.pi
            if n == 3:
                cmd[0] = oe.e[0, 2] / np.pi                              # evader 0 keeps its heading: straight at the target
            out["action"][t, n], out["cmd"][t, n] = act, cmd
            oe.evader_step(cmd)
            r, done, active = oe.step(act)
            out["reward"][t, n], out["done"][t, n], out["active"][t, n] = r.astype(np.float32), done, active
        snap(t + 1)
    return out


@functools.lru_cache(maxsize=None)
def episode(kind, P, E, N):
    """the case and the oracle's trace of it.  Index t of p, e, p_state, e_state, pp_adj, pe_adj is the state tick t starts from (T is the
    final one), index t of action, cmd, reward, active, done belongs to tick t.  Records p (N, C, P), e (N, C, E) / env_3d (N, 7) as on
    the device.  Treat it as read-only: it is shared."""
    ep = _e3d_episode(P, N) if kind == "e3d" else _n2n_episode(P, E, N)
    for v in ep.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ep


def done_before(ep):
    """(T + 1, N) bool: the environment reported done in an earlier tick"""
    db = np.zeros((T + 1, ep["N"]), bool)
    db[1:] = np.cumsum(ep["done"], 0) > 0
    return db


def min_initial_distance(ep):
    p0 = ep["init"][0]
    D = 3 if ep["kind"] == "e3d" else 2
    d = np.linalg.norm(p0[:, :, None, :D] - p0[:, None, :, :D], axis=-1)
    off = p0[:, :, -1] == 0
    return float((d + 1e9 * (np.eye(d.shape[1], dtype=bool)[None] | off[:, :, None] | off[:, None, :])).min())
