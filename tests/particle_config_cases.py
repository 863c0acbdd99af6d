"""env_3d and env_n2n away from their default constants and on the edge of every range test.

Two things the other cases of these environments leave open.  They all run at the default physical constants, so a literal standing
where a field of e3d_config / n2n_config belongs, or a rate limit taken from the wrong field, changes nothing they see; and their
random placements never come within an ulp of a radius, so the kernels' replacement of `norm(..) <= r` by `sq(..) <= sq_threshold(r)`
(csrc/e3d_env.hip, csrc/n2n_env.hip) has never been evaluated where it could differ from the reference.

Configs: CONFIGS[kind] names off-default configs whose every physical field differs from the default and is no dyadic rational.
`tight` has the radii 0.7 / 2.1 / 6.1, for each of which the largest double T with sqrt(T) <= r lies one ulp ABOVE fl(r r); `far` has
the sensing range above the communication range.  THRESHOLD_OFFSET states T - fl(r r) in ulps for every radius in use.

Edge states: for a radius r, displacements d whose squared norm -- the oracle's chain fma(c, c, fma(b, b, a a)), evaluated exactly in
rationals and rounded once per fma -- is exactly T (class `on`: inside), one double above T (`above`: outside), or on the other side of T
than the unfused sum (a a + b b) + c c (`order`), found by a seeded search over directions.  Every coordinate of d is a multiple of
Q = 2^-49 and the pair stands at base + d and base with base a multiple of Q near 9, so both positions are exact doubles below 16 and
the difference a kernel forms is d itself.  edge_batch() puts one such pair into each environment -- two pursuers (kill, comm), a
pursuer and an evader (kill, sen) or an evader and the target (reach), in the first or in the last slots -- with every other agent on
a lattice 8 apart and 20 away; nobody moves (env_3d: v = 0 and a speed command of -1; env_n2n: action 0 and evaders with v = 0), so
one tick evaluates the injected positions.  The ORACLE (oracle/e3d_oracle.c, oracle/n2n_oracle.c) gives the expected outputs.

Episodes: episode(kind, name) is the oracle's trace of N = 40 environments over T = 30 ticks under an off-default config, in the
format of tests/wide_team_cases.py.

Shared by tests/test_particle_config_cases_cpu.py and tests/test_particle_config_gpu.py."""
import functools
import math
from fractions import Fraction

import numpy as np

from tests import guidance_ref
from tests import wide_team_cases as wc

PI = math.pi
DEFAULTS = dict(
    e3d=dict(max_step=200, p_vmax=0.7, e_vmax=1.0, p_sen_range=3.0, p_comm_range=6.0, kill_radius=0.5, ang_lmt=PI / 4, v_lmt=0.4, step_size=0.5),
    n2n=dict(episode_limit=100, p_vmax=0.3, e_vmax=1.0, p_sen_range=3.0, p_comm_range=6.0, kill_radius=0.5, ang_lmt=PI / 4, step_size=0.5))
_TIGHT = dict(kill_radius=0.7, p_sen_range=2.1, p_comm_range=6.1, p_vmax=1.1, e_vmax=0.6, ang_lmt=PI / 7, step_size=0.3)
_FAR = dict(kill_radius=0.35, p_sen_range=5.3, p_comm_range=4.7, p_vmax=0.9, e_vmax=1.3, ang_lmt=PI / 5, step_size=0.45)
CONFIGS = dict(
    e3d=dict(tight=dict(_TIGHT, v_lmt=0.15, max_step=7), far=dict(_FAR, v_lmt=0.3, max_step=23)),
    n2n=dict(tight=dict(_TIGHT, episode_limit=7), far=dict(_FAR, episode_limit=23)))
LIMIT_KEY = dict(e3d="max_step", n2n="episode_limit")
PHYSICAL = ("p_vmax", "e_vmax", "p_sen_range", "p_comm_range", "kill_radius", "ang_lmt", "v_lmt", "step_size")
KINDS = ("e3d", "n2n")
DIMS = dict(e3d=3, n2n=2)
STATE_W = dict(e3d=6, n2n=3)      # the columns of p_state / e_state

# T - fl(r r) in ulps, T the largest double with sqrt(T) <= r: the radii whose threshold is NOT the rounded square stay in the set
THRESHOLD_OFFSET = {0.7: 1, 2.1: 1, 6.1: 1, 1.1: 1, 0.35: 1, 0.5: 1, 3.0: 0, 6.0: 0, 0.3: 0, 4.7: 0, 5.3: 0}


def config(kind, name):
    """the keyword arguments ParticleEnv and oracle.*.make_cfg take, every field named"""
    return dict(DEFAULTS[kind]) if name == "default" else dict(DEFAULTS[kind], **CONFIGS[kind][name])


def oracle_cfg(kind, name, P, E=1):
    if kind == "e3d":
        from oracle import e3d_oracle as eo
        return eo.make_cfg(P, **config(kind, name))
    from oracle import n2n_oracle as no
    return no.make_cfg(P, E, **config(kind, name))


def features_cfg(name):
    """the dict tests/e3d_features_ref.py and tests/central_critic_ref.py read (e3d_features_cases.CFG under a config)"""
    c = config("e3d", name)
    return {k: c[k] for k in ("p_vmax", "e_vmax", "kill_radius", "max_step", "p_comm_range", "p_sen_range")}


# ---- the squared norm and its threshold, exactly ------------------------------------------------------------------------------------------
def fma(a, b, c):
    """the correctly rounded a b + c"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def sq_fma(d):
    """the oracle's norm3 / norm2 before the root: fma(c, c, fma(b, b, a a))"""
    s = d[0] * d[0]
    for x in d[1:]:
        s = fma(x, x, s)
    return s


def sq_plain(d):
    """(a a + b b) + c c, every operation rounded"""
    s = d[0] * d[0]
    for x in d[1:]:
        s = s + x * x
    return s


def sq_threshold(r):
    """the largest double t with sqrt(t) <= r (math.sqrt is the correctly rounded root)"""
    t = r * r
    while not math.sqrt(t) <= r:
        t = math.nextafter(t, 0.0)
    while math.sqrt(math.nextafter(t, math.inf)) <= r:
        t = math.nextafter(t, math.inf)
    return t


def threshold_offset(r):
    """T - fl(r r) in ulps"""
    t, sq, n = sq_threshold(r), r * r, 0
    while sq < t:
        sq, n = math.nextafter(sq, math.inf), n + 1
    while sq > t:
        sq, n = math.nextafter(sq, 0.0), n - 1
    return n


# ---- displacements on the edge ------------------------------------------------------------------------------------------------------------
Q = 2.0 ** -49
DRAWS, CHUNK, KEEP = 200_000, 20_000, 6
CLASSES = ("on", "above", "order")


@functools.lru_cache(maxsize=None)
def displacements(r, D):
    """-> {class: up to KEEP displacements (tuples of D doubles, multiples of Q)} from DRAWS seeded directions on the sphere / circle of
    radius r.  A displacement of class `order` may also be `on` or `above`."""
    T = sq_threshold(r)
    up = math.nextafter(T, math.inf)
    near = 8 * (up - T)
    rng = np.random.RandomState(int(round(r * 1000)) * 10 + D)
    found = {c: [] for c in CLASSES}
    for _ in range(DRAWS // CHUNK):
        u = rng.normal(size=(CHUNK, D))
        d = np.round(u / np.linalg.norm(u, axis=1, keepdims=True) * r / Q) * Q
        for k in np.flatnonzero(np.abs((d * d).sum(1) - T) <= near):
            v = tuple(float(x) for x in d[k])
            f, pl = sq_fma(v), sq_plain(v)
            for cls, hit in (("on", f == T), ("above", f == up), ("order", (f <= T) != (pl <= T))):
                if hit and len(found[cls]) < KEEP:
                    found[cls].append(v)
        if all(len(v) == KEEP for v in found.values()):
            break
    return found


def inside(d, r):
    """norm(d) <= r as the oracle evaluates it"""
    return sq_fma(d) <= sq_threshold(r)


RELATIONS = ("pp_kill", "pe_kill", "reach", "pp_comm", "pe_sen")
RADIUS_OF = dict(pp_kill="kill_radius", pe_kill="kill_radius", reach="kill_radius", pp_comm="p_comm_range", pe_sen="p_sen_range")
EDGE_CONFIGS = ("tight", "default")
EDGE_TEAMS = dict(e3d=((3, 1), (9, 1), (33, 1)), n2n=((3, 2), (16, 8), (33, 2)))    # (P, E): lane groups of 8, 16 and 64
EDGE_CASES = [(kind, name, P, E) for kind in KINDS for name in EDGE_CONFIGS for P, E in EDGE_TEAMS[kind]]
EDGE_IDS = lambda c: f"{c[0]}-{c[1]}-P{c[2]}-E{c[3]}"
# (kind, radius, class) the search does not find within DRAWS; everything else is present.  tests/test_particle_config_cases_cpu.py pins it.
EMPTY = frozenset()


def edge_radii(kind):
    return sorted({config(kind, name)[RADIUS_OF[rel]] for name in EDGE_CONFIGS for rel in RELATIONS})


def present(kind, r):
    return tuple(c for c in CLASSES if displacements(r, DIMS[kind])[c])


def _lattice(n, D):
    side = int(math.ceil(n ** (1.0 / D) - 1e-9))
    cells = np.stack(np.meshgrid(*[np.arange(side)] * D, indexing="ij"), -1).reshape(-1, D)[:n]
    return 30.0 + 8.0 * cells


def _exact_pair(rng, d):
    """base, base + d with fl(base + d) - base == d in every coordinate; the draw is repeated until it holds"""
    d = np.array(d)
    while True:
        base = 9.0 + rng.randint(-2 ** 48, 2 ** 48, len(d), dtype=np.int64) * Q
        a = base + d
        if all(Fraction(x) == Fraction(b) + Fraction(y) for x, b, y in zip(a, base, d)) and np.array_equal(a - base, d):
            return a, base


@functools.lru_cache(maxsize=None)
def edge_batch(kind, name, P, E):
    """one environment per (relation, class present, first / last slots), the ORACLE's outputs of observe, one still tick and observe.
    -> dict: rows [(relation, class, last, d, i, j)], init (p (N, P, C), e, target) in the host order of reset(init=...), action, cmd,
    the oracle's pp_adj0 / pe_adj0 (before the tick), reward, active, done, p / e (the records after the tick, as on the device),
    pp_adj1 / pe_adj1 / p_state1 / e_state1 (after), inside (N,) bool: the class label.  Read-only: it is shared."""
    cfg, D = config(kind, name), DIMS[kind]
    C = 2 * D + 1                                                          # e3d: x y z phi gamma v active; n2n: x y phi v active
    rows = []
    for rel in RELATIONS:
        r = cfg[RADIUS_OF[rel]]
        for cls in CLASSES:
            ds = displacements(r, D)[cls]
            for last in ((False, True) if ds else ()):
                rows.append((rel, cls, last, ds[(2 * RELATIONS.index(rel) + last) % len(ds)]))
    N = len(rows)
    rng = np.random.RandomState(500 + 10 * P + E + (name == "tight"))
    p, e, tg = np.zeros((N, P, C)), np.zeros((N, E, C)), np.full((N, D), 100.0)
    cells = _lattice(P + E, D)
    p[:, :, :D], e[:, :, :D] = cells[:P], cells[P:]
    p[:, :, D], e[:, :, D] = rng.uniform(-PI, PI, (N, P)), rng.uniform(-PI, PI, (N, E))
    if kind == "e3d":
        p[:, :, 4], e[:, :, 4] = rng.uniform(-1.2, 1.2, (N, P)), rng.uniform(-1.2, 1.2, (N, E))
    p[:, :, -1], e[:, :, -1] = 1.0, 1.0
    out_rows = []
    for n, (rel, cls, last, d) in enumerate(rows):
        a, b = _exact_pair(rng, d)
        i, k = (P - 1 if last else 0), (E - 1 if last else 0)
        if rel in ("pp_kill", "pp_comm"):
            i, j = (P - 2, P - 1) if last else (0, 1)
            p[n, i, :D], p[n, j, :D] = a, b
        elif rel == "reach":
            i, j = k, -1
            e[n, k, :D], tg[n] = a, b
        else:
            j = k
            p[n, i, :D], e[n, k, :D] = a, b
        out_rows.append((rel, cls, last, d, i, j))
    if kind == "e3d":
        action = np.stack((p[:, :, 3] / PI, p[:, :, 4] / (PI / 2), np.full((N, P), -1.0)), -1)
        cmd = np.stack((e[:, 0, 3] / PI, e[:, 0, 4] / (PI / 2), np.full(N, -1.0)), -1)
        e_init = e[:, 0]
    else:
        action, cmd, e_init = np.zeros((N, P), np.int32), e[:, :, 2] / PI, e
    out = dict(kind=kind, name=name, P=P, E=E, N=N, rows=out_rows, init=(p, e_init, tg), action=action, cmd=cmd,
               inside=np.array([inside(d, cfg[RADIUS_OF[rel]]) for rel, _, _, d, _, _ in out_rows]),
               reward=np.zeros((N, P), np.float32), active=np.zeros((N, P), np.uint8), done=np.zeros(N, bool),
               p=np.zeros((N, C, P)), e=np.zeros((N, C, E)) if kind == "n2n" else np.zeros((N, C)))
    for t in (0, 1):
        out.update({f"p_state{t}": np.zeros((N, P, STATE_W[kind]), np.float32), f"e_state{t}": np.zeros((N, E, STATE_W[kind]), np.float32),
                    f"pp_adj{t}": np.zeros((N, P, P), np.float32), f"pe_adj{t}": np.zeros((N, P, E), np.float32)})
    ocfg = oracle_cfg(kind, name, P, E)
    for n in range(N):
        oe = _oracle_env(kind, ocfg, p[n], e_init[n], tg[n])
        out["p_state0"][n], out["e_state0"][n], out["pp_adj0"][n], out["pe_adj0"][n] = oe.observe()
        oe.evader_step(cmd[n])
        r, out["done"][n], out["active"][n] = oe.step(action[n])
        out["reward"][n] = r.astype(np.float32)
        out["p"][n], out["e"][n] = oe.p.T, (oe.e.T if kind == "n2n" else oe.e[0])
        out["p_state1"][n], out["e_state1"][n], out["pp_adj1"][n], out["pe_adj1"][n] = oe.observe()
    return _frozen(out)


def _oracle_env(kind, ocfg, p, e, tg):
    if kind == "e3d":
        from oracle import e3d_oracle as eo
        return eo.OracleE3d(ocfg, p, e, tg)
    from oracle import n2n_oracle as no
    return no.OracleN2n(ocfg, p, e, tg)


def _frozen(d):
    for v in d.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


def observed_inside(b, n, pp_adj0, pe_adj0, reward, active, done, e_record):
    """the class label of environment n read off outputs (the oracle's or a kernel's): True inside, False outside; an AssertionError
    when they are neither.  e_record: the evader record(s) after the tick as on the device."""
    rel, _, _, _, i, j = b["rows"][n]
    P = b["P"]
    e_on = (np.asarray(e_record[n])[-1] != 0).reshape(-1)
    others = [q for q in range(P) if q not in ((i, j) if rel.startswith("pp") else (i,) if rel.startswith("pe") else ())]
    assert np.all(reward[n, others] == 0) and np.all(active[n, others] == 1), "a pursuer outside the pair was touched"
    if rel == "pp_kill":
        got = (reward[n, i], reward[n, j], active[n, i], active[n, j])
        assert got in ((-1, -1, 0, 0), (0, 0, 1, 1)), got
        return got[0] == -1
    if rel == "pe_kill":
        got = (reward[n, i], active[n, i], bool(e_on[j]))
        assert got in ((1, 0, False), (0, 1, True)), got
        assert bool(done[n]) == (got[0] == 1 and not e_on.any())
        return got[0] == 1
    assert np.all(reward[n] == 0) and np.all(active[n] == 1) and e_on.all()
    if rel == "reach":
        return bool(done[n])
    assert not done[n]
    if rel == "pp_comm":
        assert pp_adj0[n, i, j] == pp_adj0[n, j, i] and pp_adj0[n, i, j] in (0, 1)
        return pp_adj0[n, i, j] == 1
    assert pe_adj0[n, i, j] in (0, 1)
    return pe_adj0[n, i, j] == 1


# ---- random episodes under the off-default configs ----------------------------------------------------------------------------------------
EP_N, EP_T = 40, 30
EP_TEAM = dict(e3d=(8, 1), n2n=(16, 4))
EP_CASES = [(kind, name) for kind in KINDS for name in CONFIGS[kind]]
EP_IDS = lambda c: f"{c[0]}-{c[1]}"
KERNEL_TICKS = (0, 8)     # the states the guidance, policy-input and feature kernels are compared on
REACH_ENV = 3             # the environment whose target lies where an evader starts


def _bearing(dx, dy):
    return np.arctan2(dy, dx)


@functools.lru_cache(maxsize=None)
def episode(kind, name):
    """the ORACLE's trace under config `name`, keys and index conventions of wide_team_cases.episode: half of the pursuers steered at
    the (nearest) evader, explicit evader commands -- in the even environments into the team, in the odd ones random.  The initial
    states are wide_team_cases' jittered grids (two environments start with the lower half of the team parked)."""
    P, E = EP_TEAM[kind]
    N, T, D = EP_N, EP_T, DIMS[kind]
    C = 2 * D + 1
    ocfg = oracle_cfg(kind, name, P, E)
    e3d = kind == "e3d"
    p0, e0, tg = wc.e3d_init(P, N, seed=1) if e3d else wc.n2n_init(P, E, N, seed=1)
    # REACH_ENV: the target stands where evader 0 is after its first move straight ahead, so tick 0 ends that episode at the target
    R = REACH_ENV
    straight = np.array([e0[R, 3] / PI, e0[R, 4] / (PI / 2), 2 * e0[R, 5] / ocfg.e_vmax - 1]) if e3d else e0[R, :, 2] / PI
    probe = _oracle_env(kind, ocfg, p0[R], e0[R], tg[R])
    probe.evader_step(straight)
    tg[R] = probe.e[0, :D]
    envs = [_oracle_env(kind, ocfg, p0[n], e0[n], tg[n]) for n in range(N)]
    rng = np.random.RandomState(9000 + 10 * P + E + sorted(CONFIGS[kind]).index(name))
    out = dict(kind=kind, name=name, P=P, E=E, N=N, init=(p0, e0, tg), max_step=config(kind, name)[LIMIT_KEY[kind]],
               action=np.zeros((T, N, P, 3)) if e3d else np.zeros((T, N, P), np.int32), cmd=np.zeros((T, N, 3 if e3d else E)),
               p=np.zeros((T + 1, N, C, P)), e=np.zeros((T + 1, N, C) if e3d else (T + 1, N, C, E)),
               reward=np.zeros((T, N, P), np.float32), active=np.zeros((T, N, P), np.uint8), done=np.zeros((T, N), bool),
               p_state=np.zeros((T + 1, N, P, STATE_W[kind]), np.float32), e_state=np.zeros((T + 1, N, E, STATE_W[kind]), np.float32),
               pp_adj=np.zeros((T + 1, N, P, P), np.float32), pe_adj=np.zeros((T + 1, N, P, E), np.float32))

    def snap(t):
        for n, oe in enumerate(envs):
            out["p"][t, n], out["e"][t, n] = oe.p.T, (oe.e[0] if e3d else oe.e.T)
            out["p_state"][t, n], out["e_state"][t, n], out["pp_adj"][t, n], out["pe_adj"][t, n] = oe.observe()

    snap(0)
    for t in range(T):
        for n, oe in enumerate(envs):
            chase = rng.random_sample(P) < 0.5
            if e3d:
                act = rng.uniform(-1, 1, (P, 3))
                d = oe.e[0, :3] - oe.p[:, :3]
                act[:, 0] = np.where(chase, _bearing(d[:, 0], d[:, 1]) / PI, act[:, 0])
                act[:, 1] = np.where(chase, np.arctan2(d[:, 2], np.hypot(d[:, 0], d[:, 1])) / (PI / 2), act[:, 1])
                act[:, 2] = np.where(chase, 1.0, act[:, 2])
                cmd = rng.uniform(-1, 1, 3)
                if n % 2 == 0:
                    c = 10.0 - oe.e[0, :3]
                    cmd = np.array([_bearing(c[0], c[1]) / PI, np.arctan2(c[2], np.hypot(c[0], c[1])) / (PI / 2), 1.0])
                move = oe.e[0, 6] > 0 and oe.p[:, 6].sum() > 0    # ParticleEnv.step: the evader moves only while the episode has both sides
            else:
                act = rng.randint(0, 9, P).astype(np.int32)
                d = oe.e[None, :, :2] - oe.p[:, None, :2]                    # (P, E, 2)
                k = np.where(oe.e[None, :, 4] > 0, np.hypot(d[..., 0], d[..., 1]), np.inf).argmin(1)
                dk = d[np.arange(P), k]
                act = np.where(chase, guidance_ref.octant(_bearing(dk[:, 0], dk[:, 1])), act).astype(np.int32)
                cmd = rng.uniform(-1, 1, E)
                if n % 2 == 0:
                    cmd = _bearing(10.0 - oe.e[:, 0], 10.0 - oe.e[:, 1]) / PI
                move = True
            if n == R and t == 0:
                cmd = straight
            out["action"][t, n], out["cmd"][t, n] = act, cmd
            if move:
                oe.evader_step(cmd)
            r, done, active = oe.step(act)
            out["reward"][t, n], out["done"][t, n], out["active"][t, n] = r.astype(np.float32), done, active
        snap(t + 1)
    return _frozen(out)


def done_before(ep):
    """(T + 1, N) bool: the environment reported done in an earlier tick"""
    db = np.zeros((EP_T + 1, ep["N"]), bool)
    db[1:] = np.cumsum(ep["done"], 0) > 0
    return db


def episode_events(ep):
    """what the episode holds, on the oracle's trace alone: pursuers culled by a collision, evaders caught, environments ended by an
    evader at the target, and the environments still running at tick 6 whose tick 6 (t == 7) reports done for the time limit alone"""
    T, N, E = EP_T, ep["N"], ep["E"]
    p_on = ep["p"][:, :, -1, :] != 0
    e_on = (ep["e"][:, :, -1] != 0).reshape(T + 1, N, E)
    died = p_on[:-1] & ~p_on[1:]
    caught = e_on[:-1] & ~e_on[1:]
    cfg = config(ep["kind"], ep["name"])
    from tests import shaping_ref
    ended = np.array([shaping_ref.ended_after(ep["p"][t + 1], ep["e"][t + 1], ep["init"][2], cfg["kill_radius"]) for t in range(T)])
    first = ep["done"] & ~done_before(ep)[:T]
    return dict(collided=int((died & (ep["reward"] < 0)).sum()), caught=int(caught.sum()),
                reached=int((first & ended & p_on[1:].any(-1) & e_on[1:].any(-1)).sum()),
                time_limit_at_7=int((first[6] & ~ended[6]).sum()) if T > 6 else 0, ended=ended)
