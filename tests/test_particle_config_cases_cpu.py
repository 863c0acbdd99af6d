"""The cases of tests/particle_config_cases.py do what they are there for, checked on the ORACLES and the Python references alone (no
GPU, no kernel): the configs are off-default in every field, the edge displacements sit where they claim to, the oracle labels every edge
state as the exact arithmetic says, a classifier with the naive threshold or the unfused sum would get some of them wrong, the Python
references of the reach test agree with the oracle, and the episodes hold the events tests/test_particle_config_gpu.py counts on."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import guidance_ref
from tests import e3d_features_ref
from tests import n2n_policy_ref
from tests import particle_config_cases as pc
from tests import shaping_ref


def _dyadic(x):
    """x is k / 2^m with a short numerator: what a constant like 0.5 or 3.0 is and 0.7 or pi / 7 is not"""
    f = Fraction(x)
    return f.numerator.bit_length() <= 20


# ---- configs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.KINDS)
def test_every_physical_field_is_off_default_and_no_dyadic_rational(kind):
    assert len(pc.CONFIGS[kind]) >= 2
    for name in pc.CONFIGS[kind]:
        cfg, dflt = pc.config(kind, name), pc.DEFAULTS[kind]
        assert set(cfg) == set(dflt)
        for k in dflt:
            assert cfg[k] != dflt[k], (name, k)
            if k in pc.PHYSICAL:
                assert not _dyadic(cfg[k]), (name, k)
        # displacement per tick at most about three times the default's: the 1e-9 of the episode tests was set for the default's
        for v in ("p_vmax", "e_vmax"):
            assert cfg[v] * cfg["step_size"] <= 3.0 * dflt[v] * dflt["step_size"], (name, v)
        assert cfg[pc.LIMIT_KEY[kind]] <= pc.EP_T
    tight, far = pc.config(kind, "tight"), pc.config(kind, "far")
    want = dict(kill_radius=0.7, p_sen_range=2.1, p_comm_range=6.1, p_vmax=1.1, e_vmax=0.6, ang_lmt=math.pi / 7, step_size=0.3)
    assert all(tight[k] == v for k, v in want.items()) and tight[pc.LIMIT_KEY[kind]] == 7 and (kind == "n2n" or tight["v_lmt"] == 0.15)
    assert far["p_sen_range"] > far["p_comm_range"] and far[pc.LIMIT_KEY[kind]] > tight[pc.LIMIT_KEY[kind]]
    assert _dyadic(0.5) and _dyadic(3.0) and _dyadic(6.0)


def test_the_configs_are_what_the_oracle_and_the_feature_references_receive():
    c = pc.oracle_cfg("e3d", "tight", 8)
    assert (c.P, c.max_step, c.kill_radius, c.p_sen_range, c.p_comm_range, c.p_vmax, c.e_vmax, c.v_lmt, c.step_size) == \
        (8, 7, 0.7, 2.1, 6.1, 1.1, 0.6, 0.15, 0.3) and c.ang_lmt == math.pi / 7
    c = pc.oracle_cfg("n2n", "far", 16, 4)
    assert (c.P, c.E, c.episode_limit, c.kill_radius, c.p_sen_range, c.p_comm_range, c.p_vmax, c.e_vmax, c.step_size) == \
        (16, 4, 23, 0.35, 5.3, 4.7, 0.9, 1.3, 0.45) and c.ang_lmt == math.pi / 5
    from tests import e3d_features_cases as fc
    assert pc.features_cfg("default") == fc.CFG and set(pc.features_cfg("far")) == set(fc.CFG)


# ---- the threshold ------------------------------------------------------------------------------------------------------------------------
def test_threshold_offsets():
    """T, the largest double with sqrt(T) <= r, against fl(r r): one ulp above for 0.7, 2.1, 6.1, 1.1, 0.35 and 0.5, equal for 3.0,
    6.0, 0.3, 4.7 and 5.3; every radius of every config is in the table, and both kinds of radius are among the edge radii"""
    assert {r for r, n in pc.THRESHOLD_OFFSET.items() if n == 1} == {0.7, 2.1, 6.1, 1.1, 0.35, 0.5}
    assert {r for r, n in pc.THRESHOLD_OFFSET.items() if n == 0} == {3.0, 6.0, 0.3, 4.7, 5.3}
    for r, n in pc.THRESHOLD_OFFSET.items():
        T = pc.sq_threshold(r)
        assert pc.threshold_offset(r) == n, r
        assert math.sqrt(T) <= r < math.sqrt(math.nextafter(T, math.inf))
        assert (T != r * r) == (n != 0)
    for kind in pc.KINDS:
        for name in ("default",) + tuple(pc.CONFIGS[kind]):
            for k in ("kill_radius", "p_sen_range", "p_comm_range"):
                assert pc.config(kind, name)[k] in pc.THRESHOLD_OFFSET
        offs = {pc.THRESHOLD_OFFSET[r] for r in pc.edge_radii(kind)}
        assert offs == {0, 1}
        assert all(pc.THRESHOLD_OFFSET[pc.config(kind, "tight")[k]] == 1 for k in ("kill_radius", "p_sen_range", "p_comm_range"))


def test_fraction_fma_is_the_c_fma():
    """pc.fma against libm's fma through the oracle's own norm: sqrt(pc.sq_fma(d)) is what the oracle compares with r, so the labels
    test below would fail too; here directly, on values whose product needs all 106 bits"""
    rng = np.random.RandomState(0)
    for a, b, c in rng.uniform(-8, 8, (200, 3)):
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        got = pc.fma(a, b, c)
        lo, hi = math.nextafter(got, -math.inf), math.nextafter(got, math.inf)
        assert abs(Fraction(got) - exact) <= min(abs(Fraction(lo) - exact), abs(Fraction(hi) - exact))


# ---- displacements ------------------------------------------------------------------------------------------------------------------------
CLASS_TABLE = [(kind, r) for kind in pc.KINDS for r in pc.edge_radii(kind)]


@pytest.mark.parametrize("kind,r", CLASS_TABLE, ids=[f"{k}-{r}" for k, r in CLASS_TABLE])
def test_displacements_sit_where_their_class_says(kind, r):
    D = pc.DIMS[kind]
    T = pc.sq_threshold(r)
    up = math.nextafter(T, math.inf)
    found = pc.displacements(r, D)
    print(f"{kind} r {r}: T = fl(r r) + {pc.threshold_offset(r)} ulp, classes " + ", ".join(f"{c} {len(found[c])}" for c in pc.CLASSES))
    for cls in pc.CLASSES:
        assert bool(found[cls]) == ((kind, r, cls) not in pc.EMPTY), (cls, len(found[cls]))
        assert len(set(found[cls])) == len(found[cls])
        for d in found[cls]:
            assert len(d) == D and all(x == round(x / pc.Q) * pc.Q for x in d)
            # the chain once more, every step in rationals
            s = Fraction(d[0]) * Fraction(d[0])
            s = Fraction(float(s))
            for x in d[1:]:
                s = Fraction(float(Fraction(x) * Fraction(x) + s))
            f = float(s)
            assert f == pc.sq_fma(d)
            assert abs(math.sqrt(f) - r) <= 4 * math.ulp(r)
            if cls == "on":
                assert f == T and pc.inside(d, r)
            elif cls == "above":
                assert f == up and not pc.inside(d, r)
            else:
                assert (f <= T) != (pc.sq_plain(d) <= T)


def test_empty_table_and_tight_has_every_class():
    """EMPTY is pinned: with displacements on the 2^-49 grid the 200 000 draws find all three classes at every edge radius of both
    environments, so the table is empty; under `tight` every relation has `on` and `above`"""
    assert pc.EMPTY == frozenset()
    for kind in pc.KINDS:
        cfg = pc.config(kind, "tight")
        for rel in pc.RELATIONS:
            assert {"on", "above"} <= set(pc.present(kind, cfg[pc.RADIUS_OF[rel]])), (kind, rel)
        for r in pc.edge_radii(kind):
            assert all(((kind, r, c) in pc.EMPTY) != (c in pc.present(kind, r)) for c in pc.CLASSES)


# ---- edge states --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.EDGE_CASES, ids=pc.EDGE_IDS)
def test_placement_is_exact_and_everybody_else_is_far(case):
    kind, name, P, E = case
    b = pc.edge_batch(*case)
    cfg, D = pc.config(kind, name), pc.DIMS[kind]
    p, e, tg = b["init"]
    e = e.reshape(b["N"], E, -1)
    assert b["N"] < 100 and b["N"] == 2 * sum(len(pc.present(kind, cfg[pc.RADIUS_OF[rel]])) for rel in pc.RELATIONS)
    far = max(cfg[k] for k in ("kill_radius", "p_sen_range", "p_comm_range"))
    lasts = 0
    for n, (rel, cls, last, d, i, j) in enumerate(b["rows"]):
        pts = {("p", q): p[n, q, :D] for q in range(P)}
        pts.update({("e", q): e[n, q, :D] for q in range(E)})
        pts[("t", 0)] = tg[n]
        pair = {"pp_kill": (("p", i), ("p", j)), "pp_comm": (("p", i), ("p", j)), "pe_kill": (("p", i), ("e", j)), "pe_sen": (("p", i), ("e", j)),
                "reach": (("e", i), ("t", 0))}[rel]
        a, base = pts[pair[0]], pts[pair[1]]
        for x, y, z in zip(a, base, d):                                    # fl(base + d) - base == d, and nothing was rounded
            assert x - y == z and y - x == -z and Fraction(x) == Fraction(y) + Fraction(z) and abs(x) < 16 and abs(y) < 16
        keys = list(pts)
        for u in range(len(keys)):
            for w in range(u + 1, len(keys)):
                if {keys[u], keys[w]} != set(pair) and not (keys[u][0] == "t" and keys[w][0] == "p") and not (keys[u][0] == "p" and keys[w][0] == "t"):
                    assert np.linalg.norm(pts[keys[u]] - pts[keys[w]]) > far + 1.0, (n, keys[u], keys[w])
        # the slots: the first or the last of the team
        if rel.startswith("pp"):
            assert (i, j) == ((P - 2, P - 1) if last else (0, 1))
        elif rel.startswith("pe"):
            assert (i, j) == ((P - 1, E - 1) if last else (0, 0))
        else:
            assert i == (E - 1 if last else 0)
        lasts += last
        assert b["inside"][n] == {"on": True, "above": False}.get(cls, pc.inside(d, cfg[pc.RADIUS_OF[rel]]))
    assert 2 * lasts == b["N"]
    # nobody moves: speeds 0; env_3d commands a speed of -1 -> 0, env_n2n the action 0
    assert not p[:, :, -2].any() and not e[:, :, -2].any()
    assert np.all(b["action"][..., 2] == -1) and np.all(b["cmd"][:, 2] == -1) if kind == "e3d" else not b["action"].any()


def test_team_shapes_cover_the_lane_groups():
    from tests import wide_team_cases as wc
    assert [wc.lanes(P, E) for P, E in pc.EDGE_TEAMS["e3d"]] == [8, 16, 64] and [wc.lanes(P, E) for P, E in pc.EDGE_TEAMS["n2n"]] == [8, 16, 64]
    assert pc.EDGE_TEAMS["e3d"] == ((3, 1), (9, 1), (33, 1)) and pc.EDGE_TEAMS["n2n"] == ((3, 2), (16, 8), (33, 2))


@pytest.mark.parametrize("case", pc.EDGE_CASES, ids=pc.EDGE_IDS)
def test_oracle_labels_every_edge_state_as_the_exact_arithmetic_does(case):
    """reward, active, done and both adjacencies of the C oracle after observe and one still tick give the class label; the records
    did not move"""
    kind, name, P, E = case
    b = pc.edge_batch(*case)
    D = pc.DIMS[kind]
    for n in range(b["N"]):
        got = pc.observed_inside(b, n, b["pp_adj0"], b["pe_adj0"], b["reward"], b["active"], b["done"], b["e"])
        assert got == b["inside"][n], (n, b["rows"][n][:3])
    p0, e0, _ = b["init"]
    on = b["p"][:, -1] != 0
    assert np.array_equal(np.where(on[:, None], b["p"][:, :D], 0), np.where(on[:, None], p0.transpose(0, 2, 1)[:, :D], 0))
    assert np.all(b["p"][:, :D].transpose(0, 2, 1)[~on] == 1000.0)
    assert b["inside"].any() and not b["inside"].all()


@pytest.mark.parametrize("kind", pc.KINDS)
def test_naive_classifiers_get_edge_states_wrong(kind):
    """restated in Python: `sq <= fl(r r)` on the fma chain, the same on the unfused sum, and the right threshold on the unfused sum.
    Against the oracle's labels (pe_adj / pp_adj / done / reward of the edge states) the first two fail at every radius whose T is not
    fl(r r), the third wherever the class `order` is present"""
    D = pc.DIMS[kind]
    for name in pc.EDGE_CONFIGS:
        P, E = pc.EDGE_TEAMS[kind][0]
        b = pc.edge_batch(kind, name, P, E)
        cfg = pc.config(kind, name)
        label = np.array([pc.observed_inside(b, n, b["pp_adj0"], b["pe_adj0"], b["reward"], b["active"], b["done"], b["e"]) for n in range(b["N"])])
        radius = np.array([cfg[pc.RADIUS_OF[row[0]]] for row in b["rows"]])
        naive_thr = np.array([pc.sq_fma(row[3]) <= r * r for row, r in zip(b["rows"], radius)])
        naive_both = np.array([pc.sq_plain(row[3]) <= r * r for row, r in zip(b["rows"], radius)])
        naive_sum = np.array([pc.sq_plain(row[3]) <= pc.sq_threshold(r) for row, r in zip(b["rows"], radius)])
        strict = np.array([pc.sq_fma(row[3]) < pc.sq_threshold(r) for row, r in zip(b["rows"], radius)])
        one_up = np.array([pc.sq_fma(row[3]) <= math.nextafter(pc.sq_threshold(r), math.inf) for row, r in zip(b["rows"], radius)])
        for r in sorted(set(radius)):
            at = radius == r
            wrong = {k: int((v[at] != label[at]).sum()) for k, v in (("r r", naive_thr), ("r r, unfused", naive_both), ("unfused", naive_sum),
                                                                     ("<", strict), ("T + 1 ulp", one_up))}
            print(f"{kind} {name} r {r} (T = fl(r r) + {pc.THRESHOLD_OFFSET[r]} ulp): wrong labels of {int(at.sum())}: {wrong}")
            if pc.THRESHOLD_OFFSET[r] != 0:
                assert wrong["r r"] > 0 and wrong["r r, unfused"] > 0
            if "order" in pc.present(kind, r):
                assert wrong["unfused"] > 0
            assert wrong["<"] > 0 and wrong["T + 1 ulp"] > 0


# ---- the Python references of the reach test ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.EDGE_CASES, ids=pc.EDGE_IDS)
def test_python_references_agree_with_the_oracle_on_the_reach_states(case):
    """shaping_ref.ended_after and n2n_policy_ref.policy_record on the records after the still tick against the oracle's done; on every
    state of the batch `ended` is done (the time limit is far), and the reach states are among them"""
    kind, name, P, E = case
    b = pc.edge_batch(*case)
    cfg = pc.config(kind, name)
    N = b["N"]
    reach = [n for n, row in enumerate(b["rows"]) if row[0] == "reach"]
    assert len(reach) >= 4 and b["done"][reach].any() and not b["done"][reach].all()
    ended = shaping_ref.ended_after(b["p"], b["e"], b["init"][2], cfg["kill_radius"])
    assert np.array_equal(ended, b["done"]), np.flatnonzero(ended != b["done"])
    if kind == "n2n":
        acc = n2n_policy_ref.policy_record(b["p"], b["e"], b["init"][2], b["reward"], b["done"].astype(np.uint8), np.ones((N, P), np.float32),
                                           np.zeros((N, P), np.float32), n2n_policy_ref.new_accumulators(N), cfg["kill_radius"])[4]
        assert np.array_equal(acc["ended"] != 0, b["done"]), np.flatnonzero((acc["ended"] != 0) != b["done"])


def test_within_is_the_plain_norm_away_from_the_edge():
    rng = np.random.RandomState(3)
    d = rng.uniform(-4, 4, (3, 500))
    assert np.array_equal(shaping_ref.within(d, 3.0), np.linalg.norm(d, axis=0) <= 3.0)
    assert shaping_ref.within(np.zeros((2, 1)), 0.5).all()


# ---- numpy's own norm ---------------------------------------------------------------------------------------------------------------------
def test_numpy_norm_labels_the_edge_displacements():
    """what the reference environment itself evaluates: np.linalg.norm(d) <= r.  Only where this host's numpy computes the norm as the
    fma chain (the oracle's premise, measured where the traces were recorded) does the comparison say anything"""
    rng = np.random.RandomState(11)
    for D in (2, 3):
        for v in rng.uniform(-10, 10, (1000, D)):
            if np.linalg.norm(v) != math.sqrt(pc.sq_fma(tuple(float(x) for x in v))):
                pytest.skip(f"np.linalg.norm of a {D}-vector is not sqrt of the fma chain on this host")
    n = 0
    for kind in pc.KINDS:
        for r in pc.edge_radii(kind):
            for cls in pc.CLASSES:
                for d in pc.displacements(r, pc.DIMS[kind])[cls]:
                    assert bool(np.linalg.norm(np.array(d)) <= r) == pc.inside(d, r), (kind, r, cls, d)
                    assert bool(np.linalg.norm(-np.array(d)) <= r) == pc.inside(d, r)
                    n += 1
    assert n >= 100


# ---- episodes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.EP_CASES, ids=pc.EP_IDS)
def test_episode_collides_captures_reaches_and_runs_into_the_time_limit(case):
    kind, name = case
    ep = pc.episode(*case)
    cfg = pc.config(kind, name)
    P, E, N, T = ep["P"], ep["E"], ep["N"], pc.EP_T
    assert (N, T, (P, E)) == (40, 30, {"e3d": (8, 1), "n2n": (16, 4)}[kind]) and ep["max_step"] == cfg[pc.LIMIT_KEY[kind]]
    p0 = ep["init"][0]
    D = pc.DIMS[kind]
    dist = np.linalg.norm(p0[:, :, None, :D] - p0[:, None, :, :D], axis=-1)
    off = p0[:, :, -1] == 0
    assert (dist + 1e9 * (np.eye(P, dtype=bool)[None] | off[:, :, None] | off[:, None, :])).min() > cfg["kill_radius"]
    ev = pc.episode_events(ep)
    db = pc.done_before(ep)
    print(f"{pc.EP_IDS(case)}: {ev['collided']} pursuers culled by collision, {ev['caught']} evaders caught, {ev['reached']} episodes ended at the "
          f"target, {ev['time_limit_at_7']} ended by the time limit at t == 7, {int((~db[8]).sum())} of {N} running at tick 8")
    assert ev["collided"] > 0 and ev["caught"] > 0 and ev["reached"] > 0
    assert ep["done"][0, pc.REACH_ENV] and ev["ended"][0, pc.REACH_ENV]
    if ep["max_step"] == 7:
        assert ev["time_limit_at_7"] > 0
        assert ep["done"][6:].all() and not ep["done"][:6].all()
    else:
        assert (~db[8]).any()                                             # the states of tick 8 are those of running episodes
        first = ep["done"] & ~db[:T]
        assert (first[ep["max_step"] - 1] & ~ev["ended"][ep["max_step"] - 1]).any()   # ... and its own time limit ends some
    on = ep["p"][:, :, -1, :] != 0                                        # (the ticks go on after done, and so do the comparisons)
    rows = ep["pp_adj"][on]
    mixed = (rows.min(1) == 0) & (rows.max(1) == 1)
    pe = ep["pe_adj"][on]
    print(f"{pc.EP_IDS(case)}: pp_adj mixed in {mixed.mean():.3f} of {len(rows)} active rows, pe_adj ones {pe.mean():.3f}")
    assert mixed.any() and not mixed.all() and pe.min() == 0 and pe.max() == 1
    # the ranges are the config's: under the default ranges the oracle gives other adjacencies on these very records
    other = pc.oracle_cfg(kind, "default", P, E)
    differ = 0
    for n in range(N):
        o = pc._oracle_env(kind, other, ep["p"][8, n].T, ep["e"][8, n] if kind == "e3d" else ep["e"][8, n].T, ep["init"][2][n])
        _, _, pp_o, pe_o = o.observe()
        differ += int((pp_o != ep["pp_adj"][8, n]).sum() + (pe_o != ep["pe_adj"][8, n]).sum())
    assert differ > 0


@pytest.mark.parametrize("case", pc.EP_CASES, ids=pc.EP_IDS)
def test_kernel_states_are_worth_comparing(case):
    """ticks 0 and 8: active and inactive pursuers; no env_n2n bearing within 1e-9 of an octant boundary under the default guidance
    parameters of the config; env_3d: no near tie between team-mate distances (e3d_features_ref.nearest_gap)"""
    kind, name = case
    ep = pc.episode(*case)
    cfg = pc.config(kind, name)
    assert pc.KERNEL_TICKS == (0, 8)
    t = pc.KERNEL_TICKS[-1]
    assert (ep["p"][t][:, -1] == 0).any() and (ep["p"][t][:, -1] != 0).any()
    e_on = (ep["e"][t][:, -1] != 0).reshape(ep["N"], -1)
    assert (~e_on.any(1)).any() and e_on.any(1).any()
    for t in pc.KERNEL_TICKS:
        if kind == "n2n":
            _, bearing = guidance_ref.n2n_actions(ep["p"][t], ep["e"][t], cfg["p_vmax"], *guidance_ref.default_params(cfg["kill_radius"]), with_bearing=True)
            assert not guidance_ref.near_octant_boundary(bearing).any()
        else:
            gap, rows = e3d_features_ref.nearest_gap(ep["p"][t])
            assert rows == int((ep["p"][t][:, 6] != 0).sum()) and gap >= 1e-9
