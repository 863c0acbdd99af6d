"""The env_3d and env_n2n kernels above 16 pursuers on the MI355X: the lane groups of 32 and 64 lanes per environment (PT) of the tick,
observe, policy-input, record (plain, scaled, shaped, team), shaping-begin and guidance kernels, the P-strided feature kernels, and the
PM = 32 / 64 instances and both launch shapes of the SLSQP evader -- each against the oracle or the numpy restatement its narrow-team
test uses, under that test's assertions, on the episodes of tests/wide_team_cases.py (checked on the CPU by
tests/test_wide_team_cases_cpu.py) and the problems of tests/golden/evader_*_wide.npz.

No test here calls reset() without init: the placement loops cannot seat such teams.  Every environment's own device tensors stand in
storage with canary rows behind the last environment and, where the interface takes a row stride, canary columns behind the row, and
every test ends on the canaries."""
import numpy as np
import pytest
import torch

from tests.helpers import no_gc_during_capture

from tests import e3d_features_ref
from tests import evader_cases as ec
from tests import guidance_cases as gc
from tests import guidance_ref
from tests import n2n_policy_ref
from tests import obs_norm_ref
from tests import reward_scale_ref as scale_ref
from tests import shaping_ref
from tests import team_reward_ref
from tests import wide_team_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda"
GAMMA, COEF, ALPHA = 0.99, 0.1, 0.5
PAD_ROWS, PAD_COLS = 3, 5
CANARY = {torch.float32: 7.0, torch.float64: 7.0, torch.int32: 77, torch.uint8: 0xA5}
# (scaling, shaping, team): each option alone, none, and the three together as the trainers run them
VARIANTS = [(False, False, None), (True, False, None), (False, True, None), (False, False, ALPHA), (True, True, ALPHA)]


# ---- canary-padded storage ------------------------------------------------------------------------------------------------------------
class Guard:
    """tensors whose storage continues behind them: PAD_ROWS rows behind the last environment and, for strided ones, PAD_COLS
    elements behind every environment's row, all holding a canary"""

    def __init__(self):
        self.items = []

    def make(self, name, shape, dtype, strided, fill=None):
        N, row = shape[0], int(np.prod(shape[1:], dtype=np.int64))
        width = row + (PAD_COLS if strided else 0)
        big = torch.full((N + PAD_ROWS, width), CANARY[dtype], dtype=dtype, device=DEV)
        inner = torch.empty(shape[1:]).stride() if len(shape) > 1 else ()
        view = torch.as_strided(big, tuple(shape), (width, *inner))
        view.fill_(CANARY[dtype] if fill is None else fill)
        self.items.append((name, big, N, row, dtype))
        return view

    def check(self):
        for name, big, N, row, dtype in self.items:
            assert bool((big[N:] == CANARY[dtype]).all()), f"{name}: written behind the last environment"
            assert bool((big[:N, row:] == CANARY[dtype]).all()), f"{name}: written behind the row"


def _env(case, evader="rule"):
    """the environment of a case on canary-padded storage, loaded with the case's initial state -> (env, episode, guard)"""
    kind, P, E, N = case
    ep = wc.episode(*case)
    if kind == "n2n":
        from distributed_multi_agent_reinforcement_learning_amd.n2n_env import ParticleEnv
        env = ParticleEnv(num_envs=N, episode_limit=ep["max_step"], evader=evader)
        env.initialize(P, E)
    else:
        from distributed_multi_agent_reinforcement_learning_amd.e3d_env import ParticleEnv
        env = ParticleEnv(num_envs=N, max_step=ep["max_step"], evader=evader)
        env.initialize(P)
    g = Guard()
    for name in ("p", "e", "target", "t_dev", "reward_t", "active_t", "done_t", "_cmd_slsqp"):   # dense in the interface: rows behind N
        t = getattr(env, name)
        setattr(env, name, g.make(name, t.shape, t.dtype, False, fill=0))
    env.st.p, env.st.e, env.st.target, env.st.time_step = env.p.data_ptr(), env.e.data_ptr(), env.target.data_ptr(), env.t_dev.data_ptr()
    for k, t in list(env.obs.items()):                                                          # strided: columns behind the row too
        env.obs[k] = g.make(k, t.shape, t.dtype, True, fill=0)
        setattr(env._obs_struct, k, env.obs[k].data_ptr())
        setattr(env._obs_struct, k + "_stride", env.obs[k].stride(0))
    env.reset(init=ep["init"])
    return env, ep, g


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)                           # a copy: the shared episodes are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _inject(env, ep, t):
    """the oracle's records and adjacencies of the state tick t starts from, written where the tick leaves its own"""
    env.p.copy_(_t(ep["p"][t])); env.e.copy_(_t(ep["e"][t]))
    env.obs["pp_adj"].copy_(_t(ep["pp_adj"][t])); env.obs["pe_adj"].copy_(_t(ep["pe_adj"][t]))


def _step(env, ep, t):
    env.evader_step(np.array(ep["cmd"][t]))                             # a copy: the shared episode is read-only
    return env.step(_t(ep["action"][t]))


# ---- tick and observe against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_tick_and_observe_match_the_oracle(case):
    """the figures of tests/test_e3d_gpu.py and tests/test_n2n_gpu.py: reward, active, done and both adjacencies identical at every tick,
    f64 records within 1e-9, fp32 p_state / e_state within 1e-5; observe() on the same records gives the tick's bytes"""
    kind, P, E, N = case
    env, ep, guard = _env(case)
    culled = caught = 0
    for t in range(wc.T + 1):
        p, e = env.p.cpu().numpy(), env.e.cpu().numpy()
        assert np.max(np.abs(p - ep["p"][t])) <= 1e-9 and np.max(np.abs(e - ep["e"][t])) <= 1e-9, t
        obs = {k: v.clone() for k, v in env.obs.items()}
        for k in ("pp_adj", "pe_adj"):
            assert np.array_equal(obs[k].cpu().numpy(), ep[k][t]), (k, t)
        for k in ("p_state", "e_state"):
            assert np.allclose(obs[k].cpu().numpy(), ep[k][t], rtol=0, atol=1e-5), (k, t)
        for v in env.obs.values():
            v.fill_(3.0)
        env.observe()
        for k in obs:
            assert _same_bytes(env.obs[k], obs[k]), (k, t)
        if t == wc.T:
            break
        r, done, act = _step(env, ep, t)
        assert np.array_equal(r.cpu().numpy(), ep["reward"][t]), t
        assert np.array_equal(act.cpu().numpy(), ep["active"][t]), t
        assert np.array_equal(done.cpu().numpy() != 0, ep["done"][t]), t
        after_p, after_e = env.p[:, -1].cpu().numpy() != 0, (env.e[:, -1].cpu().numpy() != 0).reshape(N, -1)
        culled += int(((p[:, -1] != 0) & ~after_p & (r.cpu().numpy() < 0)).sum())
        caught += int(((e[:, -1] != 0).reshape(N, -1) & ~after_e).sum())
    assert np.array_equal(env.t_dev.cpu().numpy(), np.full(N, wc.T))
    print(f"{wc.IDS(case)}: {culled} pursuers culled by collision, {caught} evaders caught")
    assert culled > 0 and caught > 0
    guard.check()


# ---- n2n_policy_inputs ----------------------------------------------------------------------------------------------------------------
def _policy_outs(g, N, P, E):
    return dict(p4=g.make("p4", (N, P, 4), torch.float32, True), e4=g.make("e4", (N, E, 4), torch.float32, True),
                e_ref=g.make("e_ref", (N, 4), torch.float32, True), live=g.make("live", (N, P), torch.float32, True),
                pp_adj=g.make("pp_adj_out", (N, P, P), torch.float32, True), pe_adj=g.make("pe_adj_out", (N, P, E), torch.float32, True))


@pytest.mark.parametrize("case", [c for c in wc.CASES if c[0] == "n2n"], ids=wc.IDS)
def test_n2n_policy_inputs_match_numpy(case):
    """the assertions of tests/test_n2n_agent_gpu.py (n2n_policy_ref.assert_policy_inputs) on the start and two mid-episode states,
    with the episode's done_before mask and without one"""
    kind, P, E, N = case
    env, ep, guard = _env(case)
    db_all = wc.done_before(ep)
    seen = dict(dead_p=0, dead_e=0, done=0)
    for t in wc.GUIDANCE_TICKS:
        _inject(env, ep, t)
        for db in (db_all[t].astype(np.uint8), None):
            outs = _policy_outs(guard, N, P, E)
            env.policy_inputs(**outs, done_before=None if db is None else _t(db))
            want = n2n_policy_ref.assert_policy_inputs({k: v.cpu().numpy() for k, v in outs.items()}, ep["p"][t], ep["e"][t], ep["pp_adj"][t],
                                                       ep["pe_adj"][t], db)
        seen["dead_p"] += int((ep["p"][t][:, 4] == 0).sum()); seen["dead_e"] += int((ep["e"][t][:, 4] == 0).sum())
        seen["done"] += int(db_all[t].sum())
    assert all(v > 0 for v in seen.values()), seen
    guard.check()


# ---- the record launches over whole episodes ------------------------------------------------------------------------------------------
class Launch:
    """one variant of the record launch with its own states on the device and their host mirrors (after tests/test_team_reward_gpu.py)"""

    def __init__(self, env, guard, N, P, scaling, shaping, team):
        self.scaling, self.shaping, self.team = scaling, shaping, team
        self.name = f"scaling {scaling} shaping {shaping} team {team}"
        self.rs = guard.make("reward_scale", (N, 1 + 3 * P), torch.float64, False, fill=0.0) if scaling else None
        self.rs_host = scale_ref.new_state(N, P) if scaling else None
        self.phi = self.phi_host = None
        if shaping:
            self.phi = guard.make("shaping_phi", (N, P), torch.float64, False, fill=123.0)
            env.shaping_phi = self.phi
            env.shaping_begin()
            self.phi_host = shaping_ref.potential(env.p.cpu().numpy(), env.e.cpu().numpy(), COEF)
            assert np.array_equal(_bits(self.phi.cpu().numpy()), _bits(self.phi_host))

    def run(self, env, guard, kind, N, P, acc, live, value):
        env.reward_scale, env.shaping_phi = self.rs, self.phi
        acc = {k: guard.make(k, v.shape, v.dtype, False).copy_(v) for k, v in acc.items()}
        out = {k: guard.make(k, (N, P), torch.float32, True) for k in ("r", "active", "v", "v_next", "live_next")}
        extra = dict(live_next=out["live_next"]) if kind == "e3d" else {}
        kw = {} if self.team is None else dict(team_coef=self.team)
        env.policy_record(acc, live, value, out["r"], out["active"], out["v"], out["v_next"], **extra,
                          scale_gamma=GAMMA if self.scaling else None, shaping_gamma=GAMMA if self.shaping else None, **kw)
        return out, acc

    def want_r(self, raw, lv, db, p_after, e_after, ended):
        """the reward row by the restatement of each option, composed as its own test composes them; advances the host mirrors"""
        if self.team is not None:
            return team_reward_ref.record_step(raw, lv, db, self.team, GAMMA, self.rs_host, self.phi_host, p_after, e_after, ended, COEF)
        x = raw
        if self.shaping:
            x, _, _ = shaping_ref.step(self.phi_host, raw, lv, db, p_after, e_after, ended, COEF, GAMMA)
        if self.scaling:
            return scale_ref.step(self.rs_host, x, lv, db, GAMMA)
        return shaping_ref.buffer_reward(x, lv) if self.shaping else raw * lv


def _bookkeeping(acc, raw, lv, value, done, p_after, e_after, ended_now):
    """the accumulators and masked rows of one record launch, in numpy: what tests/n2n_policy_ref.policy_record states for env_n2n and
    the torch bookkeeping of tests/test_reward_scale_gpu.py for env_3d, for either environment"""
    db = acc["done_before"] != 0
    p_on = p_after[:, -1, :] != 0
    no_evader = ~(e_after[:, -1] != 0).reshape(len(db), -1).any(1)
    out = dict(ended=((acc["ended"] != 0) | (ended_now & ~db)).astype(np.uint8),
               captured=((acc["captured"] != 0) | (no_evader & ~db)).astype(np.uint8),
               length=(acc["length"] + (~db).astype(np.float32)).astype(np.float32), done_before=(db | (done != 0)).astype(np.uint8))
    rl = (raw * lv).astype(np.float32)
    s = np.zeros(len(db), np.float32)
    for k in range(rl.shape[1]):
        s = (s + rl[:, k]).astype(np.float32)
    out["ret"] = (acc["ret"] + s).astype(np.float32)
    rows = dict(active=lv, v=(value * lv).astype(np.float32), v_next_zero=~p_on | (out["ended"] != 0)[:, None],
                live_next=(p_on & (out["done_before"] == 0)[:, None]).astype(np.float32))
    return out, rows


@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_record_launches_match_their_restatements_over_the_episode(case):
    """the episode's 25 ticks through e3d_ / n2n_policy_record with no option, with each of the three and with all three together, each variant
    with its own states: r (fp32), reward_scale and shaping_phi (f64) equal the restatements bit for bit (tests/reward_scale_ref.py,
    shaping_ref.py, team_reward_ref.py), environments done before the step untouched; active, v, v_next, live_next and the five
    accumulators are the plain launch's bytes, and the plain launch's are the bookkeeping's (env_n2n: n2n_policy_ref.policy_record)"""
    kind, P, E, N = case
    env, ep, guard = _env(case)
    env.enable_reward_shaping(COEF)
    launches = [Launch(env, guard, N, P, *v) for v in VARIANTS]
    acc = {k: v for k, v in env.new_accumulators().items()}
    live = _t((ep["p"][0][:, -1, :] != 0).astype(np.float32))
    gen = torch.Generator(device=DEV).manual_seed(100 * P + E)
    seen = dict(shaped=0, shared=0, scaled=0, deaths=0, done_rows=0, live=0)
    for t in range(wc.T):
        _step(env, ep, t)
        value = torch.randn(N, P, generator=gen, device=DEV)
        raw, lv, val = env.reward_t.cpu().numpy(), live.cpu().numpy(), value.cpu().numpy()
        assert np.array_equal(raw, ep["reward"][t])
        acc_np = {k: v.cpu().numpy() for k, v in acc.items()}
        db = acc_np["done_before"] != 0
        p_after, e_after, target = env.p.cpu().numpy(), env.e.cpu().numpy(), env.target.cpu().numpy()
        ended_now = shaping_ref.ended_after(p_after, e_after, target, env.kill_radius)
        acc_want, rows = _bookkeeping(acc_np, raw, lv, val, env.done_t.cpu().numpy(), p_after, e_after, ended_now)
        ended = acc_want["ended"] != 0
        plain_out = plain_acc = None
        for L in launches:
            before = {k: (None if x is None else x.cpu().numpy()) for k, x in (("rs", L.rs), ("phi", L.phi))}
            out, acc_after = L.run(env, guard, kind, N, P, acc, live, value)
            got = out["r"].cpu().numpy()
            want = L.want_r(raw, lv, db, p_after, e_after, ended)
            assert np.array_equal(_bits(got), _bits(want)), (L.name, t, np.abs(got - want).max())
            assert np.all(got[lv == 0] == 0.0)
            if L.scaling:
                rs = L.rs.cpu().numpy()
                assert np.array_equal(_bits(rs), _bits(L.rs_host)), (L.name, t)
                assert np.array_equal(_bits(rs[db]), _bits(before["rs"][db]))
            if L.shaping:
                phi = L.phi.cpu().numpy()
                assert np.array_equal(_bits(phi), _bits(L.phi_host)), (L.name, t)
                assert np.array_equal(_bits(phi[db]), _bits(before["phi"][db]))
            if plain_out is None:                       # the plain launch against the bookkeeping
                plain_out, plain_acc = out, acc_after
                got_acc = {k: v.cpu().numpy() for k, v in acc_after.items()}
                for k in ("ended", "captured", "length", "done_before"):
                    assert np.array_equal(got_acc[k], acc_want[k]), (k, t)
                assert np.all(np.abs(got_acc["ret"] - acc_want["ret"]) <= 1e-6 * np.maximum(np.abs(acc_want["ret"]), 1.0)), t
                assert np.array_equal(out["active"].cpu().numpy(), rows["active"]) and np.array_equal(out["v"].cpu().numpy(), rows["v"])
                assert np.array_equal(out["v_next"].cpu().numpy(), np.where(rows["v_next_zero"], np.float32(0), np.float32(7)))
                if kind == "e3d":
                    assert np.array_equal(out["live_next"].cpu().numpy(), rows["live_next"])
                else:
                    n2n_policy_ref.assert_policy_record({k: out[k].cpu().numpy() for k in ("r", "active", "v", "v_next")}, got_acc, p_after,
                                                        e_after, target, raw, env.done_t.cpu().numpy(), lv, val, acc_np, env.kill_radius)
            else:
                for k in ("active", "v", "v_next") + (("live_next",) if kind == "e3d" else ()):
                    assert _same_bytes(out[k], plain_out[k]), (k, L.name, t)
                for k in acc_after:
                    assert _same_bytes(acc_after[k], plain_acc[k]), (k, L.name, t)
                on = lv != 0
                key = "shared" if L.team is not None and not L.scaling else "scaled" if L.scaling and not L.shaping else "shaped"
                seen[key] += int(((got != raw * lv) & on).sum())
        seen["live"] += int((lv != 0).sum()); seen["deaths"] += int(((lv != 0) & (p_after[:, -1, :] == 0)).sum())
        seen["done_rows"] += int(db.sum())
        acc = {k: v.clone() for k, v in plain_acc.items()}
        live = _t(rows["live_next"])
    final = {k: v.cpu().numpy() for k, v in acc.items()}
    print(f"{wc.IDS(case)}: {seen}, ended {int(final['ended'].sum())}, captured {int(final['captured'].sum())} of {N}")
    assert final["done_before"].all() and final["ended"].any() and not final["ended"].all() and final["captured"].any()
    assert np.array_equal(final["length"], (~wc.done_before(ep)[:wc.T]).sum(0).astype(np.float32))
    assert min(seen.values()) > 0, seen
    guard.check()


# ---- shaping_begin and the scripted pursuers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_shaping_begin_matches_the_potential(case):
    kind, P, E, N = case
    env, ep, guard = _env(case)
    env.enable_reward_shaping(COEF)
    for t in wc.GUIDANCE_TICKS:
        _inject(env, ep, t)
        env.shaping_phi = guard.make("shaping_phi", (N, P), torch.float64, False, fill=123.0)
        env.shaping_begin()
        want = shaping_ref.potential(ep["p"][t], ep["e"][t], COEF)
        assert np.array_equal(_bits(env.shaping_phi.cpu().numpy()), _bits(want)), t
        assert (want < 0).any() and (t != wc.GUIDANCE_TICKS[-1] or (want == 0).any())
    guard.check()


@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_guidance_matches_the_reference(case):
    """the rules of tests/test_guidance_gpu.py.  env_3d: the three commands within 1e-12 of the f64 reference, the speed command and
    hold rows exact.  env_n2n: the int32 actions equal the reference's except on rows whose bearing lies within 1e-9 of an octant
    boundary; tests/test_wide_team_cases_cpu.py asserts that the wide states have none"""
    kind, P, E, N = case
    env, ep, guard = _env(case)
    for t in wc.GUIDANCE_TICKS:
        _inject(env, ep, t)
        p, e = ep["p"][t], ep["e"][t]
        for lead, sr, gain in gc.PARAMS:
            env.set_guidance(lead, sr, gain)
            if kind == "e3d":
                out = guard.make("actions", (N, P, 3), torch.float64, False)
                got = env.guidance_actions(out).cpu().numpy()
                want = guidance_ref.e3d_actions(p, e, gc.E3D_P_VMAX, lead, sr, gain)
                hold = guidance_ref.hold_rows_e3d(p, e, gc.E3D_P_VMAX, lead, sr, gain)
                assert np.abs(got).max() <= 1.0 and np.abs(got - want).max() <= 1e-12, (t, lead, sr, gain)
                assert np.array_equal(got[..., 2], want[..., 2]) and np.array_equal(got[hold], want[hold])
                assert (~hold).any() and (t != wc.GUIDANCE_TICKS[-1] or hold.any())
            else:
                out = guard.make("actions", (N, P), torch.int32, False)
                got = env.guidance_actions(out).cpu().numpy()
                want, b = guidance_ref.n2n_actions(p, e, gc.N2N_P_VMAX, lead, sr, gain, with_bearing=True)
                skip = guidance_ref.near_octant_boundary(b)
                assert not skip.any() and skip.mean() <= 0.01
                assert got.dtype == np.int32 and np.array_equal(got[~skip], want[~skip]), (t, lead, sr, gain)
                assert (got != 0).any() and (t != wc.GUIDANCE_TICKS[-1] or (got == 0).any())
        assert torch.equal(env.p, _t(p)) and torch.equal(env.e, _t(e))     # the records are only read
    guard.check()


# ---- e3d_policy_features and e3d_policy_features_norm at 363 rows -----------------------------------------------------------------------
def test_e3d_policy_features_and_their_normalised_forms_at_33_pursuers():
    """P = 33, N = 11: 363 feature rows, two workgroups of 256 with the second partial, a row stride of 33 in every team loop.  The raw
    features against e3d_features_ref.policy_features at the 1e-6 of tests/test_gauss_gpu.py; the normalised ones, with and without
    accumulation, under the assertions of tests/test_obs_norm_gpu.py: bit for bit obs_norm_ref.normalise of the raw features, inactive
    rows exactly 0, the slot count exact and the sums within c 2^-52 sum |term|"""
    case = ("e3d", 33, 1, 11)
    kind, P, E, N = case
    env, ep, guard = _env(case)
    CLIP, EPS = 1.5, 2.0 ** -52
    feats = lambda name: (guard.make(name + "_a", (N, P, 16), torch.float32, False), guard.make(name + "_c", (N, P, 16), torch.float32, False))
    db = wc.done_before(ep)
    # a non-trivial normaliser state from the features of another state of the episode
    _inject(env, ep, 4)
    fa, fc = env.policy_features(*feats("seed"))
    st = obs_norm_ref.merge(obs_norm_ref.new_state(), obs_norm_ref.sums(obs_norm_ref.new_state(), fa.cpu().numpy(), fc.cpu().numpy(),
                                                                        ep["p"][4][:, 6] != 0))
    assert st[0, 0] > 0 and not np.array_equal(st[0], st[1])
    state = guard.make("norm_state", (2, 33), torch.float64, False).copy_(_t(st))
    n_slots = env.L.e3d_obs_norm_slots(N * P)
    assert n_slots == 2 and N * P == 363
    for t in wc.GUIDANCE_TICKS:
        _inject(env, ep, t)
        p, e = ep["p"][t], ep["e"][t]
        active = p[:, 6] != 0
        fa, fc = env.policy_features(*feats("raw"))
        xa, xc = fa.cpu().numpy(), fc.cpu().numpy()
        ra, rc = e3d_features_ref.policy_features(p, e, ep["pp_adj"][t], ep["pe_adj"][t][..., 0])
        np.testing.assert_allclose(xa, ra, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(xc, rc, rtol=1e-6, atol=1e-6)
        na, nc = env.policy_features(*feats("norm"), state, CLIP)
        wa, wc_ = obs_norm_ref.normalise(st, xa, xc, active, CLIP)
        ga, gc_ = na.cpu().numpy(), nc.cpu().numpy()
        assert np.array_equal(_bits(ga), _bits(wa)) and np.array_equal(_bits(gc_), _bits(wc_)), t
        assert (np.abs(wa) == np.float32(CLIP)).any() and (np.abs(wa[active]) < np.float32(CLIP)).any()
        assert not ga[~active].any() and not gc_[~active].any()
        assert np.array_equal(_bits(state.cpu().numpy()), _bits(st))
        # the same outputs when the launch also accumulates; the sums of the raw features over the live rows
        live = (active & ~db[t][:, None]).astype(np.float32)
        slots = guard.make("slots", (n_slots, 2, 33), torch.float64, False, fill=0.0)
        na2, nc2 = env.policy_features(*feats("norm_acc"), state, CLIP, _t(live), slots)
        assert torch.equal(na2, na) and torch.equal(nc2, nc)
        counted = live != 0
        want = obs_norm_ref.sums(st, xa, xc, counted)
        got = slots.cpu().numpy().sum(0)
        bound = np.zeros((2, 33))
        for k, x in enumerate((xa, xc)):
            d = obs_norm_ref.terms(st[k], x, counted)
            bound[k, 1:17], bound[k, 17:] = np.abs(d).sum(0), (d * d).sum(0)
        c = want[0, 0]
        assert c == counted.sum() and np.array_equal(got[:, 0], want[:, 0])
        assert np.all(np.abs(got - want)[:, 1:] <= (c * EPS * bound)[:, 1:]), t
        assert (slots[:, 0, 0] > 0).all()                                  # both workgroups own a slot and counted rows
    guard.check()


# ---- repeat: every launch twice on the same inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.ONE_PER_PT, ids=wc.IDS)
def test_every_launch_repeats_bit_for_bit(case):
    """from the oracle's state of tick 8: observe, policy inputs, guidance, shaping_begin, the SLSQP evader, the five record variants
    and the tick itself, each launched twice on the same inputs, give the same bytes"""
    kind, P, E, N = case
    runs = []
    for _ in range(2):
        env, ep, guard = _env(case, evader="slsqp")
        env.enable_reward_shaping(COEF)
        t = 8
        _inject(env, ep, t)
        got = {}
        env.observe()
        got.update({"obs_" + k: v.clone() for k, v in env.obs.items()})
        _inject(env, ep, t)
        if kind == "n2n":
            outs = _policy_outs(guard, N, P, E)
            env.policy_inputs(**outs, done_before=_t(wc.done_before(ep)[t].astype(np.uint8)))
            got.update({"in_" + k: v.clone() for k, v in outs.items()})
        got["guidance"] = env.guidance_actions().clone()
        env.shaping_phi = guard.make("shaping_phi", (N, P), torch.float64, False, fill=123.0)
        env.shaping_begin()
        got["phi0"] = env.shaping_phi.clone()
        nit = guard.make("nit", (N, E) if kind == "n2n" else (N,), torch.int32, False, fill=0)
        env.evader_step(nit=nit)
        got["cmd"], got["nit"] = env._cmd.clone(), nit.clone()
        launches = [Launch(env, guard, N, P, *v) for v in VARIANTS]
        _step(env, ep, t)
        got.update({k: getattr(env, k).clone() for k in ("p", "e", "t_dev", "reward_t", "active_t", "done_t")})
        got.update({"tick_" + k: v.clone() for k, v in env.obs.items()})
        acc = env.new_accumulators()
        acc["done_before"].copy_(_t(wc.done_before(ep)[t].astype(np.uint8)))
        live = _t(((ep["p"][t][:, -1, :] != 0) & ~wc.done_before(ep)[t][:, None]).astype(np.float32))
        value = torch.randn(N, P, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV)
        for i, L in enumerate(launches):
            out, acc_after = L.run(env, guard, kind, N, P, acc, live, value)
            got.update({f"rec{i}_{k}": v.clone() for k, v in out.items() if kind == "e3d" or k != "live_next"})
            got.update({f"rec{i}_acc_{k}": v.clone() for k, v in acc_after.items()})
            if L.rs is not None:
                got[f"rec{i}_rs"] = L.rs.clone()
            if L.phi is not None:
                got[f"rec{i}_phi"] = L.phi.clone()
        guard.check()
        runs.append(got)
    assert runs[0].keys() == runs[1].keys() and len(runs[0]) > 40
    for k in runs[0]:
        assert _same_bytes(runs[0][k], runs[1][k]), k
    assert (runs[0]["nit"] > 0).any()


# ---- tick + evader + record captured at PT 64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in wc.ONE_PER_PT if wc.lanes(c[1], c[2]) == 64], ids=wc.IDS)
def test_captured_evader_step_and_record_replay_like_eager(case):
    """evader_step() + step() + policy_record() with the three options, captured as one linear stream and replayed, reach the bytes of
    the same calls made eagerly (after test_captured_evader_and_step_replay_like_eager of tests/test_evader_gpu.py)"""
    kind, P, E, N = case
    K = 6
    ep = wc.episode(*case)
    act = _t(ep["action"][0])

    def make():
        env, _, guard = _env(case, evader="slsqp")
        env.enable_reward_shaping(COEF)
        env.enable_reward_scaling()
        env.shaping_begin()
        io = dict(acc=env.new_accumulators(), live=torch.ones(N, P, device=DEV), value=torch.full((N, P), 0.5, device=DEV),
                  r=guard.make("r", (N, P), torch.float32, True), v_next=guard.make("v_next", (N, P), torch.float32, True))
        return env, guard, io

    def calls(env, io):
        env.evader_step()
        env.step(act)
        extra = dict(live_next=io["live"]) if kind == "e3d" else {}
        env.policy_record(io["acc"], io["live"], io["value"], r=io["r"], v_next=io["v_next"], **extra, scale_gamma=GAMMA, shaping_gamma=GAMMA,
                          team_coef=ALPHA)

    eager, g_eager, io_eager = make()
    for _ in range(K):
        calls(eager, io_eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    warm, _, io_warm = make()
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch recommends before a capture
        calls(warm, io_warm)
    torch.cuda.current_stream().wait_stream(side)
    graphed, g_graphed, io_graphed = make()
    graph = torch.cuda.CUDAGraph()
    with no_gc_during_capture(), torch.cuda.graph(graph):
        calls(graphed, io_graphed)
    for _ in range(K):
        graph.replay()
    torch.cuda.synchronize()
    for name in ("p", "e", "t_dev", "_cmd", "reward_t", "active_t", "done_t", "reward_scale", "shaping_phi"):
        assert _same_bytes(getattr(graphed, name), getattr(eager, name)), name
    for k in ("r", "v_next", "live"):
        assert _same_bytes(io_graphed[k], io_eager[k]), k
    for k in io_eager["acc"]:
        assert _same_bytes(io_graphed["acc"][k], io_eager["acc"][k]), k
    assert bool((eager.t_dev == K).all()) and bool(io_eager["acc"]["length"].max() > 1)
    g_eager.check(); g_graphed.check()


# ---- the SLSQP evader above 16 pursuers -----------------------------------------------------------------------------------------------------
def _n2n_device(g):
    from distributed_multi_agent_reinforcement_learning_amd.n2n_env import ParticleEnv
    M = len(g["p"])
    env = ParticleEnv(num_envs=M, evader="slsqp", **dict(zip(ec.N2N_KEYS, map(float, g["cfg"]))))
    env.initialize(g["P"], g["E"])
    env.reset(init=(g["p"].transpose(0, 2, 1), g["e"].transpose(0, 2, 1), g["target"]))
    guard = Guard()
    env._cmd_slsqp = guard.make("cmd", (M, g["E"]), torch.float64, False)
    nit = guard.make("nit", (M, g["E"]), torch.int32, False)
    env.evader_step(nit=nit)
    torch.cuda.synchronize()
    guard.check()
    return env._cmd.cpu().numpy(), nit.cpu().numpy()


def _e3d_device(g):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_env import ParticleEnv
    M = len(g["p"])
    env = ParticleEnv(num_envs=M, evader="slsqp", **dict(zip(ec.E3D_KEYS, map(float, g["cfg"]))))
    env.initialize(g["P"])
    env.reset(init=(g["p"].transpose(0, 2, 1), g["e"], g["target"]))
    guard = Guard()
    env._cmd_slsqp = guard.make("cmd", (M, 3), torch.float64, False)
    nit = guard.make("nit", (M,), torch.int32, False)
    env.evader_step(nit=nit)
    torch.cuda.synchronize()
    guard.check()
    return env._cmd.cpu().numpy(), nit.cpu().numpy()


@pytest.mark.parametrize("k", range(len(ec.N2N_WIDE_P)), ids=[f"P{P}" for P in ec.N2N_WIDE_P])
def test_n2n_device_evader_matches_reference_above_16_pursuers(k):
    g = ec.n2n_wide_groups()[k]
    ec.n2n_wide_check(g, *_n2n_device(g))


@pytest.mark.parametrize("k", range(len(ec.E3D_WIDE_P)), ids=[f"P{P}" for P in ec.E3D_WIDE_P])
def test_e3d_device_evader_matches_reference_above_16_pursuers(k):
    g = ec.e3d_wide_groups()[k]
    assert len(g["p"]) % 32 != 0                                          # the last workgroup of either launch shape is partial
    ec.e3d_wide_check(g, *_e3d_device(g))


def test_wide_device_evader_matches_host_path():
    """the rules of test_device_matches_host_path (tests/test_evader_gpu.py) at env_n2n P = 64 and at env_3d P = 42 and 43, the last
    launch with 64 lanes per workgroup (64 512 B of dynamic LDS) and the first with 32, the problem count no multiple of 32"""
    from distributed_multi_agent_reinforcement_learning_amd import e3d_env as E, n2n_env as N
    g = [x for x in ec.n2n_wide_groups() if x["P"] == 64][0]
    assert len(g["p"]) % 32 != 0
    assert np.abs(_n2n_device(g)[0] - ec.n2n_host(N.load_library(), g)[0]).max() <= 1e-6
    for P in (42, 43):
        g = [x for x in ec.e3d_wide_groups() if x["P"] == P][0]
        assert len(g["p"]) % 32 != 0 and (3 * P * 64 * 8 > 65536) == (P == 43)
        dev, host = _e3d_device(g)[0], ec.e3d_host(E.load_library(), g)[0]
        share = np.mean(np.abs(dev - host).max(1) <= 1e-6)
        print(f"env_3d P {P}: device within 1e-6 of the host path on {share:.3f} of {len(dev)} problems")
        assert share >= 0.95
