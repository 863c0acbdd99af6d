"""GPU checks of algo.team_reward (the team option of e3d_policy_record / n2n_policy_record, include/policy_record.h): the record launch with sharing against
tests/team_reward_ref.py bit for bit -- alone, with reward scaling, with distance shaping, with both --, every other output byte for
byte against the unshared launch, alpha = 0 against the unshared entry points, determinism, and the option in the trainers: absent,
on, deterministic, resumed, and out of evaluation and the scripted pursuers' episodes.

Five environments, so the last wave is partial; the group widths 8 (P = 3, 8) and 16 (P = 9, 16).  More than 16 pursuers:
tests/test_wide_teams_gpu.py."""
import itertools

import numpy as np
import pytest
import torch

from tests import reward_scale_ref as scale_ref
from tests import shaping_ref
from tests import team_reward_ref as ref

pytestmark = pytest.mark.gpu

CONFIG = {"e3d": "cfg5", "n2n": "cfg4_n2n"}
GAMMA, COEF = 0.99, 0.1
N, TICKS = 5, 12
SHAPES = [("e3d", 3, 1), ("e3d", 8, 1), ("e3d", 9, 1), ("n2n", 3, 2), ("n2n", 16, 1), ("n2n", 16, 8)]
ALPHAS = (0.25, 0.5, 1.0)
MODES = list(itertools.product((False, True), (False, True)))   # (scaling, shaping)
DEV = "cuda"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _env(kind, P, E):
    if kind == "n2n":
        from distributed_multi_agent_reinforcement_learning_amd.n2n_env import ParticleEnv
        env = ParticleEnv(num_envs=N, seeds=list(range(N)), evader="rule")
        env.initialize(P, E)
    else:
        from distributed_multi_agent_reinforcement_learning_amd.e3d_env import ParticleEnv
        env = ParticleEnv(num_envs=N, seeds=list(range(N)), evader="rule")
        env.initialize(P)
    return env


class Launch:
    """one variant of the record launch with its own states on the device (the environment's attributes are pointed at them for
    the call) and, for the variants held to the restatement, their host mirrors"""

    def __init__(self, env, P, scaling, shaping, team_coef):
        self.scaling, self.shaping, self.team_coef = scaling, shaping, team_coef
        self.rs = torch.zeros((N, 1 + 3 * P), dtype=torch.float64, device=DEV) if scaling else None
        self.phi = None
        if shaping:
            self.phi = torch.full((N, P), 123.0, dtype=torch.float64, device=DEV)
            env.shaping_phi = self.phi
            env.shaping_begin()
        self.rs_host = scale_ref.new_state(N, P) if scaling else None
        self.phi_host = shaping_ref.potential(env.p.cpu().numpy(), env.e.cpu().numpy(), COEF) if shaping else None
        if shaping:
            assert np.array_equal(_bits(self.phi.cpu().numpy()), _bits(self.phi_host))

    def clone(self):
        c = object.__new__(Launch)
        c.__dict__.update(self.__dict__)
        c.rs, c.phi = (None if t is None else t.clone() for t in (self.rs, self.phi))
        return c

    def run(self, env, kind, P, acc, live, value):
        """-> (outputs, accumulators after) of this variant on a copy of the accumulators"""
        env.reward_scale, env.shaping_phi = self.rs, self.phi
        acc = {k: v.clone() for k, v in acc.items()}
        out = {k: torch.full((N, 3, P), 7.0, device=DEV)[:, 1] for k in ("r", "active", "v", "v_next", "live_next")}
        extra = dict(live_next=out["live_next"]) if kind == "e3d" else {}
        kw = {} if self.team_coef is None else dict(team_coef=self.team_coef)
        env.policy_record(acc, live, value, out["r"], out["active"], out["v"], out["v_next"], **extra,
                          scale_gamma=GAMMA if self.scaling else None, shaping_gamma=GAMMA if self.shaping else None, **kw)
        return out, acc


def _inject(env, t, P, gen):
    """rewards no random walk of 12 ticks would pay, written where the tick wrote its own: a capture and two collisions in one step,
    fractional rewards on a whole team, a reward on a row that is not live, rewards in the environment done before the run"""
    r = env.reward_t
    if t % 3 == 0:
        r[0, 0] += 1.0
        r[0, 1] -= 1.0
        r[0, 2] -= 1.0
    if t % 4 == 1:
        r[3] = torch.rand(P, generator=gen, device=DEV) * 2 - 1
    if t % 2 == 0:
        r[1, 0] = 0.5            # pursuer 0 of environment 1 is inactive from the start: the row is not live
        r[1, 1] = -2.0
    if t == 5:
        r[4, P - 1] = 1.0
    r[2] = 1.0 + t               # environment 2 was done before the run
    r.add_(0.0)                  # (-0.0 + 0.0 is +0.0: the environments never pay -0.0, see csrc/team_reward.hpp)


def _rollout(kind, P, E, variants, per_tick):
    """12 ticks from random actions under the closed-form evader.  Pursuer 0 of environment 1 and the last pursuer of environment 3
    are inactive from the start, pursuer 1 of environment 0 is switched off before tick 1 (it dies in that step), environment 2 is
    done before the run.  Every tick: the unshared plain launch advances the accumulators; per_tick(ctx) gets the accumulators before
    it, its outputs, the accumulators after it and everything the restatement needs, read back."""
    env = _env(kind, P, E)
    env.enable_reward_shaping(COEF)
    env.reset()
    env.p[1, -1, 0] = 0.0
    env.p[3, -1, P - 1] = 0.0
    launches = [Launch(env, P, *v) for v in variants]
    plain = Launch(env, P, False, False, None)
    gen = torch.Generator(device=DEV).manual_seed(100 * P + E)
    acc = env.new_accumulators()
    acc["done_before"][2] = 1
    live = ((env.p[:, -1, :] != 0) & (acc["done_before"] == 0)[:, None]).float()
    for t in range(TICKS):
        if t == 1:
            env.p[0, -1, 1] = 0.0
        if kind == "e3d":
            action = torch.rand(N, P, 3, generator=gen, device=DEV, dtype=torch.float64) * 2 - 1
        else:
            action = torch.randint(0, 9, (N, P), generator=gen, device=DEV, dtype=torch.int32)
        env.evader_step()
        env.step(action)
        _inject(env, t, P, gen)
        value = torch.randn(N, P, generator=gen, device=DEV)
        out_u, acc_after = plain.run(env, kind, P, acc, live, value)
        raw, lv = env.reward_t.cpu().numpy(), live.cpu().numpy()
        assert np.array_equal(_bits(out_u["r"].cpu().numpy()), _bits(raw * lv))            # the unshared launch is what it was
        ctx = dict(env=env, kind=kind, P=P, t=t, acc=acc, live=live, value=value, out_u=out_u, acc_after=acc_after, raw=raw, lv=lv,
                   db=acc["done_before"].cpu().numpy() != 0, p_after=env.p.cpu().numpy(), e_after=env.e.cpu().numpy(),
                   ended=acc_after["ended"].cpu().numpy() != 0)
        per_tick(ctx, launches)
        acc = acc_after
        dn = acc["done_before"].cpu().numpy() != 0
        live = torch.from_numpy(((ctx["p_after"][:, -1, :] != 0) & ~dn[:, None]).astype(np.float32)).to(DEV)
        if kind == "e3d":
            assert torch.equal(live, out_u["live_next"].contiguous())


def _others_equal(ctx, out, acc, what):
    for k in ("active", "v", "v_next") + (("live_next",) if ctx["kind"] == "e3d" else ()):
        assert _same_bytes(out[k], ctx["out_u"][k]), (k, what, ctx["t"])
    for k in acc:
        assert _same_bytes(acc[k], ctx["acc_after"][k]), (k, what, ctx["t"])


# ---- the kernels against the restatement, and against the unshared launch ------------------------------------------------------------
@pytest.mark.parametrize("kind,P,E", SHAPES)
def test_team_record_matches_the_restatement_bit_for_bit(kind, P, E):
    """alpha in (0.25, 0.5, 1.0) x scaling off / on x shaping off / on, each with its own states, over the same 12 ticks: the buffer's
    r (fp32), reward_scale and shaping_phi (f64) equal tests/team_reward_ref.record_step bit for bit, environments done before the
    step untouched; active, v, v_next, live_next and the five accumulators are the unshared launch's bytes."""
    seen = dict(shared=0, live=0, mates=0, deaths=0)

    def per_tick(ctx, launches):
        env, raw, lv, db = ctx["env"], ctx["raw"], ctx["lv"], ctx["db"]
        for L in launches:
            what = (L.team_coef, L.scaling, L.shaping)
            rs_before = L.rs.cpu().numpy() if L.scaling else None
            phi_before = L.phi.cpu().numpy() if L.shaping else None
            out, acc = L.run(env, kind, P, ctx["acc"], ctx["live"], ctx["value"])
            _others_equal(ctx, out, acc, what)
            want = ref.record_step(raw, lv, db, L.team_coef, GAMMA, L.rs_host, L.phi_host, ctx["p_after"], ctx["e_after"], ctx["ended"], COEF)
            got = out["r"].cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (what, ctx["t"], np.abs(got - want).max())
            assert np.all(got[lv == 0] == 0.0)
            if L.scaling:
                rs = L.rs.cpu().numpy()
                assert np.array_equal(_bits(rs), _bits(L.rs_host)), (what, ctx["t"])
                assert np.array_equal(_bits(rs[db]), _bits(rs_before[db])) and rs[~db, 0].min() == ctx["t"] + 1
            if L.shaping:
                phi = L.phi.cpu().numpy()
                assert np.array_equal(_bits(phi), _bits(L.phi_host)), (what, ctx["t"])
                assert np.array_equal(_bits(phi[db]), _bits(phi_before[db]))
            if not L.scaling and not L.shaping:
                live = lv != 0
                seen["shared"] += int(((got != raw * lv) & live).sum())
                seen["live"] += int(live.sum())
                seen["mates"] += int((live & (raw == 0) & (got != 0)).sum())
        seen["deaths"] += int(((lv != 0) & (ctx["p_after"][:, -1, :] == 0)).sum())

    _rollout(kind, P, E, [(s, h, a) for a in ALPHAS for s, h in MODES], per_tick)
    print(f"{kind} P={P} E={E}: {seen['live']} live rows over the three plain variants, r != raw * live on {seen['shared']}, "
          f"{seen['mates']} rows paid for a team-mate's reward, {seen['deaths']} deaths")
    assert seen["mates"] > 0 and seen["shared"] > seen["mates"] and seen["deaths"] >= 1


@pytest.mark.parametrize("kind,P,E", SHAPES)
def test_alpha_zero_is_the_unshared_entry_points_byte_for_byte(kind, P, E):
    """team_coef = 0.0 goes through the TEAM instantiations and must leave r, reward_scale, shaping_phi and everything else the bytes
    of the entry points without sharing, in all four scaling / shaping combinations"""
    def per_tick(ctx, launches):
        env = ctx["env"]
        for team, plain in zip(launches[:4], launches[4:]):
            what = ("alpha 0", team.scaling, team.shaping)
            out_t, acc_t = team.run(env, kind, P, ctx["acc"], ctx["live"], ctx["value"])
            out_p, acc_p = plain.run(env, kind, P, ctx["acc"], ctx["live"], ctx["value"])
            _others_equal(ctx, out_t, acc_t, what)
            assert _same_bytes(out_t["r"], out_p["r"]), (what, ctx["t"])
            for a, b in ((team.rs, plain.rs), (team.phi, plain.phi)):
                assert (a is None and b is None) or _same_bytes(a, b), (what, ctx["t"])
            assert all(_same_bytes(acc_t[k], acc_p[k]) for k in acc_t)

    _rollout(kind, P, E, [(s, h, 0.0) for s, h in MODES] + [(s, h, None) for s, h in MODES], per_tick)


@pytest.mark.parametrize("kind,P,E", [("e3d", 9, 1), ("n2n", 16, 8)])
def test_two_calls_give_identical_bits(kind, P, E):
    def per_tick(ctx, launches):
        env = ctx["env"]
        for L in launches:
            twin = L.clone()
            a, acc_a = L.run(env, kind, P, ctx["acc"], ctx["live"], ctx["value"])
            b, acc_b = twin.run(env, kind, P, ctx["acc"], ctx["live"], ctx["value"])
            assert all(_same_bytes(a[k], b[k]) for k in a) and all(_same_bytes(acc_a[k], acc_b[k]) for k in acc_a)
            assert _same_bytes(L.rs, twin.rs) and _same_bytes(L.phi, twin.phi)

    _rollout(kind, P, E, [(True, True, 0.5)], per_tick)


@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_bad_coefficient_and_missing_state_are_refused(kind):
    env = _env(kind, 4, 1)
    env.reset()
    acc = env.new_accumulators()
    live = torch.ones(N, 4, device=DEV)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="policy_record failed with code [34]0001"):
            env.policy_record(acc, live, team_coef=bad)
    with pytest.raises(RuntimeError, match="enable_reward_scaling"):
        env.policy_record(acc, live, scale_gamma=GAMMA, team_coef=0.5)
    with pytest.raises(RuntimeError, match="enable_reward_shaping"):
        env.policy_record(acc, live, shaping_gamma=GAMMA, team_coef=0.5)
    assert not any(v.any() for v in acc.values())                       # nothing was launched


# ---- the option in the trainers -----------------------------------------------------------------------------------------------------
N_ENVS, T, P_NUM = 16, 20, 3
LOG = ("mean_return", "critic_loss", "actor_loss", "eval_return", "capture_rate", "episode_length")


def _cfg(kind, **ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config(CONFIG[kind], **{"runtime.num_envs": N_ENVS, "env.max_steps": T, "env.num_defender": P_NUM,
                                            f"runtime.{kind}_evader": "rule", **ov})


def _trainer(kind, cfg, pay=True):
    """pay: pursuer 0 of training environment 0 is paid +1 in tick 5 of every rollout, written where the tick wrote its reward -- a
    random policy earns nothing in 20 ticks, and sharing nothing is sharing untested"""
    from distributed_multi_agent_reinforcement_learning_amd import e3d_agent, n2n_agent
    tr = (e3d_agent.E3dTrainer if kind == "e3d" else n2n_agent.N2nTrainer)(cfg, num_eval_envs=4, eval_every=1)
    if pay:
        env, step = tr.env, tr.env.step

        def paid_step(action):
            res = step(action)
            if env.time_step == 6:
                env.reward_t[0, 0] += 1.0
            return res
        env.step = paid_step
    return tr


def _weights_equal(a, b):
    for x, y in ((a.agent.actor, b.agent.actor), (a.agent.critic, b.agent.critic)):
        sx, sy = x.state_dict(), y.state_dict()
        if list(sx) != list(sy) or not all(torch.equal(sx[k], sy[k]) for k in sx):
            return False
    return True


def _same_logs(la, lb):
    return set(la) == set(lb) and all(np.float64(la[k]).tobytes() == np.float64(lb[k]).tobytes() for k in LOG)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_option_absent_is_the_run_that_never_mentions_it(tmp_path, kind):
    a = _trainer(kind, _cfg(kind, **{"algo.save_cwd": str(tmp_path / "a")}))
    b = _trainer(kind, _cfg(kind, **{"algo.save_cwd": str(tmp_path / "b"), "algo.team_reward": 0}))
    assert a.agent.team_reward == b.agent.team_reward == 0.0 and b.agent._team_coef(object()) is None
    for _ in range(3):
        la, lb = a.iterate()[1], b.iterate()[1]
        assert _same_logs(la, lb)
        assert _same_bytes(a.agent.buffer["r"], b.agent.buffer["r"])
    assert _weights_equal(a, b)
    pa, pb = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    a.save_resume(pa); b.save_resume(pb)
    on = _trainer(kind, _cfg(kind, **{"algo.save_cwd": str(tmp_path / "c"), "algo.team_reward": 0.5}))
    on.iterate()
    pc = str(tmp_path / "c.pt")
    on.save_resume(pc)
    keys = [sorted(torch.load(p, weights_only=False)) for p in (pa, pb, pc)]
    assert keys[0] == keys[1] == keys[2]                                 # the option is stateless: nothing of it is in a bundle
    assert on.agent.policy_meta() == a.agent.policy_meta() and set(la) == set(on.iterate()[1])   # ... nor a log key


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_option_on_shares_the_buffer_reward_and_nothing_else(kind, monkeypatch):
    """The first rollout's actions do not depend on rewards, so with identical seeds it visits the same states with the option on and
    off.  Pursuer 0 of environment 0 is paid +1 in tick 5: with alpha = 1 its live team-mates' rows hold 1 as well, every other buffer
    entry, mean_return and the rollout statistics are equal.  Evaluation and the scripted pursuers' episodes never share: the record
    launch gets a team_coef on the training rollout only."""
    from distributed_multi_agent_reinforcement_learning_amd import e3d_env, n2n_env
    from distributed_multi_agent_reinforcement_learning_amd.particle_agent import episode_triple
    Env = (e3d_env if kind == "e3d" else n2n_env).ParticleEnv
    record, coefs = Env.policy_record, []
    monkeypatch.setattr(Env, "policy_record", lambda self, *a, **k: (coefs.append(k.get("team_coef")), record(self, *a, **k))[1])
    on, off = _trainer(kind, _cfg(kind, **{"algo.team_reward": 1.0})), _trainer(kind, _cfg(kind))
    assert on.agent.team_reward == 1.0 and off.agent.team_reward == 0.0
    assert on.evaluate() == off.evaluate()                               # same initial weights, same evaluation seeds
    guided = [episode_triple(tr.agent.run_episode(tr.make_eval_env(), None, policy="guidance")) for tr in (on, off)]
    assert all(torch.equal(x, y) for x, y in zip(*guided))
    assert coefs and all(c is None for c in coefs)                       # run_episode(env, None) and policy="guidance" share nothing
    del coefs[:]
    mean_on, buf_on, steps, stats_on = on.agent.explore_env(on.env)
    assert coefs == [1.0] * T
    del coefs[:]
    mean_off, buf_off, _, stats_off = off.agent.explore_env(off.env)
    assert coefs == [None] * T
    assert mean_on == mean_off and stats_on == stats_off                 # the return stays the raw reward
    for k in buf_off:
        if k != "r":
            assert torch.equal(buf_on[k], buf_off[k]), k
    active = buf_off["active"]
    assert (active[0, 5] != 0).all() and buf_off["r"][0, 5, 0] >= 1.0
    # without scaling and shaping, alpha = 1: every live row holds the step's team total (small integers: exact in fp32 and f64)
    assert torch.equal(buf_on["r"], buf_off["r"].sum(-1, keepdim=True) * active)
    differ = buf_on["r"] != buf_off["r"]
    assert differ[0, 5].any() and torch.equal(buf_on["r"][active == 0], buf_off["r"][active == 0])
    print(f"{kind}: r[0, 5] off {buf_off['r'][0, 5].tolist()} on {buf_on['r'][0, 5].tolist()}, {int(differ.sum())} rows differ")
    # every differing row is a live row of a step in which a team-mate was paid
    paid = (buf_off["r"] != 0).any(-1, keepdim=True)
    assert not (differ & ~(paid & (buf_off["active"] != 0))).any()
    rows = []
    for tr in (on, off):
        tr.total_steps += steps
        with torch.enable_grad():
            rows.append(tr.agent.train(tr.agent.buffer, tr.total_steps))
        tr.agent.ac_optimizer.step()
    assert np.isfinite(rows).all() and rows[0][0] != rows[1][0]          # the critic regresses on another target
    assert not _weights_equal(on, off)
    off.agent.actor.load_state_dict(on.agent.actor.state_dict()); off.agent.critic.load_state_dict(on.agent.critic.state_dict())
    assert on.evaluate() == off.evaluate()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_option_on_is_deterministic_and_resumes_bit_for_bit(tmp_path, kind):
    ov = {"algo.save_cwd": str(tmp_path / "model"), "algo.team_reward": 0.5, "algo.use_reward_scaling": True, "algo.reward_shaping": "distance"}
    a, twin = _trainer(kind, _cfg(kind, **ov)), _trainer(kind, _cfg(kind, **ov))
    path = str(tmp_path / "resume.pt")
    logs_a, logs_t = [], []
    for it in range(3):
        logs_a.append(a.iterate()[1]); logs_t.append(twin.iterate()[1])
        if it == 1:
            a.save_resume(path)
    assert all(_same_logs(x, y) for x, y in zip(logs_a, logs_t))         # two runs agree bit for bit
    assert _weights_equal(a, twin) and torch.equal(a.agent.buffer["r"], twin.agent.buffer["r"])
    b = _trainer(kind, _cfg(kind, **ov))
    b.load_resume(path)
    assert _same_logs(b.iterate()[1], logs_a[2])                         # a resume after iteration 2 continues bit for bit
    assert _weights_equal(a, b) and torch.equal(a.agent.buffer["r"], b.agent.buffer["r"])
    assert torch.equal(a.env.reward_scale, b.env.reward_scale) and torch.equal(a.env.shaping_phi, b.env.shaping_phi)
