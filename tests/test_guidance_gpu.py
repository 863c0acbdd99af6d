"""The scripted lead-pursuit pursuers on the MI355X: the two guidance kernels against tests/guidance_ref.py on small states built for
where the lane layout can go wrong, the closed loop (deterministic, and the oracle's when stepped with the reference's actions), the
rollout mode `run_episode(policy="guidance")` that moves nothing else, the trainers' `runtime.eval_baseline`, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guidance_cases as gc
from tests import guidance_ref as ref

pytestmark = pytest.mark.gpu

T_LOOP, N_LOOP = 40, 64


def _e3d_env(N, P, **kw):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_env import ParticleEnv
    env = ParticleEnv(num_envs=N, **kw)
    env.initialize(P)
    return env


def _n2n_env(N, P, E, **kw):
    from distributed_multi_agent_reinforcement_learning_amd.n2n_env import ParticleEnv
    env = ParticleEnv(num_envs=N, **kw)
    env.initialize(P, E)
    return env


# ---- the kernels against the specification ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", gc.E3D_P)
def test_e3d_guidance_matches_the_reference(P):
    """a0, a1, a2 within 1e-12 of the f64 reference (the commands lie in [-1, 1]; the only inexact steps are f64 sqrt, divisions and
    atan2 / cos / sin, a few ulp ~ 1e-15, so the bound leaves a thousand-fold margin and still catches any formula, index or ordering
    error); hold rows and a2 exact.  N = 5: the last wave is partial; P = 3, 8 (PT 8), 9 (PT 16)."""
    env = _e3d_env(gc.N, P)
    env.reset(init=gc.e3d_case(P))
    p, e = env.p.cpu().numpy(), env.e.cpu().numpy()
    assert np.array_equal(p, gc.records(*gc.e3d_case(P)[:2])[0])
    out = torch.full((gc.N, P, 3), 7.0, dtype=torch.float64, device=env.device)
    for lead, sr, gain in gc.PARAMS:
        env.set_guidance(lead, sr, gain)
        got = env.guidance_actions(out)
        assert got is out
        got = got.cpu().numpy()
        want = ref.e3d_actions(p, e, gc.E3D_P_VMAX, lead, sr, gain)
        hold = ref.hold_rows_e3d(p, e, gc.E3D_P_VMAX, lead, sr, gain)
        err = np.abs(got - want).max()
        print(f"e3d P {P} lead {lead} sep_range {sr} gain {gain}: max |a - ref| {err:.2e}, {int(hold.sum())} hold rows")
        assert np.abs(got).max() <= 1.0 and err <= 1e-12
        assert np.array_equal(got[..., 2], want[..., 2]) and np.array_equal(got[hold], want[hold]) and hold.sum() == P + 3
    assert torch.equal(env.p.cpu(), torch.from_numpy(p)) and torch.equal(env.e.cpu(), torch.from_numpy(e))   # the records are only read
    env.set_guidance()                                                  # the defaults: lead 1, 4 kill radii, gain 1
    assert np.abs(env.guidance_actions().cpu().numpy() - ref.e3d_actions(p, e, gc.E3D_P_VMAX, *ref.default_params(gc.KILL_RADIUS))).max() <= 1e-12


@pytest.mark.parametrize("P,E", gc.N2N_PE)
def test_n2n_guidance_matches_the_reference(P, E):
    """int32 actions equal to the reference except on rows whose bearing lies within 1e-9 of an octant boundary, of which the inputs
    have none (asserted here as in the CPU test), so nothing is left out"""
    env = _n2n_env(gc.N, P, E)
    env.reset(init=gc.n2n_case(P, E))
    p, e = env.p.cpu().numpy(), env.e.cpu().numpy()
    out = torch.full((gc.N, P), 77, dtype=torch.int32, device=env.device)
    for lead, sr, gain in gc.PARAMS:
        env.set_guidance(lead, sr, gain)
        got = env.guidance_actions(out).cpu().numpy()
        want, b = ref.n2n_actions(p, e, gc.N2N_P_VMAX, lead, sr, gain, with_bearing=True)
        skip = ref.near_octant_boundary(b)
        assert not skip.any() and skip.mean() <= 0.01
        print(f"n2n P {P} E {E} lead {lead} sep_range {sr} gain {gain}: {int((got != want).sum())} of {got.size} rows differ, {int(skip.sum())} left out")
        assert got.dtype == np.int32 and np.array_equal(got[~skip], want[~skip])
        assert np.all(got[2] == 0) and (got == 0).sum() == P + 3
    assert torch.equal(env.p.cpu(), torch.from_numpy(p)) and torch.equal(env.e.cpu(), torch.from_numpy(e))


# ---- closed loop --------------------------------------------------------------------------------------------------------------------
def _cfg(name, **ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config(name, **{"env.max_steps": T_LOOP, "runtime.num_envs": N_LOOP, **ov})


@pytest.fixture(scope="module")
def e3d_agent():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    torch.manual_seed(0)
    return E3dMAPPO(_cfg("cfg5"), N_LOOP, 8)


@pytest.fixture(scope="module")
def n2n_agent():
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO
    torch.manual_seed(0)
    return N2nMAPPO(_cfg("cfg4_n2n"), N_LOOP, 8)


def test_e3d_guidance_episode_is_deterministic(e3d_agent):
    """64 environments of cfg5 (P = 8, the SLSQP evader), T = 40, twice from the same seeds: bit-identical"""
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import make_env
    runs, states = [], set(e3d_agent._states)
    for _ in range(2):
        env = make_env(_cfg("cfg5"), N_LOOP, seed_offset=10 ** 6, training=False)
        assert env.evader == "slsqp" and env.p_num == 8 and env.max_step == T_LOOP
        ret, cap, length = e3d_agent.run_episode(env, None, policy="guidance")
        runs.append((ret.clone(), cap.clone(), length.clone(), env.p.clone(), env.e.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    ret, cap, length = runs[0][:3]
    assert cap.dtype == torch.bool and ret.shape == cap.shape == length.shape == (N_LOOP,)
    assert float(length.min()) >= 1 and float(length.max()) <= T_LOOP and torch.isfinite(ret).all()
    assert set(e3d_agent._states) == states                              # no rollout state was created: no sampler, no counter


def test_n2n_guidance_episode_is_deterministic(n2n_agent):
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import make_env
    runs, states = [], set(n2n_agent._states)
    for _ in range(2):
        env = make_env(_cfg("cfg4_n2n"), N_LOOP, seed_offset=10 ** 6, training=False)
        assert env.evader == "slsqp" and env.p_num == 16 and env.episode_limit == T_LOOP
        acc = n2n_agent.run_episode(env, None, policy="guidance")
        runs.append([acc[k].clone() for k in ("ret", "captured", "length", "done_before", "ended")] + [env.p.clone(), env.e.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][2].min()) >= 1 and float(runs[0][2].max()) <= T_LOOP and bool(runs[0][3].all())
    assert set(n2n_agent._states) == states


def test_e3d_closed_loop_matches_the_oracle():
    """10 ticks under the closed-form evader: the device's guidance actions drive the device, the reference's actions the oracle; states
    within 1e-9 (the trace tolerance of tests/test_e3d_gpu.py), rewards, active flags and done equal"""
    from oracle import e3d_oracle as eo
    N, P = N_LOOP, 8
    env = _e3d_env(N, P, seeds=list(range(500, 500 + N)), max_step=T_LOOP)
    env.reset()
    p0, e0, tg = env.last_init
    cfg = eo.make_cfg(P, T_LOOP)
    oenvs = [eo.OracleE3d(cfg, p0[n], e0[n], tg[n]) for n in range(N)]
    params = ref.default_params(cfg.kill_radius)
    for t in range(10):
        act = env.guidance_actions()
        env.evader_step()
        cmd = env._cmd.cpu().numpy()
        r, done, active = (x.cpu().numpy() for x in env.step(act))
        act = act.cpu().numpy()
        p, e = env.p.permute(0, 2, 1).cpu().numpy(), env.e.cpu().numpy()
        for n, oe in enumerate(oenvs):
            a_ref = ref.e3d_actions(oe.p.T[None], oe.e, cfg.p_vmax, *params)[0]
            assert np.abs(act[n] - a_ref).max() <= 1e-8, (t, n)          # (the states they are computed from agree to 1e-9)
            if oe.e[0, 6] > 0 and oe.p[:, 6].sum() > 0:
                oe.evader_step(cmd[n])
            ro, do, ao = oe.step(a_ref)
            assert np.array_equal(r[n], ro.astype(np.float32)) and np.array_equal(active[n], ao) and bool(done[n]) == do, (t, n)
            assert np.max(np.abs(p[n] - oe.p)) <= 1e-9 and np.max(np.abs(e[n] - oe.e[0])) <= 1e-9, (t, n)


def test_n2n_closed_loop_matches_the_oracle():
    from oracle import n2n_oracle as no
    N, P, E = N_LOOP, 16, 1
    env = _n2n_env(N, P, E, seeds=list(range(700, 700 + N)), episode_limit=T_LOOP)
    env.reset()
    p0, e0, tg = env.last_init
    cfg = no.make_cfg(P, E, T_LOOP)
    oenvs = [no.OracleN2n(cfg, p0[n], e0[n], tg[n]) for n in range(N)]
    params = ref.default_params(cfg.kill_radius)
    left_out = rows = 0
    for t in range(10):
        act = env.guidance_actions()
        env.evader_step()
        cmd = env._cmd.cpu().numpy()
        r, done, active = (x.cpu().numpy() for x in env.step(act))
        act = act.cpu().numpy()
        p, e = env.p.permute(0, 2, 1).cpu().numpy(), env.e.permute(0, 2, 1).cpu().numpy()
        for n, oe in enumerate(oenvs):
            a_ref, b = ref.n2n_actions(oe.p.T[None], oe.e.T[None], cfg.p_vmax, *params, with_bearing=True)
            edge = ref.near_octant_boundary(b[0], 1e-8)                  # (the states agree to 1e-9)
            left_out, rows = left_out + int(edge.sum()), rows + P
            assert np.array_equal(act[n][~edge], a_ref[0][~edge]), (t, n)
            oe.evader_step(cmd[n])
            ro, do, ao = oe.step(act[n])                                 # on an edge row the oracle follows the device
            assert np.array_equal(r[n], ro.astype(np.float32)) and np.array_equal(active[n], ao) and bool(done[n]) == do, (t, n)
            assert np.max(np.abs(p[n] - oe.p)) <= 1e-9 and np.max(np.abs(e[n] - oe.e)) <= 1e-9, (t, n)
    assert left_out <= 0.01 * rows, (left_out, rows)


# ---- nothing else moves ---------------------------------------------------------------------------------------------------------------
def _network_episode(agent, env):
    out = agent.run_episode(env, None)
    out = (out["ret"], out["captured"], out["length"]) if isinstance(out, dict) else out
    return [x.clone() for x in out]


@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_a_guidance_episode_moves_nothing_of_the_agent_or_the_training_state(kind, e3d_agent, n2n_agent):
    """after a guidance episode the agent's sampling counter and GRU buffers and the environment's reward-scaling (n, mean, S) and
    shaping state are what they were, and a network episode from the same reset generators and counter reproduces the earlier one"""
    if kind == "e3d":
        from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import make_env
        agent, name = e3d_agent, "cfg5"
    else:
        from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import make_env
        agent, name = n2n_agent, "cfg4_n2n"
    N = 16
    env = make_env(_cfg(name, **{"algo.use_reward_scaling": True, "algo.reward_shaping": "distance"}), N)
    env.reward_scale.uniform_(0.5, 1.5)                                  # as if earlier rollouts had filled them
    env.shaping_phi.uniform_(-2.0, -1.0)
    gen0 = env.get_resetter_state()
    st = agent._state(env)
    c0 = st.counter.clone()
    first = _network_episode(agent, env)
    c1, ha, hc, t1 = st.counter.clone(), st.hbuf_a.clone(), st.hbuf_c.clone(), st.t
    rs, phi = env.reward_scale.clone(), env.shaping_phi.clone()
    assert int(c1) > int(c0)
    agent.run_episode(env, None, policy="guidance")
    assert agent._state(env) is st and torch.equal(st.counter, c1) and st.t == t1
    assert torch.equal(st.hbuf_a, ha) and torch.equal(st.hbuf_c, hc)
    P = env.p_num
    assert torch.equal(env.reward_scale[:, :1 + 2 * P], rs[:, :1 + 2 * P]) and torch.equal(env.shaping_phi, phi)
    assert not env.reward_scale[:, 1 + 2 * P:].any()                     # (R is zeroed by every reset, as at any episode start)
    env.set_resetter_state(gen0)
    st.counter.copy_(c0)
    again = _network_episode(agent, env)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


# ---- the trainers' baseline -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_eval_baseline_is_computed_once_and_only_when_asked_for(kind, monkeypatch):
    if kind == "e3d":
        from distributed_multi_agent_reinforcement_learning_amd import e3d_env as envmod
        from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dTrainer as Tr
        name = "cfg5"
    else:
        from distributed_multi_agent_reinforcement_learning_amd import n2n_env as envmod
        from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nTrainer as Tr
        name = "cfg4_n2n"
    calls = []
    inner = envmod.ParticleEnv.guidance_actions
    monkeypatch.setattr(envmod.ParticleEnv, "guidance_actions", lambda self, out=None: (calls.append(1), inner(self, out))[1])
    T, keys = 12, {"eval_return", "eval_capture_rate", "eval_episode_length"}
    ov = {"env.max_steps": T, "runtime.num_envs": 8}
    plain = Tr(_cfg(name, **ov), num_eval_envs=8, tuned_gemms=False)
    rec = plain.evaluate()
    assert set(rec) == keys and not calls and plain.eval_baseline is None  # the key absent: exactly the parent's record
    tr = Tr(_cfg(name, **ov, **{"runtime.eval_baseline": "guidance"}), num_eval_envs=8, tuned_gemms=False)
    gen0 = tr.make_eval_env().get_resetter_state()
    a, b = tr.evaluate(), tr.evaluate()
    from distributed_multi_agent_reinforcement_learning_amd.guidance import BASELINE_LOG_KEYS
    assert set(a) == set(b) == keys | set(BASELINE_LOG_KEYS)
    assert len(calls) == T                                               # one episode of T launches for both evaluations
    assert all(a[k] == b[k] and np.isfinite(a[k]) for k in BASELINE_LOG_KEYS)
    assert 0.0 <= a["baseline_capture_rate"] <= 1.0 and 1.0 <= a["baseline_episode_length"] <= T
    # the baseline has environments of its own: the evaluation's first episode is the plain trainer's
    assert all(a[k] == rec[k] for k in keys)
    assert not np.array_equal(tr.eval_env.get_resetter_state(), gen0)   # (two evaluations advanced the evaluation generators, nothing else)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_guidance_with_a_buffer_raises(e3d_agent, n2n_agent):
    env = _e3d_env(4, 8, max_step=4)
    with pytest.raises(ValueError, match="guidance"):
        e3d_agent.run_episode(env, e3d_agent.new_buffer(4, 4, 8), policy="guidance")
    env = _n2n_env(4, 16, 1, episode_limit=4)
    with pytest.raises(ValueError, match="guidance"):
        n2n_agent.run_episode(env, n2n_agent.new_buffer(4, 4, 16, 1), policy="guidance")
    with pytest.raises(ValueError, match="policy"):
        n2n_agent.run_episode(env, None, policy="pso")


def test_baseline_flag_is_refused_on_a_pursuit_config(capsys):
    from distributed_multi_agent_reinforcement_learning_amd import main as cli
    with pytest.raises(SystemExit):
        cli.main(["--config", "cfg2", "--baseline", "guidance"])
    assert "--baseline" in capsys.readouterr().err


def test_null_pointers_return_the_null_error():
    env = _e3d_env(4, 3)
    env.reset()
    out = env.guidance_actions()
    args = [C.byref(env.c), C.byref(env.st), C.byref(env.guidance), C.c_void_p(out.data_ptr()), None]
    assert env.L.e3d_pursuer_guidance(*args) == 0
    for k in range(4):
        bad = list(args); bad[k] = None
        assert env.L.e3d_pursuer_guidance(*bad) == 40002
    env = _n2n_env(4, 3, 2)
    env.reset()
    out = env.guidance_actions()
    args = [C.byref(env.c), C.byref(env.st), C.byref(env.guidance), C.c_void_p(out.data_ptr()), None]
    assert env.L.n2n_pursuer_guidance(*args) == 0
    for k in range(4):
        bad = list(args); bad[k] = None
        assert env.L.n2n_pursuer_guidance(*bad) == 30002
    env.guidance.sep_range = float("nan")
    assert env.L.n2n_pursuer_guidance(*args) == 30001
    torch.cuda.synchronize()


def test_main_baseline_prints_the_evaluation_keys(capsys):
    """main --baseline guidance needs no model directory and prints the JSON keys of --evaluate, on the evaluation seeds"""
    import json
    from distributed_multi_agent_reinforcement_learning_amd import main as cli
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import guidance_episode, make_env
    res = cli.main(["--config", "cfg5", "--baseline", "guidance", "--eval-envs", "8", "env.max_steps=12"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == res and set(res) == {"eval_return", "eval_capture_rate", "eval_episode_length"}
    env = make_env(_cfg("cfg5", **{"env.max_steps": 12}), 8, seed_offset=10 ** 6, training=False)
    ret, cap, length = guidance_episode(env)
    assert res["eval_return"] == float(ret.mean()) and res["eval_episode_length"] == float(length.mean())
