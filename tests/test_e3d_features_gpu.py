"""GPU checks of env_3d's line-of-sight policy features (algo.e3d_features: pursuit): the kernel
e3d_pursuit_features against tests/e3d_features_ref.py in every lane layout and evader model, the relay of a sighting along long
chains, what a launch writes and leaves alone, and the E3dMAPPO agent / E3dTrainer on the 32-wide buffer (rollout-update agreement,
determinism, checkpoints and resume, the options off, imitation on a fixed buffer)."""
import numpy as np
import pytest
import torch

from tests import e3d_features_cases as fc
from tests import e3d_features_ref as ref

pytestmark = pytest.mark.gpu

MODES = ref.EVADER_OBS


def _env(c):
    """a ParticleEnv holding the records and adjacencies of a case dict"""
    from distributed_multi_agent_reinforcement_learning_amd.e3d_env import ParticleEnv
    N, _, P = c["p"].shape
    env = ParticleEnv(num_envs=N, evader="rule")
    env.initialize(P)
    # injected initial conditions (host order (N, P, 7)): the reset's own placement cannot seat 33 pursuers 4 apart in its 10^3 box
    env.reset(init=(np.ascontiguousarray(c["p"].transpose(0, 2, 1)), c["e"], c["target"]))
    env.p.copy_(torch.from_numpy(c["p"]))
    env.e.copy_(torch.from_numpy(c["e"]))
    env.target.copy_(torch.from_numpy(c["target"]))
    env.t_dev.copy_(torch.from_numpy(c["time_step"]))
    env.obs["pp_adj"].copy_(torch.from_numpy(c["pp_adj"]))
    env.obs["pe_adj"].copy_(torch.from_numpy(c["pe_adj"])[..., None])
    return env


def _launch(env, mode, fill=7.0):
    shape = (env.num_envs, env.p_num, 32)
    fa, fcr = torch.full(shape, fill, device="cuda"), torch.full(shape, fill, device="cuda")
    env.pursuit_features(fa, fcr, mode)
    return fa, fcr


_REF = {}


def _want(P, mode):
    """the specification on the shared case, computed once per (P, mode)"""
    if (P, mode) not in _REF:
        c = fc.random_case(P)
        _REF[P, mode] = ref.pursuit_features(fc.CFG, c["p"], c["e"], c["target"], c["time_step"], c["pp_adj"], c["pe_adj"], mode)
    return _REF[P, mode]


@pytest.mark.parametrize("P", fc.P_CASES)
def test_kernel_matches_the_specification(P):
    """N = 5 (a partial last wave), every PT instance, all three modes; rtol = atol = 1e-6 (test_policy_features_match_numpy's figures),
    the k column, the rows of inactive pursuers and every column the law leaves at zero exact"""
    c = fc.random_case(P)
    gap, rows = ref.nearest_gap(c["p"])          # on the reference alone: no near tie could swap the nearest two, in any row
    assert rows == int((c["p"][:, 6] != 0).sum()) and gap >= fc.MIN_GAP, (gap, rows)
    env = _env(c)
    dead, gone = c["p"][:, 6] == 0, c["e"][:, 6] == 0
    assert dead.any() and gone.sum() == 1
    for mode in MODES:
        got = [t.cpu().numpy() for t in _launch(env, mode)]
        for g, w in zip(got, _want(P, mode)):
            print(f"P {P} {mode}: max abs err {np.abs(g.astype(np.float64) - w).max():.3g}")
            np.testing.assert_allclose(g, w, rtol=1e-6, atol=1e-6)
            assert np.array_equal(g[..., ref.K_COL], w[..., ref.K_COL])
            assert np.all(g[dead] == 0) and np.all(g[gone][..., ref.EVADER_COLS] == 0)
            assert np.all(g[w == 0] == 0)
    k = {m: _want(P, m)[0][..., ref.K_COL] for m in MODES}
    assert np.all(k["sensed"] <= k["team"]) and np.all(k["team"] <= k["global"])
    if P >= 3:   # the modes differ on these cases: the comparison above is not one mode three times
        assert (k["sensed"] != k["team"]).any() and (k["team"] != k["global"]).any()


@pytest.mark.parametrize("P", [9, 33])
def test_long_chains_relay_to_every_lane(P):
    """a line of P pursuers that hear their two neighbours only, the last one alone sensing: the case a closure with too few rounds
    gets wrong (P - 1 hops: 8 at PT 16, 32 at PT 64).  With the middle pursuer inactive the relay stops there."""
    env = _env(fc.chain_case(P))
    assert env.obs["pe_adj"][0, :, 0].tolist() == [0.0] * (P - 1) + [1.0]
    assert _launch(env, "sensed")[0][0, :, ref.K_COL].tolist() == [0.0] * (P - 1) + [1.0]
    assert _launch(env, "team")[0][0, :, ref.K_COL].tolist() == [1.0] * P
    mid = P // 2
    env = _env(fc.chain_case(P, dead=mid))
    fa, fcr = _launch(env, "team")
    assert fa[0, :, ref.K_COL].tolist() == [0.0] * (mid + 1) + [1.0] * (P - mid - 1)
    assert fcr[0, :, ref.K_COL].tolist() == [1.0] * mid + [0.0] + [1.0] * (P - mid - 1)
    # the reversed chain: the first pursuer senses, the sighting travels towards higher lanes
    c = fc.chain_case(P)
    c["e"][0, 0] = -1.0
    c["pe_adj"] = np.array([[1.0] + [0.0] * (P - 1)], np.float32)
    assert _launch(_env(c), "team")[0][0, :, ref.K_COL].tolist() == [1.0] * P


@pytest.mark.parametrize("P", [8, 33])
def test_launch_is_deterministic_and_writes_only_its_outputs(P):
    c = fc.random_case(P)
    env = _env(c)
    keep = {k: t.clone() for k, t in (("p", env.p), ("e", env.e), ("target", env.target), ("t", env.t_dev), ("pp", env.obs["pp_adj"]),
                                      ("pe", env.obs["pe_adj"]), ("ps", env.obs["p_state"]), ("es", env.obs["e_state"]))}
    for mode in MODES:
        a1, c1 = _launch(env, mode, 7.0)
        a2, c2 = _launch(env, mode, -3.0)
        assert torch.equal(a1, a2) and torch.equal(c1, c2)            # identical bytes, whatever the outputs held: fully overwritten
        assert not (a1 == 7.0).any() and not (c1 == 7.0).any()
    for k, t in (("p", env.p), ("e", env.e), ("target", env.target), ("t", env.t_dev), ("pp", env.obs["pp_adj"]), ("pe", env.obs["pe_adj"]),
                 ("ps", env.obs["p_state"]), ("es", env.obs["e_state"])):
        assert torch.equal(t, keep[k]), k


def test_method_checks_its_arguments():
    env = _env(fc.random_case(3))
    fa, fcr = torch.zeros(fc.N, 3, 32, device="cuda"), torch.zeros(fc.N, 3, 32, device="cuda")
    with pytest.raises(ValueError, match="evader_obs"):
        env.pursuit_features(fa, fcr, "nearest")
    with pytest.raises(AssertionError):
        env.pursuit_features(torch.zeros(fc.N, 3, 16, device="cuda"), fcr)
    with pytest.raises(AssertionError):
        env.pursuit_features(fa.double(), fcr)
    assert env.pursuit_features(fa, fcr)[0] is fa                      # the default mode is "sensed"
    assert torch.equal(fa, _launch(env, "sensed")[0])


# ---- agent and trainer -----------------------------------------------------------------------------------------------------------------
N_ENVS, T, P_NUM = 16, 20, 3
PURSUIT = {"algo.e3d_features": "pursuit", "algo.e3d_evader_obs": "team"}


def _cfg(**ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config("cfg5", **{"runtime.num_envs": N_ENVS, "env.max_steps": T, "env.num_defender": P_NUM, "runtime.e3d_evader": "rule", **ov})


def _agent(cfg):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO, make_env
    env = make_env(cfg, N_ENVS)
    torch.manual_seed(0)
    return E3dMAPPO(cfg, N_ENVS, max(1, round(N_ENVS / 10))), env


def _trainer(cfg, **kw):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dTrainer
    return E3dTrainer(cfg, num_eval_envs=4, **kw)


def _weights(tr):
    return {f"{n}.{k}": v.clone() for n, m in (("actor", tr.agent.actor), ("critic", tr.agent.critic)) for k, v in m.state_dict().items()}


def test_agent_buffer_is_32_wide_and_the_update_forward_reproduces_the_rollout():
    agent, env = _agent(_cfg(**PURSUIT))
    assert agent.feat_dim == 32 and agent.actor.shared_net.fc1.weight.shape == (128, 32)
    _, buf, steps, _ = agent.explore_env(env)
    assert tuple(buf["feat_a"].shape) == tuple(buf["feat_c"].shape) == (N_ENVS, T, P_NUM, 32)
    live = buf["active"] == 1
    assert live.sum() > 0 and torch.isfinite(buf["feat_a"]).all() and torch.isfinite(buf["feat_c"]).all()
    # the buffer holds the kernel's rows: the critic always knows an active evader, the clock runs, dead rows are zero
    assert torch.all(buf["feat_c"][:, 0, :, ref.K_COL] == 1) and torch.all(buf["feat_a"][:, 5, :, 31][live[:, 5]] == 5 / T)
    assert (buf["feat_a"][..., 3:6].norm(dim=-1)[live] - 1).abs().max().item() <= 1e-5      # u_i is a unit vector on every live row
    with torch.enable_grad():
        mu, values = agent.sequence_forward(buf["feat_a"], buf["feat_c"], N_ENVS, T)
    lp = torch.distributions.Normal(mu.detach(), torch.exp(agent.actor.log_std.detach())).log_prob(buf["a_n"]).sum(-1)
    assert (lp - buf["a_logprob_n"])[live].abs().max().item() <= 1e-4
    assert (values.detach() - buf["v_n"][:, :T])[live].abs().max().item() <= 1e-4


@pytest.mark.timeout(300)
def test_trainer_determinism_checkpoint_and_resume(tmp_path):
    cfg = _cfg(**PURSUIT, **{"algo.epochs": 2})
    path = str(tmp_path / "resume.pt")
    runs = []
    for save in (True, False):
        tr = _trainer(cfg, eval_every=1)
        logs = []
        for it in range(2):
            logs.append(tr.iterate()[1])
            if save and it == 0:
                tr.save_resume(path)
        runs.append((tr, logs))
    (a, logs_a), (b, logs_b) = runs
    for log in logs_a:
        assert all(np.isfinite(log[k]) for k in ("critic_loss", "actor_loss", "mean_return", "eval_return"))
    assert logs_a == logs_b                                                          # two runs give identical logs
    bundle = torch.load(path, weights_only=False)
    assert bundle["policy"] == dict(e3d_features="pursuit", e3d_evader_obs="team")
    c = _trainer(cfg, eval_every=1)
    c.load_resume(path)
    assert c.iterate()[1] == logs_a[1]                                               # iteration 2 bit for bit
    wa, wc = _weights(a), _weights(c)
    assert list(wa) == list(wc) and all(torch.equal(wa[k], wc[k]) for k in wa)
    # files of one feature set are refused by an agent of another, naming the key
    basic = _trainer(_cfg(**{"algo.epochs": 2}))
    with pytest.raises(ValueError, match="algo.e3d_features"):
        basic.load_resume(path)
    a.agent.save_model(str(tmp_path / "ckpt"))
    sd = torch.load(str(tmp_path / "ckpt" / "e3d_state_dicts.pt"), weights_only=False)
    assert sd["policy"] == dict(e3d_features="pursuit", e3d_evader_obs="team")
    with pytest.raises(ValueError, match="algo.e3d_features"):
        basic.agent.load_model(str(tmp_path / "ckpt"))
    other = _trainer(_cfg(**{**PURSUIT, "algo.e3d_evader_obs": "global", "algo.epochs": 2}))
    with pytest.raises(ValueError, match="algo.e3d_evader_obs"):
        other.agent.load_model(str(tmp_path / "ckpt"))
    c.agent.load_model(str(tmp_path / "ckpt"))                                       # ... and accepted by its own
    basic.agent.save_model(str(tmp_path / "basic"))
    with pytest.raises(ValueError, match="algo.e3d_features"):
        c.agent.load_model(str(tmp_path / "basic"))                                  # a file without the entry means basic


def test_obs_norm_with_pursuit_raises():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    with pytest.raises(ValueError, match="algo.use_obs_norm.*algo.e3d_features"):
        E3dMAPPO(_cfg(**PURSUIT, **{"algo.use_obs_norm": True}), N_ENVS, 2)


def test_keys_absent_is_the_basic_run_without_a_policy_entry(tmp_path, monkeypatch):
    """without the keys the agent takes the code path it had before them: 16 columns, ParticleEnv.policy_features, no pursuit launch,
    the log lines of a run that names the defaults, and files without a "policy" entry"""
    from distributed_multi_agent_reinforcement_learning_amd.e3d_env import ParticleEnv
    calls = {"basic": 0, "pursuit": 0}
    basic, pursuit = ParticleEnv.policy_features, ParticleEnv.pursuit_features
    monkeypatch.setattr(ParticleEnv, "policy_features", lambda self, *a, **k: (calls.__setitem__("basic", calls["basic"] + 1), basic(self, *a, **k))[1])
    monkeypatch.setattr(ParticleEnv, "pursuit_features", lambda self, *a, **k: (calls.__setitem__("pursuit", calls["pursuit"] + 1), pursuit(self, *a, **k))[1])
    runs = []
    for ov in ({}, {"algo.e3d_features": "basic", "algo.e3d_evader_obs": "sensed"}):
        tr = _trainer(_cfg(**ov, **{"algo.epochs": 2}))
        log = tr.iterate()[1]
        p = str(tmp_path / f"resume{len(runs)}.pt")
        tr.save_resume(p)
        tr.agent.save_model(str(tmp_path / f"ckpt{len(runs)}"))
        runs.append((tr, log, torch.load(p, weights_only=False), torch.load(str(tmp_path / f"ckpt{len(runs)}" / "e3d_state_dicts.pt"), weights_only=False)))
    (a, log_a, bundle_a, sd_a), (b, log_b, bundle_b, sd_b) = runs
    assert calls["pursuit"] == 0 and calls["basic"] == 2 * (T + 1)
    assert log_a == log_b and set(bundle_a) == set(bundle_b) and "policy" not in bundle_a and set(sd_a) == set(sd_b) and "policy" not in sd_a
    assert a.agent.feat_dim == 16 and a.agent.policy_meta() is None and tuple(a.agent.buffer["feat_a"].shape) == (N_ENVS, T, P_NUM, 16)
    assert a.agent.actor.shared_net.fc1.weight.shape == (128, 16)
    wa, wb = _weights(a), _weights(b)
    assert all(torch.equal(wa[k], wb[k]) for k in wa)


@pytest.mark.timeout(300)
def test_imitation_loss_falls_on_a_fixed_buffer():
    """the setting of test_imitation_gpu.test_imitation_loss_falls_on_a_fixed_buffer (16 environments, 20 ticks, 30 updates) on the
    pursuit features with the teacher's own knowledge of the evader (global); the ratio is a figure of DESIGN.md section 7g"""
    agent, env = _agent(_cfg(**{**PURSUIT, "algo.e3d_evader_obs": "global", "algo.bc_iterations": 3, "algo.epochs": 2}))
    _, buf, steps, _ = agent.explore_expert(env, 1.0)
    assert tuple(buf["feat_a"].shape) == (N_ENVS, T, P_NUM, 32) and tuple(buf["a_star"].shape) == (N_ENVS, T, P_NUM, 3)
    losses = []
    for _ in range(30):
        with torch.enable_grad():
            _, bc_loss = agent.train(buf, steps, imitation=True)
        agent.ac_optimizer.step()
        losses.append(bc_loss)
    print(f"pursuit/global: bc_loss {losses[0]:.6g} -> {losses[-1]:.6g} (ratio {losses[-1] / losses[0]:.4f}), metric {agent.bc_metric(*agent.last_bc):.4g}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
