"""GPU checks of the env_3d actor's team attention (algo.e3d_comm: attention): the kernels team_attention_fwd /
team_attention_bwd against tests/team_attention_ref.py in float64 on both sides of every P bucket, the exact self-only case, scores
around 1e3, group independence, determinism and what a launch writes; team_comm_mask against the numpy rule; and the E3dMAPPO agent /
E3dTrainer with the layer (the option off, the zero start, rollout-update agreement, messages along links only, gradients against an
f64 torch re-evaluation, determinism, checkpoints, resume, and the option next to minibatch_steps and the imitation terms)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gauss_ref
from tests import team_attention_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 1024   # floats on either side of every output


def _ops():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops


def _inputs(G, P, seed, q_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(G * P, 384, generator=g)
    qkv[:, :256] *= q_scale
    return qkv, torch.randn(G * P, 128, generator=g)


def _masks(G, P, seed):
    """name -> (G, P) int64 words: all self-only, all full, random with dead pursuers, the random ones with garbage at or above P"""
    rng = np.random.default_rng(seed)
    own = (np.uint64(1) << np.arange(P, dtype=np.uint64))[None].repeat(G, 0)
    full = np.full((G, P), np.uint64(0xFFFFFFFFFFFFFFFF) >> np.uint64(64 - P))
    rnd = ref.comm_words(rng.random((G, P, P)) < 0.7, rng.random((G, P)) < 0.75).view(np.uint64)
    out = {"self": own, "full": full, "random": rnd}
    if P < 64:
        out["garbage"] = rnd | (rng.integers(0, 2 ** 63, (G, P), dtype=np.uint64) << np.uint64(P))
    return {k: v.view(np.int64) for k, v in out.items()}


def _guarded(n, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _launch(qkv, words, H, d_out, fill=7.0):
    """both kernels through the C ABI on outputs with guard bands -> out, lse, d_qkv (the bands checked, the inputs too)"""
    ops = _ops()
    L = ops.load_library()
    G, P = words.shape
    qkv_d, words_d, d_out_d = qkv.cuda(), torch.from_numpy(words).cuda(), d_out.cuda()
    keep = [t.clone() for t in (qkv_d, words_d, d_out_d)]
    bufs = [_guarded(n, fill) for n in (G * P * 128, G * H * P, G * P * 384)]
    (_, out), (_, lse), (_, d_qkv) = bufs
    ptr, st = ops._ptr, ops._stream()
    assert L.team_attention_fwd(G, P, H, ptr(qkv_d), ptr(words_d), ptr(out), ptr(lse), st) == 0
    assert L.team_attention_bwd(G, P, H, ptr(qkv_d), ptr(words_d), ptr(lse), ptr(d_out_d), ptr(d_qkv), st) == 0
    torch.cuda.synchronize()
    for (whole, part), name in zip(bufs, ("out", "lse", "d_qkv")):
        assert (whole[:GUARD] == fill).all() and (whole[-GUARD:] == fill).all(), f"{name}: a guard band was written"
        assert not (part == fill).any(), f"{name}: an element was left unwritten"
    for a, b in zip(keep, (qkv_d, words_d, d_out_d)):
        assert torch.equal(a, b)
    return out.view(G * P, 128).clone(), lse.view(G, H, P).clone(), d_qkv.view(G * P, 384).clone()


def _check(tag, got, qkv, words, H, d_out):
    """err <= 4 x (the fp32 reference's own distance from f64, the larger of its CPU and GPU evaluation) + 2e-5 x scale, per output"""
    want = ref.attention_grads(qkv.double().cuda(), words, H, d_out.double().cuda())
    w32 = [ref.attention_grads(qkv.to(dev), words, H, d_out.to(dev)) for dev in ("cpu", "cuda")]
    worst = 0.0
    for k, name in enumerate(("out", "lse", "d_qkv")):
        r = want[k].cpu()
        noise = max((o[k].double().cpu() - r).abs().max().item() for o in w32)
        scale, err = r.abs().max().item(), (got[k].double().cpu() - r).abs().max().item()
        bound = 4 * noise + 2e-5 * scale
        print(f"{tag} {name}: err {err:.3g} noise {noise:.3g} scale {scale:.3g} ratio {err / bound:.3g}")
        assert torch.isfinite(got[k]).all() and err <= bound, (tag, name, err, noise, scale)
        worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("G", [1, 5, 67])
@pytest.mark.parametrize("P", [1, 2, 3, 8, 9, 16, 17, 33, 64])
def test_kernels_match_the_f64_reference(P, G):
    qkv, d_out = _inputs(G, P, 1000 * P + G)
    for H in ((1, 4, 8) if P == 8 else (4,)):
        for name, words in _masks(G, P, P + G).items():
            got = _launch(qkv, words, H, d_out)
            _check(f"P {P} G {G} H {H} {name}", got, qkv, words, H, d_out)
            if name == "self":     # a query that hears only itself: v exactly, and the gradient goes to v alone
                q = qkv.cuda()
                assert torch.equal(got[0], q[:, 256:]) and torch.equal(got[2][:, 256:], d_out.cuda()) and not got[2][:, :256].any()
            if name == "garbage":  # the bits at or above P are not read
                for a, b in zip(got, _launch(qkv, _masks(G, P, P + G)["random"], H, d_out)):
                    assert torch.equal(a, b)


@pytest.mark.parametrize("P, H", [(8, 4), (8, 1), (17, 4), (64, 8)])
def test_scores_around_1e3_stay_finite_and_accurate(P, H):
    G = 5
    qkv, d_out = _inputs(G, P, 5, q_scale=1000.0 ** 0.5 * 1.2)   # q . k / sqrt(D) has unit variance: s has a std of about 1.4e3
    s = (qkv[:, :128 // H] * qkv[:, 128:128 + 128 // H]).sum(1) / (128 // H) ** 0.5
    assert s.abs().max().item() > 1e3
    words = _masks(G, P, 9)["random"]
    _check(f"large scores P {P} H {H}", _launch(qkv, words, H, d_out), qkv, words, H, d_out)


@pytest.mark.parametrize("P", [3, 8, 9, 33, 64])
def test_a_group_does_not_depend_on_its_launch_and_launches_are_deterministic(P):
    G, H = 67, 4
    qkv, d_out = _inputs(G, P, P)
    words = _masks(G, P, P)["random"]
    a, b = _launch(qkv, words, H, d_out, 7.0), _launch(qkv, words, H, d_out, -3.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                             # the same bits, whatever the outputs held
    for g in (0, 1, 31, 66):
        alone = _launch(qkv[g * P:(g + 1) * P], words[g:g + 1], H, d_out[g * P:(g + 1) * P])
        assert torch.equal(alone[0], a[0][g * P:(g + 1) * P]) and torch.equal(alone[1], a[1][g:g + 1]) and torch.equal(alone[2], a[2][g * P:(g + 1) * P])


def test_autograd_function_and_its_argument_checks():
    ops = _ops()
    G, P, H = 5, 8, 4
    qkv, d_out = _inputs(G, P, 2)
    words = _masks(G, P, 2)["random"]
    want = _launch(qkv, words, H, d_out)
    x, w = qkv.cuda().requires_grad_(True), torch.from_numpy(words).cuda()
    out = ops.team_attention(x, w, H)
    out.backward(d_out.cuda())
    assert torch.equal(out, want[0]) and torch.equal(x.grad, want[2])
    with torch.no_grad():
        assert torch.equal(ops.team_attention(x, w, H), want[0])               # the rollout's call: the same kernel without lse
    with pytest.raises(ValueError, match="heads"):
        ops.team_attention(x, w, 3)
    with pytest.raises(AssertionError):
        ops.team_attention(x[:-1], w, H)
    with pytest.raises(AssertionError):
        ops.team_attention(x, w.int(), H)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.team_attention(qkv, w, H)
    assert ops.team_attention(x[:0], w[:0], H).shape == (0, 128)              # G = 0


# ---- comm_mask ---------------------------------------------------------------------------------------------------------------------------
def test_comm_mask_on_hand_made_adjacencies_through_a_strided_destination():
    ops = _ops()
    adj, live, want = ref.hand_made_masks()
    words = np.array([[sum(1 << j for j in js) for js in g] for g in want], np.int64)
    buf = torch.full((3, 4, 3), -1, dtype=torch.int64, device="cuda")         # buf["comm"][:, t]
    got = ops.comm_mask(torch.from_numpy(adj).cuda(), torch.from_numpy(live).cuda(), buf[:, 2])
    assert got.data_ptr() == buf[:, 2].data_ptr() and np.array_equal(buf[:, 2].cpu().numpy(), words)
    assert (buf[:, [0, 1, 3]] == -1).all()
    with pytest.raises(AssertionError):
        ops.comm_mask(torch.from_numpy(adj).cuda(), torch.from_numpy(live).cuda(), buf[:, 2].int())
    with pytest.raises(AssertionError):
        ops.comm_mask(torch.from_numpy(adj).cuda(), torch.from_numpy(live).cuda()[:, :2], buf[:, 2])


@pytest.mark.parametrize("P", [3, 8, 17])
def test_comm_mask_on_a_stepped_environment(P):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_env import ParticleEnv
    ops = _ops()
    N = 5
    env = ParticleEnv(num_envs=N, seeds=list(range(N)), evader="rule")
    env.initialize(P)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(P)
    seen = 0
    for t in range(6):
        env.evader_step()
        env.step((torch.rand((N, P, 3), generator=g, device="cuda") * 2 - 1).double())
        live = env.active_t.float()
        live[t % N, t % P] = 0                                                 # ... and a pursuer the trainer counts as done
        words = ops.comm_mask(env.obs["pp_adj"], live, torch.zeros((N, P), dtype=torch.int64, device="cuda"))
        want = ref.comm_words(env.obs["pp_adj"].cpu().numpy(), live.cpu().numpy())
        assert np.array_equal(words.cpu().numpy(), want)
        seen += int((ref.hears(want, P).sum(-1) > 1).sum())
    print(f"P {P}: {seen} rows heard a team-mate")


# ---- agent and trainer -----------------------------------------------------------------------------------------------------------------
N_ENVS, T, P_NUM = 16, 20, 3
PURSUIT = {"algo.e3d_features": "pursuit", "algo.e3d_evader_obs": "team"}
COMM = {**PURSUIT, "algo.e3d_comm": "attention"}


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


def _stir(agent, seed=0):
    """comm.out away from its zero start (and qkv's bias off zero), so that messages arrive"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for p in agent.actor.comm.out.parameters():
            p.copy_(torch.randn(p.shape, generator=g, device="cuda") * 0.05)


def test_off_is_off(tmp_path):
    """the key absent and `none` given: the same weights after two iterations, the same log keys, no comm field, the same files"""
    runs = []
    for ov in ({}, {"algo.e3d_comm": "none"}):
        tr = _trainer(_cfg(**PURSUIT, **ov, **{"algo.epochs": 2}))
        logs = [tr.iterate()[1] for _ in range(2)]
        tr.agent.save_model(str(tmp_path / f"ckpt{len(runs)}"))
        runs.append((tr, logs, torch.load(str(tmp_path / f"ckpt{len(runs)}" / "e3d_state_dicts.pt"), weights_only=False)))
    (a, logs_a, sd_a), (b, logs_b, sd_b) = runs
    assert logs_a == logs_b and [set(l) for l in logs_a] == [set(l) for l in logs_b]
    wa, wb = _weights(a), _weights(b)
    assert list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa) and not any("comm" in k for k in wa)
    for tr, _, sd in runs:
        assert "comm" not in tr.agent.buffer and not hasattr(tr.agent.actor, "comm") and tr.agent.e3d_comm == "none"
        assert sd["policy"] == tr.agent.policy_meta() == dict(e3d_features="pursuit", e3d_evader_obs="team") and set(sd) == set(sd_a)
    assert _agent(_cfg())[0].policy_meta() is None


def test_zero_start_is_the_first_rollout_of_none(monkeypatch):
    ops = _ops()
    seen = []
    mask = ops.comm_mask
    monkeypatch.setattr(ops, "comm_mask", lambda adj, live, out: (seen.append((adj.clone(), live.clone())), mask(adj, live, out))[1])
    bufs = {}
    for name, ov in (("none", PURSUIT), ("attention", COMM)):
        agent, env = _agent(_cfg(**ov))
        _, buf, _, _ = agent.explore_env(env)
        bufs[name] = {k: v.clone() for k, v in buf.items()}
    assert not agent.actor.comm.out.weight.any() and not agent.actor.comm.out.bias.any() and agent.actor.comm.qkv.weight.shape == (384, 128)
    assert [n for n, _ in agent.actor.named_parameters()][-4:] == ["comm.qkv.weight", "comm.qkv.bias", "comm.out.weight", "comm.out.bias"]
    assert all(a is b for a, b in zip(agent.ac_parameters[-4:], agent.actor.comm.parameters()))
    for k in ("feat_a", "a_n", "a_logprob_n", "v_n", "r", "active"):
        assert torch.equal(bufs["none"][k], bufs["attention"][k]), k
    assert "comm" not in bufs["none"] and bufs["attention"]["comm"].shape == (N_ENVS, T, P_NUM) and bufs["attention"]["comm"].dtype == torch.int64
    assert len(seen) == T
    heard = 0
    for t in (0, 1, T // 2, T - 1):
        want = ref.comm_words(seen[t][0].cpu().numpy(), seen[t][1].cpu().numpy())
        assert np.array_equal(bufs["attention"]["comm"][:, t].cpu().numpy(), want)
        heard += int((ref.hears(want, P_NUM).sum(-1) > 1).sum())
    print(f"rows that heard a team-mate at the four ticks: {heard}")


def test_update_forward_reproduces_the_rollout_and_messages_travel_along_links_only():
    agent, env = _agent(_cfg(**COMM))
    _stir(agent)
    _, buf, steps, _ = agent.explore_env(env)
    live = buf["active"] == 1
    with torch.no_grad():
        mu, values = agent.sequence_forward(buf["feat_a"], buf["feat_c"], N_ENVS, T, words=buf["comm"])
    lp = torch.distributions.Normal(mu, torch.exp(agent.actor.log_std.detach())).log_prob(buf["a_n"]).sum(-1)
    print(f"logp {(lp - buf['a_logprob_n'])[live].abs().max().item():.3g} values {(values - buf['v_n'][:, :T])[live].abs().max().item():.3g}")
    assert live.sum() > 0 and (lp - buf["a_logprob_n"])[live].abs().max().item() <= 1e-4
    assert (values - buf["v_n"][:, :T])[live].abs().max().item() <= 1e-4
    # hand-made words: pursuers 0 and 1 hear each other, 2 hears nobody; a perturbation of pursuer 0 at (n, t) reaches 1 and not 2
    words = torch.tensor([0b011, 0b011, 0b100], dtype=torch.int64, device="cuda").expand(N_ENVS, T, P_NUM).contiguous()
    n, t = 3, 7
    feat = buf["feat_a"].clone()
    feat[n, t, 0] += 0.5
    with torch.no_grad():
        mu0, _ = agent.sequence_forward(buf["feat_a"], buf["feat_c"], N_ENVS, T, words=words)
        mu1, _ = agent.sequence_forward(feat, buf["feat_c"], N_ENVS, T, words=words)
    diff = (mu1 - mu0).abs().amax(-1)                                          # (N, T, P)
    assert diff[n, t, 0] > 0 and diff[n, t, 1] > 0 and diff[n, t:, 1].max() > 0
    assert not diff[:, :, 2].any() and not diff[:n].any() and not diff[n + 1:].any() and not diff[n, :t].any()


def _oracle_grads(actor0, critic0, buf, adv, v_target, mb, eps, ent, clip, heads, dtype, device):
    """test_central_critic_gpu._oracle_grads with the reference layer between the actor's encoder and its GRU"""
    actor, critic = copy.deepcopy(actor0).to(device, dtype), copy.deepcopy(critic0).to(device, dtype)
    N, T_, P = buf["r"].shape
    cv = lambda x: None if x is None else x.to(device, dtype)

    def enc(m, x):
        h = F.relu(F.linear(x, m.shared_net.fc1.weight, m.shared_net.fc1.bias))
        return F.relu(F.linear(h, m.shared_net.fc2.weight, m.shared_net.fc2.bias))

    for n0 in range(0, N, mb):
        n1 = min(n0 + mb, N)
        B = n1 - n0
        outs = []
        for m, key in ((actor, "feat_a"), (critic, "feat_c")):
            x = enc(m, cv(buf[key][n0:n1]))                                  # (B, T, P, E)
            if m is actor:
                c = m.comm
                x = ref.layer(x.reshape(B * T_ * P, -1), buf["comm"][n0:n1].reshape(B * T_, P), heads, c.qkv.weight, c.qkv.bias, c.out.weight,
                              c.out.bias).reshape(B, T_, P, -1)
            x = x.permute(1, 0, 2, 3).reshape(T_, B * P, -1)
            y, _ = m.GRU(x)
            outs.append(y.reshape(T_, B, P, -1))
        mu = F.linear(outs[0], actor.Mean.weight, actor.Mean.bias).permute(1, 0, 2, 3)
        values = critic.Mean(outs[1]).permute(1, 0, 2, 3)[..., 0]
        la, lc = gauss_ref.torch_ppo_loss_gauss(mu, actor.log_std, cv(buf["a_n"][n0:n1]), values, cv(buf["a_logprob_n"][n0:n1]), cv(adv[n0:n1]),
                                                cv(buf["active"][n0:n1]), cv(buf["v_n"][n0:n1, :-1]) if clip else None, cv(v_target[n0:n1]),
                                                eps, ent, clip)
        (la + lc).backward()
    return {("actor." + k): p.grad.double().cpu() for k, p in actor.named_parameters()} | \
           {("critic." + k): p.grad.double().cpu() for k, p in critic.named_parameters()}


def test_agent_gradients_match_f64_torch():
    """the criterion of test_gauss_gpu.test_agent_gradients_match_f64_torch for every tensor, the four of the layer included:
    err <= 4 x the fp32 oracles' own distance from f64 + 2e-5 x scale"""
    ops = _ops()
    agent, env = _agent(_cfg(**COMM))
    _stir(agent)
    _, buf, steps, _ = agent.explore_env(env)
    buf = {k: v.clone() for k, v in buf.items()}
    with torch.no_grad():                    # move the policy away from the rollout's, so that ratios leave 1
        g = torch.Generator(device="cuda").manual_seed(0)
        agent.actor.log_std.add_(0.1)
        for p in list(agent.actor.Mean.parameters()) + list(agent.actor.shared_net.fc2.parameters()) + list(agent.actor.comm.out.parameters()):
            p.add_(torch.randn(p.shape, generator=g, device="cuda") * 0.05 * p.abs().mean())
    actor0, critic0 = copy.deepcopy(agent.actor), copy.deepcopy(agent.critic)   # (the critic's spectral-norm vectors as the update finds them)
    agent.use_grad_clip = False
    with torch.enable_grad():
        agent.train(buf, steps)
    adv, v_target = ops.gae_advnorm(buf["r"], buf["v_n"], buf["active"], agent.gamma, agent.lamda, agent.use_adv_norm)
    args = (buf, adv, v_target, agent.mini_batch_size, agent.epsilon, agent.entropy_coef, agent.use_value_clip, agent.e3d_comm_heads)
    want = _oracle_grads(actor0, critic0, *args, torch.float64, "cuda")
    o32 = [_oracle_grads(actor0, critic0, *args, torch.float32, "cuda"), _oracle_grads(actor0, critic0, *args, torch.float32, "cpu")]
    got = {("actor." + k): p.grad for k, p in agent.actor.named_parameters()} | {("critic." + k): p.grad for k, p in agent.critic.named_parameters()}
    assert set(got) == set(want) and "actor.comm.qkv.weight" in got
    for k, r in want.items():
        gk = got[k].double().cpu()
        noise = max((o[k] - r).abs().max().item() for o in o32)
        scale = r.abs().max().item()
        err = (gk - r).abs().max().item()
        print(f"{k}: err {err:.3g} fp32 oracles {noise:.3g} scale {scale:.3g}")
        assert err <= 4 * noise + 2e-5 * scale, (k, err, noise, scale)
    assert want["actor.comm.qkv.weight"].abs().max().item() > 0 and want["actor.comm.out.weight"].abs().max().item() > 0
    assert got["actor.comm.qkv.weight"].abs().max().item() > 0 and got["actor.comm.out.weight"].abs().max().item() > 0


@pytest.mark.timeout(300)
def test_trainer_determinism_checkpoint_evaluate_and_resume(tmp_path):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dTrainer
    from distributed_multi_agent_reinforcement_learning_amd.main import evaluate_saved
    cfg = _cfg(**COMM, **{"algo.epochs": 2})
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
    assert logs_a == logs_b                                                          # two runs give identical logs ...
    wa, wb = _weights(a), _weights(b)
    assert all(torch.equal(wa[k], wb[k]) for k in wa) and wa["actor.comm.out.weight"].any()   # ... and weights; the layer has left zero
    meta = dict(e3d_features="pursuit", e3d_evader_obs="team", e3d_comm="attention", e3d_comm_heads=4)
    bundle = torch.load(path, weights_only=False)
    assert bundle["policy"] == meta and "comm" not in bundle
    c = _trainer(cfg, eval_every=1)
    c.load_resume(path)
    assert c.iterate()[1] == logs_a[1]                                               # iteration 2 bit for bit
    wc = _weights(c)
    assert list(wa) == list(wc) and all(torch.equal(wa[k], wc[k]) for k in wa)
    a.agent.save_model(str(tmp_path / "comm"))
    assert torch.load(str(tmp_path / "comm" / "e3d_state_dicts.pt"), weights_only=False)["policy"] == meta
    res = evaluate_saved(E3dTrainer, cfg, str(tmp_path / "comm"), 4)                 # the --evaluate path
    assert np.isfinite(res["eval_return"])
    # a none agent refuses an attention file and vice versa, and another head count is another policy
    none = _trainer(_cfg(**PURSUIT, **{"algo.epochs": 2}))
    with pytest.raises(ValueError, match="algo.e3d_comm"):
        none.load_resume(path)
    with pytest.raises(ValueError, match="algo.e3d_comm"):
        none.agent.load_model(str(tmp_path / "comm"))
    none.agent.save_model(str(tmp_path / "none"))
    with pytest.raises(ValueError, match="algo.e3d_comm"):
        c.agent.load_model(str(tmp_path / "none"))                                   # a file without the entry means none
    with pytest.raises(ValueError, match="algo.e3d_comm_heads"):
        _trainer(_cfg(**COMM, **{"algo.e3d_comm_heads": 2})).agent.load_model(str(tmp_path / "comm"))


@pytest.mark.parametrize("ov", [{"algo.minibatch_steps": True}, {"algo.bc_iterations": 1, "algo.bc_coef": 0.5},
                                {"algo.e3d_critic": "central", "algo.gauss_std": "state", "algo.gauss_squash": "tanh", "algo.e3d_comm_heads": 8}])
def test_the_option_runs_next_to_the_others(ov):
    tr = _trainer(_cfg(**COMM, **ov, **{"algo.epochs": 2}))
    for _ in range(2):
        log = tr.iterate()[1]
        assert all(np.isfinite(v) for v in log.values() if isinstance(v, float)) and np.isfinite(log["critic_loss"]) and np.isfinite(log["actor_loss"]), log
    assert tr.agent.actor.comm.out.weight.any()
