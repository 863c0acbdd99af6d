"""GPU checks of algo.use_value_norm (csrc/value_norm.hpp; ops.gae_advnorm_vn / value_norm_update / value_norm_targets) against
tests/value_norm_ref.py: the identity state reproduces gae_advnorm byte for byte, the masked denormalisation, the deterministic f64
sums, the state update and the normalised targets, both trainers with the option on and off, resume, and the one-rank RCCL path."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import value_norm_ref as ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CONFIG = {"e3d": "cfg5", "n2n": "cfg4_n2n"}
U = 2.0 ** -53          # f64 unit roundoff
SHAPES = [(7, 13, 5), (64, 150, 8), (512, 200, 8), (1024, 100, 16),   # ..., cfg5 and cfg4_n2n per rank
          (65_537, 2, 1), (8_193, 3, 8)]   # past k_gae_scan_vn's 256 x 256 lanes: one sequence, and eight with P > 1, in the loop's second trip


def _ops():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops


def _cfg(kind, **ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config(CONFIG[kind], **ov)


def _trainer(kind, cfg, **kw):
    if kind == "e3d":
        from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dTrainer as T
    else:
        from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nTrainer as T
    return T(cfg, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _inputs(shape, seed):
    """a buffer as the rollouts leave it: environments that end early (every later row dead, no bootstrap), pursuers that die on the
    way or are dead from the start, episodes cut by the time limit whose bootstrap is kept, and some whose bootstrap is masked although
    the last row is live; r, v are zero wherever their mask is"""
    N, T, P = shape
    rng = np.random.default_rng(seed)
    length = np.where(rng.random(N) < 0.5, T, rng.integers(1, T + 1, N))
    death = np.where(rng.random((N, P)) < 0.6, T, rng.integers(0, T + 1, (N, P)))
    keep = rng.random((N, 1)) < 0.7
    length[:3], death[:2], death[2, 0], keep[:2, 0] = (T, T, max(1, T // 2)), T, 0, (True, False)   # every kind of row, whatever the draw
    t = np.arange(T)[None, :, None]
    active = ((t < length[:, None, None]) & (t < death[:, None, :])).astype(np.float32)
    vmask = (active[:, T - 1] * keep).astype(np.float32)
    v = (rng.standard_normal((N, T + 1, P)) * 2).astype(np.float32) * ref.value_masks(active, vmask)
    r = rng.standard_normal((N, T, P)).astype(np.float32) * active
    assert (active == 0).any() and (vmask == 0).any() and (vmask != 0).any() and ((vmask == 0) & (active[:, T - 1] != 0)).any()
    return r, v, active, vmask


def _dev(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def _state(mean, var, beta=0.9):
    """a state with the given statistics after one update (numpy), and its device copy"""
    st = ref.update(ref.new_state(), np.array([mean * 8.0, (var + mean * mean) * 8.0, 8.0]), beta)
    return st, torch.from_numpy(st.copy()).cuda()


# ---- gae_advnorm_vn -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape", SHAPES)
def test_identity_state_gives_gae_advnorm_byte_for_byte(shape):
    ops = _ops()
    r, v, active, vmask = _dev(*_inputs(shape, 1))
    st = ops.value_norm_state("cuda")
    for norm in (True, False):
        adv0, vt0 = ops.gae_advnorm(r, v, active, 0.99, 0.95, norm)
        adv1, vt1, sums = ops.gae_advnorm_vn(r, v, active, vmask, st, 0.99, 0.95, norm)
        assert np.array_equal(_bits(adv1.cpu().numpy()), _bits(adv0.cpu().numpy())), norm
        assert np.array_equal(_bits(vt1.cpu().numpy()), _bits(vt0.cpu().numpy())), norm
    assert not st.any() and float(sums[2]) == float(active.sum())


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mean,var", [(5.0, 9.0), (-2.0, 1.5)])
def test_denormalised_gae_matches_the_f64_reference(shape, mean, var):
    """tolerances: test_ops_gpu.test_gae_advnorm's (v_target and the raw advantage rtol = atol = 1e-5, the normalised advantage
    1e-4) on values of std 2; the absolute part is scaled to the denormalised values' rms here (fp32 rounding is relative)"""
    ops = _ops()
    r, v, active, vmask = _inputs(shape, 2)
    st, st_d = _state(mean, var)
    m, sd = ref.stats(st)
    assert m == pytest.approx(mean) and sd == pytest.approx(math.sqrt(var))
    d = _dev(r, v, active, vmask)
    masks = ref.value_masks(active, vmask)
    vd = ref.denormalise(st, v, masks)
    scale = max(1.0, float(np.sqrt((vd[masks != 0] ** 2).mean())) / 2.0)
    for norm in (False, True):
        adv_ref, vt_ref = ref.gae(st, r, v, active, vmask, 0.99, 0.95, norm)
        adv, vt, _ = ops.gae_advnorm_vn(*d, st_d, 0.99, 0.95, norm)
        adv, vt = adv.cpu().numpy().astype(np.float64), vt.cpu().numpy().astype(np.float64)
        e_vt, e_adv = np.abs(vt - vt_ref).max(), np.abs(adv - adv_ref).max()
        print(f"{shape} mean {mean} norm {norm}: max |v_target err| {e_vt:.3e}, max |adv err| {e_adv:.3e}, scale {scale:.2f}")
        assert np.allclose(vt, vt_ref, rtol=1e-5, atol=1e-5 * scale)
        if norm:
            assert np.allclose(adv, adv_ref, rtol=1e-4, atol=1e-4)
        else:
            assert np.allclose(adv, adv_ref, rtol=1e-5, atol=1e-5 * scale)
            # every dead row and every masked next-value counts as exactly 0 ...
            dead = active == 0
            assert np.all(adv[dead] == 0) and np.all(vt[dead] == 0)
            # ... where the unmasked 0 std + mean = mean would show: the last live step of a row whose next value is masked
            nxt = masks[:, 1:]
            edge = (active != 0) & (nxt == 0)
            assert edge.sum() > 0
            delta = r.astype(np.float64) - vd[:, :-1]
            assert np.allclose(adv[edge], delta[edge], rtol=1e-5, atol=1e-5 * scale)
            assert np.abs(adv[edge] - (delta[edge] + 0.99 * mean)).min() > 100 * 1e-5 * scale   # the unmasked reading is far off


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape", SHAPES)
def test_sums_are_deterministic_and_within_the_f64_accumulation_bound(shape):
    """(S1, S2, c) over the kernel's own fp32 v_target on live rows: y and y^2 are exact in f64, so any summation order of n terms is
    within n 2^-53 sum |term| of the exact sum (math.fsum); c is exact"""
    ops = _ops()
    r, v, active, vmask = _inputs(shape, 3)
    d = _dev(r, v, active, vmask)
    _, st_d = _state(4.0, 6.0)
    _, vt, s_a = ops.gae_advnorm_vn(*d, st_d, 0.99, 0.95, True)
    _, vt_b, s_b = ops.gae_advnorm_vn(*d, st_d, 0.99, 0.95, True)
    assert np.array_equal(_bits(s_a.cpu().numpy()), _bits(s_b.cpu().numpy())) and torch.equal(vt, vt_b)
    y = vt.cpu().numpy().astype(np.float64)[active != 0]
    n = y.size
    S1, S2, c = s_a.tolist()
    assert c == n
    e1, e2 = abs(S1 - math.fsum(y)), abs(S2 - math.fsum(y * y))
    b1, b2 = n * U * math.fsum(np.abs(y)), n * U * math.fsum(y * y)
    print(f"{shape}: n {n}, |S1 err| {e1:.3e} (bound {b1:.3e}), |S2 err| {e2:.3e} (bound {b2:.3e})")
    assert e1 <= b1 and e2 <= b2


# ---- value_norm_update / value_norm_targets -------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("beta", [0.99999, 0.9])
def test_update_matches_the_reference(beta):
    """the state follows the stated expressions operation by operation: within 4 roundings (2^-53 each) of the two terms' magnitudes"""
    ops = _ops()
    rng = np.random.default_rng(5)
    st, st_d = ref.new_state(), ops.value_norm_state("cuda")
    for k in range(6):
        n = 0.0 if k == 3 else float(rng.integers(100, 5000))           # update 3 is empty: nothing may change
        s = np.array([rng.standard_normal() * 3 * n, (9 + rng.random()) * n, n])
        before, prev = st_d.clone(), st.copy()
        ref.update(st, s, beta)
        ops.value_norm_update(st_d, torch.from_numpy(s).cuda(), beta)
        got = st_d.cpu().numpy()
        if n == 0.0:
            assert torch.equal(st_d, before)
            continue
        terms = beta * np.abs(prev) + (1 - beta) * np.array([abs(s[0]) / n, s[1] / n, 1.0])     # the magnitudes that get rounded
        assert np.all(np.abs(got - st) <= 4 * U * terms), (k, got, st)
    assert st[2] > 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape", SHAPES)
def test_targets_match_the_reference(shape):
    ops = _ops()
    r, v, active, vmask = _inputs(shape, 6)
    st, st_d = _state(3.0, 20.0)
    y = (np.random.default_rng(7).standard_normal(shape) * 5 + 3).astype(np.float32)
    got = ops.value_norm_targets(*_dev(y, active), st_d).cpu().numpy()
    want = ref.targets(st, y, active)
    assert np.all(got[active == 0] == 0)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    print(f"{shape}: max target error {np.max(err / ulp):.3f} fp32 ulp")
    assert np.all(err <= ulp)
    ident = ops.value_norm_targets(*_dev(y, active), ops.value_norm_state("cuda")).cpu().numpy()
    assert np.array_equal(_bits(ident), _bits(np.where(active != 0, y, np.float32(0))))            # before the first update the targets are the raw ones


# ---- trainers -----------------------------------------------------------------------------------------------------------------------------
def _forward_values(kind, agent, buf):
    N, T = buf["r"].shape[:2]
    with torch.no_grad():
        if kind == "e3d":
            return agent.sequence_forward(buf["feat_a"], buf["feat_c"], N, T)[1]
        return agent.sequence_forward(buf, 0, N)[1]


def _run(kind, on, iterations, N=64, epochs=3, follow=False):
    """`iterations` of the trainer's iterate(), epoch by epoch -> per-iteration records.  follow: the reference restatement runs
    beside the device state, fed with this run's own live targets, and is compared after every update."""
    from distributed_multi_agent_reinforcement_learning_amd.trainer import allreduce_sum_
    ops = _ops()
    tr = _trainer(kind, _cfg(kind, **{"runtime.num_envs": N, "algo.epochs": epochs, "algo.use_value_norm": on}), num_eval_envs=8)
    agent, vn = tr.agent, tr.agent.value_norm
    assert (vn is not None) == on
    st_ref, bound = ref.new_state(), np.zeros(3)
    recs = []
    for it in range(iterations):
        mean_r, buf, steps, stats = agent.explore_env(tr.env)
        tr.total_steps += steps * tr.world
        rec = dict(buf={k: v.clone() for k, v in buf.items()}, losses=[], states=[])
        live = buf["active"] == 1
        if on:
            # GAE under the statistics in force, without touching the state (iteration 0: the identity)
            rec["adv"], rec["v_raw"], _ = ops.gae_advnorm_vn(buf["r"], buf["v_n"], buf["active"], buf["v_mask"], vn.state.clone(),
                                                             agent.gamma, agent.lamda, agent.use_adv_norm)
            assert torch.equal(buf["v_n"][:, -1] != 0, (buf["v_n"][:, -1] != 0) & (buf["v_mask"] != 0))
        else:
            rec["adv"], rec["v_raw"] = ops.gae_advnorm(buf["r"], buf["v_n"], buf["active"], agent.gamma, agent.lamda, agent.use_adv_norm)
        # the update's forward reproduces the values the rollout stored (normalised ones with the option on): the existing
        # rollout-vs-update tests' 1e-4
        err = (_forward_values(kind, agent, buf) - buf["v_n"][:, :-1])[live].abs().max().item()
        print(f"{kind} on={on} iteration {it}: live rows {int(live.sum())}, forward-vs-rollout value error {err:.2e}")
        assert err <= 1e-4
        for e in range(epochs):
            with torch.enable_grad():
                rec["losses"].append(agent.train(buf, tr.total_steps))
            allreduce_sum_(tr.bucket.flat)
            agent.ac_optimizer.step()
            if not on:
                continue
            rec["states"].append(vn.state.clone())
            if follow:
                v_raw, sums = vn.last
                y = v_raw.cpu().numpy().astype(np.float64)[live.cpu().numpy()]
                n = y.size
                assert float(sums[2]) == n and n > 0
                ref.update(st_ref, ref.sums(v_raw.cpu().numpy(), buf["active"].cpu().numpy()), vn.beta)
                # both sums are within n 2^-53 sum |term| of the exact one (device order, numpy order); the moving average keeps
                # beta of the earlier difference and adds (1 - beta) / c of the new one, plus a few roundings of the state itself
                w = 1.0 - vn.beta
                bound = vn.beta * bound + w * 2 * n * U * np.array([np.abs(y).mean(), (y * y).mean(), 0.0]) + 8 * U * np.abs(st_ref)
                got = vn.state.cpu().numpy()
                assert np.all(np.abs(got - st_ref) <= bound), (it, e, got, st_ref, bound)
                assert got[2] == st_ref[2]
        tr.iteration += 1
        recs.append(rec)
    weights = {k: v.clone() for m in (agent.actor, agent.critic) for k, v in m.state_dict().items()}
    return tr, recs, weights


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_trainer_with_value_norm(kind):
    ops = _ops()
    calls0 = dict(ops.value_norm_calls)
    tr_a, a, w_a = _run(kind, True, 3, follow=True)
    assert ops.value_norm_calls["value_norm_update"] - calls0["value_norm_update"] == 9      # once per train() call
    assert ops.value_norm_calls["value_norm_targets"] - calls0["value_norm_targets"] == 9
    tr_b, b, w_b = _run(kind, True, 3)
    for ra, rb in zip(a, b):                                   # two runs: the same bits everywhere
        assert ra["losses"] == rb["losses"]
        assert all(torch.equal(x, y) for x, y in zip(ra["states"], rb["states"]))
        assert all(torch.equal(ra["buf"][k], rb["buf"][k]) for k in ra["buf"]) and torch.equal(ra["adv"], rb["adv"])
    assert all(torch.equal(w_a[k], w_b[k]) for k in w_a)
    assert torch.equal(tr_a.agent.value_norm.state, tr_b.agent.value_norm.state)
    mean, sd = ref.stats(tr_a.agent.value_norm.state.cpu().numpy())
    print(f"{kind}: state {tr_a.agent.value_norm.state.tolist()}, mean {mean:.4f}, std {sd:.4f}")
    assert float(tr_a.agent.value_norm.state[2]) > 0 and "v_mask" in a[0]["buf"]
    # iteration 1 under the identity: the option-off run's buffer and advantages, bit for bit
    calls1 = dict(ops.value_norm_calls)
    tr_c, c, _ = _run(kind, False, 1)
    assert ops.value_norm_calls == calls1                      # option off: none of the three ops runs
    assert "v_mask" not in c[0]["buf"] and set(a[0]["buf"]) == set(c[0]["buf"]) | {"v_mask"}
    for k in c[0]["buf"]:
        assert torch.equal(a[0]["buf"][k], c[0]["buf"][k]), k
    assert np.array_equal(_bits(a[0]["adv"].cpu().numpy()), _bits(c[0]["adv"].cpu().numpy()))
    assert np.array_equal(_bits(a[0]["v_raw"].cpu().numpy()), _bits(c[0]["v_raw"].cpu().numpy()))
    # evaluation never touches the state
    before = tr_a.agent.value_norm.state.clone()
    res = tr_a.evaluate()
    assert np.isfinite(res["eval_return"]) and torch.equal(tr_a.agent.value_norm.state, before)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_option_off_keeps_todays_files(tmp_path, kind):
    ops = _ops()
    calls = dict(ops.value_norm_calls)
    tr = _trainer(kind, _cfg(kind, **{"runtime.num_envs": 16, "algo.epochs": 2, "algo.save_cwd": str(tmp_path / "model")}), num_eval_envs=8)
    tr.iterate()
    assert ops.value_norm_calls == calls and "v_mask" not in tr.agent.buffer and tr.agent.value_norm is None
    path = str(tmp_path / "resume.pt")
    tr.save_resume(path)
    assert set(torch.load(path, weights_only=False)) == {
        "actor", "critic", "optimizer", "total_steps", "iteration", "lr", "resetter", "n_episode", "sample_counter", "eval_resetter",
        "eval_n_episode", "eval_sample_counter", "recorder", "best_eval_return", "num_envs", "world", "rank"}
    cwd = str(tmp_path / "model")
    tr.agent.save_model(cwd)
    tr.agent.save_model(cwd, best=True)
    if kind == "e3d":
        assert sorted(os.listdir(cwd)) == ["e3d_state_dicts.pt", "e3d_state_dicts_best.pt"]
        assert set(torch.load(os.path.join(cwd, "e3d_state_dicts.pt"))) == {"actor", "critic"}
    else:
        assert sorted(os.listdir(cwd)) == ["n2n_actor.pth", "n2n_actor_best.pth", "n2n_critic.pth", "n2n_critic_best.pth"]
    tr.agent.load_model(cwd)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_resume_with_value_norm_continues_bit_for_bit(tmp_path, kind):
    ov = {"runtime.num_envs": 16, "algo.epochs": 2, "algo.save_cwd": str(tmp_path / "model"), "algo.use_value_norm": True,
          "algo.value_norm_beta": 0.999}
    a = _trainer(kind, _cfg(kind, **ov), num_eval_envs=8, eval_every=1)
    a.iterate(); a.iterate()
    path = str(tmp_path / "resume.pt")
    a.save_resume(path)
    entry = torch.load(path, weights_only=False)["value_norm"]
    assert entry["beta"] == 0.999 and torch.equal(entry["state"], a.agent.value_norm.state.cpu()) and float(entry["state"][2]) > 0
    logs_a = [a.iterate()[1] for _ in range(2)]
    b = _trainer(kind, _cfg(kind, **ov), num_eval_envs=8, eval_every=1)
    b.load_resume(path)
    logs_b = [b.iterate()[1] for _ in range(2)]
    assert torch.equal(a.agent.value_norm.state, b.agent.value_norm.state)
    for x, y in ((a.agent.actor, b.agent.actor), (a.agent.critic, b.agent.critic)):
        sx, sy = x.state_dict(), y.state_dict()
        assert all(torch.equal(sx[k], sy[k]) for k in sx)
    for la, lb in zip(logs_a, logs_b):
        for k in ("mean_return", "critic_loss", "actor_loss", "eval_return"):
            assert la[k] == lb[k], k
    assert all(torch.equal(a.agent.buffer[k], b.agent.buffer[k]) for k in a.agent.buffer)
    # bundles of the other setting or another beta are refused, both ways
    off = _trainer(kind, _cfg(kind, **{**ov, "algo.use_value_norm": False}), num_eval_envs=8)
    with pytest.raises(ValueError, match="algo.use_value_norm"):
        off.load_resume(path)
    other = _trainer(kind, _cfg(kind, **{**ov, "algo.value_norm_beta": 0.99}), num_eval_envs=8)
    with pytest.raises(ValueError, match="algo.value_norm_beta"):
        other.load_resume(path)
    off.iterate()
    path_off = str(tmp_path / "resume_off.pt")
    off.save_resume(path_off)
    with pytest.raises(ValueError, match="algo.use_value_norm"):
        b.load_resume(path_off)
    # model files: the state travels with the weights; a mismatch between file and option is refused, both ways
    cwd_on, cwd_off = str(tmp_path / "on"), str(tmp_path / "off")
    for best in (False, True):
        a.agent.save_model(cwd_on, best=best)
        off.agent.save_model(cwd_off, best=best)
    if kind == "e3d":
        sd = torch.load(os.path.join(cwd_on, "e3d_state_dicts_best.pt"))
        assert set(sd) == {"actor", "critic", "value_norm"} and torch.equal(sd["value_norm"]["state"], a.agent.value_norm.state.cpu())
    else:
        assert {"n2n_value_norm.pth", "n2n_value_norm_best.pth"} <= set(os.listdir(cwd_on))
        assert not any("value_norm" in f for f in os.listdir(cwd_off))
    other.agent.load_model(cwd_on, best=True)            # weights load under any beta, with their state
    assert torch.equal(other.agent.value_norm.state, a.agent.value_norm.state)
    for best in (False, True):
        with pytest.raises(ValueError, match="algo.use_value_norm"):
            off.agent.load_model(cwd_on, best=best)
        with pytest.raises(ValueError, match="algo.use_value_norm"):
            b.agent.load_model(cwd_off, best=best)


# ---- the one-rank RCCL path ---------------------------------------------------------------------------------------------------------------
RCCL_RUN = r"""
import json, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dTrainer
cfg = baseline_config("cfg5", **{"runtime.num_envs": 16, "algo.epochs": 2, "algo.use_value_norm": True, "algo.value_norm_beta": 0.999})
tr = E3dTrainer(cfg, num_eval_envs=8)
calls = []
if sys.argv[2] == "nccl":
    assert dist.is_initialized() and dist.get_backend() == "nccl" and dist.get_world_size() == 1
    real = dist.all_reduce
    def counted(t, *a, **k):
        calls.append((str(t.dtype), t.numel(), t.is_cuda))
        return real(t, *a, **k)
    dist.all_reduce = counted
else:
    assert not dist.is_initialized()
logs = [tr.iterate()[1] for _ in range(2)]
torch.cuda.synchronize()
print(json.dumps(dict(state=[x.hex() for x in tr.agent.value_norm.state.tolist()], losses=[(l["critic_loss"], l["actor_loss"]) for l in logs],
                      vn_calls=[c for c in calls if c[0] == "torch.float64"], calls=len(calls))))
if dist.is_initialized():
    dist.destroy_process_group()
"""


@pytest.mark.timeout(900)
def test_one_rank_rccl_gives_the_state_of_the_no_collective_path():
    """with a process group of one rank (RCCL) every update all-reduces (S1, S2, c), three f64 on the device, once; the sum over one
    rank changes nothing, so state and losses are those of the run without a group"""
    out = {}
    for mode in ("none", "nccl"):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DMARL_DIST_BACKEND"):
            env.pop(k, None)
        if mode == "nccl":
            env.update(DMARL_DIST_BACKEND="nccl", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
        res = subprocess.run([sys.executable, "-c", RCCL_RUN, ROOT, mode], env=env, capture_output=True, text=True, timeout=420, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-3000:]
        out[mode] = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert out["nccl"]["state"] == out["none"]["state"] and out["nccl"]["losses"] == out["none"]["losses"]
    assert float.fromhex(out["none"]["state"][2]) > 0
    assert out["none"]["calls"] == 0
    assert out["nccl"]["vn_calls"] == [["torch.float64", 3, True]] * 4 and out["nccl"]["calls"] == 8    # per epoch: the sums and the gradients
