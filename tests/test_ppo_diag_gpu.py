"""GPU checks of algo.update_diagnostics / algo.target_kl (csrc/ppo_diag.hpp, the DIAG instances of the four PPO loss kernels) against
tests/ppo_diag_ref.py: the eight sums of every kernel, accumulation and determinism, byte identity of losses and gradients with the
plain calls, the three trainers with the option on and off, the early stop, the one-rank RCCL path and resume."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ppo_diag_ref as ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CONFIG = {"e3d": "cfg5", "n2n": "cfg4_n2n"}
EPS, COEF = 0.2, 0.01
# rows = d0 d1 d2: 1, 255, 257 and 65 536 + 77 (past the PPO_BLOCKS x 256 cap: the grid-stride loop and all 256 partials)
SHAPES = [(1, 1, 1), (3, 17, 5), (1, 257, 1), (3, 21871, 1)]
SUM_RTOL = 1e-12        # f64 summation order only


def _ops():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _time_major(x):
    """(d0, d1, d2, ...) numpy -> a device tensor of that shape stored time-major, as the heads' outputs are (a permuted view)"""
    return _dev(np.swapaxes(x, 0, 1)).transpose(0, 1)


def _lp_tol(kind, x):
    """the tolerance the existing tests allow on the kernel's fp32 log-probability / entropy against f64: rtol 1e-5 with atol 1e-5
    (tests/test_gauss_gpu.py, tests/test_ops_gpu.py) or atol 2e-5 (tests/test_gauss_sd_gpu.py, the _ex kernels)"""
    return 1e-5 * np.abs(x) + (2e-5 if kind == "gauss_ex" else 1e-5)


def _case(kind, shape, A, seed, all_inactive=False, state=False, tanh=False):
    """numpy inputs of one loss call and the f64 (lp_now, entropy) of its policy"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    c = dict(kind=kind, shape=shape, A=A, state=state, tanh=tanh)
    c["adv"], c["v_old"], c["v_tgt"] = f(*shape), f(*shape), (f(*shape) * 2 + 1).astype(np.float32)
    c["v_now"] = (c["v_tgt"] + f(*shape) * 0.7).astype(np.float32)
    c["active"] = np.zeros(shape, np.float32) if all_inactive else (rng.random(shape) > 1 / 3).astype(np.float32)
    if not all_inactive:
        c["active"].reshape(-1)[0] = 1.0                       # (the one-row case stays live)
    if kind == "plain":
        c["lp_now"], c["ent"] = (f(*shape) * 2 - 3).astype(np.float32), (f(*shape) * 0.3 + 2).astype(np.float32)
        lp64, ent64 = c["lp_now"].astype(np.float64), c["ent"].astype(np.float64)
    elif kind == "prob":
        logits = f(*shape, A) * 2
        e = np.exp(logits - logits.max(-1, keepdims=True))
        c["prob"] = (e / e.sum(-1, keepdims=True)).astype(np.float32) * np.float32(1.25)        # unnormalised: the kernel renormalises
        c["action"] = rng.integers(0, A, shape).astype(np.float32)
        lp64, ent64 = ref.categorical(c["prob"], c["action"])
    else:
        c["mu"], c["action"] = f(*shape, A), f(*shape, A) * 1.2
        c["lo"], c["hi"] = (-1.0, 0.5) if kind == "gauss_ex" else (-math.inf, math.inf)
        c["ls"] = (f(*shape, A) * 0.8 - 0.3).astype(np.float32) if state else (f(A) * 0.8 - 0.3).astype(np.float32)   # some outside the bounds
        lp64, ent64 = ref.gaussian(c["mu"], c["ls"], c["action"], c["lo"], c["hi"], tanh)
    lp_old = (lp64 + rng.standard_normal(shape) * 0.15).astype(np.float32)
    # no row's f64 ratio within 1e-4 relative of 1 - eps or 1 + eps, so fp32 and f64 agree on which side it is (sum 2 is exact)
    for _ in range(3):
        ratio = np.exp(lp64 - lp_old)
        near = (np.abs(ratio / (1 - EPS) - 1) < 1e-4) | (np.abs(ratio / (1 + EPS) - 1) < 1e-4)
        lp_old = np.where(near, lp_old - np.float32(0.01), lp_old).astype(np.float32)
    ratio = np.exp(lp64 - lp_old)
    assert not ((np.abs(ratio / (1 - EPS) - 1) < 1e-4) | (np.abs(ratio / (1 + EPS) - 1) < 1e-4)).any()   # checked before any launch
    c["lp_old"], c["lp64"], c["ent64"] = lp_old, lp64, ent64
    return c


def _call(c, value_clip, diag=None):
    """one loss call on fresh leaves -> (la, lc, gradients...) as device tensors"""
    ops, kind = _ops(), c["kind"]
    dense = {k: _dev(c[k]) for k in ("adv", "v_old", "v_tgt", "active", "lp_old")}
    v = _time_major(c["v_now"][..., None]).requires_grad_(True)
    v_old = dense["v_old"] if value_clip else None
    tail = (dense["lp_old"], dense["adv"], dense["active"], v_old, dense["v_tgt"], EPS, COEF, value_clip)
    kw = {} if diag is None else {"diag": diag}
    if kind == "plain":
        lp, ent = _dev(c["lp_now"]).requires_grad_(True), _dev(c["ent"]).requires_grad_(True)
        leaves = [lp, ent, v]
        la, lc = ops.ppo_loss(lp, ent, v[..., 0], *tail, **kw)
    elif kind == "prob":
        p = _time_major(c["prob"]).requires_grad_(True)
        leaves = [p, v]
        la, lc = ops.ppo_loss_prob(p, _dev(c["action"]), v[..., 0], *tail, **kw)
    else:
        mu = _time_major(c["mu"]).requires_grad_(True)
        ls = (_time_major(c["ls"]) if c["state"] else _dev(c["ls"])).requires_grad_(True)
        leaves = [mu, ls, v]
        if kind == "gauss":
            la, lc = ops.ppo_loss_gauss(mu, ls, _dev(c["action"]), v[..., 0], *tail, **kw)
        else:
            la, lc = ops.ppo_loss_gauss_ex(mu, ls, _dev(c["action"]), v[..., 0], *tail, log_std_min=c["lo"], log_std_max=c["hi"],
                                           squash="tanh" if c["tanh"] else "clip", **kw)
    (la + lc).backward()
    return [la.detach(), lc.detach()] + [x.grad for x in leaves]


def _check(c, value_clip):
    """the plain call, then the diag call twice into one tensor: bytes of losses and gradients, accumulation, the sums against the
    restatement"""
    ops, kind = _ops(), c["kind"]
    plain = _call(c, value_clip)
    diag = torch.zeros(8, dtype=torch.float64, device="cuda")
    with_diag = _call(c, value_clip, diag)
    once = diag.clone()
    again = _call(c, value_clip, diag)
    for a, b, d in zip(plain, with_diag, again):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), d.view(torch.int32))
    assert torch.equal(diag, 2 * once)                          # diag accumulates: s, then s + s
    fresh = torch.zeros(8, dtype=torch.float64, device="cuda")
    _call(c, value_clip, fresh)
    assert torch.equal(fresh.view(torch.int64), once.view(torch.int64))   # two runs, the same bits
    got = once.cpu().numpy()
    live = c["active"].reshape(-1) != 0
    if kind == "plain":      # lp_now and ent are inputs: every term is reproducible from the kernel's own fp32 lr and ratio
        lr, ratio = (x.cpu().numpy() for x in ops.ppo_ratio(_dev(c["lp_now"]), _dev(c["lp_old"])))
        assert np.array_equal(lr, c["lp_now"] - c["lp_old"])
        t = ref.row_terms(lr, ratio, c["ent"], c["v_now"], c["v_tgt"], c["active"], np.float32(EPS))
        bound = np.zeros(8)
    else:                    # the kernel forms lp_now and the entropy in fp32: the restatement has them in f64
        lr64 = (c["lp64"] - c["lp_old"]).reshape(-1)
        ratio64 = np.exp(lr64)
        assert not ((np.abs(ratio64 / (1 - EPS) - 1) < 1e-4) | (np.abs(ratio64 / (1 + EPS) - 1) < 1e-4)).any()   # sum 2's precondition
        t = ref.row_terms(lr64, ratio64, c["ent64"], c["v_now"], c["v_tgt"], c["active"], EPS)
        # a log-probability off by at most tol moves lr by tol: d k3 / d lr = expm1(lr) = ratio - 1 and d ratio / d lr = ratio, so a
        # row's k3 term moves by |ratio - 1| tol and its ratio by ratio tol; the entropy term moves by its own tol
        tol_lp, tol_ent = _lp_tol(kind, c["lp64"]).reshape(-1), _lp_tol(kind, c["ent64"]).reshape(-1)
        bound = np.zeros(8)
        bound[1] = (np.abs(ratio64 - 1) * tol_lp)[live].sum()
        bound[3] = tol_ent[live].sum()
        bound[7] = (ratio64 * tol_lp)[live].sum()
    want = ref.sums(t)
    err = np.abs(got - want)
    print(f"{kind} {c['shape']} A={c['A']} clip={value_clip}: c={got[0]:.0f} sums {got.tolist()} err {err.tolist()} bound {bound.tolist()}")
    assert got[0] == want[0] == live.sum() and got[2] == want[2]          # the integer sums are exact
    for k in (1, 3, 4, 5, 6, 7):
        assert err[k] <= bound[k] + SUM_RTOL * abs(want[k]), (k, got[k], want[k], err[k], bound[k])
    if live.any():
        assert all(math.isfinite(v) or name == "explained_variance" for name, v in ref.derive(got).items())
    return got


# ---- the four kernels against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value_clip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_ppo_loss_sums(shape, value_clip):
    _check(_case("plain", shape, 0, 11), value_clip)


@pytest.mark.parametrize("A", [1, 9, 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_ppo_loss_prob_sums(shape, A):
    _check(_case("prob", shape, A, 12 + A), value_clip=(A != 9))


@pytest.mark.parametrize("A", [1, 3, 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_ppo_loss_gauss_sums(shape, A):
    _check(_case("gauss", shape, A, 13 + A), value_clip=(A != 3))


@pytest.mark.parametrize("tanh", [False, True])
@pytest.mark.parametrize("A", [3, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_ppo_loss_gauss_ex_state_sums(shape, A, tanh):
    _check(_case("gauss_ex", shape, A, 14 + A, state=True, tanh=tanh), value_clip=(A == 3))


@pytest.mark.parametrize("tanh", [False, True])
def test_ppo_loss_gauss_ex_param_sums(tanh):
    _check(_case("gauss_ex", SHAPES[1], 16, 15, state=False, tanh=tanh), value_clip=True)


@pytest.mark.parametrize("kind,A,state", [("plain", 0, False), ("prob", 9, False), ("gauss", 3, False), ("gauss_ex", 3, True)])
def test_every_row_inactive_adds_nothing(kind, A, state):
    ops, c = _ops(), _case(kind, SHAPES[1], A, 16, all_inactive=True, state=state)
    diag = torch.full((8,), 0.0, dtype=torch.float64, device="cuda")
    _call(c, True, diag)
    assert torch.equal(diag, torch.zeros_like(diag))
    from distributed_multi_agent_reinforcement_learning_amd.update_diag import derive
    assert all(math.isnan(v) for v in derive(diag.tolist()).values())


def test_state_mode_diag_stops_at_the_heads_action_count():
    c = _case("gauss_ex", SHAPES[1], 9, 17, state=True)
    _call(c, True)                                              # the plain call takes it
    with pytest.raises(RuntimeError, match="bad argument"):
        _call(c, True, torch.zeros(8, dtype=torch.float64, device="cuda"))


# ---- trainers -------------------------------------------------------------------------------------------------------------------------------
KEYS = ("approx_kl", "clip_fraction", "entropy", "explained_variance", "ratio_mean", "grad_norm")


def _cfg(kind, **ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config(CONFIG[kind], **{"runtime.num_envs": 16, "env.max_steps": 24, **ov})


def _trainer(kind, cfg, **kw):
    if kind == "e3d":
        from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dTrainer as T
    else:
        from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nTrainer as T
    return T(cfg, num_eval_envs=8, **kw)


def _weights(agent):
    sd = {f"{n}.{k}": v.detach().clone() for n, m in (("actor", agent.actor), ("critic", agent.critic)) for k, v in m.state_dict().items()}
    for i, p in enumerate(agent.ac_parameters):
        for k, v in agent.ac_optimizer.state.get(p, {}).items():
            sd[f"adam.{i}.{k}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    return sd


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k      # (a loaded optimizer keeps its step counters where the bundle put them)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_trainer_diagnostics_leave_the_run_alone(kind):
    off = _trainer(kind, _cfg(kind, **{"algo.epochs": 2}))
    logs_off = [off.iterate()[1] for _ in range(2)]
    on = _trainer(kind, _cfg(kind, **{"algo.epochs": 2, "algo.update_diagnostics": True}))
    logs_on = [on.iterate()[1] for _ in range(2)]
    _same(_weights(off.agent), _weights(on.agent))              # byte for byte, Adam's state included
    assert off.agent.diag is None and off.agent.last_update_diag is None and off.last_epoch_diags == []
    for lo, ln in zip(logs_off, logs_on):
        assert set(ln) == set(lo) | set(KEYS) | {"epochs_run"} and all(lo[k] == ln[k] for k in lo)
        assert ln["epochs_run"] == 2 and all(math.isfinite(ln[k]) for k in KEYS), ln
        assert 0 <= ln["clip_fraction"] <= 1 and ln["approx_kl"] >= 0 and ln["grad_norm"] > 0
    d0 = on.last_epoch_diags[0]
    print(f"{kind}: epochs {on.last_epoch_diags}")
    # the update's forward reproduces the rollout (an existing test pins |logp - stored logp| <= 1e-4): k3 <= about lr^2 / 2 <= 5e-9
    assert len(on.last_epoch_diags) == 2 and d0["approx_kl"] < 1e-6 and abs(d0["ratio_mean"] - 1) < 1e-3 and d0["clip_fraction"] == 0


@pytest.mark.timeout(600)
def test_pursuit_trainer_diagnostics_loop_and_grouped_epoch():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.trainer import Trainer
    runs = {}
    for name, ov in (("off", {}), ("grouped", {"algo.update_diagnostics": True}), ("loop", {"algo.update_diagnostics": True, "runtime.update_group": 1})):
        tr = Trainer(baseline_config("cfg1", **{"runtime.num_envs": 16, **ov}))
        sums = []
        for _ in range(2):
            tr.iterate()
            sums.append(None if tr.agent.diag is None else list(tr.agent.diag.last_sums))
        runs[name] = (tr, sums, _weights(tr.agent))
    assert runs["grouped"][0].agent.last_update_group > 1 and runs["loop"][0].agent.last_update_group == 1
    _same(runs["off"][2], runs["grouped"][2])
    _same(runs["off"][2], runs["loop"][2])
    assert runs["grouped"][1] == runs["loop"][1]                # the same eight sums, bit for bit
    d = runs["grouped"][0].agent.last_update_diag
    print("pursuit:", d, runs["grouped"][1])
    assert set(d) == set(KEYS) and all(math.isfinite(v) for v in d.values()) and runs["grouped"][1][1][0] > 0
    assert runs["off"][0].agent.last_update_diag is None


# ---- early stop -------------------------------------------------------------------------------------------------------------------------------
STOP = {"algo.epochs": 4, "algo.lr": 3e-3, "runtime.seed": 3}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_target_kl_stops_the_epochs(kind):
    off = _trainer(kind, _cfg(kind, **STOP))
    off.iterate()
    far = _trainer(kind, _cfg(kind, **STOP, **{"algo.target_kl": 1e30}))
    _, log = far.iterate()
    kls = [d["approx_kl"] for d in far.last_epoch_diags]
    print(f"{kind}: approx_kl per epoch {kls}")
    assert len(kls) == 4 and log["epochs_run"] == 4
    _same(_weights(off.agent), _weights(far.agent))
    target = 0.5 * (kls[0] + max(kls))
    s = ref.stop_epoch(kls, target)
    assert s is not None and 1 <= s <= 3, (kls, target, s)
    cut = _trainer(kind, _cfg(kind, **STOP, **{"algo.target_kl": target}))
    _, log = cut.iterate()
    assert log["epochs_run"] == s and len(cut.last_epoch_diags) == s + 1 and log["approx_kl"] == kls[s] > target
    assert [d["approx_kl"] for d in cut.last_epoch_diags] == kls[:s + 1]
    short = _trainer(kind, _cfg(kind, **{**STOP, "algo.epochs": s}))
    short.iterate()
    # the discarded epoch left nothing behind in the weights and in Adam's state, byte for byte; its forward pass did advance the
    # spectral-norm power-iteration vectors (buffers that move with every forward, not weights), which stand like the value normaliser's step
    wa, wb = _weights(cut.agent), _weights(short.agent)
    assert set(wa) == set(wb)
    moved = {k for k in wa if not torch.equal(wa[k], wb[k])}
    assert all(k.endswith(("weight_u", "weight_v")) for k in moved), moved
    names = [f"{n}.{k}" for n, m in (("actor", cut.agent.actor), ("critic", cut.agent.critic)) for k, _ in m.named_parameters()]
    assert names and not (set(names) & moved) and not any(k.startswith("adam.") for k in moved)


RCCL_RUN = r"""
import json, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dTrainer
cfg = baseline_config("cfg5", **{"runtime.num_envs": 16, "env.max_steps": 24, "algo.epochs": 2, "algo.target_kl": 1e30})
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
print(json.dumps(dict(diag=[[float(v).hex() for v in l.values()] for l in logs], sums=[float(v).hex() for v in tr.agent.diag.last_sums],
                      f64_calls=[c for c in calls if c[0] == "torch.float64"], calls=len(calls))))
if dist.is_initialized():
    dist.destroy_process_group()
"""


@pytest.mark.timeout(900)
def test_one_rank_rccl_gives_the_values_of_the_no_collective_path():
    """with a process group of one rank (RCCL) every train() all-reduces the eight sums, 64 bytes of f64 on the device, once; the sum
    over one rank changes nothing, so the log is that of the run without a group, which makes no collective at all"""
    out = {}
    for mode in ("none", "nccl"):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DMARL_DIST_BACKEND"):
            env.pop(k, None)
        if mode == "nccl":
            env.update(DMARL_DIST_BACKEND="nccl", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29534")
        res = subprocess.run([sys.executable, "-c", RCCL_RUN, ROOT, mode], env=env, capture_output=True, text=True, timeout=420, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-3000:]
        out[mode] = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert out["nccl"]["diag"] == out["none"]["diag"] and out["nccl"]["sums"] == out["none"]["sums"]
    assert out["none"]["calls"] == 0
    assert out["nccl"]["f64_calls"] == [["torch.float64", 8, True]] * 4 and out["nccl"]["calls"] == 8    # per epoch: the sums and the gradients


# ---- resume -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_resume_with_target_kl_continues_bit_for_bit(tmp_path, kind):
    ov = {**STOP, "algo.target_kl": 0.01, "algo.save_cwd": str(tmp_path / "model")}
    a = _trainer(kind, _cfg(kind, **ov))
    a.iterate()
    path = str(tmp_path / "resume.pt")
    a.save_resume(path)
    assert set(torch.load(path, weights_only=False)) == {                  # nothing new in the bundle
        "actor", "critic", "optimizer", "total_steps", "iteration", "lr", "resetter", "n_episode", "sample_counter", "eval_resetter",
        "eval_n_episode", "eval_sample_counter", "recorder", "best_eval_return", "num_envs", "world", "rank"}
    _, log_a = a.iterate()
    b = _trainer(kind, _cfg(kind, **ov))
    b.load_resume(path)
    _, log_b = b.iterate()
    print(f"{kind}: iteration 2 {log_a}")
    assert json.dumps(log_a) == json.dumps(log_b) and json.dumps(a.last_epoch_diags) == json.dumps(b.last_epoch_diags)
    _same(_weights(a.agent), _weights(b.agent))
