"""GPU checks of teacher-regularised PPO (algo.bc_coef): the two fused loss launches against tests/kickstart_ref.py,
their critic part against the PPO launches bit for bit, their actor part against the PPO launch plus lambda times the imitation launch,
the three sums and the update diagnostics, the argument checks of the C entry points, and the agents / trainers of env_3d (cfg5) and
env_n2n (cfg4_n2n): the gradient of train(kick=), the labelled on-policy rollout, the log keys over the lambda schedule, determinism,
resume, the feature off, the KL early stop, and an imitation term that falls on a fixed buffer.

The inputs are the time-major cases of tests/test_imitation_gpu.py (a third of the rows inactive, holding finite garbage) with the PPO
inputs added: the sampled action, logp_old within a few percent of the row's own log-probability -- every ratio 1e-3 clear of the clip
edges 1 -+ EPS, as tests/test_gauss_sd_gpu.py keeps it -- and the advantage."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import kickstart_ref as ref
from tests import ppo_diag_ref as pd
from tests.test_imitation_gpu import (COMBOS, EPS, HI, LO, METRIC, N_ENVS, OFF_KEYS, SHAPES, T, _bt, _cat_case, _cfg, _close, _gauss_case,
                                      _loss_close, _mod, _r32, _trainer, _weights)

pytestmark = pytest.mark.gpu

ENT = 0.01
LAMBDAS = (0.0, 0.3, 2.5)
SUM_RTOL = 1e-12        # f64 summation order only (tests/test_ppo_diag_gpu.py)
BAD_ARG = 20001         # include/mappo_ops.h MO_ERR_BAD_ARG


def _ops():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops


def _f(x):
    return None if x is None else x.float().cuda()


def _add_ppo_inputs(c, lp, g):
    """logp_old (every ratio 1e-3 clear of the clip edges) and adv; the inactive rows hold finite garbage"""
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    shape = c["active"].shape
    dead = c["active"] == 0
    lp_old = lp + r(*shape) * 0.06
    lp_old[dead] = lp[dead] + r(int(dead.sum())) * 3.0
    lp_old = _r32(lp_old)
    for _ in range(3):
        ratio = torch.exp(lp - lp_old)
        near = ((ratio - (1 - EPS)).abs() < 2e-3) | ((ratio - (1 + EPS)).abs() < 2e-3)
        lp_old = _r32(torch.where(near & ~dead, lp_old - 0.01, lp_old))
    ratio = torch.exp(lp - lp_old)[~dead]
    assert not (((ratio - (1 - EPS)).abs() < 1e-3) | ((ratio - (1 + EPS)).abs() < 1e-3)).any()
    adv = r(*shape)
    adv[dead] = r(int(dead.sum())) * 30.0
    c["lp_old"], c["adv"], c["lp64"] = lp_old, _r32(adv), lp
    return c


def _kick_gauss_case(mb, T_, P, A, state, roll, seed, squash):
    c = _gauss_case(mb, T_, P, A, state, roll, seed)
    g = torch.Generator().manual_seed(seed + 77)
    mu, ls_raw = _bt(c["mu_tm"]), _bt(c["ls_tm"])
    ls = ls_raw.expand(mu.shape).clamp(LO, HI)
    c["action"] = _r32(mu + torch.exp(ls) * torch.randn(mu.shape, generator=g, dtype=torch.float64))    # around mu, the garbage rows' too
    lp, ent = pd.gaussian(mu.numpy(), ls_raw.numpy(), c["action"].numpy(), LO, HI, squash == "tanh")
    c["ent64"] = ent
    return _add_ppo_inputs(c, torch.from_numpy(lp), g)


def _kick_cat_case(mb, T_, P, A, seed):
    c = _cat_case(mb, T_, P, A, seed)
    g = torch.Generator().manual_seed(seed + 77)
    c["action"] = torch.randint(0, A, (mb, T_, P), generator=g).double()
    lp, ent = pd.categorical(_bt(c["prob_tm"]).numpy(), c["action"].numpy())
    c["ent64"] = ent
    return _add_ppo_inputs(c, torch.from_numpy(lp), g)


def _gauss_kw(fit_std, wrap0, squash, metric):
    return dict(log_std_min=LO, log_std_max=HI, squash=squash, fit_std=fit_std, wrap0=wrap0, metric=metric)


def _gpu_kick_gauss(c, coef, clip, kw, sums=None, diag=None):
    mu_tm, ls_tm, v_tm = (_f(c[k]).requires_grad_() for k in ("mu_tm", "ls_tm", "v_tm"))
    la, lc = _ops().ppo_bc_loss_gauss(_bt(mu_tm), _bt(ls_tm), _f(c["action"]), _f(c["target"]), v_tm.permute(1, 0, 2, 3)[..., 0], _f(c["lp_old"]),
                                      _f(c["adv"]), _f(c["active"]), _f(c["vo"]) if clip else None, _f(c["vt"]), EPS, ENT, coef, clip,
                                      sums=sums, diag=diag, **kw)
    (la + lc).backward()
    return la.detach(), lc.detach(), mu_tm.grad, ls_tm.grad, v_tm.grad


def _gpu_ppo_gauss(c, clip, squash):
    mu_tm, ls_tm, v_tm = (_f(c[k]).requires_grad_() for k in ("mu_tm", "ls_tm", "v_tm"))
    la, lc = _ops().ppo_loss_gauss_ex(_bt(mu_tm), _bt(ls_tm), _f(c["action"]), v_tm.permute(1, 0, 2, 3)[..., 0], _f(c["lp_old"]), _f(c["adv"]),
                                      _f(c["active"]), _f(c["vo"]) if clip else None, _f(c["vt"]), EPS, ENT, clip, log_std_min=LO, log_std_max=HI,
                                      squash=squash)
    (la + lc).backward()
    return la.detach(), lc.detach(), mu_tm.grad, ls_tm.grad, v_tm.grad


def _gpu_bc_gauss(c, clip, fit_std, wrap0, metric):
    mu_tm, ls_tm, v_tm = (_f(c[k]).requires_grad_() for k in ("mu_tm", "ls_tm", "v_tm"))
    la, lc = _ops().bc_loss_gauss(_bt(mu_tm), _bt(ls_tm), _f(c["target"]), v_tm.permute(1, 0, 2, 3)[..., 0], _f(c["active"]),
                                  _f(c["vo"]) if clip else None, _f(c["vt"]), EPS, clip, log_std_min=LO, log_std_max=HI, fit_std=fit_std,
                                  wrap0=wrap0, metric=metric)
    (la + lc).backward()
    return la.detach(), lc.detach(), mu_tm.grad, ls_tm.grad, v_tm.grad


def _ref_gauss(c, coef, clip, fit_std, wrap0, squash, metric):
    n = lambda k: c[k].numpy()
    return ref.ppo_bc_loss_gauss(_bt(c["mu_tm"]).numpy(), _bt(c["ls_tm"]).numpy(), n("action"), n("target"), c["v_tm"].permute(1, 0, 2, 3)[..., 0].numpy(),
                                 n("lp_old"), n("adv"), n("active"), n("vo"), n("vt"), EPS, ENT, coef, clip, LO, HI, squash, fit_std, wrap0, metric)


def _tm(x):
    """a batch-major f64 numpy gradient as the time-major tensor the leaves have"""
    x = torch.from_numpy(np.ascontiguousarray(x))
    return x.permute(1, 0, 2, 3) if x.dim() == 4 else x.permute(1, 0, 2)[..., None]


def _dead_rows_are_zero(c, grads):
    dead = c["active"] == 0
    for g in grads:
        if g.dim() == 4:                                           # (the log_std vector of param mode has no rows)
            rows = g.permute(1, 0, 2, 3)[dead.to(g.device)]
            assert not rows.any(), "an inactive row has a gradient"


def _squashes(A):
    return ("clip", "tanh", "direction") if A == 4 else ("clip", "tanh")


@pytest.mark.parametrize("state", [False, True], ids=["param", "state"])
@pytest.mark.parametrize("A", [1, 3, 4, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ppo_bc_loss_gauss(shape, A, state):
    """checks 1-3 and the repeatability of check 4 on one case per (fit_std, wrap0, value clip) combination; the squash mode and lambda
    go round with the combination (A = 4 takes the angle metric and sees direction)"""
    mb, T_, P = shape
    metric = "angle" if A == 4 else "mse"
    for k, (fit_std, wrap0, clip) in enumerate(COMBOS):
        squash, coef = _squashes(A)[k % len(_squashes(A))], LAMBDAS[(k + k // 3) % 3]
        c = _kick_gauss_case(mb, T_, P, A, state, k, 1000 * A + mb + k, squash)
        kw = _gauss_kw(fit_std, wrap0, squash, metric)
        sums = torch.tensor([3.0, 5.0, 7.0], dtype=torch.float64, device="cuda")     # the call adds to what is there
        la, lc, gmu, gls, gv = got = _gpu_kick_gauss(c, coef, clip, kw, sums)
        want = _ref_gauss(c, coef, clip, fit_std, wrap0, squash, metric)
        tag = f"gauss {shape} A={A} state={state} {squash} fit={fit_std} wrap={wrap0} clip={clip} coef={coef}"
        # 1. against the specification
        _loss_close(la, want["actor_loss"], tag + " actor")
        _loss_close(lc, want["critic_loss"], tag + " critic")
        assert gmu.stride() == c["mu_tm"].stride()
        _close(gmu, _tm(want["g_mu"]), tag + " g_mu")
        _close(gls, _tm(want["g_ls"]) if state else want["g_ls"], tag + " g_ls")
        _close(gv, _tm(want["g_v"]), tag + " g_v")
        _dead_rows_are_zero(c, (gmu, gls, gv) if state else (gmu, gv))
        # 4. the three sums: the call added once; rows exact
        s = sums.cpu().numpy() - [3.0, 5.0, 7.0]
        for j, name in ((0, "metric sum"), (2, "imitation sum")):
            print(f"{tag} {name}: {s[j]:.9g} against {want['sums'][j]:.9g}")
            assert abs(s[j] - want["sums"][j]) <= 1e-5 * abs(want["sums"][j]), (tag, name)
        assert s[1] == want["sums"][1]
        # 2. the critic part carries the bits of the PPO launch on the same inputs
        pa, pc, pmu, pls, pv = _gpu_ppo_gauss(c, clip, squash)
        assert torch.equal(lc, pc) and torch.equal(gv, pv), tag
        # 3. the actor part is the PPO launch plus lambda times the imitation launch
        ba, _, bmu, bls, _ = _gpu_bc_gauss(c, clip, fit_std, wrap0, metric)
        _loss_close(la, pa.double() + coef * ba.double(), tag + " actor against ppo + coef bc")
        _close(gmu, pmu.double().cpu() + coef * bmu.double().cpu(), tag + " g_mu against ppo + coef bc")
        _close(gls, pls.double().cpu() + coef * bls.double().cpu(), tag + " g_ls against ppo + coef bc")
        if coef == 0.0:
            assert torch.equal(gv, pv)
        # 4. two calls give the same bits, with and without sums
        for x, y in zip(got, _gpu_kick_gauss(c, coef, clip, kw)):
            assert torch.equal(x, y), tag


def _gpu_kick_cat(c, coef, clip, sums=None, diag=None):
    prob_tm, v_tm = (_f(c[k]).requires_grad_() for k in ("prob_tm", "v_tm"))
    la, lc = _ops().ppo_bc_loss_cat(_bt(prob_tm), _f(c["action"]), _f(c["label"]), v_tm.permute(1, 0, 2, 3)[..., 0], _f(c["lp_old"]), _f(c["adv"]),
                                    _f(c["active"]), _f(c["vo"]) if clip else None, _f(c["vt"]), EPS, ENT, coef, clip, sums=sums, diag=diag)
    (la + lc).backward()
    return la.detach(), lc.detach(), prob_tm.grad, v_tm.grad


def _ref_cat(c, coef, clip):
    n = lambda k: c[k].numpy()
    return ref.ppo_bc_loss_cat(_bt(c["prob_tm"]).numpy(), n("action"), n("label"), c["v_tm"].permute(1, 0, 2, 3)[..., 0].numpy(), n("lp_old"), n("adv"),
                               n("active"), n("vo"), n("vt"), EPS, ENT, coef, clip)


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("A", [9, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ppo_bc_loss_cat(shape, A, clip):
    """checks 1-3 and the repeatability of check 4, at every lambda"""
    ops = _ops()
    c = _kick_cat_case(*shape, A, seed=100 * A + shape[0])
    vo = _f(c["vo"]) if clip else None
    prob2, v2 = (_f(c[k]).requires_grad_() for k in ("prob_tm", "v_tm"))
    pa, pc = ops.ppo_loss_prob(_bt(prob2), _f(c["action"]), v2.permute(1, 0, 2, 3)[..., 0], _f(c["lp_old"]), _f(c["adv"]), _f(c["active"]), vo,
                               _f(c["vt"]), EPS, ENT, clip)
    (pa + pc).backward()
    prob3, v3 = (_f(c[k]).requires_grad_() for k in ("prob_tm", "v_tm"))
    ba, bc_c = ops.bc_loss_cat(_bt(prob3), _f(c["label"]), v3.permute(1, 0, 2, 3)[..., 0], _f(c["active"]), vo, _f(c["vt"]), EPS, clip)
    (ba + bc_c).backward()
    for coef in LAMBDAS:
        sums = torch.tensor([2.0, 7.0, 9.0], dtype=torch.float64, device="cuda")
        la, lc, gp, gv = got = _gpu_kick_cat(c, coef, clip, sums)
        want = _ref_cat(c, coef, clip)
        tag = f"cat {shape} A={A} clip={clip} coef={coef}"
        _loss_close(la, want["actor_loss"], tag + " actor")
        _loss_close(lc, want["critic_loss"], tag + " critic")
        assert gp.stride() == c["prob_tm"].stride()
        _close(gp, _tm(want["g_prob"]), tag + " g_prob")
        _close(gv, _tm(want["g_v"]), tag + " g_v")
        _dead_rows_are_zero(c, (gp, gv))
        s = sums.cpu().numpy() - [2.0, 7.0, 9.0]
        assert s[0] == want["sums"][0] and s[1] == want["sums"][1], (tag, s, want["sums"])           # hits and rows exact
        print(f"{tag} imitation sum: {s[2]:.9g} against {want['sums'][2]:.9g}")
        assert abs(s[2] - want["sums"][2]) <= 1e-5 * abs(want["sums"][2]), tag
        assert torch.equal(lc, pc.detach()) and torch.equal(gv, v2.grad), tag                        # the PPO launch's critic bits
        _loss_close(la, pa.detach().double() + coef * ba.detach().double(), tag + " actor against ppo + coef bc")
        _close(gp, prob2.grad.double().cpu() + coef * prob3.grad.double().cpu(), tag + " g_prob against ppo + coef bc")
        for x, y in zip(got, _gpu_kick_cat(c, coef, clip)):
            assert torch.equal(x, y), tag


# ---- check 4: sums accumulate, the diagnostics, bytes with and without sums / diag -----------------------------------------------------
def _check_sums_and_diag(call, c, want, kind, tag):
    """call(sums, diag) -> losses and gradients.  The plain call, the call with both twice into the same tensors, the call with diag
    alone: the same bytes; two calls add twice; the eight sums within tests/test_ppo_diag_gpu.py's bounds (the kernel forms lp_now and
    the entropy in fp32, the restatement has them in f64); the three sums against the reference (env_n2n: the hits exact)"""
    plain = call(None, None)
    sums, diag = torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")
    with_both = call(sums, diag)
    once_s, once_d = sums.clone(), diag.clone()
    again, only_diag = call(sums, diag), call(None, torch.zeros(8, dtype=torch.float64, device="cuda"))
    for a, *others in zip(plain, with_both, again, only_diag):
        assert all(torch.equal(a.view(torch.int32), o.view(torch.int32)) for o in others), tag
    assert torch.equal(sums, 2 * once_s) and torch.equal(diag, 2 * once_d), tag
    tol = lambda x: 1e-5 * np.abs(x) + (2e-5 if kind == "gauss" else 1e-5)
    live = c["active"].numpy().reshape(-1) != 0
    lp64, ent64 = c["lp64"].numpy().reshape(-1), np.asarray(c["ent64"]).reshape(-1)
    ratio64 = np.exp(lp64 - c["lp_old"].numpy().reshape(-1))
    bound = np.zeros(8)
    bound[1], bound[3], bound[7] = (np.abs(ratio64 - 1) * tol(lp64))[live].sum(), tol(ent64)[live].sum(), (ratio64 * tol(lp64))[live].sum()
    got, s = once_d.cpu().numpy(), once_s.cpu().numpy()
    err = np.abs(got - want["diag"])
    print(f"{tag}: diag {got.tolist()} err {err.tolist()} bound {bound.tolist()}; sums {s.tolist()} against {want['sums'].tolist()}")
    assert got[0] == want["diag"][0] and got[2] == want["diag"][2], tag           # the integer sums are exact
    for k in (1, 3, 4, 5, 6, 7):
        assert err[k] <= bound[k] + SUM_RTOL * abs(want["diag"][k]), (tag, k, got[k], want["diag"][k], err[k], bound[k])
    assert s[1] == want["sums"][1] and (kind == "gauss" or s[0] == want["sums"][0]), tag
    assert all(abs(s[j] - want["sums"][j]) <= 1e-5 * abs(want["sums"][j]) for j in (0, 2)), tag


DIAG_KINDS = [("param", 1, "clip"), ("param", 16, "tanh"), ("state", 3, "tanh"), ("state", 4, "direction")]


@pytest.mark.parametrize("mode,A,squash", DIAG_KINDS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gauss_sums_and_diagnostics(shape, mode, A, squash):
    metric = "angle" if A == 4 else "mse"
    c = _kick_gauss_case(*shape, A, mode == "state", 1, 50 * A + shape[0], squash)
    kw = _gauss_kw(True, True, squash, metric)
    _check_sums_and_diag(lambda sums, diag: _gpu_kick_gauss(c, 0.3, True, kw, sums, diag), c, _ref_gauss(c, 0.3, True, True, True, squash, metric),
                         "gauss", f"gauss {shape} {mode} A={A} {squash}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cat_sums_and_diagnostics(shape):
    c = _kick_cat_case(*shape, 9, seed=31 + shape[0])
    _check_sums_and_diag(lambda sums, diag: _gpu_kick_cat(c, 0.3, True, sums, diag), c, _ref_cat(c, 0.3, True), "cat", f"cat {shape}")


# ---- check 5 and the overwrite of check 1: the C entry points, called directly ------------------------------------------------------
class _Raw:
    """the arguments of ppo_bc_loss_gauss_fwd_bwd / ppo_bc_loss_cat_fwd_bwd on one small case, in the order of include/mappo_ops.h, with
    the outputs pre-filled with 7.0"""

    def __init__(self, kind, state=True, A=None):
        self.kind, L = kind, _ops().load_library()
        self.c = c = _kick_gauss_case(3, 7, 5, A or 3, state, 1, 11 + (A or 3), "clip") if kind == "gauss" else _kick_cat_case(3, 7, 5, A or 9, 13)
        self.fn = L.ppo_bc_loss_gauss_fwd_bwd if kind == "gauss" else L.ppo_bc_loss_cat_fwd_bwd
        x, v = _f(c["mu_tm" if kind == "gauss" else "prob_tm"]), _f(c["v_tm"])
        T_, mb, P, A = x.shape
        d = {k: _f(c[k]).contiguous() for k in ("action", "lp_old", "adv", "active", "vo", "vt")}
        full = lambda *shape: torch.full(shape, 7.0, device="cuda")
        self.g_x, self.g_v, self.losses = torch.full_like(x, 7.0), full(mb, T_, P), full(2)      # g_v: dense over the rows, as `active`
        self.sums, self.diag = torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")
        xs, vs = _bt(x).stride(), v.permute(1, 0, 2, 3)[..., 0].stride()
        a = dict(n=mb * T_ * P, A=A, x=x, grad_x=self.g_x, d1=T_, d2=P, x_s0=xs[0], x_s1=xs[1], x_s2=xs[2])
        if kind == "gauss":
            ls = _f(c["ls_tm"])
            self.g_ls = torch.full_like(ls, 7.0)
            lss = _bt(ls).stride()[:3] if state else (0, 0, 0)
            a.update(ls_raw=ls, grad_log_std=self.g_ls, l_s0=lss[0], l_s1=lss[1], l_s2=lss[2], lo=LO, hi=HI, squash=0, fit_std=1, wrap0=1, metric=0,
                     action=d["action"], target=_f(c["target"]).contiguous())
        else:
            a.update(action=d["action"], label=_f(c["label"]).contiguous())
        a.update(logp_old=d["lp_old"], adv=d["adv"], active=d["active"], values_now=v, v_s0=vs[0], v_s1=vs[1], v_s2=vs[2], values_old=d["vo"],
                 v_target=d["vt"], active_sum=d["active"].sum().reshape(1), eps=EPS, ent=ENT, coef=0.3, clip=1, losses=self.losses,
                 grad_values=self.g_v, sums=self.sums, diag=self.diag, workspace=torch.empty(L.ppo_bc_loss_workspace(), dtype=torch.uint8, device="cuda"))
        self.args = a

    def call(self, **ov):
        assert set(ov) <= set(self.args), ov
        vals = [(C.c_void_p(v.data_ptr() if v is not None else 0) if (v is None or torch.is_tensor(v)) else v) for v in {**self.args, **ov}.values()]
        rc = self.fn(*vals, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return (self.g_x, self.g_v, self.losses) + ((self.g_ls,) if self.kind == "gauss" else ())

    def untouched(self):
        return all(bool((t == 7.0).all()) for t in self.outputs()) and not self.sums.any() and not self.diag.any()


@pytest.mark.parametrize("kind,state", [("gauss", False), ("gauss", True), ("cat", True)], ids=["gauss_param", "gauss_state", "cat"])
def test_outputs_prefilled_are_overwritten(kind, state):
    raw = _Raw(kind, state)
    assert raw.call() == 0
    assert not any(bool((t == 7.0).any()) for t in raw.outputs())                                 # every element written
    rows = raw.c["active"].sum().item()
    assert raw.sums[1].item() == rows and raw.diag[0].item() == rows
    if kind == "gauss":                                                                           # and with the bits of the op
        la, lc, gmu, gls, gv = _gpu_kick_gauss(raw.c, 0.3, True, _gauss_kw(True, True, "clip", "mse"))
        assert torch.equal(raw.g_x, gmu) and torch.equal(raw.g_ls, gls) and torch.equal(raw.g_v, gv.permute(1, 0, 2, 3)[..., 0])
        assert torch.equal(raw.losses, torch.stack((la, lc)))


COMMON_BAD = [{k: None} for k in ("x", "grad_x", "action", "logp_old", "adv", "active", "values_now", "values_old", "v_target", "active_sum", "losses",
                                   "grad_values", "workspace")]
COMMON_BAD += [{"A": 0}, {"A": 17}, {"n": 0}, {"d1": 0}, {"d2": 4}, {"coef": -0.1}, {"coef": float("nan")}, {"coef": float("inf")}]
GAUSS_BAD = [{"ls_raw": None}, {"grad_log_std": None}, {"target": None}, {"squash": 3}, {"metric": 2}, {"lo": 0.5, "hi": 0.5}, {"lo": float("nan")}]


@pytest.mark.parametrize("kind", ["gauss", "cat"])
def test_bad_arguments_return_the_error_without_a_launch(kind):
    raw = _Raw(kind)
    for ov in COMMON_BAD + (GAUSS_BAD if kind == "gauss" else [{"label": None}]):
        assert raw.call(**ov) == BAD_ARG, ov
        assert raw.untouched(), ov
    if kind == "gauss":
        two = _Raw("gauss", A=1)                                    # the angle metric needs three dimensions
        assert two.call(metric=1) == BAD_ARG and two.untouched()
        wide = _Raw("gauss", A=16)                                  # the diagnostics of a per-row ls_raw exist at A = 3 and 4
        assert wide.call() == BAD_ARG and wide.untouched()
        assert wide.call(diag=None) == 0 and not wide.diag.any()
    assert raw.call(values_old=None, clip=0) == 0                   # no value clip: values_old may be NULL
    assert raw.call(sums=None, diag=None) == 0


# ---- agents and trainers ------------------------------------------------------------------------------------------------------------
KICK = {"algo.bc_iterations": 2, "algo.bc_coef": 0.5, "algo.bc_coef_decay": 0.5, "algo.bc_coef_iterations": 2, "algo.epochs": 2}
KICK_KEYS = {"bc_coef", "bc_aux_loss"}
BC_KEYS = {"phase", "bc_beta", "bc_loss"}


def _agent(kind, cfg, mini_batch_size):
    m = _mod(kind)
    env = m.make_env(cfg, N_ENVS)
    torch.manual_seed(0)
    return (m.E3dMAPPO if kind == "e3d" else m.N2nMAPPO)(cfg, N_ENVS, mini_batch_size), env


def _grads(agent):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).double() for p in agent.ac_parameters])


def _state(agent):
    return {name: {k: v.clone() for k, v in m.state_dict().items()} for name, m in (("actor", agent.actor), ("critic", agent.critic))}


def _restore(agent, state):
    agent.actor.load_state_dict(state["actor"])
    agent.critic.load_state_dict(state["critic"])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind,ov", [("e3d", {}), ("e3d", {"algo.gauss_squash": "direction", "algo.gauss_std": "state", "algo.bc_fit_std": True}),
                                     ("n2n", {})], ids=["e3d", "e3d_direction_state", "n2n"])
def test_train_kick_gradient_is_ppo_plus_lambda_imitation(kind, ov):
    """check 6: one mini-batch of the whole buffer, no gradient clip -- the gradient train(kick=) leaves is that of _minibatch_loss plus
    lambda times the actor part of _imitation_loss, both from the existing ops.  The weights (and the spectral norm's vectors, which a
    forward in training mode advances) are put back before each of the three forwards."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    lam = 0.7
    agent, env = _agent(kind, _cfg(kind, **{"algo.bc_coef": 1.0, "algo.use_grad_clip": False, **ov}), N_ENVS)
    assert agent.value_norm is None and agent.bc is None and agent.kick_sums is not None
    _, buf, steps, _ = agent.explore_expert(env, 0.0)
    state = _state(agent)
    with torch.enable_grad():
        agent.train(buf, steps, kick=lam)
    got = _grads(agent)
    s, c, b = agent.last_kick
    assert c == buf["active"].sum().item() and math.isfinite(b) and math.isfinite(agent.bc_metric(s, c))
    adv, v_target = ops.gae_advnorm(buf["r"], buf["v_n"], buf["active"], agent.gamma, agent.lamda, agent.use_adv_norm)
    agent.ac_optimizer.zero_grad()
    with torch.enable_grad():
        _restore(agent, state)
        la, lc = agent._minibatch_loss(buf, 0, N_ENVS, adv, v_target, {})
        (la + lc).backward()
        _restore(agent, state)
        la_bc, _ = agent._imitation_loss(buf, 0, N_ENVS, v_target, None)
        (lam * la_bc).backward()
    want = _grads(agent)
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    print(f"{kind} {ov}: bucket gradient max error {err:.3e}, largest entry {scale:.3e}; aux loss {b / c:.6g} against {la_bc.item():.6g}")
    assert scale > 0 and err <= 1e-5 * scale
    assert abs(b / c - la_bc.item()) <= 1e-5 * abs(la_bc.item()) + 1e-7


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_regularised_rollout_is_on_policy_and_labelled(kind, monkeypatch):
    """check 7: explore_expert(env, 0.0) under algo.bc_coef alone -- no environment follows the teacher, every row is labelled"""
    agent, env = _agent(kind, _cfg(kind, **{"algo.bc_coef": 0.5}), 2)
    guides, executed = [], []
    step = env.step

    def recording_step(action):
        guides.append(env._guidance_out.clone())                  # what guidance_actions wrote for this tick
        executed.append(action.clone())
        return step(action)

    monkeypatch.setattr(env, "step", recording_step)
    mean_r, buf, steps, stats = agent.explore_expert(env, 0.0)
    assert steps == N_ENVS * T and len(guides) == T and np.isfinite(mean_r)
    guides, executed = torch.stack(guides, 1), torch.stack(executed, 1)              # (N, T, P, ..)
    assert not (guides == executed).reshape(N_ENVS, -1).all(1).any()                  # no environment follows the teacher
    assert torch.equal(buf["a_star"], guides.float())                                 # bc_select's labels of guidance_actions, on every row
    if kind == "n2n":
        assert torch.equal(buf["a_n"], executed.float())                              # the executed action is the network's sample
    else:
        assert torch.equal(buf["a_n"].clamp(-1.0, 1.0).double(), executed)            # ... its clamp to the environment's range


def _counting_select(monkeypatch):
    from distributed_multi_agent_reinforcement_learning_amd import ops
    calls, real = [0], ops.bc_select

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "bc_select", counted)
    return calls


@pytest.mark.timeout(300)
@pytest.mark.parametrize("minibatch_steps", [False, True], ids=["epoch_steps", "minibatch_steps"])
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_trainer_schedule_determinism_and_resume(tmp_path, kind, minibatch_steps, monkeypatch):
    """check 8: two imitation iterations, PPO iterations 0 and 1 with lambda 0.5 and 0.25, PPO iteration 2 past the cut-off"""
    cfg = _cfg(kind, **KICK, **{"algo.minibatch_steps": minibatch_steps})
    calls = _counting_select(monkeypatch)
    path = str(tmp_path / "resume.pt")
    runs = []
    for save in (True, False):
        tr = _trainer(kind, cfg)
        logs, per_iteration = [], []
        for it in range(5):
            before = calls[0]
            logs.append(tr.iterate()[1])
            per_iteration.append(calls[0] - before)
            if save and it == 2:
                tr.save_resume(path)
        assert per_iteration == [T, T, T, T, 0]                    # the teacher leaves the rollout with lambda
        runs.append((tr, logs))
    (a, logs_a), (b, logs_b) = runs
    for log in logs_a[:2]:                                         # imitation iterations log as today
        assert BC_KEYS | {METRIC[kind]} <= set(log) and log["phase"] == "imitation" and not (KICK_KEYS & set(log))
    for j, log in enumerate(logs_a[2:4]):
        assert KICK_KEYS | {METRIC[kind]} <= set(log) and not (BC_KEYS & set(log)) and log["bc_coef"] == 0.5 * 0.5 ** j
        assert np.isfinite(log["bc_aux_loss"]) and np.isfinite(log[METRIC[kind]]) and np.isfinite(log["actor_loss"])
    assert not ((KICK_KEYS | BC_KEYS | {METRIC[kind]}) & set(logs_a[4]))
    assert logs_a == logs_b                                        # two runs give identical logs
    bundle = torch.load(path, weights_only=False)
    assert set(bundle) == OFF_KEYS | {"bc_iterations", "bc_coef"} | ({"minibatch_steps"} if minibatch_steps else set())
    assert bundle["bc_coef"] == (0.5, 0.5, 2)
    c = _trainer(kind, cfg)
    c.load_resume(path)
    assert [c.iterate()[1] for _ in range(2)] == logs_a[3:]        # iterations 4 and 5 bit for bit
    wa, wc = _weights(a), _weights(c)
    assert list(wa) == list(wc) and all(torch.equal(wa[k], wc[k]) for k in wa)
    for ov in ({"algo.bc_coef": 0.25}, {"algo.bc_coef": 0.0}, {"algo.bc_coef_decay": 0.9}):
        other = _trainer(kind, _cfg(kind, **{**KICK, "algo.minibatch_steps": minibatch_steps, **ov}))
        with pytest.raises(ValueError, match=r"algo\.bc_coef"):
            other.load_resume(path)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_kickstart_from_scratch_and_the_kl_stop(tmp_path, kind):
    """check 8, the rest: bc_iterations 0 -- the first iteration is a regularised PPO iteration; a bundle of a run without the feature is
    refused; with update_diagnostics and a tiny target_kl the epoch loop stops after the first epoch past the target"""
    tr = _trainer(kind, _cfg(kind, **{"algo.bc_coef": 0.5, "algo.epochs": 2}))
    log = tr.iterate()[1]
    assert KICK_KEYS | {METRIC[kind]} <= set(log) and log["bc_coef"] == 0.5 and "phase" not in log and np.isfinite(log["bc_aux_loss"])
    off = _trainer(kind, _cfg(kind))
    off.iterate()
    path = str(tmp_path / "off.pt")
    off.save_resume(path)
    with pytest.raises(ValueError, match=r"algo\.bc_coef"):
        tr.load_resume(path)
    from distributed_multi_agent_reinforcement_learning_amd.update_diag import LOG_KEYS
    cut = _trainer(kind, _cfg(kind, **{"algo.bc_coef": 0.5, "algo.epochs": 4, "algo.update_diagnostics": True, "algo.target_kl": 1e-9}))
    log = cut.iterate()[1]
    # the first epoch runs on the rollout's own policy (KL 0 up to fp32 rounding), the second is past the target: its gradient is
    # discarded and the loop ends with one epoch of steps taken
    assert log["epochs_run"] == 1 and len(cut.last_epoch_diags) == 2 and log["approx_kl"] > 1e-9
    assert set(LOG_KEYS) | KICK_KEYS | {METRIC[kind]} <= set(log) and all(math.isfinite(log[k]) for k in LOG_KEYS)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_feature_off_is_a_run_that_never_mentions_the_keys(tmp_path, kind):
    """check 9"""
    runs = []
    for ov in ({}, {"algo.bc_coef": 0, "algo.bc_coef_decay": 0.5, "algo.bc_coef_iterations": 3}):
        tr = _trainer(kind, _cfg(kind, **ov))
        logs = [tr.iterate()[1] for _ in range(2)]
        path = str(tmp_path / f"resume{len(runs)}.pt")
        tr.save_resume(path)
        runs.append((tr, logs, torch.load(path, weights_only=False)))
    (a, logs_a, bundle_a), (b, logs_b, bundle_b) = runs
    assert logs_a == logs_b and not any((KICK_KEYS | BC_KEYS | set(METRIC.values())) & set(log) for log in logs_a)
    assert set(a.agent.buffer) == set(b.agent.buffer) and "a_star" not in a.agent.buffer
    assert set(bundle_a) == set(bundle_b) == OFF_KEYS
    assert a.agent.kick_sums is None and b.agent.kick_sums is None and a.agent.last_kick is None
    wa, wb = _weights(a), _weights(b)
    assert all(torch.equal(wa[k], wb[k]) for k in wa)
    with pytest.raises(ValueError, match="algo.bc_iterations"):
        a.agent.explore_expert(a.env, 0.0)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_imitation_term_falls_on_a_fixed_buffer(kind):
    """check 10: tests/test_imitation_gpu.py's fixed-buffer protocol with train(kick=1.0) on the feature's own rollout (labelled,
    on-policy): 30 updates, the unweighted imitation term of the last below that of the first.  Measured ratios: DESIGN.md section 7i."""
    agent, env = _agent(kind, _cfg(kind, **{"algo.bc_coef": 1.0}), 2)
    _, buf, steps, _ = agent.explore_expert(env, 0.0)
    aux = []
    for _ in range(30):
        with torch.enable_grad():
            agent.train(buf, steps, kick=1.0)
        agent.ac_optimizer.step()
        s, c, b = agent.last_kick
        aux.append(b / c)
    print(f"{kind}: bc_aux_loss {aux[0]:.6g} -> {aux[-1]:.6g} (ratio {aux[-1] / aux[0]:.4f}), metric {agent.bc_metric(s, c):.4g}")
    assert np.isfinite(aux).all() and aux[-1] < aux[0]
