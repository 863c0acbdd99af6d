"""`algo.use_layer_norm`: the kernels of csrc/layer_norm.hpp against F.layer_norm in f64 on guarded buffers (criterion of
tests/test_pool_agg_gpu.py: err <= 4 x torch's own fp32 error on CPU / GPU + 2e-5 max|reference|), bits, refusals, one case per agent."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from distributed_multi_agent_reinforcement_learning_amd import ops
from tests.test_pool_agg_gpu import FILL, GUARD, _within

pytestmark = pytest.mark.gpu
E, EPS, BAD_ARG, U = 128, 1e-5, 20001, ops.FEAT_NORM_UNROLL      # U: csrc/layer_norm.hpp FN_U
# (R, max_blocks): three idle waves | a second trip on one workgroup | two partial blocks and a second stride | one row past a full unrolled trip
SHAPES = [(1, 0), (5, 1), (13, 2), (4 * U * 2 + 1, 2)]
NAMES = ("y", "dx", "d_weight", "d_bias")
PTRS = ("x", "weight", "bias", "y", "g", "dx", "d_weight", "d_bias")
FWD, BWD = {"x", "ldx", "weight", "bias", "y", "ldy"}, {"x", "ldx", "weight", "g", "ldg", "dx", "lddx", "d_weight", "d_bias"}   # what each entry reads


def _inputs(R, jobs, shifted):
    rn = functools.partial(torch.randn, generator=torch.manual_seed(R + 100 * jobs))   # per job (x, weight, bias, g); shifted: an uncentred variance fails it
    return [((50 + 0.5 * rn(R, E)) if shifted else rn(R, E), 1 + 0.5 * rn(E), 0.5 * rn(E), rn(R, E)) for _ in range(jobs)]


def _formula(t, dtype, device):
    x, w, b, g = [v.to(device=device, dtype=dtype) for v in t]
    x, w, b = x.requires_grad_(), w.requires_grad_(), b.requires_grad_()
    y = F.layer_norm(x, (E,), w, b, EPS)
    return [y.detach().cpu()] + [v.cpu() for v in torch.autograd.grad(y, (x, w, b), g)]


@functools.lru_cache(maxsize=None)
def _noisy_reference(R, jobs, shifted):
    out = []   # per job (the f64 reference, the fp32 noise per tensor); computed once per input set, shared by the layouts
    for t in _inputs(R, jobs, shifted):
        ref, cpu, gpu = _formula(t, torch.float64, "cpu"), _formula(t, torch.float32, "cpu"), _formula(t, torch.float32, "cuda")
        out.append((ref, [max((a.double() - r).abs().max().item(), (b.double() - r).abs().max().item()) for a, b, r in zip(cpu, gpu, ref)]))
    return out


def _launch(ts, max_blocks, ld=E):
    """both entry points, all jobs in one launch each, guarded outputs, everything in the left halves of rows ld apart -> per job NAMES"""
    L, R, n = ops.load_library(), ts[0][0].shape[0], len(ts)
    arr, keep, outs = (ops.FeatNormJob * n)(), [], []
    for a, t in zip(arr, ts):
        x, g, w, b = torch.randn(R, ld).cuda(), torch.randn(R, ld).cuda(), t[1].cuda(), t[2].cuda()
        x[:, :E], g[:, :E] = t[0].cuda(), t[3].cuda()
        bufs = [torch.full((k + 2 * GUARD,), FILL, device="cuda") for k in (R * ld, R * ld, E, E)]
        y, dx, dw, db = [buf[GUARD:-GUARD].data_ptr() for buf in bufs]
        keep.append((x, g, w, b)), outs.append(bufs)
        a.x, a.ldx, a.weight, a.bias, a.g, a.ldg = x.data_ptr(), ld, w.data_ptr(), b.data_ptr(), g.data_ptr(), ld
        a.y, a.ldy, a.dx, a.lddx, a.d_weight, a.d_bias = y, ld, dx, ld, dw, db
    ws = torch.empty(L.feat_norm_bwd_workspace(E, n, max_blocks), dtype=torch.uint8, device="cuda")
    assert L.feat_norm_fwd_multi(n, C.cast(arr, C.c_void_p), R, E, EPS, max_blocks, ops._stream()) == 0
    assert L.feat_norm_bwd_multi(n, C.cast(arr, C.c_void_p), R, E, EPS, ops._ptr(ws), max_blocks, ops._stream()) == 0
    torch.cuda.synchronize()
    res = [[] for _ in outs]
    for got, bufs in zip(res, outs):
        for buf, name in zip(bufs, NAMES):
            assert (buf[:GUARD] == FILL).all() and (buf[-GUARD:] == FILL).all(), f"{name}: a guard band was written"
            rows = buf[GUARD:-GUARD].view(-1, ld if name in ("y", "dx") else E)
            assert (rows[:, E:] == FILL).all() and not (rows[:, :E] == FILL).any(), f"{name}: the right half was written, or an element was not"
            got.append(rows[:, :E].clone() if name in ("y", "dx") else rows[0].clone())
    return res


@pytest.mark.parametrize("shifted", [False, True], ids=["randn", "shifted"])
@pytest.mark.parametrize("jobs", [1, 2])
@pytest.mark.parametrize("ld", [E, 2 * E], ids=["dense", "ld256"])
@pytest.mark.parametrize("R,max_blocks", SHAPES)
def test_kernels_against_f64(R, max_blocks, ld, jobs, shifted):
    got = _launch(_inputs(R, jobs, shifted), max_blocks, ld)
    for k, (g, (ref, noise)) in enumerate(zip(got, _noisy_reference(R, jobs, shifted))):
        _within(g, ref, noise, f"R{R} mb{max_blocks} ld{ld} job {k}/{jobs} shifted={shifted}", NAMES)


def test_bits_do_not_depend_on_the_launch_or_the_batch():
    # two jobs in one launch = two single-job launches = a second run, bit for bit; y, dx of rows [0, 13) are the same inside a batch of 33
    ts = _inputs(33, 2, False)
    both, again, single = _launch(ts, 2), _launch(ts, 2), [_launch([t], 2)[0] for t in ts]
    for a, b, c in zip(both, again, single):
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))
    head = _launch([tuple(v[:13] if v.dim() == 2 else v for v in t) for t in ts], 2)
    for a, h in zip(both, head):
        assert torch.equal(a[0][:13], h[0]) and torch.equal(a[1][:13], h[1]), "a row's y / dx depends on other rows"


REFUSALS = ([("width", dict(width=64)), ("R<0", dict(R=-1)), ("n_jobs=0", dict(n_jobs=0)), ("n_jobs=5", dict(n_jobs=5)), ("workspace NULL", dict(ws=None))]
            + [(f"eps={e}", dict(eps=e)) for e in (0.0, -1.0, math.inf, math.nan)]
            + [(f"{f} NULL", {f: None}) for f in PTRS] + [(f"{f} misaligned", {f: 4}) for f in PTRS]
            + [(f"{f}={v}", {f: v}) for f in ("ldx", "ldy", "ldg", "lddx") for v in (126, 129)]
            + [("y over x", dict(y="x")), ("dx over x", dict(dx="x"))])


@pytest.mark.parametrize("what,change", REFUSALS + [("R=0", dict(R=0))], ids=lambda v: v if isinstance(v, str) else "")
def test_refusals_leave_the_outputs_untouched(what, change):
    # every bad argument: MO_ERR_BAD_ARG from the entry point(s) that read it, before any write; R = 0: success, and nothing written
    L, R = ops.load_library(), 5
    t = {f: torch.randn(R, E, device="cuda") if f in ("x", "g") else torch.randn(E, device="cuda") for f in ("x", "g", "weight", "bias")}
    t.update({f: torch.full((R * E if f in ("y", "dx") else E,), FILL, device="cuda") for f in ("y", "dx", "d_weight", "d_bias")})
    fields = {**{f: t[f].data_ptr() for f in PTRS}, "ldx": E, "ldy": E, "ldg": E, "lddx": E}
    args = dict(n_jobs=1, R=R, width=E, eps=EPS, ws=torch.empty(L.feat_norm_bwd_workspace(E, 4, 0), dtype=torch.uint8, device="cuda"))
    hit = set()
    for k, v in change.items():
        if k in args:
            args[k], hit = v, FWD | BWD if k != "ws" else {"d_bias"}   # (the workspace: an argument of the backward alone)
        else:
            fields[k] = None if v is None else fields[v] if isinstance(v, str) else fields[k] + 4 if k in PTRS else v
            hit.add(k)
    arr = (ops.FeatNormJob * 8)(*[ops.FeatNormJob(**fields) for _ in range(8)])
    head = (args["n_jobs"], C.cast(arr, C.c_void_p), args["R"], args["width"], args["eps"])
    rc_f, rc_b = L.feat_norm_fwd_multi(*head, 0, ops._stream()), L.feat_norm_bwd_multi(*head, ops._ptr(args["ws"]), 0, ops._stream())
    torch.cuda.synchronize()
    want = 0 if what == "R=0" else BAD_ARG
    assert rc_f == (want if hit & FWD else 0) and rc_b == (want if hit & BWD else 0), (what, rc_f, rc_b)
    untouched = (("y",) if hit & FWD else ()) + (("dx", "d_weight", "d_bias") if hit & BWD else ())
    assert all((t[f] == FILL).all() for f in untouched), f"{what}: an output was written"


# one case per agent, at the smallest environment count its GPU tests use
CFG = {"e3d": ("cfg5", {"runtime.num_envs": 16, "env.max_steps": 20, "env.num_defender": 3, "runtime.e3d_evader": "rule"}),
       "n2n": ("cfg4_n2n", {"runtime.num_envs": 8, "env.max_steps": 10, "runtime.n2n_evader": "rule"})}


def _trainer(kind, on=True):
    from distributed_multi_agent_reinforcement_learning_amd import e3d_agent, n2n_agent
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    cfg = baseline_config(CFG[kind][0], **CFG[kind][1], **{"algo.epochs": 2}, **({"algo.use_layer_norm": True} if on else {}))
    return (e3d_agent.E3dTrainer if kind == "e3d" else n2n_agent.N2nTrainer)(cfg, num_eval_envs=4, eval_every=1)


def _rollout_against_update(kind, tr):
    # random feat_norm weights: the stored log-probabilities are the update forward's, within the agents' own option-off tolerance (1e-4)
    agent, N = tr.agent, tr.env.num_envs
    with torch.no_grad():
        for m in (agent.actor.feat_norm, agent.critic.feat_norm):
            m.weight.copy_(1 + 0.3 * torch.randn(E)), m.bias.copy_(0.3 * torch.randn(E))
    calls = ops.feat_norm_calls
    buf = agent.explore_env(tr.env)[1]
    T = buf["r"].shape[1]
    assert ops.feat_norm_calls == calls + T + 1, "one launch a tick and one for the bootstrap value"
    with torch.enable_grad():
        if kind == "e3d":
            mu, values = agent.sequence_forward(buf["feat_a"], buf["feat_c"], N, T)
            lp = torch.distributions.Normal(mu.detach(), torch.exp(agent.actor.log_std.detach())).log_prob(buf["a_n"]).sum(-1)
        else:
            prob, values = agent.sequence_forward(buf, 0, N)
            lp = torch.distributions.Categorical(prob.detach()).log_prob(buf["a_n"])
    live = buf["active"] == 1
    err_lp, err_v = (lp - buf["a_logprob_n"])[live].abs().max().item(), (values.detach() - buf["v_n"][:, :T])[live].abs().max().item()
    print(f"{kind}: live rows {int(live.sum())}, log-prob error {err_lp:.3e}, value error {err_v:.3e}")
    assert live.sum() > 0 and err_lp <= 1e-4 and err_v <= 1e-4


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["e3d", "n2n"])
def test_agent_rollout_update_determinism_resume_and_refusals(kind, tmp_path):
    _rollout_against_update(kind, _trainer(kind))
    path, runs = str(tmp_path / "resume.pt"), []
    for save in (True, False):
        tr, logs = _trainer(kind), []
        for it in range(2):
            logs.append(tr.iterate()[1])
            if save and it == 0:
                tr.save_resume(path)
        runs.append((tr, logs))
    (a, logs_a), (_, logs_b) = runs
    assert all(math.isfinite(float(v)) for log in logs_a for v in log.values() if isinstance(v, (int, float)))
    assert logs_a == logs_b                                                          # two runs give identical logs
    for net in (a.agent.actor, a.agent.critic):
        assert list(net.state_dict())[-2:] == ["feat_norm.weight", "feat_norm.bias"] and not torch.equal(net.feat_norm.weight, torch.ones_like(net.feat_norm.weight))
    c = _trainer(kind)
    c.load_resume(path)
    assert c.iterate()[1] == logs_a[1]                                               # iteration 2 bit for bit
    assert all(torch.equal(x, y) for m, n in ((a.agent.actor, c.agent.actor), (a.agent.critic, c.agent.critic)) for x, y in zip(m.state_dict().values(), n.state_dict().values()))
    off = _trainer(kind, on=False)
    a.agent.save_model(str(tmp_path / "on")), off.agent.save_model(str(tmp_path / "off"))
    for load in (lambda: off.load_resume(path), lambda: off.agent.load_model(str(tmp_path / "on")), lambda: a.agent.load_model(str(tmp_path / "off"))):
        with pytest.raises(ValueError, match="algo.use_layer_norm"):
            load()
    c.agent.load_model(str(tmp_path / "on"))                                         # ... and accepted by its own
