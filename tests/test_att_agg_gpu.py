"""The attention aggregator's kernels (csrc/att_agg.hpp, include/mappo_ops.h dhgn_att_agg3_fwd / dhgn_att_agg_bwd) against the formula in f64 on
guarded outputs; alpha = 0 against the mean's reference; row independence and run-to-run bits; DHGN with `vertex_level_aggregator: att`
against f64, forward_pair against forward, two trainer iterations; the entry points' refusals.
Criterion per tensor: err <= 4 x (distance of the same formula in fp32 torch from f64, the larger of CPU and GPU) + 2e-5 max|reference|.

The inputs' seed is chosen from the f64 reference alone, by the rule of tests/test_gnn_pairs_gpu.py: a ReLU decision at a pre-activation
that fp32 cannot tell from zero belongs to no fp32 evaluation.  SEED is the first seed (0, 1, ..) at which no pre-activation z of a pair
listed by the random adjacency, in any case of CASES, lies within 1e-6 of zero in f64 (a CPU scan over _inputs and _z64 below: seed 0
has a listed |z| of 7.0e-7; the closest at seed 1 is 1.36e-6).  torch's fp32 pre-activations stand 2.5e-7 rms from f64 on this data
(the 33-row case).  The all-ones and valid masks list every pair and cannot be kept clear of zero; they rest on the noise term."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
GUARD, FILL, BAD_ARG, E = 256, 7.0, 20001, 128   # include/mappo_ops.h MO_ERR_BAD_ARG
CASES = [(1, 1, 0, 4, 1), (3, 1, 1, 4, 1), (5, 4, 4, 8, 1), (5, 4, 63, 4, 1), (5, 4, 64, 4, 1), (5, 4, 65, 4, 1), (12, 3, 130, 4, 6),
         (33, 8, 176, 4, 1), (5, 16, 48, 4, 1)]   # (R, P, K, din, q_div); a pass-A chunk: 64 pairs
SEED = 1      # (the docstring says how it is chosen)
NAMES = ("out", "dW", "db", "d_alpha")
ids = lambda c: "R%d-P%d-K%d-din%d-q%d" % c


def _ops():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops


def _inputs(R, P, K, din, q_div, seed=SEED, alpha_scale=1.0):
    """-> [p, q, e | None, W, b, alpha, gout], the random adjacency (row (0, 0) all zero) and kvalid (0, a middle value, K in turn)"""
    g = torch.manual_seed(seed)
    lin = torch.nn.Linear(din, E)                                       # the default initialisation
    p, q = torch.rand(R, P, 4, generator=g) * 20, torch.rand(R // q_div, K, 4, generator=g) * 20
    e = torch.rand(R, 4, generator=g) * 20 if din == 8 else None
    adj = (torch.rand(R, P, K, generator=g) < 0.3).float()
    adj[0, 0] = 0
    alpha = torch.randn(E, generator=g) / math.sqrt(E) * alpha_scale
    kvalid = torch.tensor([0, K // 2, K], dtype=torch.int32)[torch.arange(R // q_div) % 3]
    return [p, q, e, lin.weight.detach(), lin.bias.detach(), alpha, torch.randn(R, P, E, generator=g)], adj, kvalid


def _dense(source, adj, kvalid, q_div):
    if source != "valid":
        return torch.ones_like(adj) if source == "ones" else adj
    return (torch.arange(adj.shape[2])[None, :] < kvalid.repeat_interleave(q_div)[:, None]).float()[:, None, :].expand_as(adj)


def _z64(t, q_div):
    p, q, e, W, b = [None if x is None else x.double() for x in t[:5]]
    x = p[:, :, None] - q.repeat_interleave(q_div, 0)[:, None]
    if e is not None:
        x = torch.cat((x, (p - e[:, None])[:, :, None].expand_as(x)), -1)
    return x, x @ W.T + b


def _reference(t, a, q_div, dtype, device):
    """the specification (the issue's formula): out and the three parameter gradients for gout, evaluated in `dtype` on `device`"""
    p, q, e, W, b, alpha, gout = [None if x is None else x.to(device=device, dtype=dtype) for x in t]
    a = a.to(device=device, dtype=dtype)
    W, b, alpha = [x.requires_grad_() for x in (W, b, alpha)]
    x = p[:, :, None] - q.repeat_interleave(q_div, 0)[:, None]
    if e is not None:
        x = torch.cat((x, (p - e[:, None])[:, :, None].expand_as(x)), -1)
    m = torch.relu(x @ W.T + b)                                                          # (R, P, K, E)
    s = torch.where(a != 0, m @ alpha, torch.full_like(a, float("-inf")))
    big = s.amax(-1, keepdim=True).clamp_min(-3e38) if a.shape[2] else s.new_zeros(*a.shape[:2], 1)
    u = a * torch.exp(s - big)
    den = u.abs().sum(-1, keepdim=True)
    out = (u[..., None] * m).sum(2) / torch.where(den > 0, den, torch.ones_like(den)) + 0 * (W.sum() + b.sum() + alpha.sum())
    return [out.detach().cpu()] + [g.cpu() for g in torch.autograd.grad(out, (W, b, alpha), gout)]


def _launch(t, source, adj, kvalid, q_div, rows=None, alpha=None):
    """both entry points on guarded outputs (the relation in all three slots of the forward) -> [out (R, P, 3, E), dW, db, d_alpha]"""
    ops = _ops()
    L, ptr = ops.load_library(), ops._ptr
    p, q, e, W, b, al, gout = [None if x is None else x.cuda() for x in t]
    al = al if alpha is None else alpha.cuda()
    adj, kvalid = adj.cuda(), kvalid.cuda()
    if rows is not None:
        p, adj, gout = [x[rows].contiguous() for x in (p, adj, gout)]
        e = None if e is None else e[rows].contiguous()
        q, kvalid, q_div = q[[r // q_div for r in rows]].contiguous(), kvalid[[r // q_div for r in rows]].contiguous(), 1
    R, P, K, din = p.shape[0], p.shape[1], q.shape[1], W.shape[1]
    mode = {"tensor": ops.ADJ_TENSOR, "bits": ops.ADJ_BITS, "ones": ops.ADJ_ONES, "valid": ops.ADJ_VALID}[source]
    a_dev = ops.pack_adj_bits(adj) if source == "bits" else adj
    a_rs = a_dev.shape[1] * a_dev.shape[2]
    gout3 = gout[:, :, None, :].expand(R, P, 3, E).contiguous()
    ins = [x for x in (p, q, e, a_dev, kvalid, W, b, al, gout3) if x is not None]
    keep = [x.clone() for x in ins]
    bufs = [torch.full((n + 2 * GUARD,), FILL, device="cuda") for n in (R * P * 3 * E, E * din, E, E)]
    outs = [x[GUARD:-GUARD] for x in bufs]
    arr = (ops.AttRel * 3)()
    for m in arr:
        m.K, m.din, m.q_div, m.adj_mode, m.q, m.q_rs, m.adj, m.adj_rs = K, din, q_div, mode, q.data_ptr(), 4 * K, a_dev.data_ptr(), a_rs
        m.e, m.e_rs = (e.data_ptr(), 4) if e is not None else (None, 0)
        m.kvalid, m.W, m.b, m.alpha = kvalid.data_ptr(), W.data_ptr(), b.data_ptr(), al.data_ptr()
    assert L.dhgn_att_agg3_fwd(C.cast(arr, C.c_void_p), R, P, E, ptr(p), 4 * P, ptr(outs[0]), 3 * E, ops._stream()) == 0
    ws = torch.empty(L.dhgn_att_agg_bwd_workspace(E, din), dtype=torch.uint8, device="cuda")
    assert L.dhgn_att_agg_bwd(R, P, K, E, din, ptr(p), 4 * P, ptr(q), 4 * K, q_div, ptr(e), 4 if e is not None else 0, ptr(a_dev), a_rs, mode, ptr(kvalid),
                              ptr(W), ptr(b), ptr(al), C.c_void_p(gout3.data_ptr() + 4 * E), 3 * E, *[ptr(x) for x in outs[1:]], ptr(ws), ops._stream()) == 0
    torch.cuda.synchronize()
    for buf, x, name in zip(bufs, outs, NAMES):
        assert (buf[:GUARD] == FILL).all() and (buf[-GUARD:] == FILL).all(), f"{name}: a guard band was written"
        assert not (x == FILL).any(), f"{name}: an element was left unwritten"
    assert all(torch.equal(x, y) for x, y in zip(keep, ins)), "an input was changed"
    return [outs[0].view(R, P, 3, E).clone()] + [x.clone() for x in outs[1:]]


_refs = {}


def _case(case, source, alpha_scale=1.0):
    """inputs, f64 reference and the fp32 noise of a case: computed once, shared"""
    key = (case, "tensor" if source == "bits" else source, alpha_scale)
    if key not in _refs:
        t, adj, kvalid = _inputs(*case, alpha_scale=alpha_scale)
        a = _dense(source, adj, kvalid, case[4])
        ref = _reference(t, a, case[4], torch.float64, "cpu")
        f32 = [_reference(t, a, case[4], torch.float32, dev) for dev in ("cpu", "cuda")]
        noise = [max((x.double() - r).abs().max().item(), (y.double() - r).abs().max().item()) for x, y, r in zip(*f32, ref)]
        _refs[key] = (t, adj, kvalid, ref, noise)
    return _refs[key]


def _within(got, ref, noise, what, names=NAMES):
    worst = 0.0
    for g, r, nz, name in zip(got, ref, noise, names):
        assert torch.isfinite(g).all(), f"{what} {name}: not finite"
        err, bound = (g.double().cpu().reshape(r.shape) - r).abs().max().item(), 4 * nz + 2e-5 * r.abs().max().item()
        assert math.isfinite(bound), f"{what} {name}: the bound is not finite"
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))     # (an all-zero case: nothing but exact zeros passes)
        worst = max(worst, ratio)
        print(f"{what} {name}: err {err:.3e} bound {bound:.3e} ratio {ratio:.3f}")
    assert worst <= 1.0, f"{what}: worst err / bound {worst:.3f}"


def _check(case, source, alpha_scale=1.0):
    t, adj, kvalid, ref, noise = _case(case, source, alpha_scale)
    got = _launch(t, source, adj, kvalid, case[4])
    assert torch.equal(got[0][:, :, 0], got[0][:, :, 1]) and torch.equal(got[0][:, :, 0], got[0][:, :, 2]), "the three slots differ"
    _within([got[0][:, :, 1]] + got[1:], ref, noise, f"{case} {source}")
    return got


@pytest.mark.parametrize("source", ["tensor", "bits", "ones", "valid"])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_kernels_against_f64(case, source):
    got = _check(case, source)
    if source in ("tensor", "bits") or case[2] == 0:
        assert (got[0][0, 0] == 0).all(), "a segment with nothing listed must give exact zeros"
    if case[2] == 0:
        assert all((g == 0).all() for g in got[1:]), "an empty relation must give exact-zero gradients"


def test_wide_score_spread_stays_finite():
    """alpha scaled until a segment's f64 scores spread by more than 200 (segment (1, 0): 272; max |s| 449): exp(s) alone overflows fp32"""
    case, scale = CASES[7], 40.0
    t, adj, _ = _inputs(*case, alpha_scale=scale)
    s = torch.relu(_z64(t, 1)[1]) @ t[5].double()
    s0 = s[1, 0][adj[1, 0] != 0]
    assert s0.max() - s0.min() > 200 and s.abs().max() > 89
    _check(case, "tensor", scale)


@pytest.mark.parametrize("case,source", [(CASES[2], "tensor"), (CASES[6], "ones"), (CASES[7], "valid")], ids=["tensor", "ones", "valid"])
def test_alpha_zero_is_the_mean(case, source):
    from tests import msg_ref
    t, adj, kvalid = _inputs(*case)
    got = _launch(t, source, adj, kvalid, case[4], alpha=torch.zeros(E))[0][:, :, 0]
    ref = msg_ref.msg_agg(t[0], t[1], t[2], t[3], t[4], source, adj=adj, kvalid=kvalid.numpy(), q_div=case[4])["out"]
    print(f"{case} {source}: alpha = 0 against the mean, fwd_err {msg_ref.fwd_err(got, ref):.3f}")
    assert msg_ref.fwd_err(got, ref) <= 1.0


def test_rows_independent_and_bits_repeat():
    t, adj, kvalid = _case(CASES[7], "tensor")[:3]
    full, again = _launch(t, "tensor", adj, kvalid, 1), _launch(t, "tensor", adj, kvalid, 1)
    assert all(torch.equal(a, b) for a, b in zip(full, again)), "two launches differ"
    for r in (0, 1, 32):
        assert torch.equal(_launch(t, "tensor", adj, kvalid, 1, rows=[r])[0][0], full[0][r]), f"row {r} alone differs from the full launch"


def _torch_model(net, args, critic, dtype):
    """DHGN.forward (depth 1) of a copy of `net` in `dtype`, in plain torch on ops.att_agg_formula -> [y] + parameter gradients"""
    import copy
    import torch.nn.functional as F
    ops, net = _ops(), copy.deepcopy(net).to(dtype)
    p, e, o, adj_p, adj_e, adj_o, hist, d_y, T = [x.to(dtype) if torch.is_tensor(x) else x for x in args]
    R, P = p.shape[:2]
    rels = ((p, e.reshape(R, 4), adj_p, 1), (e, None, adj_e, 1), (o, None, adj_o, T))
    m3 = torch.stack([ops.att_agg_formula(p, q, ee, torch.ones_like(a) if critic else a, net.MSG_layers[r].weight, net.MSG_layers[r].bias,
                                          net.alpha[f"AGG_vertex_{r}"].reshape(-1), qd) for r, (q, ee, a, qd) in enumerate(rels)], 2)
    emb = torch.relu(net.AGG_layers["AGG_vertex_0"](m3)).reshape(R, P, 3 * E)
    h0 = net.semantic_layer(torch.cat([p, emb], -1))
    a = torch.ones_like(adj_p) if critic else adj_p
    nb = F.normalize(a, p=1, dim=-1) @ hist
    y = torch.relu(net.FCRA_layers[0](torch.cat([torch.relu(net.AGG_layers["AGG_fcra_0"](nb)), h0], -1)))
    return [y.detach()] + list(torch.autograd.grad(y, list(net.parameters()), d_y))


@pytest.mark.parametrize("critic", [False, True])
def test_dhgn_att_against_f64(critic):
    from distributed_multi_agent_reinforcement_learning_amd.model import DHGN
    from tests.helpers import product_cfg
    ops = _ops()
    torch.manual_seed(3)
    B, T, P, O = 3, 4, 4, 21
    net = DHGN(4, E, False, product_cfg(P, 20, 20, depth=1, **{"algo.vertex_level_aggregator": "att"}).algo).cuda()
    assert all((net.alpha[f"AGG_vertex_{r}"] == 0).all() and net.alpha[f"AGG_vertex_{r}"].shape == (E, 1) for r in range(3))
    with torch.no_grad():
        for al in net.alpha.values():
            al.copy_(torch.randn(E, 1) / math.sqrt(E))
    R = B * T
    p, e, o = torch.rand(R, P, 4, device="cuda") * 20, torch.rand(R, 1, 4, device="cuda") * 20, torch.rand(B, O, 4, device="cuda") * 20
    adj_p, adj_e, adj_o = [(torch.rand(R, P, k, device="cuda") < 0.4).float() for k in (P, 1, O)]
    hist, d_y = torch.randn(R, P, E, device="cuda"), torch.randn(R, P, E, device="cuda")
    calls, y = ops.att_agg_calls, net(p, e, o, adj_p, adj_e, adj_o, [hist], critic, None, T)
    got = [y.detach()] + list(torch.autograd.grad(y, list(net.parameters()), d_y))
    assert ops.att_agg_calls == calls + 1, "the fused path did not run"
    args = (p, e, o, adj_p, adj_e, adj_o, hist, d_y, T)
    ref = [x.cpu() for x in _torch_model(net, args, critic, torch.float64)]
    noise = [(x.double().cpu() - r).abs().max().item() for x, r in zip(_torch_model(net, args, critic, torch.float32), ref)]
    _within(got, ref, noise, f"DHGN att critic={critic}", ["y"] + [n for n, _ in net.named_parameters()])
    with torch.no_grad():
        pair = net.forward_pair(p, e, o, adj_p, adj_e, adj_o, [hist], [hist], None, T)
        both = [net(p, e, o, adj_p, adj_e, adj_o, [hist], c, None, T) for c in (False, True)]
    for slot in (0, 1):
        torch.testing.assert_close(pair[slot], both[slot], rtol=1e-5, atol=1e-6)


def test_it_trains():
    from distributed_multi_agent_reinforcement_learning_amd.trainer import Trainer
    from tests.helpers import product_cfg
    tr = Trainer(product_cfg(4, 20, 20, T=20, **{"runtime.seed": 5, "algo.vertex_level_aggregator": "att"}), num_envs=16)
    alphas = {k: v for k, v in tr.agent.actor.state_dict().items() if ".alpha." in k}
    assert len(alphas) == 3 and all((v == 0).all() for v in alphas.values())
    for _ in range(2):
        tr.iterate()
        assert all(math.isfinite(float(x)) for x in tr.last_log)
    sd = {k: v.clone() for k, v in tr.agent.actor.state_dict().items()}
    # ONE evader: its relation's only neighbour has weight 1 whatever alpha is, d out / d alpha_1 is identically zero; the optimiser owns all three
    moved = {k[-1]: bool((sd[k] != 0).any()) for k in alphas}
    assert moved == {"0": True, "1": False, "2": True}, moved
    owned = {id(q) for q in tr.agent.ac_parameters}
    assert all(id(v) in owned for v in tr.agent.actor.shared_net.alpha.values())
    with torch.no_grad():
        for v in tr.agent.actor.shared_net.alpha.values():
            v.zero_()
    tr.agent.actor.load_state_dict(sd)
    assert all(torch.equal(tr.agent.actor.state_dict()[k], sd[k]) for k in alphas)


def test_refusals():
    ops = _ops()
    L, ptr = ops.load_library(), ops._ptr
    (p, q, e, W, b, al, gout), adj, kvalid = _inputs(4, 2, 3, 4, 2)
    p, q, W, b, al, adj = [x.cuda() for x in (p, q, W, b, al, adj)]
    out = torch.full((4 * 2 * 3 * E + 4,), FILL, device="cuda")
    arr = (ops.AttRel * 3)()
    for m in arr:
        m.K, m.din, m.q_div, m.adj_mode, m.q, m.q_rs, m.adj, m.adj_rs = 3, 4, 2, ops.ADJ_TENSOR, q.data_ptr(), 12, adj.data_ptr(), 6
        m.W, m.b, m.alpha = W.data_ptr(), b.data_ptr(), al.data_ptr()

    def fwd(R=4, width=E, p_=p, out_=out):
        return L.dhgn_att_agg3_fwd(C.cast(arr, C.c_void_p), R, 2, width, ptr(p_), 8, ptr(out_), 3 * E, ops._stream())
    assert fwd(width=64) == BAD_ARG and fwd(p_=None) == BAD_ARG and fwd(out_=out[1:]) == BAD_ARG
    assert fwd(R=0) == 0
    torch.cuda.synchronize()
    assert (out == FILL).all(), "a refused call wrote"
    assert fwd() == 0
