"""GPU parity of the fused HIP ops (include/mappo_ops.h) against the plain-torch oracle."""
import numpy as np
import pytest
import torch

from oracle import model_oracle as mo

pytestmark = pytest.mark.gpu


def _ref_msg_agg(p, q, e, adj, W, b, r0):
    """materialised reference: coordinate + message + normalised matmul (oracle.encoder's inner part), fp32 CPU"""
    rel = p.unsqueeze(-2) - q.unsqueeze(-3)
    if r0:
        t2 = (p.unsqueeze(-2) - e.unsqueeze(-3)).expand(*rel.shape)
        rel = torch.cat((rel, t2), -1)
    msg = torch.relu(torch.nn.functional.linear(rel, W, b))
    a = torch.nn.functional.normalize(adj.unsqueeze(-2), p=1, dim=-1)
    return torch.matmul(a, msg).squeeze(-2)


@pytest.mark.parametrize("E", [128, 64, 256])   # one wave per row with two features per lane (128, 256) or one (64)
@pytest.mark.parametrize("rel", [0, 1, 2])
@pytest.mark.parametrize("mode", ["tensor", "ones", "valid"])
def test_msg_agg_forward_backward(rel, mode, E):
    from distributed_multi_agent_reinforcement_learning_amd import ops
    if mode == "valid" and rel != 2:
        pytest.skip("ADJ_VALID is the obstacle relation of the batched rollout")
    if E != 128 and mode == "ones" and rel != 2:
        pytest.skip("the other widths are covered on the obstacle relation and the actor forms")
    torch.manual_seed(rel * 7 + len(mode))
    N, T, P, O = 5, 6, 8, 176
    R = N * T
    p = torch.randn(N, T, P, 4) * 10 + 20
    e = torch.randn(N, T, 1, 4) * 10 + 20
    o = torch.zeros(N, O, 4)
    kvalid = torch.randint(20, 100, (N,), dtype=torch.int32)
    for n in range(N):
        o[n, :kvalid[n], :2] = torch.randint(0, 40, (int(kvalid[n]), 2)).float()
    K = {0: P, 1: 1, 2: O}[rel]
    din = 8 if rel == 0 else 4
    adj = (torch.rand(N, T, P, K) < (0.15 if rel == 2 else 0.6)).float()
    if rel == 2:
        adj = adj * (torch.arange(O)[None, None, None, :] < kvalid[:, None, None, None])
        adj[0, 0, 0] = 0  # an all-zero row must stay zero
    W = (torch.randn(E, din) * 0.3).requires_grad_(True)
    b = (torch.randn(E) * 0.1).requires_grad_(True)
    # reference (rows in (n, t) order)
    q_full = {0: p, 1: e, 2: o[:, None].expand(N, T, O, 4)}[rel]
    if mode == "tensor":
        adj_ref = adj
    elif mode == "ones":
        adj_ref = torch.ones_like(adj)
    else:
        adj_ref = (torch.arange(O)[None, None, None, :] < kvalid[:, None, None, None]).float().expand(N, T, P, O)
    ref = _ref_msg_agg(p, q_full, e, adj_ref, W, b, rel == 0)
    g = torch.randn_like(ref)
    ref.backward(g)
    # device op on strided rows: tensors laid out (N, T+2, ...) and sliced, like replay-buffer slices
    def strided(x):
        big = torch.zeros(x.shape[0], x.shape[1] + 2, *x.shape[2:], device="cuda")
        big[:, 1:-1] = x.cuda()
        return big[:, 1:-1]
    Wd = W.detach().clone().cuda().requires_grad_(True)
    bd = b.detach().clone().cuda().requires_grad_(True)
    outs = []
    for t in range(T):  # one call per step on a strided slice [:, t] (rollout form)
        ps, es, as_ = strided(p)[:, t], strided(e)[:, t], strided(adj)[:, t]
        q = {0: ps, 1: es, 2: o.cuda()}[rel]
        am = {"tensor": ops.ADJ_TENSOR, "ones": ops.ADJ_ONES, "valid": ops.ADJ_VALID}[mode]
        outs.append(ops.msg_agg(ps, q, es.reshape(N, 4) if rel == 0 else None, as_, Wd, bd, am, kvalid.cuda(), 1))
    out_rollout = torch.stack(outs, 1)
    assert torch.allclose(out_rollout.cpu(), ref.detach(), rtol=2e-5, atol=2e-5)
    # training form: contiguous (n, t) rows, obstacles shared over T through q_div
    pr, er, ar = p.reshape(R, P, 4).cuda(), e.reshape(R, 1, 4).cuda(), adj.reshape(R, P, K).cuda()
    q = {0: pr, 1: er, 2: o.cuda()}[rel]
    am = {"tensor": ops.ADJ_TENSOR, "ones": ops.ADJ_ONES, "valid": ops.ADJ_VALID}[mode]
    out = ops.msg_agg(pr, q, er.reshape(R, 4) if rel == 0 else None, ar, Wd, bd, am, kvalid.cuda(), T if rel == 2 else 1)
    assert torch.allclose(out.reshape(N, T, P, E).cpu(), ref.detach(), rtol=2e-5, atol=2e-5)
    out.backward(g.reshape(R, P, E).cuda())
    assert torch.allclose(Wd.grad.cpu(), W.grad, rtol=2e-4, atol=2e-4 * W.grad.abs().max().item())
    assert torch.allclose(bd.grad.cpu(), b.grad, rtol=2e-4, atol=2e-4 * b.grad.abs().max().item())


def test_msg_agg_rejects_cpu_tensors():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.msg_agg(torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), None, torch.ones(1, 2, 2), torch.zeros(128, 4), torch.zeros(128))


@pytest.mark.parametrize("shape", [(7, 13, 4), (64, 150, 8)])
def test_gae_advnorm(shape):
    from distributed_multi_agent_reinforcement_learning_amd import ops
    N, T, P = shape
    torch.manual_seed(N)
    r = torch.randn(N, T, P)
    v = torch.randn(N, T + 1, P) * 2
    active = (torch.rand(N, T, P) < 0.9).float()
    adv_ref, vt_ref = mo.gae(r, v, active, 0.99, 0.95, True)
    adv, vt = ops.gae_advnorm(r.cuda(), v.cuda(), active.cuda(), 0.99, 0.95, True)
    assert torch.allclose(vt.cpu(), vt_ref, rtol=1e-5, atol=1e-5)
    assert torch.allclose(adv.cpu(), adv_ref, rtol=1e-4, atol=1e-4)   # north-star tolerance: advantages within 1e-4
    adv_ref, _ = mo.gae(r, v, active, 0.99, 0.95, False)
    adv, _ = ops.gae_advnorm(r.cuda(), v.cuda(), active.cuda(), 0.99, 0.95, False)
    assert torch.allclose(adv.cpu(), adv_ref, rtol=1e-5, atol=1e-5)


def test_categorical_sample_and_greedy():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(0)
    probs = torch.softmax(torch.randn(4096, 8, 9) * 2, -1).cuda()
    a, lp = ops.categorical_sample(probs, 3, 0, greedy=True)
    assert torch.equal(a.long(), probs.argmax(-1))
    a, lp = ops.categorical_sample(probs, 3, 0)
    dist = torch.distributions.Categorical(probs=probs)
    assert torch.allclose(lp, dist.log_prob(a.long()), rtol=1e-5, atol=1e-6)
    a2, _ = ops.categorical_sample(probs, 3, 0)
    assert torch.equal(a, a2)                      # counter based: reproducible
    a3, _ = ops.categorical_sample(probs, 3, a.numel())
    assert not torch.equal(a, a3)
    # frequencies follow the probabilities
    one = torch.softmax(torch.randn(9), 0)
    many = one[None].expand(200000, 9).contiguous().cuda()
    s, _ = ops.categorical_sample(many, 11, 0)
    freq = torch.bincount(s.long().cpu(), minlength=9).float() / 200000
    assert torch.allclose(freq, one, atol=5e-3)


@pytest.mark.parametrize("T,B", [(1, 64), (9, 40), (37, 333)])
def test_fused_gru_matches_torch_gru(T, B):
    """ops.gru (MFMA GEMMs + fused gate kernels) == torch.nn.GRU on the CPU (fp32), outputs and all gradients."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(T)
    ref = torch.nn.GRU(128, 128, 2)
    x = torch.randn(T, B, 128, requires_grad=True)
    h0 = torch.randn(2, B, 128, requires_grad=True)
    out_ref, hn_ref = ref(x, h0)
    g = torch.randn_like(out_ref)
    gh = torch.randn_like(hn_ref)
    (out_ref * g).sum().backward(retain_graph=True)
    (hn_ref * gh).sum().backward()
    dev = torch.nn.GRU(128, 128, 2).cuda()
    dev.load_state_dict(ref.state_dict())
    xd = x.detach().cuda().requires_grad_(True)
    hd = h0.detach().cuda().requires_grad_(True)
    out, hn = ops.gru(xd, hd, dev)
    assert torch.allclose(out.cpu(), out_ref, rtol=1e-5, atol=1e-5) and torch.allclose(hn.cpu(), hn_ref, rtol=1e-5, atol=1e-5)
    ((out * g.cuda()).sum() + (hn * gh.cuda()).sum()).backward()
    assert torch.allclose(xd.grad.cpu(), x.grad, rtol=1e-4, atol=1e-5)
    assert torch.allclose(hd.grad.cpu(), h0.grad, rtol=1e-4, atol=1e-5)
    for (k, p), (_, q) in zip(ref.named_parameters(), dev.named_parameters()):
        assert torch.allclose(q.grad.cpu(), p.grad, rtol=1e-4, atol=1e-4 * p.grad.abs().max().item()), k


@pytest.mark.gpu
@pytest.mark.parametrize("K,M,N,pad", [(492000, 384, 128, 0), (492000, 128, 384, 4), (487203, 128, 128, 0), (4099, 256, 128, 0),
                                       (4096, 128, 256, 8), (65537, 384, 128, 0)])
def test_wgrad_matches_f64_reference(K, M, N, pad):
    """ops.wgrad vs a float64 a^T b; tails, strided rows, accumulate, run-to-run determinism.  In the default split_bf16 mode every
    shape here is in SPLIT_WGRAD_SHAPES and runs csrc/sb_wgrad.hpp k_sb_wgrad (K % 16 tails); only MAPPO_WGRAD=fp32 sends them to
    csrc/mappo_ops.hip k_wgrad (K % 4 tails), which tests/test_wgrad_edges_gpu.py runs on purpose"""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    g = torch.Generator(device="cuda").manual_seed(K + M)
    a_full = torch.randn((K, M + pad), generator=g, device="cuda")
    b_full = torch.randn((K, N + pad), generator=g, device="cuda")
    a, b = a_full[:, :M], b_full[:, :N]
    ref = torch.zeros((M, N), dtype=torch.float64, device="cuda")
    for s in range(0, K, 65536):  # chunked: bounds the f64 copies
        ref += a[s:s + 65536].double().t() @ b[s:s + 65536].double()
    got = ops.wgrad(a, b)
    scale = float(K) ** 0.5
    assert (got.double() - ref).abs().max().item() < 2e-5 * scale  # fp32 accumulation of K unit-variance products
    again = ops.wgrad(a, b)
    assert torch.equal(got, again)
    base = torch.randn((M, N), generator=g, device="cuda")
    acc = base.clone()
    ops.wgrad(a, b, out=acc, accumulate=True)
    assert (acc.double() - (ref + base.double())).abs().max().item() < 2e-5 * scale + 1e-5


@pytest.mark.gpu
def test_wgrad_unsupported_shapes_use_blas():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    a = torch.randn((5000, 9), device="cuda")
    b = torch.randn((5000, 128), device="cuda")
    torch.testing.assert_close(ops.wgrad(a, b), a.t() @ b, rtol=1e-4, atol=1e-3)


@pytest.mark.gpu
def test_linear_autograd_matches_torch():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((8192, 3, 128), generator=g, device="cuda", requires_grad=True)
    W = torch.randn((128, 132), generator=g, device="cuda", requires_grad=True)
    bias = torch.randn((128,), generator=g, device="cuda", requires_grad=True)
    gout = torch.randn((8192, 3, 128), generator=g, device="cuda")
    y = ops.linear(x, W[:, 4:], bias)
    y.backward(gout)
    got = (y.detach().clone(), x.grad.clone(), W.grad.clone(), bias.grad.clone())
    x.grad = W.grad = bias.grad = None
    y2 = torch.nn.functional.linear(x, W[:, 4:], bias)
    y2.backward(gout)
    for u, v in zip(got, (y2.detach(), x.grad, W.grad, bias.grad)):
        torch.testing.assert_close(u, v, rtol=1e-4, atol=2e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1024, 4099, 32768])
def test_fused_gru_cell_matches_torch_gru(B):
    """rollout step (T = 1, no autograd): k_gru_cell == torch.nn.GRU on the CPU; rows that do not fill a 16-row tile"""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(B)
    ref = torch.nn.GRU(128, 128, 2)
    x = torch.randn(1, B, 128)
    h0 = torch.randn(2, B, 128)
    with torch.no_grad():
        out_ref, hn_ref = ref(x, h0)
        dev = torch.nn.GRU(128, 128, 2).cuda()
        dev.load_state_dict(ref.state_dict())
        out, hn = ops.gru(x.cuda(), h0.cuda(), dev)
        again, _ = ops.gru(x.cuda(), h0.cuda(), dev)
    assert torch.allclose(out.cpu(), out_ref, rtol=1e-5, atol=2e-6) and torch.allclose(hn.cpu(), hn_ref, rtol=1e-5, atol=2e-6)
    assert torch.equal(out, again)


@pytest.mark.gpu
def test_rollout_record_matches_tensor_copies():
    """k_rollout_record: rows of several dense tensors into [n, t] slots of (N, T, ...) buffers, int32 -> float32, return sum"""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    N, T, P = 37, 5, 8
    srcs = [torch.randn((N, P, 176), generator=g, device="cuda"), torch.randn((N, 1, 4), generator=g, device="cuda"),
            torch.randn((N, P), generator=g, device="cuda"), torch.randint(0, 9, (N, P), generator=g, device="cuda", dtype=torch.int32)]
    bufs = [torch.zeros((N + 3, T) + tuple(s.shape[1:]), device="cuda") for s in srcs]
    raw = torch.randn((N, P), generator=g, device="cuda")
    ret = torch.ones(N, device="cuda")
    ops.rollout_record([(s, b[2:2 + N, 3]) for s, b in zip(srcs, bufs)], raw, ret)
    for s, b in zip(srcs, bufs):
        want = torch.zeros_like(b)
        want[2:2 + N, 3] = s.float()
        assert torch.equal(b, want)
    torch.testing.assert_close(ret, 1.0 + raw.sum(-1), rtol=1e-6, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("full_addend", [False, True])
def test_linear_relu_autograd_matches_torch(full_addend):
    """ops.linear(..., relu=True): relu in the GEMM epilogue (1-D bias) or behind an accumulating GEMM (full addend)"""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.randn((8192, 128), generator=g, device="cuda", requires_grad=True)
    W = torch.randn((128, 128), generator=g, device="cuda", requires_grad=True)
    b = torch.randn((8192, 128) if full_addend else (128,), generator=g, device="cuda", requires_grad=True)
    gout = torch.randn((8192, 128), generator=g, device="cuda")
    y = ops.linear(x, W, b, relu=True)
    y.backward(gout)
    got = (y.detach().clone(), x.grad.clone(), W.grad.clone(), b.grad.clone())
    x.grad = W.grad = b.grad = None
    y2 = torch.relu(torch.nn.functional.linear(x, W) + b)
    y2.backward(gout)
    for u, v in zip(got, (y2.detach(), x.grad, W.grad, b.grad)):
        torch.testing.assert_close(u, v, rtol=1e-4, atol=2e-3)
    with torch.no_grad():
        out = torch.empty_like(y2)
        z = ops.linear(x, W, b, relu=True, out=out if full_addend else None)
        torch.testing.assert_close(z, y2.detach(), rtol=1e-5, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("value_clip", [True, False])
def test_ppo_loss_matches_autograd_oracle(value_clip):
    """k_ppo_loss (losses + gradients in one launch) vs the op-by-op torch graph of the oracle, including exact ties
    (ratio == 1 where logp_now == logp_old), ratios outside the clip range on both sides, masked elements"""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    g = torch.Generator().manual_seed(9)
    shape = (37, 150, 8)
    lp_old = -torch.rand(shape, generator=g) * 2
    lp_now = lp_old + torch.randn(shape, generator=g) * 0.05
    lp_now[::3] = lp_old[::3]                                  # exact ties of min(surr1, surr2)
    ent = torch.rand(shape, generator=g) * 2
    adv = torch.randn(shape, generator=g)
    active = (torch.rand(shape, generator=g) > 0.1).float()
    v_n = torch.randn((shape[0], shape[1] + 1, shape[2]), generator=g)
    v_now = v_n[:, :-1] + torch.randn(shape, generator=g) * 0.05
    v_tgt = torch.randn(shape, generator=g)
    eps, coef = 0.05, 0.05
    a = lp_now.clone().requires_grad_(True); e = ent.clone().requires_grad_(True); v = v_now.clone().requires_grad_(True)
    la, lc = mo.ppo_losses(a, e, v, {"a_logprob_n": lp_old, "active": active, "v_n": v_n}, adv, v_tgt, eps, coef, value_clip)
    (la + lc).backward()
    ad = lp_now.cuda().requires_grad_(True); ed = ent.cuda().requires_grad_(True); vd = v_now.cuda().requires_grad_(True)
    la2, lc2 = ops.ppo_loss(ad, ed, vd, lp_old.cuda(), adv.cuda(), active.cuda(), v_n[:, :-1].cuda() if value_clip else None, v_tgt.cuda(),
                            eps, coef, value_clip)
    (la2 + lc2).backward()
    torch.testing.assert_close(la2.cpu(), la.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(lc2.cpu(), lc.detach(), rtol=1e-5, atol=1e-6)
    for got, want in ((ad.grad, a.grad), (ed.grad, e.grad), (vd.grad, v.grad)):
        torch.testing.assert_close(got.cpu(), want, rtol=1e-5, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("value_clip", [True, False])
@pytest.mark.parametrize("A,sharp", [(9, 1.0), (9, 40.0), (5, 8.0), (16, 1.0), (1, 1.0)])
def test_ppo_loss_from_probabilities_equals_the_categorical_route(A, sharp, value_clip):
    """ops.ppo_loss_prob (Categorical(prob).log_prob / .entropy() inside the loss launch, gradient with respect to prob written out)
    against torch.distributions.Categorical + ops.ppo_loss on the same time-major head outputs: both losses and the gradients that
    reach the logits and the values.  sharp = 40 drives probabilities below finfo.eps and to 1 (probs_to_logits' clamp is active and
    blocks the gradient there); rows with an inactive mask, exact ratio ties and both clip sides as in the test above."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    g = torch.Generator(device="cuda").manual_seed(A + int(sharp))
    T, mb, P = 150, 23, 8
    logits = torch.randn((T, mb, P, A), generator=g, device="cuda") * sharp
    vals = torch.randn((T, mb, P, 1), generator=g, device="cuda")
    shape = (mb, T, P)
    action = torch.randint(0, A, shape, generator=g, device="cuda").float()
    with torch.no_grad():
        lp0 = torch.distributions.Categorical(torch.softmax(logits, -1).permute(1, 0, 2, 3)).log_prob(action)
    lp_old = lp0 + torch.randn(shape, generator=g, device="cuda") * 0.05
    lp_old[::3] = lp0[::3]                                     # exact ties of min(surr1, surr2)
    adv = torch.randn(shape, generator=g, device="cuda")
    active = (torch.rand(shape, generator=g, device="cuda") > 0.1).float()
    v_n = torch.randn((mb, T + 1, P), generator=g, device="cuda")
    v_tgt = torch.randn(shape, generator=g, device="cuda")
    eps, coef = 0.05, 0.05
    res = []
    for fused in (False, True):
        z, v = logits.clone().requires_grad_(True), vals.clone().requires_grad_(True)
        prob, values_now = torch.softmax(z, -1).permute(1, 0, 2, 3), v.permute(1, 0, 2, 3).squeeze(-1)
        v_old = v_n[:, :-1] if value_clip else None
        if fused:
            assert ops.ppo_loss_prob_ok(prob, values_now)
            la, lc = ops.ppo_loss_prob(prob, action, values_now, lp_old, adv, active, v_old, v_tgt, eps, coef, value_clip)
        else:
            dist = torch.distributions.Categorical(prob)
            la, lc = ops.ppo_loss(dist.log_prob(action), dist.entropy(), values_now, lp_old, adv, active, v_old, v_tgt, eps, coef, value_clip)
        (la + lc).backward()
        res.append((la.detach(), lc.detach(), z.grad, v.grad))
    torch.testing.assert_close(res[1][0], res[0][0], rtol=2e-6, atol=1e-7)
    torch.testing.assert_close(res[1][1], res[0][1], rtol=2e-6, atol=1e-7)
    scale = float(res[0][2].abs().max())
    assert float((res[1][2] - res[0][2]).abs().max()) <= 2e-6 * scale + 1e-12, (float((res[1][2] - res[0][2]).abs().max()), scale)
    assert torch.equal(res[1][3], res[0][3])


@pytest.mark.gpu
def test_msg_agg_empty_neighbourhoods():
    """Obstacle relation of an EMPTY map: kvalid == 0 (critic, rollout form) and an all-zero adjacency (actor) aggregate to
    exact zeros (F.normalize's 1e-12 clamp), with zero parameter gradients; mixed with rows that do have neighbours."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(3)
    N, P, O, E = 6, 8, 176, 128
    p = (torch.randn(N, P, 4) * 10 + 20).cuda()
    o = torch.zeros(N, O, 4).cuda()
    kvalid = torch.tensor([0, 0, 7, 0, 176, 1], dtype=torch.int32).cuda()
    for n in range(N):
        o[n, :int(kvalid[n]), :2] = torch.randint(0, 40, (int(kvalid[n]), 2)).float().cuda()
    W = (torch.randn(E, 4) * 0.3).cuda().requires_grad_(True)
    b = (torch.randn(E) * 0.1).cuda().requires_grad_(True)
    out = ops.msg_agg(p, o, None, None, W, b, ops.ADJ_VALID, kvalid, 1)
    empty = (kvalid == 0)
    assert torch.equal(out[empty], torch.zeros_like(out[empty])) and out[~empty].abs().sum() > 0
    ref = _ref_msg_agg(p[:, None].cpu(), o[:, None].cpu(), None,
                       (torch.arange(O)[None, None, None, :] < kvalid.cpu()[:, None, None, None]).float().expand(N, 1, P, O),
                       W.detach().cpu(), b.detach().cpu(), False)
    assert torch.allclose(out.cpu(), ref[:, 0], rtol=2e-5, atol=2e-5)
    out[empty].sum().backward()
    assert torch.equal(W.grad, torch.zeros_like(W.grad)) and torch.equal(b.grad, torch.zeros_like(b.grad))
    adj = torch.zeros(N, P, O).cuda()
    z = ops.msg_agg(p, o, None, adj, W, b, ops.ADJ_TENSOR, None, 1)
    assert torch.equal(z, torch.zeros_like(z))


@pytest.mark.parametrize("K,P", [(176, 8), (176, 4), (40, 15), (33, 8)])
def test_msg_agg_bit_packed_adjacency_equals_float_adjacency(K, P):
    """MO_ADJ_BITS (the env's o_adj_bits: bit j of row i = adj[i][j]) against MO_ADJ_TENSOR on the same 0/1 adjacency: the
    forward output and the bias gradient must be IDENTICAL bit for bit (a 0/1 weight multiplies by exactly 1; the L1 norm of a
    0/1 row is an exact integer sum; every accumulator adds in ascending j in both forms), the weight gradient to fp32
    reassociation (the packed form sums its neighbour-coordinate term edge by edge, the float form column by column);
    on strided rollout slices and on (n, t) training rows; pack / unpack round-trip."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(K + P)
    N, T, E = 6, 5, 128
    R = N * T
    p = (torch.randn(R, P, 4) * 10 + 20).cuda()
    o = torch.zeros(N, K, 4); o[:, :, :2] = torch.randint(0, 40, (N, K, 2)).float()
    o = o.cuda()
    adj = (torch.rand(R, P, K) < 0.12).float().cuda()
    adj[0, 0] = 0; adj[1, 1] = 1
    bits = ops.pack_adj_bits(adj)
    assert bits.shape == (R, P, ops.adj_row_words(K)) and bits.dtype == torch.int32
    assert torch.equal(ops.unpack_adj_bits(bits, K), adj)
    res = []
    for a, mode in ((adj, ops.ADJ_TENSOR), (bits, ops.ADJ_BITS)):
        W = (torch.randn(E, 4, generator=torch.Generator().manual_seed(1)) * 0.3).cuda().requires_grad_(True)
        b = (torch.randn(E, generator=torch.Generator().manual_seed(2)) * 0.1).cuda().requires_grad_(True)
        out = ops.msg_agg(p, o, None, a, W, b, mode, None, T)
        out.backward(torch.randn(R, P, E, generator=torch.Generator().manual_seed(3)).cuda())
        res.append((out.detach(), W.grad, b.grad))
    (out_t, dW_t, db_t), (out_b, dW_b, db_b) = res
    assert torch.equal(out_t, out_b) and torch.equal(db_t, db_b)
    assert (dW_t - dW_b).abs().max() <= 2e-6 * dW_t.abs().max(), ((dW_t - dW_b).abs().max(), dW_t.abs().max())
    # the three-relation encoder entry picks the packed mode from the dtype
    e = (torch.randn(R, 1, 4) * 10 + 20).cuda()
    adj_p = (torch.rand(R, P, P) < 0.5).float().cuda(); adj_e = (torch.rand(R, P, 1) < 0.5).float().cuda()
    Ws = [(torch.randn(E, d) * 0.3).cuda() for d in (8, 4, 4)]; bs = [torch.zeros(E).cuda() for _ in range(3)]
    args = lambda ao: (p, e, o, adj_p, adj_e, ao, Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2], False, None, T)
    with torch.no_grad():
        assert torch.equal(ops.msg_agg3(*args(adj)), ops.msg_agg3(*args(bits)))


@pytest.mark.parametrize("P,K,T", [(8, 176, 150), (4, 176, 16), (15, 97, 12), (8, 2, 9)])
def test_sorted_all_ones_relation_matches_dense_kernels(P, K, T):
    """The critic's all-ones obstacle relation in training (DHGN/mappo_parallel.py:64-65, 323-348): the sort +
    prefix-sum + binary-search kernels (O(log K) per pair) against the O(K) kernels and against the materialised fp64 reference:
    forward within 2e-5, dW / db within 2e-4 of the gradient scale (prefix sums reassociate the fp32 additions)."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(P * K + T)
    N, E = 7, 128
    R = N * T
    p = (torch.randn(R, P, 4) * 10 + 20).cuda()
    e = (torch.randn(R, 1, 4) * 10 + 20).cuda()
    o = torch.zeros(N, K, 4)
    kv = torch.randint(1, K + 1, (N,))
    for n in range(N):      # real obstacles [x, y, 0, 0], zero-padded slots: many equal d values (ties)
        o[n, :kv[n], :2] = torch.randint(0, 40, (int(kv[n]), 2)).float()
    o = o.cuda()
    adj_p = torch.ones(R, P, P).cuda(); adj_e = torch.ones(R, P, 1).cuda(); adj_o = torch.ones(R, P, K).cuda()
    g = torch.randn(R, P, 3, E, generator=torch.Generator().manual_seed(5)).cuda()
    res = {}
    for name, thr in (("sorted", 1), ("dense", 10 ** 9)):
        ops.SORTED_ONES_MIN_QDIV = thr
        Ws = [(torch.randn(E, d, generator=torch.Generator().manual_seed(10 + d)) * 0.3).cuda().requires_grad_(True) for d in (8, 4, 4)]
        bs = [(torch.randn(E, generator=torch.Generator().manual_seed(20 + k)) * 0.1).cuda().requires_grad_(True) for k in range(3)]
        out = ops.msg_agg3(p, e, o, adj_p, adj_e, adj_o, Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2], True, None, T)
        out.backward(g)
        res[name] = (out.detach(), Ws[2].grad.clone(), bs[2].grad.clone(), Ws[0].grad.clone())
    ops.SORTED_ONES_MIN_QDIV = 8
    so, de = res["sorted"], res["dense"]
    assert torch.equal(so[0][:, :, :2], de[0][:, :, :2]) and torch.equal(so[3], de[3])          # the other relations are untouched
    assert torch.allclose(so[0][:, :, 2], de[0][:, :, 2], rtol=2e-5, atol=2e-5)
    # fp64 reference of relation 2
    W64, b64 = res["dense"][1].new_tensor(0), None
    Wr = (torch.randn(E, 4, generator=torch.Generator().manual_seed(14)) * 0.3).double().requires_grad_(True)
    br = (torch.randn(E, generator=torch.Generator().manual_seed(22)) * 0.1).double().requires_grad_(True)
    rel = p.cpu().double().reshape(N, T, P, 1, 4) - o.cpu().double().reshape(N, 1, 1, K, 4)
    ref = torch.relu(torch.nn.functional.linear(rel, Wr, br)).mean(-2).reshape(R, P, E)
    ref.backward(g[:, :, 2].cpu().double())
    assert torch.allclose(so[0][:, :, 2].cpu().double(), ref.detach(), rtol=2e-5, atol=2e-5)
    for mine, want in ((so[1], Wr.grad), (so[2], br.grad)):
        assert (mine.cpu().double() - want).abs().max() <= 2e-4 * want.abs().max(), ((mine.cpu().double() - want).abs().max(), want.abs().max())


@pytest.mark.parametrize("critic", [False, True])
def test_fused_three_relation_launch_equals_three_launches(critic):
    """dhgn_msg_agg3_fwd (one launch for the defender / evader / obstacle relation of DHGN.encoder) against three
    dhgn_msg_agg_fwd launches: bit-identical, actor adjacency (float and packed) and the critic's rollout form (ADJ_VALID)."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(3 + critic)
    R, P, K, E = 300, 8, 176, 128
    p = (torch.randn(R, P, 4) * 10 + 20).cuda(); e = (torch.randn(R, 1, 4) * 10 + 20).cuda()
    o = torch.zeros(R, K, 4); o[:, :, :2] = torch.randint(0, 40, (R, K, 2)).float(); o = o.cuda()
    kv = torch.randint(0, K + 1, (R,), dtype=torch.int32).cuda()
    adj_p = (torch.rand(R, P, P) < 0.5).float().cuda(); adj_e = (torch.rand(R, P, 1) < 0.5).float().cuda()
    adj_o = (torch.rand(R, P, K) < 0.1).float().cuda()
    Ws = [(torch.randn(E, d) * 0.3).cuda() for d in (8, 4, 4)]; bs = [(torch.randn(E) * 0.1).cuda() for _ in range(3)]
    with torch.no_grad():
        for ao in ((adj_o, ops.pack_adj_bits(adj_o)) if not critic else (adj_o,)):
            fused = ops.msg_agg3(p, e, o, adj_p, adj_e, ao, Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2], critic, kv if critic else None, 1)
            mode = ops.ADJ_ONES if critic else ops.ADJ_TENSOR
            mode_o = ops.ADJ_VALID if critic else (ops.ADJ_BITS if ao.dtype == torch.int32 else ops.ADJ_TENSOR)
            r0 = ops.msg_agg(p, p, e.reshape(R, 4), adj_p, Ws[0], bs[0], mode)
            r1 = ops.msg_agg(p, e, None, adj_e, Ws[1], bs[1], mode)
            r2 = ops.msg_agg(p, o, None, ao, Ws[2], bs[2], mode_o, kv)
            assert torch.equal(fused, torch.stack((r0, r1, r2), 2))


@pytest.mark.parametrize("P,K,q_div,valid", [(8, 176, 1, True), (4, 176, 1, True), (8, 176, 5, False), (15, 40, 1, True), (8, 33, 1, False)])
def test_actor_critic_pair_launch_equals_two_launches(P, K, q_div, valid):
    """dhgn_msg_agg3_pair_fwd (actor + critic of a rollout tick from one pass over the shared messages) against
    dhgn_msg_agg3_fwd once per network: bit-identical, float and packed obstacle adjacency, with and without kvalid."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(11 + P + K)
    Rq, E = 60, 128
    R = Rq * q_div
    p = (torch.randn(R, P, 4) * 10 + 20).cuda(); e = (torch.randn(R, 1, 4) * 10 + 20).cuda()
    o = torch.zeros(Rq, K, 4); o[:, :, :2] = torch.randint(0, 40, (Rq, K, 2)).float(); o = o.cuda()
    kv = torch.randint(0, K + 1, (Rq,), dtype=torch.int32).cuda()
    kv[0] = 0; kv[1] = K
    adj_p = (torch.rand(R, P, P) < 0.5).float().cuda(); adj_e = (torch.rand(R, P, 1) < 0.5).float().cuda()
    adj_o = (torch.rand(R, P, K) < 0.1).float().cuda()
    adj_o[2] = 0.0                                    # a row no agent sees anything in
    adj_o[3, :, K - 1] = 1.0                          # an entry beyond most rows' kvalid
    Ws = [(torch.randn(E, d) * 0.3).cuda() for d in (8, 4, 4)]; bs = [(torch.randn(E) * 0.1).cuda() for _ in range(3)]
    wb = (Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2])
    with torch.no_grad():
        for ao in (adj_o, ops.pack_adj_bits(adj_o)):
            pair = ops.msg_agg3_pair(p, e, o, adj_p, adj_e, ao, *wb, kv if valid else None, q_div)
            actor = ops.msg_agg3(p, e, o, adj_p, adj_e, ao, *wb, False, None, q_div)
            critic = ops.msg_agg3(p, e, o, adj_p, adj_e, ao, *wb, True, kv if valid else None, q_div)
            assert torch.equal(pair[0], actor)
            # the same launch can leave the semantic layer's position part bp + Wp p in a (2, R, P, E) buffer
            Wsem = (torch.randn(E, 4 + 3 * E) * 0.1).cuda(); bsem = (torch.randn(E) * 0.1).cuda()
            h0 = torch.full((2, R, P, E), float("nan"), device="cuda")
            pair2 = ops.msg_agg3_pair(p, e, o, adj_p, adj_e, ao, *wb, kv if valid else None, q_div, pos=(Wsem[:, :4], bsem, h0))
            assert torch.equal(pair2, pair) and torch.equal(h0[0], h0[1])
            assert torch.allclose(h0[0], torch.nn.functional.linear(p, Wsem[:, :4], bsem), rtol=1e-5, atol=1e-5)
            if q_div >= ops.SORTED_ONES_MIN_QDIV and not valid:   # the single-network call took the sorted kernels (reassociated sums)
                assert torch.allclose(pair[1], critic, rtol=2e-5, atol=2e-5)
            else:
                assert torch.equal(pair[1], critic)


@pytest.mark.parametrize("P,K,T,packed", [(8, 176, 30, True), (4, 176, 12, True), (8, 40, 9, False), (15, 176, 10, True)])
def test_actor_critic_pair_training_form_equals_two_autograd_nodes(P, K, T, packed):
    """The update's paired message pass (ops.msg_agg3_pair_train: one forward launch for the actor's three relations + the critic's
    relations 0 and 1, the sorted all-ones kernels for the critic's obstacle relation, relations 0 and 1 of BOTH networks in one backward
    pass each) against two msg_agg3 autograd nodes: outputs bit-identical, the summed weight gradients equal to fp32 reassociation."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(5 + P + K)
    n, E = 6, 128
    R = n * T
    p = (torch.randn(R, P, 4) * 10 + 20).cuda(); e = (torch.randn(R, 1, 4) * 10 + 20).cuda()
    o = torch.zeros(n, K, 4); o[:, :, :2] = torch.randint(0, 40, (n, K, 2)).float(); o = o.cuda()
    adj_p = (torch.rand(R, P, P) < 0.5).float().cuda(); adj_e = (torch.rand(R, P, 1) < 0.5).float().cuda()
    adj_o = (torch.rand(R, P, K) < 0.1).float().cuda()
    adj_p[1] = 0.0; adj_e[2] = 0.0; adj_o[3] = 0.0
    ao = ops.pack_adj_bits(adj_o) if packed else adj_o
    ga, gc = torch.randn(R, P, 3, E, device="cuda"), torch.randn(R, P, 3, E, device="cuda")

    def params():
        torch.manual_seed(99)
        Ws = [(torch.randn(E, d) * 0.3).cuda().requires_grad_(True) for d in (8, 4, 4)]
        bs = [(torch.randn(E) * 0.1).cuda().requires_grad_(True) for _ in range(3)]
        return (Ws[0], bs[0], Ws[1], bs[1], Ws[2], bs[2])
    assert ops.msg_agg3_pair_train_ok(p, o, params()[4], T)
    wb = params()
    ma, mc = ops.msg_agg3_pair_train(p, e, o, adj_p, adj_e, ao, *wb, T)
    ((ma * ga).sum() + (mc * gc).sum()).backward()
    wr = params()
    ra = ops.msg_agg3(p, e, o, adj_p, adj_e, ao, *wr, False, None, T)
    rc = ops.msg_agg3(p, e, o, adj_p, adj_e, ao, *wr, True, None, T)
    ((ra * ga).sum() + (rc * gc).sum()).backward()
    assert torch.equal(ma, ra) and torch.equal(mc, rc)
    for a, b in zip(wb, wr):
        assert torch.allclose(a.grad, b.grad, rtol=2e-4, atol=2e-4 * float(b.grad.abs().max())), (a.shape, (a.grad - b.grad).abs().max())


@pytest.mark.parametrize("A,H", [(1, 128), (9, 128), (16, 1000)])
def test_spectral_norm_weight_matches_torch_hook(A, H):
    """spectral_norm_weight (one launch) against torch.nn.utils.spectral_norm's hook on the CPU in float64: the same u, v
    trajectory over several forwards (in-place power iteration, also under no_grad) and the same weight / sigma; the
    eval-mode form leaves u, v untouched."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(A * 1000 + H)
    lin = torch.nn.utils.spectral_norm(torch.nn.Linear(H, A)).double()
    W = lin.weight_orig.detach().float().cuda().contiguous()
    u, v = lin.weight_u.detach().float().cuda().clone(), lin.weight_v.detach().float().cuda().clone()
    x = torch.randn(5, H, dtype=torch.float64)
    with torch.no_grad():
        for it in range(4):
            lin(x)                                     # hook: power iteration in place, weight = W / sigma
            w = ops.spectral_norm_weight(W, u, v, 1e-12, 1)
            assert torch.allclose(w.cpu().double(), lin.weight.detach(), rtol=2e-5, atol=1e-7), it
            assert torch.allclose(u.cpu().double(), lin.weight_u, rtol=0, atol=2e-5) and torch.allclose(v.cpu().double(), lin.weight_v, rtol=0, atol=2e-5)
        lin.eval()
        u0, v0 = u.clone(), v.clone()
        lin(x)
        w = ops.spectral_norm_weight(W, u, v, 1e-12, 0)
        assert torch.equal(u, u0) and torch.equal(v, v0)
        assert torch.allclose(w.cpu().double(), lin.weight.detach(), rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("R,n_in,n_out", [(492000, 128, 9), (492000, 128, 1), (492000, 4, 128), (5003, 128, 16), (4100, 8, 64)])
def test_skinny_linear_autograd_matches_torch(R, n_in, n_out):
    """ops.linear_skinny (weight / bias gradient in the streaming kernel k_wgrad_skinny) against torch.nn.functional.linear with
    float64 gradients as the reference; permuted input, a column slice of a larger weight, run-to-run determinism."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    g = torch.Generator(device="cuda").manual_seed(R + n_in)
    T = 4 if R % 4 == 0 else 1
    x = torch.randn((T, R // T, n_in), generator=g, device="cuda").permute(1, 0, 2)       # non-contiguous rows, like the GRU features
    Wfull = torch.randn((n_out, n_in + 3), generator=g, device="cuda", requires_grad=True)
    bias = torch.randn((n_out,), generator=g, device="cuda", requires_grad=True)
    xg = x.clone().requires_grad_(n_in > 16)
    gout = torch.randn((R // T, T, n_out), generator=g, device="cuda")
    y = ops.linear_skinny(xg, Wfull[:, 3:], bias)
    y.backward(gout)
    got = (y.detach().clone(), Wfull.grad.clone(), bias.grad.clone(), None if xg.grad is None else xg.grad.clone())
    Wfull.grad = bias.grad = None
    y1 = ops.linear_skinny(xg, Wfull[:, 3:], bias); y1.backward(gout)
    assert torch.equal(Wfull.grad, got[1]) and torch.equal(bias.grad, got[2])
    x64, W64, b64 = x.double(), Wfull.detach().double().requires_grad_(True), bias.detach().double().requires_grad_(True)
    x64.requires_grad_(n_in > 16)
    y2 = torch.nn.functional.linear(x64, W64[:, 3:], b64)
    y2.backward(gout.double())
    scale = float(R) ** 0.5
    assert (got[0].double() - y2.detach()).abs().max() < 1e-4 * (1 + n_in ** 0.5)
    assert (got[1].double() - W64.grad).abs().max() < 2e-5 * scale
    assert (got[2].double() - b64.grad).abs().max() < 2e-5 * scale
    if got[3] is not None:
        assert (got[3].double() - x64.grad).abs().max() < 1e-4 * (1 + n_out ** 0.5)


@pytest.mark.parametrize("R,F", [(1476000, 128), (4099, 128), (5000, 64), (4096, 256), (300, 128), (5000, 36)])
def test_relu_backward_with_bias_gradient_matches_torch(R, F):
    """relu_bwd_colsum (one pass) against aten::threshold_backward (bit-identical) and a float64 column sum; shapes the kernel
    does not cover take the torch ops (same results)."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    g = torch.Generator(device="cuda").manual_seed(R + F)
    gout = torch.randn((R, F), generator=g, device="cuda")
    y = torch.relu(torch.randn((R, F), generator=g, device="cuda"))
    gin, cs = ops.relu_bwd_colsum(gout, y)
    want = torch.ops.aten.threshold_backward(gout, y, 0.0)
    assert torch.equal(gin, want)
    ref = torch.zeros(F, dtype=torch.float64, device="cuda")
    for s0 in range(0, R, 262144):
        ref += want[s0:s0 + 262144].double().sum(0)
    assert (cs.double() - ref).abs().max().item() < 2e-5 * float(R) ** 0.5
    assert torch.equal(ops.relu_bwd_colsum(gout, y)[1], cs)


@pytest.mark.parametrize("P,T,relu", [(8, 1, False), (8, 7, True), (4, 5, False), (15, 3, True)])
def test_fcra_neighbour_mean_matches_torch(P, T, relu):
    """fcra_mean (DHGN.fcra's matmul(normalize(adj, p=1), hist), actor and critic weights, optional bias + ReLU, strided history
    slices read in place) against the torch ops in float64."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(P * 10 + T)
    n, E, d = 6, 128, 2
    R = n * T
    buf = torch.randn(n, T + d, P, E, device="cuda")
    z = buf[:, 1:1 + T]                                             # (n, T, P, E) slice, not contiguous
    adj = (torch.rand(R, P, P, device="cuda") < 0.4).float()
    adj[0] = 0.0                                                    # isolated agents: normalize(0) = 0
    adj[1] = torch.rand(P, P, device="cuda") - 0.3                  # general (signed) weights
    bias = torch.randn(E, device="cuda") if relu else None
    z64 = z.reshape(R, P, E).double()

    def ref(a):
        y = torch.matmul(torch.nn.functional.normalize(a.double(), p=1, dim=-1), z64)
        if bias is not None:
            y = y + bias.double()
        return torch.relu(y) if relu else y
    got_a = ops.fcra_mean(z_actor=z if T > 1 else z.reshape(R, P, E).contiguous(), adj=adj, bias=bias, relu=relu)
    got_c = ops.fcra_mean(z_critic=z if T > 1 else z.reshape(R, P, E).contiguous(), bias=bias, relu=relu)
    both = ops.fcra_mean(z_actor=z if T > 1 else z.reshape(R, P, E).contiguous(), z_critic=z if T > 1 else z.reshape(R, P, E).contiguous(),
                         adj=adj, bias=bias, relu=relu)
    assert torch.allclose(got_a.double(), ref(adj), rtol=1e-5, atol=1e-5)
    assert torch.allclose(got_c.double(), ref(torch.ones_like(adj)), rtol=1e-5, atol=1e-5)
    assert torch.equal(both[0], got_a) and torch.equal(both[1], got_c)


@pytest.mark.parametrize("P,E", [(8, 128), (5, 128), (3, 128), (1, 128), (8, 256)])
def test_fcra_neighbour_mean_at_size_into_a_column_block(P, E):
    """fcra_mean at 6 150 rows (one pass of either grid: 1 538 of up to 4 096 workgroups of the wave-per-row kernel, 6 150 of up to
    16 384 of the lane-per-feature kernel; tests/test_nbr_mean_gpu.py passes both grids), odd agent counts, and the result written
    into the left half of an [agg | h] operand (row stride 2E): the wave-per-row kernel (E = 128, P <= 8) and the lane-per-feature
    kernel (other widths) against f64; the right half of the operand stays untouched."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(P + E)
    n, T, d = 150, 41, 3
    R = n * T
    buf = torch.randn(n, T + d, P, E, device="cuda")
    z = buf[:, 2:2 + T]
    adj = (torch.rand(R, P, P, device="cuda") < 0.5).float()
    bias = torch.randn(E, device="cuda")
    z64 = z.reshape(R, P, E).double()
    cat = torch.full((2, R, P, 2 * E), 7.0, device="cuda")
    ops.fcra_mean(z_actor=z, z_critic=z, adj=adj, bias=bias, relu=True, out=cat[..., :E])
    for k, a in enumerate((adj, torch.ones_like(adj))):
        want = torch.relu(torch.matmul(torch.nn.functional.normalize(a.double(), p=1, dim=-1), z64) + bias.double())
        assert torch.allclose(cat[k, ..., :E].double(), want, rtol=1e-5, atol=1e-5)
    assert bool((cat[..., E:] == 7.0).all())


@pytest.mark.parametrize("T,n,P", [(37, 20, 8), (150, 7, 4), (5, 6, 8)])
def test_gru_reads_encoder_row_order_in_place(T, n, P):
    """ops.gru(agents = P): the first layer's input given as the encoder's (episode, step, agent) rows equals the time-major
    call on the permuted copy -- outputs bit for bit, gradients to fp32 reordering (T = 5 takes the per-step path, which
    gathers once)."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(T + n)
    B, E = n * P, 128
    g = torch.nn.GRU(E, E, 2).cuda()
    emb = torch.randn(n * T * P, E, device="cuda")
    h0 = torch.zeros(2, B, E, device="cuda")
    gout = torch.randn(T, B, E, device="cuda")
    res = []
    for agents in (0, P):
        x = emb.clone().requires_grad_(True)
        g.zero_grad()
        if agents:
            out, _ = ops.gru(x, h0, g, agents=P, steps=T)
        else:
            out, _ = ops.gru(x.reshape(n, T, P, E).permute(1, 0, 2, 3).reshape(T, B, E), h0, g)
        (out * gout).sum().backward()
        res.append((out.detach().clone(), x.grad.clone(), [p.grad.clone() for p in g.parameters()]))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.allclose(res[0][1], res[1][1], rtol=1e-5, atol=1e-6)
    for a, b in zip(res[0][2], res[1][2]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4 * a.abs().max().item())


@pytest.mark.parametrize("R,A", [(32768, 9), (5, 9), (1001, 1), (4096, 16)])
def test_rollout_heads_match_the_separate_kernels(R, A):
    """head_linear == F.linear, and head_sample (action head + softmax + sample + log-prob + counter update in one launch)
    against softmax -> categorical_sample on the same Philox stream: identical actions except where a uniform draw falls within
    rounding of a bin edge, log-probabilities to 1e-5, the counter advanced by R, greedy = argmax."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(R + A)
    feat = torch.randn(R, 128, device="cuda")
    W = torch.randn(A, 128, device="cuda") * 0.2
    b = torch.randn(A, device="cuda") * 0.1
    with torch.no_grad():
        y = ops.head_linear(feat, W, b)
        assert torch.allclose(y, torch.nn.functional.linear(feat, W, b), rtol=1e-5, atol=1e-5)
        out_v = torch.zeros(R, A, device="cuda")
        assert ops.head_linear(feat, W, b, out=out_v).data_ptr() == out_v.data_ptr() and torch.equal(out_v, y)
        if A == 1:
            return
        c0 = 12345 + (3 << 40)
        counter = torch.full((1,), c0, dtype=torch.int64, device="cuda")
        ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
        a_n, logp = torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, device="cuda")
        ops.head_sample(feat, W, b, 77, counter, ticket, (a_n, logp))
        assert int(counter.item()) == c0 + R and int(ticket.item()) == 0
        prob = torch.softmax(torch.nn.functional.linear(feat, W, b), dim=-1)
        counter2 = torch.full((1,), c0, dtype=torch.int64, device="cuda")
        a_ref, logp_ref = ops.categorical_sample(prob, 77, 0, counter=counter2)
        same = (a_n == a_ref)
        assert same.float().mean().item() >= 0.999
        assert torch.allclose(logp[same], logp_ref[same], rtol=1e-5, atol=1e-5)
        assert torch.allclose(logp, torch.log(prob.gather(1, a_n.long()[:, None]).squeeze(1)), rtol=1e-4, atol=1e-5)
        assert R < 1000 or a_n.unique().numel() == A
        ops.head_sample(feat, W, b, 77, counter, ticket, (a_n, logp), greedy=True)
        assert torch.equal(a_n.long(), prob.argmax(-1)) or (a_n.long() != prob.argmax(-1)).float().mean().item() < 1e-3


@pytest.mark.parametrize("M,N,K", [(61500 * 8, 128, 256), (1000, 128, 128), (7, 128, 384)])
@pytest.mark.parametrize("bias,relu,addend", [(True, True, False), (True, False, False), (False, False, True), (False, True, False), (True, True, True)])
def test_gemm_nt_strided_output_and_epilogues_match_torch(M, N, K, bias, relu, addend):
    """ops.gemm_nt (include/mappo_gemm.h, hipBLASLt): out = act(x W^T + bias + addend) written into a column block of a wider
    matrix, x itself a column block -- against F.linear in fp32 (GEMM reordering tolerance); the other columns stay untouched."""
    import torch.nn.functional as F
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(K + N)
    if M > 100000:
        M = M // 4
    xw = torch.randn(M, K + 128, device="cuda")
    x = xw[:, 128:]                                   # column block, row stride K + 128
    W = torch.randn(N, K, device="cuda") * 0.1
    b = torch.randn(N, device="cuda") if bias else None
    wide = torch.full((M, 2 * N), 7.0, device="cuda")
    out = wide[:, N:]
    add = None
    if addend:
        out.copy_(torch.randn(M, N, device="cuda"))
        add = out                                     # accumulate in place (beta = 1)
    ref = F.linear(x, W, b)
    if addend:
        ref = ref + out
    if relu:
        ref = torch.relu(ref)
    got = ops.gemm_nt(x, W, b, relu, out=out, addend=add)
    assert got.data_ptr() == out.data_ptr()
    assert torch.allclose(got, ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))
    assert bool((wide[:, :N] == 7.0).all())
    dense = ops.gemm_nt(x.contiguous(), W, b, relu) if not addend else None
    if dense is not None:
        assert torch.allclose(dense, ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))


@pytest.mark.parametrize("T,n,P,agents", [(37, 20, 8, True), (150, 7, 4, True), (21, 13, 8, False)])
def test_gru_multi_equals_separate_calls(T, n, P, agents):
    """ops.gru_multi: actor's and critic's GRU (own weights, own inputs) with the recurrences of both in one launch per layer and
    direction -- outputs and every gradient bit-identical to two ops.gru calls (the same kernels on the same rows)."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(T * 7 + n)
    B, E = n * P, 128
    mods = [torch.nn.GRU(E, E, 2).cuda() for _ in range(2)]
    embs = [torch.randn(n * T * P, E, device="cuda") for _ in range(2)]
    gouts = [torch.randn(T, B, E, device="cuda") for _ in range(2)]
    h0s = [torch.zeros(2, B, E, device="cuda") for _ in range(2)]
    res = []
    for multi in (False, True):
        xs = [e.clone().requires_grad_(True) for e in embs]
        for m in mods:
            m.zero_grad()
        ins = xs if agents else [x.reshape(n, T, P, E).permute(1, 0, 2, 3).reshape(T, B, E) for x in xs]
        kw = dict(agents=P, steps=T) if agents else {}
        if multi:
            outs = ops.gru_multi(ins, h0s, mods, **kw)
        else:
            outs = [ops.gru(i, h, m, **kw)[0] for i, h, m in zip(ins, h0s, mods)]
        sum((o * g).sum() for o, g in zip(outs, gouts)).backward()
        res.append(([o.detach().clone() for o in outs], [x.grad.clone() for x in xs], [p.grad.clone() for m in mods for p in m.parameters()]))
    for a, b in zip(res[0][0] + res[0][1] + res[0][2], res[1][0] + res[1][1] + res[1][2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B", [32768, 4096, 1030, 17])
def test_split_bf16_cell_is_as_accurate_as_the_fp32_cell(B):
    """gru_cell_split_fwd_multi (k_gru_cell_sb): the rollout's GRU step from exact three-way bf16 splits of the fp32 operands, six bf16
    MFMAs per product, fp32 accumulation.  Its error against an f64 torch.nn.GRU is the fp32-MFMA kernel's (a few 1e-7: summation
    order), for two layers, both networks in one launch, row counts with a ragged last tile; the states it reads are left untouched
    and an in-place call is refused."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(B)
    mods = [torch.nn.GRU(128, 128, 2).cuda() for _ in range(2)]
    xs = [torch.randn(B, 128, device="cuda") for _ in range(2)]
    h0 = [torch.randn(2, B, 128, device="cuda") * 0.7 for _ in range(2)]
    keep = [h.clone() for h in h0]
    errs = {}
    old = ops.CELL_MODE
    try:
        with torch.no_grad():
            ref = []
            for x, h, m in zip(xs, h0, mods):
                m64 = torch.nn.GRU(128, 128, 2).cuda().double()
                m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
                ref.append(m64(x.double().unsqueeze(0), h.double())[1])
            for mode in ("fp32", "split_bf16"):
                ops.set_cell_mode(mode)
                outs = [torch.full_like(h, float("nan")) for h in h0]
                top = ops.gru_step_multi(xs, h0, mods, hiddens_out=outs)
                errs[mode] = max(float((o.double() - r).abs().max()) for o, r in zip(outs, ref))
                assert all(t.data_ptr() == o[-1].data_ptr() for t, o in zip(top, outs))
                assert all(torch.equal(h, k) for h, k in zip(h0, keep))
            if B >= ops.FUSED_CELL_MIN_ROWS:
                ops.set_cell_mode("split_bf16")
                L = ops.load_library()
                import ctypes as C
                arr = (ops.GruCellNet * 1)()
                m = mods[0]
                arr[0].x, arr[0].h_prev, arr[0].h_out = xs[0].data_ptr(), h0[0][0].data_ptr(), h0[0][0].data_ptr()
                arr[0].w_ih, arr[0].w_hh, arr[0].b_ih, arr[0].b_hh = (getattr(m, n).data_ptr() for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
                assert L.gru_cell_split_fwd_multi(1, C.cast(arr, C.c_void_p), B, 128, None) != 0      # in place: refused
    finally:
        ops.set_cell_mode(old)
    assert errs["fp32"] < 3e-6 and errs["split_bf16"] < 3e-6, errs
    assert errs["split_bf16"] <= 2.0 * errs["fp32"] + 2e-7, errs


def test_gru_multi_grouped_ragged_equals_separate_calls():
    """ops.gru_multi(grouped=True): the recurrences of several mini-batches' actor and critic layers -- different numbers of
    sequences, two of the inputs sharing one module's weights -- in one launch per layer and direction: outputs and every
    gradient bit-identical to one ops.gru call per input."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(5)
    T, P, E = 9, 8, 128
    ns = [5, 5, 3, 3, 1, 1]                                   # episodes per input (the last mini-batch is smaller)
    mods = [torch.nn.GRU(E, E, 2).cuda() for _ in range(2)]
    which = [0, 1, 0, 1, 0, 1]
    embs = [torch.randn(n * T * P, E, device="cuda") for n in ns]
    gouts = [torch.randn(T, n * P, E, device="cuda") for n in ns]
    h0s = [torch.zeros(2, n * P, E, device="cuda") for n in ns]
    res = []
    for multi in (False, True, "zero state"):
        xs = [e.clone().requires_grad_(True) for e in embs]
        for m in mods:
            m.zero_grad()
        ms = [mods[w] for w in which]
        if multi:   # ("zero state": the caller vouches for h0 == 0 and the first step's term of dW_hh is not computed: adding exact zeros or not)
            outs = ops.gru_multi(xs, h0s, ms, agents=P, steps=T, grouped=True, zero_state=multi == "zero state")
        else:
            outs = [ops.gru(x, h, m, agents=P, steps=T)[0] for x, h, m in zip(xs, h0s, ms)]
        # per input its own backward root, like the mini-batches' losses
        torch.autograd.backward([(o * g).sum() for o, g in zip(outs, gouts)])
        res.append(([o.detach().clone() for o in outs], [x.grad.clone() for x in xs], [p.grad.clone() for m in mods for p in m.parameters()]))
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert torch.equal(a, b)
    for a, b in zip(res[0][2], res[1][2]):                    # three inputs accumulate into one module's gradient: order of the sum
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    for a, b in zip(res[1][0] + res[1][1] + res[1][2], res[2][0] + res[2][1] + res[2][2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("T,B,agents", [(2, 17, 0), (3, 48, 3)])
def test_gru_matches_the_single_net_abi(T, B, agents):
    """ops.gru (one layer, the fp32 recurrence) against the documented single-network entry points gru_seq_fwd / gru_seq_bwd called
    directly: time-major rows with the dnr form, the encoder's row order (16 episodes x 3 agents) with the dgh form;
    the weight and input gradients built from the returned dgi as ops.py builds them.  The same launches on the same operands: out and
    every gradient bit for bit."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(10 * T + agents)
    H = 128
    g = torch.nn.GRU(H, H, 1).cuda()
    x = torch.randn((T * B, H) if agents else (T, B, H), device="cuda", requires_grad=True)
    h0 = torch.randn(1, B, H, device="cuda", requires_grad=True)
    gout = torch.randn(T, B, H, device="cuda")
    modes = ops.matmul_modes()
    ops.SEQ_MODE = "fp32"
    try:
        out, h_n = ops.gru(x, h0, g, agents=agents, steps=T if agents else None)
        (out * gout).sum().backward()
        L, st, p = ops.load_library(), ops._stream(), ops._ptr

        def new(*shape):
            return torch.empty(shape, device="cuda")
        with torch.no_grad():
            w_ih, w_hh, b_ih, b_hh = g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0
            x2 = x.reshape(T * B, H)
            gi = ops.gru_input_projection(x2, w_ih, b_ih)
            out2, save = new(T, B, H), new(L.gru_seq_save_elems(T, B))
            assert L.gru_seq_fwd(T, B, H, p(gi), p(w_hh), p(b_hh), p(h0[0]), p(out2), p(save), agents, st) == 0
            dgi, dh0, db_ih, db_hh = new(T * B, 3 * H), new(B, H), new(3 * H), new(3 * H)
            dgh, dnr = (new(T, B, 3 * H), None) if agents else (None, new(T, B, H))
            ws = torch.empty(L.gru_seq_bwd_workspace(B), dtype=torch.uint8, device="cuda")
            assert L.gru_seq_bwd(T, B, H, p(gout), p(save), p(out2), p(h0[0]), p(w_hh), p(dgi), p(dgh), p(dnr), p(dh0), p(db_ih), p(db_hh), agents,
                                 p(ws), st) == 0
            dw_hh = ops._gru_dw_hh(dgi, dgh, dnr, out2, h0[0], T, B, H)
            dw_ih = ops.wgrad(dgi, x2)
            dx = ops.input_grad(dgi, w_ih).reshape(x.shape)
    finally:
        ops.restore_matmul_modes(modes)
    assert torch.equal(h_n, out[-1:])
    for name, got, want in (("out", out, out2), ("x.grad", x.grad, dx), ("h0.grad", h0.grad[0], dh0), ("w_ih.grad", w_ih.grad, dw_ih),
                            ("w_hh.grad", w_hh.grad, dw_hh), ("b_ih.grad", b_ih.grad, db_ih), ("b_hh.grad", b_hh.grad, db_hh)):
        assert got.shape == want.shape and torch.equal(got, want), name


@pytest.mark.parametrize("B", [32768, 4096, 1030])
def test_gru_step_multi_equals_separate_cells(B):
    """ops.gru_step_multi: actor's and critic's rollout GRU step, the two cells of every layer in one launch, hidden states updated in
    place -- bit-identical to ops.gru per module (the same kernel on the same tiles)."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(B)
    mods = [torch.nn.GRU(128, 128, 2).cuda() for _ in range(2)]
    xs = [torch.randn(B, 128, device="cuda") for _ in range(2)]
    h0 = [torch.randn(2, B, 128, device="cuda") for _ in range(2)]
    with torch.no_grad():
        ref = [ops.gru(x.unsqueeze(0), h.clone(), m) for x, h, m in zip(xs, h0, mods)]
        hs = [h.clone() for h in h0]
        outs = ops.gru_step_multi(xs, hs, mods)
    for k in range(2):
        assert torch.equal(outs[k], ref[k][0][0]) and torch.equal(hs[k], ref[k][1])
        assert outs[k].data_ptr() == hs[k][1].data_ptr()


@pytest.mark.parametrize("N,K,R", [(128, 128, 196608), (128, 256, 65536), (128, 384, 65536), (128, 128, 37), (128, 384, 1), (256, 128, 65536 + 5),
                                   (384, 128, 65536 + 5), (256, 128, 31)])
def test_split_bf16_linear_matches_f64(N, K, R):
    """ops.split_linear (sb_gemm): act(x W^T + b + addend) for 128 / 256 / 384 outputs on exact three-way bf16 splits, strided operands
    (column blocks of wider matrices), in-place accumulation; the error against f64 is that of a plain fp32 GEMM (torch.mm); the
    columns of the wider output matrix outside the block are left untouched."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    old = ops.CELL_MODE
    ops.set_cell_mode("split_bf16")
    try:
        torch.manual_seed(K + R + N)
        xw = torch.randn(R, K + 8, device="cuda")
        x = xw[:, 4:4 + K]                                   # a column block: row stride K + 8
        Wf = torch.randn(N, K + 4, device="cuda") * 0.1
        W = Wf[:, 4:]
        b = torch.randn(N, device="cuda")
        wide = torch.randn(R, N + 128 + 4, device="cuda")
        out = wide[:, 128:128 + N]
        add0 = out.clone()
        left0, right0 = wide[:, :128].clone(), wide[:, 128 + N:].clone()
        with torch.no_grad():
            assert ops.split_linear_ok(x, W, out, out)
            y = ops.split_linear(x, W, b, True, out=out, addend=out)
            ref = torch.relu(x.double() @ W.double().t() + b.double() + add0.double())
            lib = torch.relu(torch.addmm(add0 + b, x, W.t()))
            assert y.data_ptr() == out.data_ptr()
            e_split, e_lib = float((y.double() - ref).abs().max()), float((lib.double() - ref).abs().max())
            assert e_split <= 2.0 * e_lib + 1e-6 and e_split < 2e-5 * max(1.0, float(ref.abs().max())), (e_split, e_lib)
            assert torch.equal(wide[:, :128], left0) and torch.equal(wide[:, 128 + N:], right0)   # the neighbouring columns are not touched
            y2 = ops.split_linear(x, W)                          # no bias, no addend, fresh output
            assert float((y2.double() - x.double() @ W.double().t()).abs().max()) <= 2.0 * float((x @ W.t() - x.double() @ W.double().t()).abs().max()) + 1e-6
    finally:
        ops.set_cell_mode(old)


@pytest.mark.parametrize("M,N", [(384, 128), (128, 384), (128, 128), (128, 256), (256, 128)])
def test_split_bf16_wgrad_is_as_accurate_as_the_fp32_wgrad(M, N):
    """ops.wgrad in both matmul modes against f64 (a^T b over 123 457 rows, strided operands): the split-bf16 kernel's error is the
    fp32-MFMA kernel's (both a few 1e-7 of max |C|: summation order) -- and below the BLAS library's fp32 GEMM."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(M + N)
    K = 123457
    aw = torch.randn(K, M + 4, device="cuda") * torch.rand(K, 1, device="cuda")
    a, b = aw[:, 4:], torch.randn(K, N, device="cuda")
    ref = a.double().t() @ b.double()
    old = ops.WGRAD_MODE
    errs = {}
    try:
        for mode in ("fp32", "split_bf16"):
            ops.WGRAD_MODE = mode
            c = ops.wgrad(a, b)
            c2 = ops.wgrad(a, b)
            assert torch.equal(c, c2)                       # deterministic
            acc = c.clone()
            ops.wgrad(a, b, out=acc, accumulate=True)
            assert torch.allclose(acc, 2 * c, rtol=1e-6, atol=1e-6)
            errs[mode] = float((c.double() - ref).abs().max() / ref.abs().max())
    finally:
        ops.WGRAD_MODE = old
    e_lib = float(((a.t() @ b).double() - ref).abs().max() / ref.abs().max())
    assert errs["split_bf16"] < 3e-6 and errs["split_bf16"] <= 2.0 * errs["fp32"] + 2e-7, (errs, e_lib)


@pytest.mark.parametrize("mode", ["split_bf16", "fp32"])
@pytest.mark.parametrize("N,K", [(128, 128), (128, 256), (128, 384), (384, 128)])
def test_input_grad_with_strided_gradient_matches_f64(N, K, mode):
    """ops.input_grad: g W for a Linear (N outputs, K inputs) where g is a column block of a wider matrix (the [d agg | d h] halves of
    the FCRA backward, dgi's column slices) -- the split-bf16 route (sb_gemm on W^T) and the library route against f64."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(N + K)
    R = 50000 + 3
    gw = torch.randn(R, N + 132, device="cuda")
    g = gw[:, 4:4 + N]
    W = torch.randn(N, K, device="cuda") * 0.2
    old = ops.PROJ_MODE
    ops.PROJ_MODE = mode
    try:
        with torch.no_grad():
            dx = ops.input_grad(g, W)
    finally:
        ops.PROJ_MODE = old
    ref = g.double() @ W.double()
    lib = (g @ W).double()
    e, e_lib = float((dx.double() - ref).abs().max()), float((lib - ref).abs().max())
    assert dx.shape == (R, K) and e <= 2.0 * e_lib + 1e-6, (e, e_lib)


@pytest.mark.parametrize("n_in,n_out,mask_cols", [(256, 128, 128), (256, 128, 256), (384, 128, 384), (128, 384, 128)])
def test_input_gradient_with_the_relu_backward_in_its_epilogue(n_in, n_out, mask_cols):
    """ops.input_grad_masked (sb_gemm_masked): (g W) * (y > 0) on the first mask_cols columns and its column sums -- autograd's
    threshold_backward and bias sum of the relu(Linear) in front -- against f64, with g and y column blocks of wider matrices, a ragged
    row count, and exact zeros / negative zeros / denormals in y (relu' is 0 there: threshold_backward keeps y > 0 only).  The sums are
    deterministic: two runs agree bit for bit."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(n_in + mask_cols)
    R = 70000 + 19
    gw, yw = torch.randn(R, n_out + 8, device="cuda"), torch.randn(R, n_in + 12, device="cuda")
    g, y = gw[:, 4:4 + n_out], yw[:, 8:8 + n_in]
    y[::3, ::5] = 0.0
    y[1::7, 1::4] = -0.0
    y[2::11, 2::3] = 1e-42
    W = torch.randn(n_out, n_in, device="cuda") * 0.2
    modes = ops.matmul_modes()
    ops.set_matmul_mode("split_bf16")
    try:
        with torch.no_grad():
            dx, cs = ops.input_grad_masked(g, W, y, mask_cols)
            dx2, cs2 = ops.input_grad_masked(g, W, y, mask_cols)
            plain = ops.input_grad(g, W)
        assert ops.input_grad_masked(g[:100], W, y[:100], mask_cols) is None      # below the row threshold: the caller's unfused path
    finally:
        ops.restore_matmul_modes(modes)
    keep = torch.ones(R, n_in, device="cuda", dtype=torch.bool)
    keep[:, :mask_cols] = y[:, :mask_cols] > 0
    ref = (g.double() @ W.double()) * keep
    assert dx.shape == (R, n_in) and cs.shape == (n_in,)
    assert torch.equal(dx, torch.where(keep, plain, torch.zeros_like(plain)))          # the same product, masked
    assert float((dx.double() - ref).abs().max()) < 3e-6 * float(ref.abs().max())
    assert float((cs.double() - ref.sum(0)).abs().max()) < 2e-6 * float(ref.abs().sum(0).max())
    assert torch.equal(dx, dx2) and torch.equal(cs, cs2)
    # the same with relu'(y) given as sign bits (a column block of a wider byte matrix): identical results
    packed = ((y > 0).view(R, n_in // 8, 8).to(torch.int32) * (1 << torch.arange(8, device="cuda", dtype=torch.int32))).sum(-1).to(torch.uint8)
    wide = torch.full((R, n_in // 8 + 5), 0xA5, dtype=torch.uint8, device="cuda")
    wide[:, 3:3 + n_in // 8] = packed
    ops.set_matmul_mode("split_bf16")
    try:
        with torch.no_grad():
            dxb, csb = ops.input_grad_masked(g, W, y, mask_cols, bits=wide[:, 3:3 + n_in // 8])
    finally:
        ops.restore_matmul_modes(modes)
    assert torch.equal(dxb, dx) and torch.equal(csb, cs)


@pytest.mark.parametrize("K,inplace", [(128, False), (256, False), (128, True)])
def test_split_gemm_writes_the_sign_bits_of_its_result(K, inplace):
    """sb_gemm_signs: relu(x W^T + b) [+ addend] into a column block, and bit k of byte j of a row = (result[row][8 j + k] > 0) into a
    column block of a byte matrix -- the result equals the plain kernel's bit for bit, the bytes equal the packed comparison, the
    neighbouring bytes and columns stay untouched; ragged row count."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(K)
    R, N = 40000 + 21, 128
    x = torch.randn(R, K, device="cuda")
    W, b = torch.randn(N, K, device="cuda") * 0.1, torch.randn(N, device="cuda") * 0.1
    out_w = torch.full((R, 2 * N), 3.0, device="cuda")
    ref_w = out_w.clone()
    bits_w = torch.full((R, 32), 0x5A, dtype=torch.uint8, device="cuda")
    if inplace:
        out_w[:, N:] = torch.randn(R, N, device="cuda")
        ref_w.copy_(out_w)
    modes = ops.matmul_modes()
    ops.set_matmul_mode("split_bf16")
    try:
        with torch.no_grad():
            kw = dict(addend=out_w[:, N:]) if inplace else {}
            ops.split_linear(x, W, None if inplace else b, True, out=out_w[:, N:], sign_bits=bits_w[:, 16:], **kw)
            kw = dict(addend=ref_w[:, N:]) if inplace else {}
            ops.split_linear(x, W, None if inplace else b, True, out=ref_w[:, N:], **kw)
    finally:
        ops.restore_matmul_modes(modes)
    assert torch.equal(out_w, ref_w) and bool((out_w[:, :N] == 3.0).all())
    y = out_w[:, N:]
    packed = ((y > 0).view(R, N // 8, 8).to(torch.int32) * (1 << torch.arange(8, device="cuda", dtype=torch.int32))).sum(-1).to(torch.uint8)
    assert torch.equal(bits_w[:, 16:], packed) and bool((bits_w[:, :16] == 0x5A).all())
    assert 0.2 < float((y > 0).float().mean()) < 0.8


def test_relu_link_gives_the_gradients_of_the_unlinked_layers():
    """ops.ReluLink: relu(Linear) -> Linear with the ReLU's backward handed to the consumer's input gradient equals the same two layers
    without the link (every gradient; the bias gradient to summation order), and a link nobody fills changes nothing."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(5)
    rows, E = 30000, 128
    m3 = torch.randn(rows, 3, E, device="cuda")
    gout = torch.randn(rows, E, device="cuda")
    base = [torch.randn(E, E, device="cuda") * 0.2, torch.randn(E, device="cuda") * 0.2, torch.randn(E, 3 * E, device="cuda") * 0.1]
    modes = ops.matmul_modes()
    ops.set_matmul_mode("split_bf16")
    grads = {}
    try:
        for linked in (False, True, "unused", "fp32 mask"):
            ops.RELU_BITS = linked != "fp32 mask"      # relu' from the sign bits the producer's GEMM wrote / from the saved activations
            Wa, ba, Ws = [t.clone().requires_grad_(True) for t in base]
            x = m3.clone().requires_grad_(True)
            link = ops.ReluLink() if linked else None
            emb = ops.linear(x, Wa, ba, relu=True, y_link=link)
            h = ops.linear(emb.reshape(rows, 3 * E), Ws, None, x_link=link if linked in (True, "fp32 mask") else None)
            assert link is None or (link.bits is not None) == ops.RELU_BITS
            (h * gout).sum().backward()
            grads[linked] = [t.grad for t in (Wa, ba, Ws, x)]
            assert link is None or link.db is None                               # consumed by the producer
    finally:
        ops.RELU_BITS = True
        ops.restore_matmul_modes(modes)
    for a, b in zip(grads[True], grads["fp32 mask"]):
        assert torch.equal(a, b)
    for a, b, c in zip(grads[False], grads[True], grads["unused"]):
        assert torch.equal(a, c)
        assert float((a - b).abs().max()) <= 2e-6 * float(a.abs().max()), a.shape
    assert torch.equal(grads[False][3], grads[True][3]) and torch.equal(grads[False][0], grads[True][0])


@pytest.mark.parametrize("mode", ["split_bf16", "fp32"])
def test_fcra_hop_forward_and_backward_match_f64(mode):
    """ops.fcra_hop (one DHGN.fcra hop, DHGN/mappo_parallel.py:204-233: h' = relu(FCRA([relu(AGG(nb)) | h]))) chained twice, forward
    and every gradient against an f64 torch evaluation, at a row count above the kernels' thresholds (split-bf16 GEMMs / hipBLASLt,
    the ReLU backward in the input gradient's epilogue (ReluLink) / k_relu_bwd_colsum on column blocks, k_sb_wgrad / k_wgrad).  ReLU's
    derivative is discontinuous: an activation within rounding
    noise of zero may fall on either side in fp32 and f64, which moves a weight gradient by a whole row's contribution -- so the f64
    gradients are evaluated with the ReLU masks of the product's own forward pass (read from its operand buffers)."""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(3)
    E, R, P = 128, 5000, 8
    rows = R * P
    mk = lambda *s: (torch.randn(*s, device="cuda") * 0.3)
    Wa, ba, Wf, bf = [mk(E, E) for _ in range(2)], [mk(E) for _ in range(2)], [mk(E, 2 * E) for _ in range(2)], [mk(E) for _ in range(2)]
    nb = [mk(R, P, E) for _ in range(2)]
    h0 = mk(R, P, E)
    gout = mk(R, P, E)
    params = [t.clone().requires_grad_(True) for t in Wa + ba + Wf + bf]
    cat0 = torch.empty(rows, 2 * E, device="cuda")            # hop 0's [agg | h] operand: ours, so its masks can be read afterwards
    cat0[:, E:].copy_(h0.view(rows, E))
    h0g = cat0.view(R, P, 2 * E)[..., E:].requires_grad_(True)
    modes = ops.matmul_modes()
    ops.set_matmul_mode(mode)
    try:
        h1, carry = ops.fcra_hop(nb[0], h0g, (cat0, None, None), params[0], params[2], params[4], params[6], False)
        cat1 = carry[0]
        h2, _ = ops.fcra_hop(nb[1], h1, carry, params[1], params[3], params[5], params[7], True)
        (h2 * gout).sum().backward()
    finally:
        ops.restore_matmul_modes(modes)
    masks = [(cat0[:, :E] > 0).double().view(R, P, E), (cat1[:, E:] > 0).double().view(R, P, E),
             (cat1[:, :E] > 0).double().view(R, P, E), (h2.detach() > 0).double()]
    p64 = [t.double().clone().requires_grad_(True) for t in Wa + ba + Wf + bf]
    h64 = h0.double().clone().requires_grad_(True)
    lin = torch.nn.functional.linear
    y, y_relu = h64, h64.detach()
    for k in range(2):
        z_agg = lin(nb[k].double(), p64[k], p64[2 + k])
        y = lin(torch.cat((z_agg * masks[2 * k], y), -1), p64[4 + k], p64[6 + k]) * masks[2 * k + 1]
        with torch.no_grad():
            y_relu = torch.relu(lin(torch.cat((torch.relu(z_agg), y_relu), -1), p64[4 + k], p64[6 + k]))
    (y * gout.double()).sum().backward()
    assert float((h2.detach().double() - y_relu).abs().max()) < 2e-5 * float(y_relu.abs().max())     # forward: against the plain f64 ReLU network
    for a, b in zip(params + [h0g], p64 + [h64]):
        scale = float(b.grad.abs().max())
        assert float((a.grad.double() - b.grad).abs().max()) <= 3e-5 * scale + 1e-7, (a.shape, scale)


def test_split_wgrad_with_the_left_operand_in_two_tensors():
    """wgrad_split_tn2: [A1 | A2]^T B with A1 a column slice of a wider matrix (dgi's first 2H columns) and A2 its own tensor (dnr) -- the
    GRU's dW_hh in one pass over h_prev -- equals the two separate products (same split arithmetic, same split-K partials) and f64."""
    import ctypes as C
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(11)
    K, H = 61237, 128
    dgi = torch.randn(K, 3 * H, device="cuda") * 0.1
    dnr = torch.randn(K, H, device="cuda") * 0.1
    hp = torch.randn(K, H, device="cuda")
    a1 = dgi[:, :2 * H]
    L = ops.load_library()
    out = torch.full((3 * H, H), 7.0, device="cuda")
    base = out.clone()
    ws = torch.empty(L.wgrad_split_workspace(3 * H, H), dtype=torch.uint8, device="cuda")
    ops._check(L.wgrad_split_tn2(K, 2 * H, H, H, ops._ptr(a1), a1.stride(0), ops._ptr(dnr), dnr.stride(0), ops._ptr(hp), hp.stride(0), ops._ptr(out), 1,
                                 ops._ptr(ws), ops._stream()), "wgrad_split_tn2")
    ref = torch.cat((a1, dnr), 1).double().t() @ hp.double()
    err = float((out.double() - base.double() - ref).abs().max() / ref.abs().max())
    old = ops.WGRAD_MODE
    ops.WGRAD_MODE = "split_bf16"
    try:
        two = torch.cat((ops.wgrad(a1, hp), ops.wgrad(dnr, hp)), 0)
    finally:
        ops.WGRAD_MODE = old
    assert err < 3e-6, err
    assert float((out - base - two).abs().max()) <= 1e-5 * float(two.abs().max())      # (accumulate adds into 7.0: one more rounding)
    # the product's route: ops._gru_dw_hh takes it for time-major gradients
    T, B = 40, 200
    dgi3, dnr3, out3, h0 = torch.randn(T * B, 3 * H, device="cuda"), torch.randn(T, B, H, device="cuda"), torch.randn(T, B, H, device="cuda"), torch.randn(B, H, device="cuda")
    calls = []
    real = L.wgrad_split_tn2
    L.wgrad_split_tn2 = lambda *a: (calls.append(1), real(*a))[1]
    try:
        ops.WGRAD_MODE = "split_bf16"
        dw = ops._gru_dw_hh(dgi3, None, dnr3, out3, h0, T, B, H)
    finally:
        L.wgrad_split_tn2 = real
        ops.WGRAD_MODE = old
    hprev = torch.cat((h0[None], out3[:-1]), 0).reshape(T * B, H).double()
    want = torch.cat((dgi3[:, :2 * H], dnr3.reshape(T * B, H)), 1).double().t() @ hprev
    assert calls and float((dw.double() - want).abs().max() / want.abs().max()) < 3e-6
