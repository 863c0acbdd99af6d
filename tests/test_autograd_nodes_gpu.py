"""The autograd nodes of ops.py -- the Python layer that decides which kernel sees which operand -- against the f64 restatements of
tests/autograd_nodes_cases.py: _Linear, _SkinnyLinear, _FcraHop, _EncoderTailTrain, _GRULayer, _GRULayerMulti with _gru_dw_hh,
_MsgAgg3Pair and the ReluLink hand-over, under every gradient subset, link state, side of each row threshold, matmul mode, upstream
gradient layout and a second backward, at the smallest row counts with an edge in the launch arithmetic (thresholds forced down).
Every case asserts from call counters on the C entry points which kernels ran and which did not, so a case that silently drops to
the BLAS library fails instead of passing on the library's arithmetic.  The last tests walk the update's graphs of the shipped models
and hold ReluLink's single-consumer contract.

Bound: err <= 4 noise + 2e-5 scale per gradient tensor (tests/test_update_parity_gpu.py), noise = the restatement's own fp32 error on
the CPU and the GPU under the same ReLU masks; forward 2e-5 scale against the plain f64 ReLU network; the masks of the product's
forward may differ from the plain f64 network's in at most 1e-3 of the elements."""
import time
import types

import pytest
import torch

from tests import autograd_nodes_cases as cases
from tests import msg_ref as mr

pytestmark = pytest.mark.gpu

E = cases.E
ENTRY_POINTS = ("wgrad_split_tn", "wgrad_tn", "relu_bwd_colsum", "wgrad_skinny", "sb_gemm", "sb_gemm_masked", "sb_gemm_masked_bits", "sb_gemm_signs",
                "sb_encoder_tail_train", "sb_encoder_tail_bwd", "wgrad_split_tn2", "gru_seq_split_fwd_multi", "gru_seq_split_bwd_multi",
                "gru_seq_fwd_multi", "gru_seq_bwd_multi", "gru_gates_fwd", "gru_gates_bwd", "dhgn_msg_agg_bwd_pair", "dhgn_msg_agg_bwd",
                "dhgn_msg_agg3_pair_fwd", "dhgn_msg_agg3_pair01_fwd", "dhgn_msg_agg_ones_sorted_fwd", "dhgn_msg_agg_ones_sorted_bwd", "dhgn_msg_agg_fwd",
                "dhgn_msg_agg3_fwd")
THRESHOLDS = ("WGRAD_MIN_ROWS", "RELU_BWD_MIN_ROWS", "SKINNY_MIN_ROWS", "SORTED_ONES_MIN_QDIV", "MASKED_GRAD_MIN_ROWS", "ENCODER_TAIL_TRAIN_MIN_ROWS")
SWITCHES = ("PERSISTENT_GRU_MIN_T", "RELU_BITS", "RELU_LINK", "ENCODER_TAIL_TRAIN", "MASKED_GRAD_SHAPES")
MODES = ("split_bf16", "fp32")
WORST, SLOW, REFS = {}, {}, {}
ARRIVED = {}     # what the last re-laid-out upstream gradient looked like: strides, address modulo 16


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if SLOW:
        k = max(SLOW, key=SLOW.get)
        print(f"\nslowest case {k}: {SLOW[k]:.2f} s; {len(SLOW)} cases, {sum(SLOW.values()):.1f} s in all")
    for node, (ratio, tag) in sorted(WORST.items()):
        print(f"worst err / bound, {node}: {ratio:.3f} at {tag}")
    REFS.clear()


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    SLOW[request.node.name] = time.perf_counter() - t0


@pytest.fixture
def env(monkeypatch):
    """every row threshold the test touches at 1 (saved and restored, like the matmul modes and the switches) + call counters on the
    library's entry points (tests/test_update_parity_gpu.py forced_kernels)"""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    for name in THRESHOLDS:
        monkeypatch.setattr(ops, name, 1)
    for name in SWITCHES:
        monkeypatch.setattr(ops, name, getattr(ops, name))
    monkeypatch.setattr(ops, "RELU_BITS", True)
    monkeypatch.setattr(ops, "RELU_LINK", True)
    monkeypatch.setattr(ops, "ENCODER_TAIL_TRAIN", True)
    L = ops.load_library()
    calls = {n: 0 for n in ENTRY_POINTS}

    def wrap(name):
        real = getattr(L, name)

        def counted(*a):
            calls[name] += 1
            return real(*a)
        monkeypatch.setattr(L, name, counted)
    for n in ENTRY_POINTS:
        wrap(n)
    modes = ops.matmul_modes()
    yield types.SimpleNamespace(ops=ops, calls=calls)
    ops.restore_matmul_modes(modes)


# ---- the upstream gradient's layout -------------------------------------------------------------------------------------------------
def _relayout(g, layout):
    """the same values as g (.., N) in another memory layout"""
    N = g.shape[-1]
    g2 = g.reshape(-1, N)
    rows = g2.shape[0]
    if layout == "column_block":          # columns [4, 4 + N) of a wider matrix: 16-byte aligned, row stride N + 8
        wide = torch.zeros(rows, N + 8, device=g.device)
        out = wide[:, 4:4 + N]
    elif layout == "transposed":          # unit stride over rows
        out = torch.zeros(N, rows, device=g.device).t()
    elif layout == "off_by_4_bytes":
        out = torch.zeros(rows * N + 4, device=g.device)[1:1 + rows * N].view(rows, N)
    else:
        raise KeyError(layout)
    out.copy_(g2)
    return out.view(g.shape)


class _Relayout(torch.autograd.Function):
    """identity; hands the gradient on in the layout asked for (row_broadcast: as it arrives, which the loss arranged) and records it"""

    @staticmethod
    def forward(ctx, y, layout):
        ctx.layout = layout
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        out = g if ctx.layout == "row_broadcast" else _relayout(g, ctx.layout)
        ARRIVED["strides"], ARRIVED["mod16"], ARRIVED["shape"] = out.stride(), out.data_ptr() % 16, tuple(out.shape)
        return out, None


def _loss(ys, gouts, layout):
    tot = 0.0
    for y, g in zip(ys, gouts):
        if layout == "dense":
            tot = tot + (y * g).sum()
        elif layout == "row_broadcast":   # y.sum(0): autograd expands the (N,) gradient over the rows with stride 0
            N = y.shape[-1]
            tot = tot + (_Relayout.apply(y, layout).reshape(-1, N).sum(0) * g.reshape(-1, N)[0]).sum()
        else:
            tot = tot + (_Relayout.apply(y, layout) * g).sum()
    return tot


def _check_arrival(layout, rows):
    if layout == "dense":
        return
    st = ARRIVED["strides"]
    if layout == "row_broadcast":
        assert all(s == 0 for s in st[:-1]) and st[-1] == 1, st
    elif layout == "column_block":
        assert st[-1] == 1 and st[-2] == ARRIVED["shape"][-1] + 8 and ARRIVED["mod16"] == 0, st
    elif layout == "transposed":
        assert st[-1] > 1 and st[-1] in (rows, ARRIVED["shape"][0] * (ARRIVED["shape"][1] if len(st) == 3 else 1)), st
    else:
        assert ARRIVED["mod16"] == 4 and st[-1] == 1


# ---- the nodes through ops.py --------------------------------------------------------------------------------------------------------
def _module(L, tag=""):
    m = types.SimpleNamespace(num_layers=2)
    for l in range(2):
        for attr, key in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
            setattr(m, f"{attr}_l{l}", L[f"{key}{l}{tag}"])
    return m


def _leaves(node, t, req):
    """the case's tensors on the GPU; `req` require a gradient.  The h of a hop chain is the right half of its [agg | h] operand, ours, so
    that the first hop's masks can be read afterwards (tests/test_ops_gpu.py::test_fcra_hop_forward_and_backward_match_f64)"""
    L = {}
    for k, v in t.items():
        v = v.cuda()
        if node in ("hops", "hop_gru") and k == "h":
            R, P = v.shape[:2]
            cat0 = torch.empty(R * P, 2 * E, device="cuda")
            cat0[:, E:].copy_(v.view(R * P, E))
            L["_cat0"] = cat0
            v = cat0.view(R, P, 2 * E)[..., E:]
        elif k in req or k.startswith("gout"):
            v = v.clone()
        L[k] = v.requires_grad_(True) if k in req else v
    return L


def _after_messages(ops, L, route, state="consumed"):
    """DHGN._after_messages on (m3, Wa, ba, Ws, add): the fused tail where its predicate holds (route "auto" / "tail"), else the two linked
    layers.  -> (h0 (rows, E), relu decisions of emb, links, route taken)"""
    m3 = L["m3"]
    rows = m3.shape[0]
    add = L["add"].clone()
    m3_s = m3.view(rows, 3 * E)
    ok = ops.encoder_tail_train_ok(m3_s, L["Wa"], L["ba"], L["Ws"], add)
    if route == "tail":
        assert ok
    if route != "links" and ok and (m3.requires_grad or add.requires_grad or any(L[k].requires_grad for k in ("Wa", "ba", "Ws"))):
        y = ops.encoder_tail_train(m3_s, L["Wa"], L["ba"], L["Ws"], add)
        emb = y.grad_fn.saved_tensors[1]
        return y, emb.view(rows, 3, E) > 0, [], "tail"
    link = None if state == "none" else ops.ReluLink()
    emb = ops.linear(m3, L["Wa"], L["ba"], relu=True, y_link=link)
    y = ops.linear(emb.reshape(rows, 3 * E), L["Ws"], add, consume_addend=True, x_link=None if state in ("none", "offered") else link)
    return y, emb.detach() > 0, [link] if link is not None else [], "links"


def _hop(ops, L, k, h, carry, last):
    return ops.fcra_hop(L[f"nb{k}"], h, carry, L[f"Wagg{k}"], L[f"bagg{k}"], L[f"Wf{k}"], L[f"bf{k}"], last)


def build(ops, node, L, opt):
    """-> (outputs, relu decisions of the product's forward, links of the graph, notes)"""
    masks, links, notes = {}, [], {}
    if node == "linear":
        link = ops.ReluLink() if opt.get("offer") else None
        y = ops.linear(L["x"], L["W"], L["b"], relu=True, y_link=link)
        masks["y"] = y.detach() > 0
        links += [link] if link is not None else []
    elif node == "linear_addend":
        y = ops.linear(L["x"], L["W"], L["add"])
    elif node == "linear_nobias":
        y = ops.linear(L["x"], L["W"])
    elif node in ("skinny_in", "skinny_out"):
        y = ops.linear_skinny(L["x"], L["W"], L["b"])
    elif node == "chain":
        y, masks["emb"], links, notes["route"] = _after_messages(ops, L, opt.get("route", "links"), opt.get("state", "consumed"))
    elif node == "hops":
        cat0 = L["_cat0"]
        h1, carry = _hop(ops, L, 0, L["h"], (cat0, None, None), False)
        cat1 = carry[0]
        links.append(carry[1])
        y, carry = _hop(ops, L, 1, h1, carry, True)
        links.append(carry[1])
        masks = {"agg0": cat0[:, :E] > 0, "y0": cat1[:, E:] > 0, "agg1": cat1[:, :E] > 0, "y1": y.detach() > 0}
    elif node == "gru":
        a = opt.get("agents", 0)
        T = L["x"].shape[0]
        x = cases.agent_rows(L["x"], a) if a else L["x"]
        y, _ = ops.gru(x, L["h0"], _module(L), agents=a, steps=T if a else None)
    elif node == "gru_multi":
        a = opt.get("agents", 0)
        n = sum(1 for k in L if k.startswith("x_"))
        T = L["x_0"].shape[0]
        xs = [cases.agent_rows(L[f"x_{k}"], a) if a else L[f"x_{k}"] for k in range(n)]
        y = tuple(ops.gru_multi(xs, [L[f"h0_{k}"] for k in range(n)], [_module(L, f"_{k}") for k in range(n)], agents=a, steps=T if a else None,
                                grouped=True, zero_state=opt.get("zero_state", False)))
    elif node == "hop_gru":
        cat0 = L["_cat0"]
        h1, carry = _hop(ops, L, 0, L["h"], (cat0, None, None), True)
        links.append(carry[1])
        R, P = h1.shape[:2]
        T = L["gout"].shape[0]
        masks = {"agg0": cat0[:, :E] > 0, "y0": h1.detach() > 0}
        (y,) = ops.gru_multi([h1.reshape(R * P, E)], [L["h0"]], [_module(L)], agents=P, steps=T, grouped=True,
                             x_links=[carry[1]] if opt.get("state", "consumed") == "consumed" else None)
    elif node == "tail_hop":
        h0, masks["emb"], links, notes["route"] = _after_messages(ops, L, opt.get("route", "auto"))
        h1, carry = _hop(ops, L, 0, h0.reshape(L["nb0"].shape), None, True)
        links.append(carry[1])
        masks["agg0"], masks["y0"] = h1.grad_fn.cat[:, :E] > 0, h1.detach() > 0
        y = h1
    else:
        raise KeyError(node)
    return (y if isinstance(y, tuple) else (y,)), masks, links, notes


def _reference(node, t, masks, key):
    """the f64 gradients under the product's masks, computed once per case and mask content"""
    sig = (node, key, tuple((k, hash(v.cpu().numpy().tobytes())) for k, v in sorted(masks.items())))
    if sig not in REFS:
        REFS[sig] = cases.Reference(node, t, masks, gpu=True)
    return REFS[sig]


def run(env, node, t, req, key, opt=None, layout="dense", tag="", check=True, repeat=1):
    """forward + backward of `node` with `req` requiring gradients -> namespace(grads, calls, links, ys, notes, ref, L).  check: the
    forward against the plain f64 network, the mask cap, None for frozen tensors and the f64 bound for the rest"""
    ops, opt = env.ops, dict(opt or {})
    names = cases.grad_names(node, t)
    L = _leaves(node, t, req)
    for k in env.calls:
        env.calls[k] = 0
    ys, masks, links, notes = build(ops, node, L, opt)
    loss = _loss(ys, [L[k] for k in L if k.startswith("gout")], layout)
    for r in range(repeat):
        loss.backward(retain_graph=r + 1 < repeat)
    torch.cuda.synchronize()
    res = types.SimpleNamespace(grads={k: L[k].grad for k in names}, calls=dict(env.calls), links=links, ys=[y.detach() for y in ys], notes=notes, L=L, masks=masks)
    rows = ys[0].numel() // ys[0].shape[-1]
    _check_arrival(layout, rows)
    for link in links:
        assert link.db is None, (node, tag, "a link still holds a db after backward")
    if not check:
        return res
    ref = res.ref = _reference(node, t, masks, key)
    bad, tot = ref.mismatch
    assert bad <= cases.MASK_CAP * max(tot, 1), (node, tag, bad, tot)
    for y, p in zip(res.ys, ref.plain_y):
        assert float((y.double().cpu() - p).abs().max()) <= cases.FWD_REL * float(p.abs().max()), (node, tag, "forward")
    for k in names:
        g = res.grads[k]
        if k not in req:
            assert g is None, (node, tag, k, "a frozen tensor got a gradient")
            continue
        assert g is not None, (node, tag, k, "no gradient")
        assert bool(torch.isfinite(g).all()), (node, tag, k)
        ratio = ref.ratio(k, g / repeat if repeat > 1 else g)
        if ratio > WORST.get(node, (0.0, ""))[0]:
            WORST[node] = (ratio, f"{tag} {k}")
        assert ratio <= 1.0, (node, tag, k, ratio, ref.noise[k], ref.scale[k])
    return res


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ran(calls, must=(), never=()):
    for k in must:
        assert calls[k] > 0, (k, "did not run", {n: c for n, c in calls.items() if c})
    for k in never:
        assert calls[k] == 0, (k, "ran", {n: c for n, c in calls.items() if c})


def _sweep(env, node, t, key, opt, census, chain=None, loose=None):
    """every gradient subset of a case: frozen -> None, trained -> the f64 gradient and the all-on run's bits; census(req, calls).
    loose: {subset: tensors held to the f64 bound only}, for a reason the caller states; the other tensors of such a subset keep the
    bit comparison wherever the forward took the all-on run's relu decisions (the comparison presumes the same masks)"""
    loose = loose or {}
    subs = cases.subsets(node, t, chain)
    base = run(env, node, t, subs["all"], key, opt, tag=f"{key} all")
    census(subs["all"], base.calls)
    for label, req in subs.items():
        if label == "all":
            continue
        res = run(env, node, t, req, key, opt, tag=f"{key} {label}")
        census(req, res.calls)
        if label in loose and not all(torch.equal(res.masks[m], base.masks[m]) for m in base.masks):
            continue
        for k in req:
            assert k in loose.get(label, ()) or _same_bits(res.grads[k], base.grads[k]), (node, key, label, k, "differs from the all-on run")
    return base


# ---- a, d: gradient subsets in both modes -------------------------------------------------------------------------------------------
MAKE_LINEAR = {"linear": cases.make_linear, "linear_addend": cases.make_linear_addend, "linear_nobias": cases.make_linear_nobias,
               "skinny_in": cases.make_skinny_in, "skinny_out": cases.make_skinny_out}


def _linear_census(node, mode):
    def census(req, calls):
        split = mode == "split_bf16"
        if node.startswith("skinny"):
            _ran(calls, must=("wgrad_skinny",) if ({"W", "b"} & set(req)) else (), never=() if ({"W", "b"} & set(req)) else ("wgrad_skinny",))
            _ran(calls, never=("sb_gemm", "wgrad_split_tn", "wgrad_tn", "relu_bwd_colsum"))
            return
        assert calls["sb_gemm"] == ((1 + ("x" in req)) if split else 0), calls
        mine, other = ("wgrad_split_tn", "wgrad_tn") if split else ("wgrad_tn", "wgrad_split_tn")
        assert calls[mine] == ("W" in req) and calls[other] == 0, calls
        assert calls["relu_bwd_colsum"] == (node == "linear" and "b" in req), calls
        _ran(calls, never=("sb_gemm_signs", "sb_gemm_masked", "sb_gemm_masked_bits", "wgrad_skinny", "sb_encoder_tail_train"))
    return census


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("node", sorted(MAKE_LINEAR))
def test_linear_nodes_under_every_gradient_subset(env, node, mode):
    """_Linear (ReLU + bias, a full addend, no bias) and _SkinnyLinear (few inputs, few outputs) at 1, 31, 32, 33 and 69 rows: the all-on
    case and every subset; the split / fp32 kernels of the mode ran for exactly the gradients asked for, the other mode's never"""
    env.ops.set_matmul_mode(mode)
    for rows in cases.LINEAR_ROWS:
        t = MAKE_LINEAR[node](rows)
        _sweep(env, node, t, f"{mode} rows={rows}", {}, _linear_census(node, mode))


def _chain_census(mode, route):
    def census(req, calls):
        split = mode == "split_bf16"
        producer = bool({"m3", "Wa", "ba"} & set(req))
        if route == "tail":
            assert calls["sb_encoder_tail_train"] == 1 and calls["sb_encoder_tail_bwd"] == 1, calls
            _ran(calls, never=("sb_gemm_signs", "sb_gemm_masked_bits", "sb_gemm_masked", "relu_bwd_colsum"))
            assert calls["wgrad_split_tn"] == ("Wa" in req) + ("Ws" in req), calls
            return
        _ran(calls, never=("sb_encoder_tail_train", "sb_encoder_tail_bwd", "sb_gemm_masked"))
        if split:
            assert calls["sb_gemm_signs"] == producer and calls["sb_gemm_masked_bits"] == producer and calls["relu_bwd_colsum"] == 0, calls
            assert calls["wgrad_split_tn"] == ("Wa" in req) + ("Ws" in req) and calls["wgrad_tn"] == 0, calls
        else:
            _ran(calls, never=("sb_gemm", "sb_gemm_signs", "sb_gemm_masked_bits", "wgrad_split_tn"))
            assert calls["wgrad_tn"] == ("Wa" in req) + ("Ws" in req), calls
            assert calls["relu_bwd_colsum"] == ("ba" in req), calls     # nothing fused: the producer's own pass when its bias gradient is wanted
    return census


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("route", ["links", "tail"])
def test_encoder_tail_chain_under_every_gradient_subset(env, route, mode):
    """relu(Linear) -> Linear of DHGN._after_messages as two linked _Linear nodes and as one _EncoderTailTrain (split mode only: in fp32
    mode its predicate refuses, which is asserted), producer / consumer wholly frozen included.  After every backward -- the frozen
    bias among them -- the link holds no db.
    A wholly frozen producer is not an autograd node: ops.linear evaluates it with grad mode on, where split_linear_ok refuses and the
    BLAS library computes the layer.  Its output is then the library's bits, not the split kernel's, so in split mode the consumer's
    weight gradient Ws of that subset -- the one tensor computed from the producer's output -- is held to the f64 bound only; the addend's
    gradient keeps the all-on bits (the fused tail has no such producer: it runs whole)."""
    ops = env.ops
    ops.set_matmul_mode(mode)
    loose = {"producer_frozen": ("Ws",)} if (route, mode) == ("links", "split_bf16") else None
    for rows in cases.LINEAR_ROWS:
        t = cases.make_chain(rows)
        if route == "tail" and mode == "fp32":
            L = _leaves("chain", t, ())
            assert not ops.encoder_tail_train_ok(L["m3"].view(rows, 3 * E), L["Wa"], L["ba"], L["Ws"], L["add"])
            continue
        _sweep(env, "chain", t, f"{mode} {route} rows={rows}", {"route": route}, _chain_census(mode, route), cases.CHAIN_PRODUCERS["chain"], loose=loose)


def _hops_census(mode):
    def census(req, calls):
        first = bool(set(cases.CHAIN_PRODUCERS["hops"]) & set(req))      # the first hop is in the graph (the last one always is)
        hops = 1 + first
        if mode == "split_bf16":
            # a hop under autograd writes the sign bits of both its GEMMs; its backward is one masked input gradient and two weight
            # gradients.  With the first hop frozen nobody wrote the bits of the last hop's right half: it masks from the activations.
            assert calls["sb_gemm_signs"] == 2 * hops and calls["wgrad_split_tn"] == 2 * hops and calls["wgrad_tn"] == 0, calls
            assert calls["sb_gemm_masked_bits"] == (2 if first else 0) and calls["sb_gemm_masked"] == (0 if first else 1), calls
            # the last hop's own relu' / bias-sum pass (nobody consumes its link); the first hop's rides in the last hop's input gradient
            assert calls["relu_bwd_colsum"] == 1, calls
        else:
            assert calls["wgrad_tn"] == 2 * hops and calls["relu_bwd_colsum"] == 2 * hops, calls
            _ran(calls, never=("wgrad_split_tn", "sb_gemm", "sb_gemm_signs", "sb_gemm_masked_bits", "sb_gemm_masked"))
    return census


@pytest.mark.parametrize("mode", MODES)
def test_fcra_hops_under_every_gradient_subset(env, mode):
    """two chained _FcraHop nodes at R P in {3, 33, 99}, P = 3: hop -> hop with either hop wholly frozen"""
    env.ops.set_matmul_mode(mode)
    for rows in cases.HOP_ROWS:
        t = cases.make_hops(rows // cases.HOP_P)
        _sweep(env, "hops", t, f"{mode} RP={rows}", {}, _hops_census(mode), cases.CHAIN_PRODUCERS["hops"])


def _gru_census(mode):
    """The census does not depend on the subset: _GRULayer.backward and _GRULayerMulti.backward compute dgi, both weight gradients and
    the input projection's products whatever needs_input_grad says (only dx is conditional), so a run that trains the inputs alone still
    launches every weight-gradient kernel.  That is the behaviour pinned here, wasted work in a phase with frozen GRU weights included."""
    def census(req, calls):
        split = mode == "split_bf16"
        fwd, bwd = ("gru_seq_split_fwd_multi", "gru_seq_split_bwd_multi") if split else ("gru_seq_fwd_multi", "gru_seq_bwd_multi")
        ofwd, obwd = ("gru_seq_fwd_multi", "gru_seq_bwd_multi") if split else ("gru_seq_split_fwd_multi", "gru_seq_split_bwd_multi")
        assert calls[fwd] == 2 and calls[bwd] == 2 and calls[ofwd] == 0 and calls[obwd] == 0, calls
        _ran(calls, never=("gru_gates_fwd", "gru_gates_bwd"))
        if split:
            _ran(calls, must=("sb_gemm", "wgrad_split_tn", "wgrad_split_tn2"), never=("wgrad_tn",))
        else:
            _ran(calls, must=("wgrad_tn",), never=("sb_gemm", "wgrad_split_tn", "wgrad_split_tn2"))
    return census


@pytest.mark.parametrize("mode", MODES)
def test_gru_layers_under_every_gradient_subset(env, mode):
    """ops.gru (_GRULayerMulti with one network per layer), two layers, T in {2, 3}, 15 / 16 / 17 sequences (times 3 agents in the encoder's row order): the all-on
    case and every subset of (x, h0, w_ih, w_hh, b_ih, b_hh per layer) at every shape"""
    env.ops.set_matmul_mode(mode)
    for T, B, a in cases.gru_shapes():
        t = cases.make_gru(T, B)
        _sweep(env, "gru", t, f"{mode} T={T} B={B} agents={a}", {"agents": a}, _gru_census(mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("agents", cases.GRU_AGENTS)
def test_gru_multi_under_every_gradient_subset(env, agents, mode):
    """_GRULayerMulti through ops.gru_multi(grouped=True): two and three networks with unequal numbers of sequences in one launch per
    layer and direction; each tensor of each network frozen in turn"""
    env.ops.set_matmul_mode(mode)
    m = max(agents, 1)
    for T, Bs in ((2, (15 * m, 17 * m)), (3, (16 * m, 15 * m, 17 * m))):
        t = cases.make_gru_multi(T, Bs)
        census = _gru_census(mode)
        _sweep(env, "gru_multi", t, f"{mode} T={T} Bs={Bs} agents={agents}", {"agents": agents}, census)


@pytest.mark.parametrize("mode", MODES)
def test_chains_into_the_gru_and_out_of_the_tail(env, mode):
    """last hop -> gru_multi(x_links=...) and _EncoderTailTrain -> hop: all-on, every single tensor frozen, producer wholly frozen,
    consumer wholly frozen, inputs only, parameters only.  In split mode the hop's relu' and bias sum ride in the GRU's masked input gradient (sb_gemm_masked_bits),
    the tail's runs where its predicate holds."""
    ops = env.ops
    ops.set_matmul_mode(mode)
    split = mode == "split_bf16"
    for episodes, T in ((1, 2), (11, 3)):
        t = cases.make_hop_gru(episodes, T)

        def census(req, calls):
            hop = bool(set(cases.CHAIN_PRODUCERS["hop_gru"]) & set(req))
            if split:
                assert calls["sb_gemm_masked_bits"] == 2 * hop and calls["relu_bwd_colsum"] == 0, calls   # the GRU's input gradient, the hop's
            else:
                _ran(calls, never=("sb_gemm_masked_bits", "sb_gemm_masked", "sb_gemm_signs"))
        _sweep(env, "hop_gru", t, f"{mode} episodes={episodes} T={T}", {}, census, cases.CHAIN_PRODUCERS["hop_gru"])
    for R in (1, 11, 33):
        t = cases.make_tail_hop(R)

        def census(req, calls):
            tail = bool(set(cases.CHAIN_PRODUCERS["tail_hop"]) & set(req))
            assert calls["sb_encoder_tail_train"] == (split and tail) and calls["sb_encoder_tail_bwd"] == (split and tail), calls
        # (a wholly frozen tail is two ops.linear calls outside autograd, on the BLAS library, see the chain test: Wf0, computed from its
        # output, is held to the bound only; the hop's other gradients depend on it through the relu decisions alone and keep the bits)
        _sweep(env, "tail_hop", t, f"{mode} RP={R * cases.HOP_P}", {}, census, cases.CHAIN_PRODUCERS["tail_hop"],
               loose={"producer_frozen": ("Wf0",)} if split else None)


# ---- b: link states ----------------------------------------------------------------------------------------------------------------
def test_link_states_of_the_linear_chain(env):
    """relu(Linear) -> Linear with no link, a link nobody consumes, a link consumed with the sign bits and with the fp32 activations as
    mask, and a link the consumer cannot fuse (row threshold above the rows; fp32 mode; the shape taken out of MASKED_GRAD_SHAPES; a
    gradient 4 bytes off the 16-byte boundary): f64 gradients in every state, no db left in the link -- also with the producer's bias
    frozen (_Linear.backward used to leave the consumer's column sums in the link when the bias gradient was not wanted).
    The bias gradient of the producer is the one branch that legitimately changes summation order between states: column sums out of
    the consumer's masked GEMM (per-workgroup partials) against relu_bwd_colsum / g.sum(0) -- it is held to the bound only, every other
    tensor to the bits of the unlinked run."""
    ops = env.ops
    rows = 33
    t = cases.make_chain(rows)
    names = frozenset(cases.grad_names("chain", t))
    got = {}
    for state in ("none", "offered", "consumed", "consumed_fp32_mask", "min_rows", "fp32_mode", "shape", "misaligned"):
        ops.set_matmul_mode("fp32" if state == "fp32_mode" else "split_bf16")
        ops.RELU_BITS = state != "consumed_fp32_mask"
        ops.MASKED_GRAD_MIN_ROWS = rows + 1 if state == "min_rows" else 1
        ops.MASKED_GRAD_SHAPES = {(256, 128), (128, 384)} if state == "shape" else {(256, 128), (384, 128), (128, 384)}
        st = {"none": "none", "offered": "offered"}.get(state, "consumed")
        for req in (names, names - {"ba"}):
            res = run(env, "chain", t, req, f"state={state}", {"route": "links", "state": st},
                      layout="off_by_4_bytes" if state == "misaligned" else "dense", tag=f"{state} frozen={sorted(names - req)}")
            fused = {"consumed": "sb_gemm_masked_bits", "consumed_fp32_mask": "sb_gemm_masked"}.get(state)
            for ep in ("sb_gemm_masked_bits", "sb_gemm_masked"):
                assert res.calls[ep] == (ep == fused), (state, res.calls)
            assert res.calls["sb_gemm_signs"] == (st != "none" and state not in ("consumed_fp32_mask", "fp32_mode")), (state, res.calls)
            assert res.calls["relu_bwd_colsum"] == (fused is None and "ba" in req), (state, res.calls)
            if req == names:
                got[state] = res.grads
    for state in ("offered", "min_rows", "shape"):
        for k in names:
            assert _same_bits(got[state][k], got["none"][k]), (state, k)
    for k in names:
        assert _same_bits(got["consumed"][k], got["consumed_fp32_mask"][k]), k
        if k != "ba":
            assert _same_bits(got["consumed"][k], got["none"][k]), k


def test_link_states_of_the_hop_into_the_gru(env):
    """last hop -> GRU with its link consumed by gru_multi(x_links=...) and offered but not consumed, both RELU_BITS settings and the row
    threshold above the rows: f64 gradients, no db left behind (run() asserts it for every link of the graph)"""
    ops = env.ops
    ops.set_matmul_mode("split_bf16")
    t = cases.make_hop_gru(11, 3)
    names = frozenset(cases.grad_names("hop_gru", t))
    for state, bits, min_rows, fused in (("consumed", True, 1, "sb_gemm_masked_bits"), ("consumed", False, 1, "sb_gemm_masked"), ("offered", True, 1, None),
                                         ("consumed", True, 100, None)):
        ops.RELU_BITS, ops.MASKED_GRAD_MIN_ROWS = bits, min_rows
        for req in (names, names - {"bf0"}, names - set(cases.CHAIN_PRODUCERS["hop_gru"])):
            res = run(env, "hop_gru", t, req, f"state={state}", {"state": state}, tag=f"{state} bits={bits} min_rows={min_rows}")
            hop = bool(set(cases.CHAIN_PRODUCERS["hop_gru"]) & set(req))
            if fused:
                assert res.calls[fused] == 2 * hop, (state, res.calls)
            elif min_rows == 1:    # the hop's own masked input gradient only
                assert res.calls["sb_gemm_masked_bits"] == hop and res.calls["relu_bwd_colsum"] == hop, (state, res.calls)


def test_link_states_of_the_hop_chains(env):
    """hop -> hop and _EncoderTailTrain -> hop with the sign bits on, with RELU_BITS off (the masks are read from the fp32 activations;
    the tail's predicate then refuses and DHGN._after_messages falls back to its two linked layers), with MASKED_GRAD_MIN_ROWS above the
    rows (no consumer fuses: every ReLU takes its own relu' / bias-sum pass) and with a gradient 4 bytes off the boundary into the last
    hop; all-on, the bias between the two nodes frozen, the producer wholly frozen.  f64 gradients, no db left in any link; the census
    of the all-on run shows the state.  "No link" and "a link nobody consumes" cannot be built for a hop chain: fcra_hop always offers
    its output's link and the next hop always takes it (the last hop's link is the one nobody consumes here)."""
    ops = env.ops
    ops.set_matmul_mode("split_bf16")
    rows = 33
    want = {   # (sb_gemm_masked_bits, sb_gemm_masked, relu_bwd_colsum, sb_gemm_signs, sb_encoder_tail_train) of the all-on run
        ("hops", "bits"): (2, 0, 1, 4, 0), ("hops", "fp32_mask"): (0, 2, 1, 0, 0), ("hops", "min_rows"): (0, 0, 4, 4, 0), ("hops", "misaligned"): (2, 0, 0, 4, 0),
        ("tail_hop", "bits"): (1, 0, 1, 2, 1), ("tail_hop", "fp32_mask"): (0, 2, 1, 0, 0), ("tail_hop", "min_rows"): (0, 0, 2, 2, 1),
        ("tail_hop", "misaligned"): (1, 0, 0, 2, 1)}     # (misaligned: the last hop's own relu' pass takes the torch ops, not the kernel)
    for node, bias in (("hops", "bf0"), ("tail_hop", "ba")):
        t = (cases.make_hops if node == "hops" else cases.make_tail_hop)(rows // cases.HOP_P)
        names = frozenset(cases.grad_names(node, t))
        for state in ("bits", "fp32_mask", "min_rows", "misaligned"):
            ops.RELU_BITS = state != "fp32_mask"
            ops.MASKED_GRAD_MIN_ROWS = rows + 1 if state == "min_rows" else 1
            for req in (names, names - {bias}, names - set(cases.CHAIN_PRODUCERS[node])):
                res = run(env, node, t, req, f"{node} state={state}", {}, layout="off_by_4_bytes" if state == "misaligned" else "dense",
                          tag=f"{node} {state} frozen={sorted(names - req)}")
                if req == names:
                    c = res.calls
                    got = (c["sb_gemm_masked_bits"], c["sb_gemm_masked"], c["relu_bwd_colsum"], c["sb_gemm_signs"], c["sb_encoder_tail_train"])
                    assert got == want[node, state], (node, state, got, c)
    ops.RELU_BITS, ops.MASKED_GRAD_MIN_ROWS = True, 1


# ---- c: both sides of each threshold -----------------------------------------------------------------------------------------------
def test_both_sides_of_each_row_threshold(env):
    """each threshold at R and at R + 1 for R = 33 rows, the others at 1: both routes within the f64 bound, and the census shows that the
    route changed.  Which side a setting lies on is also asserted from the predicate itself where the threshold has one that can be
    called on device tensors: WGRAD_MIN_ROWS (_wgrad_ok), SKINNY_MIN_ROWS (_skinny_ok), MASKED_GRAD_MIN_ROWS (input_grad_masked gives
    None below it) and ENCODER_TAIL_TRAIN_MIN_ROWS (encoder_tail_train_ok, also through the route DHGN._after_messages' rule takes).
    RELU_BWD_MIN_ROWS and PERSISTENT_GRU_MIN_T are compared inline in relu_bwd_colsum and ops.gru, with no predicate to
    call: for them the entry-point census is the evidence (relu_bwd_colsum; the sequence launches against the per-step gate kernels)."""
    ops = env.ops
    ops.set_matmul_mode("split_bf16")
    R = cases.THRESHOLD_ROWS
    moved = {"WGRAD_MIN_ROWS": "wgrad_split_tn", "RELU_BWD_MIN_ROWS": "relu_bwd_colsum", "SKINNY_MIN_ROWS": "wgrad_skinny",
             "MASKED_GRAD_MIN_ROWS": "sb_gemm_masked_bits", "ENCODER_TAIL_TRAIN_MIN_ROWS": "sb_encoder_tail_train"}
    for name, node, rows in cases.threshold_cases():
        if name == "PERSISTENT_GRU_MIN_T":
            continue
        assert rows == R
        t = {"linear_nobias": cases.make_linear_nobias, "linear": cases.make_linear, "skinny_in": cases.make_skinny_in, "chain": cases.make_chain}[node](R)
        req = frozenset(cases.grad_names(node, t))
        opt = {"route": "auto" if name == "ENCODER_TAIL_TRAIN_MIN_ROWS" else "links"}
        got = {}
        for value in (R, R + 1):
            setattr(ops, name, value)
            if name == "WGRAD_MIN_ROWS":
                a = torch.zeros(R, 256, device="cuda")
                assert ops._wgrad_ok(a, a[:, :128]) == (value == R)
            if name == "SKINNY_MIN_ROWS":
                assert ops._skinny_ok(torch.zeros(R, 4, device="cuda"), torch.zeros(R, 128, device="cuda")) == (value == R)
            if name == "MASKED_GRAD_MIN_ROWS":
                z = torch.zeros(R, 3 * E, device="cuda")
                assert (ops.input_grad_masked(z[:, :E], torch.zeros(E, 3 * E, device="cuda"), z, 3 * E) is not None) == (value == R)
            if name == "ENCODER_TAIL_TRAIN_MIN_ROWS":
                L = _leaves("chain", t, ())
                assert ops.encoder_tail_train_ok(L["m3"].view(R, 3 * E), L["Wa"], L["ba"], L["Ws"], L["add"]) == (value == R)
            res = got[value] = run(env, node, t, req, f"{name}={value}", opt, tag=f"{name}={value}")
            assert res.calls[moved[name]] == (value == R), (name, value, res.calls)
            if name == "ENCODER_TAIL_TRAIN_MIN_ROWS":
                assert res.notes["route"] == ("tail" if value == R else "links")
                assert res.calls["sb_gemm_signs"] == (value != R) and res.calls["sb_gemm_masked_bits"] == (value != R), res.calls
            if name == "MASKED_GRAD_MIN_ROWS":
                assert res.calls["relu_bwd_colsum"] == (value != R), res.calls
        setattr(ops, name, 1)
        if name == "ENCODER_TAIL_TRAIN_MIN_ROWS":      # the fused launches are bit-identical to the launches they replace
            for k in req:
                assert _same_bits(got[R].grads[k], got[R + 1].grads[k]), k


@pytest.mark.parametrize("mode", MODES)
def test_both_sides_of_the_persistent_gru_threshold(env, mode):
    """PERSISTENT_GRU_MIN_T at T and T + 1 for T = 2 and 3: the one-launch recurrence against the per-step gate kernels, both row orders"""
    ops = env.ops
    ops.set_matmul_mode(mode)
    fwd, bwd = ("gru_seq_split_fwd_multi", "gru_seq_split_bwd_multi") if mode == "split_bf16" else ("gru_seq_fwd_multi", "gru_seq_bwd_multi")
    for T, (B, a) in ((2, (17, 0)), (3, (48, 3))):
        t = cases.make_gru(T, B)
        req = frozenset(cases.grad_names("gru", t))
        for value in (T, T + 1):
            ops.PERSISTENT_GRU_MIN_T = value
            res = run(env, "gru", t, req, f"{mode} T={T} B={B} a={a}", {"agents": a}, tag=f"PERSISTENT_GRU_MIN_T={value}")
            if value == T:
                assert res.calls[fwd] == 2 and res.calls[bwd] == 2 and res.calls["gru_gates_fwd"] == 0 and res.calls["gru_gates_bwd"] == 0, res.calls
            else:
                assert res.calls[fwd] == 0 and res.calls[bwd] == 0 and res.calls["gru_gates_fwd"] == 2 * T and res.calls["gru_gates_bwd"] == 2 * T, res.calls
        ops.PERSISTENT_GRU_MIN_T = 2


# ---- d: the four routes of _gru_dw_hh ------------------------------------------------------------------------------------------------
def test_gru_dw_hh_routes(env):
    """dW_hh from the full dgh (the encoder's row order), from dgi's (dr, dz) columns + dnr with and without zero_h0, in the one
    wgrad_split_tn2 pass and in the two-wgrad fallback (fp32 mode; split mode below WGRAD_MIN_ROWS): f64 everywhere; zero_h0=True with
    a zero h0 and zero_h0=False with the same zero h0 give identical dW_hh"""
    ops = env.ops
    T, Bs = 3, (16, 17)
    for agents in (0, 3):
        m = max(agents, 1)
        t = cases.make_gru_multi(T, tuple(B * m for B in Bs))
        req = frozenset(cases.grad_names("gru_multi", t))
        ops.set_matmul_mode("split_bf16")
        res = run(env, "gru_multi", t, req, f"dw_hh agents={agents}", {"agents": agents}, tag="split")
        # layer 0 with agents: the full dgh (torch.mm for the first step + wgrad_split_tn for the rest); time-major layers: one tn2 pass each
        assert res.calls["wgrad_split_tn2"] == (2 if agents else 4), res.calls
        assert res.calls["wgrad_split_tn"] == (6 if agents else 4), res.calls
        ops.WGRAD_MIN_ROWS = 10 ** 6
        res = run(env, "gru_multi", t, req, f"dw_hh agents={agents}", {"agents": agents}, tag="split below WGRAD_MIN_ROWS")
        _ran(res.calls, never=("wgrad_split_tn2", "wgrad_split_tn", "wgrad_tn"))
        ops.WGRAD_MIN_ROWS = 1
        ops.set_matmul_mode("fp32")
        res = run(env, "gru_multi", t, req, f"dw_hh agents={agents}", {"agents": agents}, tag="fp32")
        assert res.calls["wgrad_split_tn2"] == 0 and res.calls["wgrad_tn"] == (10 if agents else 12), res.calls
        # zero h0
        tz = {k: (torch.zeros_like(v) if k.startswith("h0") else v) for k, v in t.items()}
        for mode in MODES:
            ops.set_matmul_mode(mode)
            a = run(env, "gru_multi", tz, req, f"dw_hh zero agents={agents}", {"agents": agents, "zero_state": True}, tag=f"{mode} zero_h0=True")
            b = run(env, "gru_multi", tz, req, f"dw_hh zero agents={agents}", {"agents": agents, "zero_state": False}, tag=f"{mode} zero_h0=False")
            for k in req:
                assert torch.equal(a.grads[k], b.grads[k]), (mode, agents, k)


# ---- e: the upstream gradient's layout ---------------------------------------------------------------------------------------------
LAYOUT_NODES = {"linear": lambda: cases.make_linear(33), "linear_addend": lambda: cases.make_linear_addend(33), "linear_nobias": lambda: cases.make_linear_nobias(33),
                "skinny_in": lambda: cases.make_skinny_in(33), "skinny_out": lambda: cases.make_skinny_out(33), "chain": lambda: cases.make_chain(33),
                "tail": lambda: cases.make_chain(33), "hops": lambda: cases.make_hops(11), "gru": lambda: cases.make_gru(3, 17),
                "gru_multi": lambda: cases.make_gru_multi(2, (15, 17)), "hop_gru": lambda: cases.make_hop_gru(11, 3),
                "tail_hop": lambda: cases.make_tail_hop(11)}


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_upstream_gradient_layouts(env, mode, layout):
    """the gradient arriving at a node dense, as a column block of a wider tensor, with unit stride over rows, 4 bytes off a 16-byte
    boundary, and broadcast over rows with stride 0 (what y.sum(0) sends back): the f64 gradients in every layout.  The kernels' entry
    points refuse a leading dimension below the row length, so a stride-0 gradient must not be handed to them; dense and column-block
    gradients still reach the kernels."""
    ops = env.ops
    ops.set_matmul_mode(mode)
    for name, make in LAYOUT_NODES.items():
        node, opt = ("chain", {"route": "tail"}) if name == "tail" else (name, {"route": "links"} if name == "chain" else {})
        if name == "tail" and mode == "fp32":
            continue
        t = make()
        if layout == "row_broadcast":
            for k in [k for k in t if k.startswith("gout")]:
                g2 = t[k].reshape(-1, t[k].shape[-1])
                t[k] = g2[:1].expand_as(g2).reshape(t[k].shape).contiguous()
        req = frozenset(cases.grad_names(node, t))
        res = run(env, node, t, req, f"{name} {layout}", opt, layout=layout, tag=f"{mode} {name} {layout}")
        if layout in ("dense", "column_block") and not name.startswith("skinny"):
            _ran(res.calls, must=("wgrad_split_tn",) if mode == "split_bf16" else ("wgrad_tn",))
        if layout in ("dense", "column_block") and name.startswith("skinny"):
            _ran(res.calls, must=("wgrad_skinny",))
        if name == "tail":
            assert res.calls["sb_encoder_tail_bwd"] == 1, res.calls


# ---- f: backward twice -------------------------------------------------------------------------------------------------------------
TWICE = {"linear": (lambda: cases.make_linear(33), {}, "b"), "chain": (lambda: cases.make_chain(33), {"route": "links"}, "ba"),
         "tail": (lambda: cases.make_chain(33), {"route": "tail"}, "ba"), "hops": (lambda: cases.make_hops(11), {}, "bf0"),
         "hop_gru": (lambda: cases.make_hop_gru(11, 3), {}, "bf0"), "gru": (lambda: cases.make_gru(3, 17), {}, "b_ih1"),
         "gru_multi": (lambda: cases.make_gru_multi(2, (15, 17)), {}, "b_ih1_0"), "tail_hop": (lambda: cases.make_tail_hop(11), {}, "ba"),
         "linear_addend": (lambda: cases.make_linear_addend(33), {}, "add"), "linear_nobias": (lambda: cases.make_linear_nobias(33), {}, "x"),
         "skinny_in": (lambda: cases.make_skinny_in(33), {}, "b"), "skinny_out": (lambda: cases.make_skinny_out(33), {}, "b")}


@pytest.mark.parametrize("name", sorted(TWICE))
def test_backward_twice_doubles_every_gradient(env, name):
    """with retain_graph=True a second backward doubles every accumulated .grad bit for bit (x + x is exact) -- also with the bias between
    producer and consumer frozen (the node's own bias or addend where it is no chain; the input for the layer without a bias) --, and a fresh forward / backward afterwards gives the first run's bits: nothing leaks through a link
    or a cached workspace"""
    env.ops.set_matmul_mode("split_bf16")
    make, opt, bias = TWICE[name]
    node = "chain" if name == "tail" else name
    t = make()
    names = frozenset(cases.grad_names(node, t))
    for req in (names, names - {bias}):
        once = run(env, node, t, req, f"twice {name}", opt, tag="once")
        twice = run(env, node, t, req, f"twice {name}", opt, tag="twice", repeat=2)
        again = run(env, node, t, req, f"twice {name}", opt, tag="again")
        for k in req:
            assert _same_bits(twice.grads[k], once.grads[k] + once.grads[k]), (name, k, "the second backward did not double")
            assert _same_bits(again.grads[k], once.grads[k]), (name, k, "a fresh run differs from the first")


# ---- _MsgAgg3, _MsgAgg3Pair --------------------------------------------------------------------------------------------------------
MSG_NAMES = ("W0", "b0", "W1", "b1", "W2", "b2")
MSG_KINDS = ("actor", "critic", "pair")     # ops.msg_agg3(is_critic=False / True), ops.msg_agg3_pair_train


def _msg_reference(t, kind, q_div):
    """tests/msg_ref.py per relation -> [(forward per output, dict with dW, db, amb_W, amb_b)]: the actor under the observed adjacencies,
    the critic under ones, the pair with both outputs and the summed parameter gradients"""
    R = t["p"].shape[0]
    rels = ((t["p"], t["e"].reshape(R, 4), "adj_p", 1), (t["e"], None, "adj_e", 1), (t["o"], None, "adj_o", q_div))
    out = []
    for r, (q, e, adj, qd) in enumerate(rels):
        W, b = t[f"W{r}"], t[f"b{r}"]
        if kind == "critic":
            g = mr.msg_agg(t["p"], q, e, W, b, "ones", q_div=qd, gout=t["gout_a"][:, :, r])
            out.append(((g["out"],), g))
            continue
        g = mr.msg_agg(t["p"], q, e, W, b, "tensor", adj=t[adj], q_div=qd, gout=t["gout_a"][:, :, r], gout_ones=t["gout_c"][:, :, r] if kind == "pair" else None)
        if kind == "pair":
            out.append(((g["out"], mr.msg_agg(t["p"], q, e, W, b, "ones", q_div=qd)["out"]), g))
        else:
            out.append(((g["out"],), g))
    return out


def _msg_census(kind, K, c):
    sorted_o = K > 0 and kind != "actor"      # the critic's all-ones obstacle relation on the sorted kernels (threshold at 1)
    assert c["dhgn_msg_agg_ones_sorted_fwd"] == sorted_o and c["dhgn_msg_agg_ones_sorted_bwd"] == sorted_o, c
    if kind == "pair":
        assert c["dhgn_msg_agg_bwd_pair"] == 2 and c["dhgn_msg_agg_bwd"] == 1, c
        assert c["dhgn_msg_agg3_pair01_fwd"] == (K > 0) and c["dhgn_msg_agg3_pair_fwd"] == (K == 0), c
    elif sorted_o:
        assert (c["dhgn_msg_agg_fwd"], c["dhgn_msg_agg_bwd"], c["dhgn_msg_agg3_fwd"]) == (2, 2, 0), c
    else:
        assert (c["dhgn_msg_agg_fwd"], c["dhgn_msg_agg_bwd"], c["dhgn_msg_agg3_fwd"]) == (0, 3, 1), c


def _msg_run(env, kind, t, req, q_div, ref, tag, layout="dense", repeat=1):
    """forward + backward of a message node with `req` of its six parameters trained -> {name: grad}; the census, the forward and every
    gradient against tests/msg_ref.py (its bounds: 2e-5 forward, 2e-4 max|ref| + the ambiguity budget), None for the frozen ones"""
    ops = env.ops
    L = {k: (v.cuda().clone().requires_grad_(True) if k in req else v.cuda()) for k, v in t.items()}
    for k in env.calls:
        env.calls[k] = 0
    args = (L["p"], L["e"], L["o"], L["adj_p"], L["adj_e"], L["adj_o"], *[L[k] for k in MSG_NAMES])
    if kind == "pair":
        assert ops.msg_agg3_pair_train_ok(L["p"], L["o"], L["W2"], q_div)
        ys, gouts = ops.msg_agg3_pair_train(*args, q_div), (L["gout_a"], L["gout_c"])
    else:
        ys, gouts = (ops.msg_agg3(*args, kind == "critic", None, q_div),), (L["gout_a"],)
    loss = _loss(ys, gouts, layout)
    for r in range(repeat):
        loss.backward(retain_graph=r + 1 < repeat)
    torch.cuda.synchronize()
    _check_arrival(layout, ys[0].numel() // E)
    calls = dict(env.calls)
    if repeat > 1:      # the backward launches once more per backward
        assert all(calls[k] % repeat == 0 for k in calls if k.endswith(("_bwd", "_bwd_pair"))), calls
        calls = {k: (v // repeat if k.endswith(("_bwd", "_bwd_pair")) else v) for k, v in calls.items()}
    _msg_census(kind, t["o"].shape[1], calls)
    grads = {k: L[k].grad for k in MSG_NAMES}
    node = "msg_agg3_pair" if kind == "pair" else "msg_agg3"
    for r in range(3):
        fwd, g = ref[r]
        for y, want in zip(ys, fwd):
            assert mr.fwd_err(y[:, :, r].detach(), want) <= 1.0, (tag, r)
        for k, key, amb in ((f"W{r}", "dW", "amb_W"), (f"b{r}", "db", "amb_b")):
            if k not in req:
                assert grads[k] is None, (tag, k)
                continue
            ratio = mr.grad_err(grads[k] / repeat, g[key], g[amb])
            if ratio > WORST.get(node, (0.0, ""))[0]:
                WORST[node] = (ratio, f"{tag} {k}")
            assert ratio <= 1.0, (tag, k, ratio)
    return grads


def _msg_case(kind, K, P):
    q_div = 5 if P == 8 else 1
    return cases.make_msg_pair(cases.MSG_R, P, K, q_div), q_div


@pytest.mark.parametrize("kind", MSG_KINDS)
@pytest.mark.parametrize("P", cases.MSG_P)
@pytest.mark.parametrize("K", cases.MSG_K)
def test_msg_nodes_under_gradient_subsets(env, K, P, kind):
    """_MsgAgg3 (actor: the observed adjacencies in one launch; critic: ones, a 33-wide obstacle relation on the sorted all-ones
    kernels) and _MsgAgg3Pair at R = 5, P in {3, 8}, with an empty and a 33-wide obstacle relation: each layer frozen in turn, biases
    only, weights only -- None for the frozen tensors, the all-on run's bits for the rest.  The nodes' other inputs are stored data."""
    t, q_div = _msg_case(kind, K, P)
    ref = _msg_reference(t, kind, q_div)
    n = MSG_NAMES
    subs = {"all": set(n), "MSG0 frozen": set(n[2:]), "MSG1 frozen": set(n[:2] + n[4:]), "MSG2 frozen": set(n[:4]), "biases only": {"b0", "b1", "b2"},
            "weights only": {"W0", "W1", "W2"}}
    base = None
    for label, req in subs.items():
        grads = _msg_run(env, kind, t, req, q_div, ref, f"{kind} P={P} K={K} {label}")
        base = base or grads
        for k in req:
            assert _same_bits(grads[k], base[k]), (label, k)


@pytest.mark.parametrize("kind", MSG_KINDS)
@pytest.mark.parametrize("K", cases.MSG_K)
def test_msg_nodes_gradient_layouts_and_second_backward(env, K, kind):
    """the five upstream-gradient layouts and the second backward for the message nodes.  Their kernels read the [E] vectors of the
    gradient with two-float loads from `gout + 4 r E`, so the nodes hand them a dense, 16-byte aligned copy (contiguous() alone keeps a
    dense gradient that starts 4 bytes off): every layout gives the dense run's bits, a second backward doubles them, a fresh run
    repeats them.  A link state does not apply: these nodes produce no ReLU output that another node masks."""
    t, q_div = _msg_case(kind, K, 3)
    ref = _msg_reference(t, kind, q_div)
    req = set(MSG_NAMES)
    dense = _msg_run(env, kind, t, req, q_div, ref, f"{kind} K={K} dense")
    for layout in cases.LAYOUTS[1:4]:
        grads = _msg_run(env, kind, t, req, q_div, ref, f"{kind} K={K} {layout}", layout=layout)
        for k in req:
            assert _same_bits(grads[k], dense[k]), (layout, k)
    tb = dict(t)
    for k in ("gout_a", "gout_c"):
        g2 = t[k].reshape(-1, E)
        tb[k] = g2[:1].expand_as(g2).reshape(t[k].shape).contiguous()
    _msg_run(env, kind, tb, req, q_div, _msg_reference(tb, kind, q_div), f"{kind} K={K} row_broadcast", layout="row_broadcast")
    twice = _msg_run(env, kind, t, req, q_div, ref, f"{kind} K={K} twice", repeat=2)
    again = _msg_run(env, kind, t, req, q_div, ref, f"{kind} K={K} again")
    for k in req:
        assert _same_bits(twice[k], dense[k] + dense[k]), (k, "the second backward did not double")
        assert _same_bits(again[k], dense[k]), (k, "a fresh run differs from the first")


# ---- g: one consumer per linked activation -----------------------------------------------------------------------------------------
VIEWS = ("ViewBackward", "ReshapeAliasBackward", "UnsafeViewBackward", "AliasBackward")


def _graph(root):
    nodes, stack, users = [], [root], {}
    seen = set()
    while stack:
        n = stack.pop()
        if n is None or id(n) in seen:
            continue
        seen.add(id(n))
        nodes.append(n)
        for m, idx in n.next_functions:
            if m is not None:
                users.setdefault((id(m), idx), []).append(n)
                stack.append(m)
    return nodes, users


def linked_outputs(loss):
    """[(producer node, number of nodes that consume its linked output, looking through pure views)] for every node of loss's graph
    that offered a ReluLink with its output (_Linear with y_link, every _FcraHop)"""
    nodes, users = _graph(loss.grad_fn)
    out = []
    for n in nodes:
        if getattr(n, "y_link", None) is None:
            continue
        cur, count = n, None
        while True:
            us = users.get((id(cur), 0), [])
            count = len(us)
            if count == 1 and type(us[0]).__name__.startswith(VIEWS):
                cur = us[0]
                continue
            break
        out.append((n, count))
    return out


def _dhgn_loss(ops, depth, tail):
    from distributed_multi_agent_reinforcement_learning_amd.model import build_actor_critic, sequence_forward_pair
    from tests.helpers import product_cfg
    P, K, batch, steps = 3, 33, 2, 3
    R = batch * steps
    ops.ENCODER_TAIL_TRAIN_MIN_ROWS = 1 if tail else 10 ** 9
    cfg = product_cfg(P, 20, 20, T=steps, depth=depth)
    torch.manual_seed(2)
    actor, critic = build_actor_critic(cfg, "cuda")
    actor, critic = actor.cuda(), critic.cuda()
    t = cases.make_msg_pair(R, P, K, 1)
    obs = dict(p_state=t["p"].cuda(), e_state=t["e"].cuda(), o_state=t["o"].cuda(), p_adj=t["adj_p"].cuda(), e_adj=t["adj_e"].cuda(), o_adj=t["adj_o"].cuda())
    g = torch.Generator().manual_seed(9)
    hist_a = [torch.randn(R, P, E, generator=g).cuda() for _ in range(depth)]
    hist_c = [torch.randn(R, P, E, generator=g).cuda() for _ in range(depth)]
    prob, values = sequence_forward_pair(actor, critic, obs, hist_a, hist_c, batch, steps)
    w = torch.randn(prob.shape, generator=g).cuda()
    return (prob * w).sum() + values.sum(), actor, critic


@pytest.mark.parametrize("tail", [True, False])
@pytest.mark.parametrize("depth", [0, 2])
def test_every_linked_activation_of_the_dhgn_update_has_one_consumer(env, depth, tail):
    """DHGN.encoder_pair_train + fcra + gru_multi (models.sequence_forward_pair) at depth 0 and 2, the encoder tail fused and as two linked
    layers: every output that carries a ReluLink (y_link of the AGG layer, carry[1] of every hop, relu_link of the last hop) is read by
    exactly one node -- autograd would otherwise add another gradient to a masked one.  The backward then runs and leaves no db."""
    ops = env.ops
    ops.set_matmul_mode("split_bf16")
    loss, actor, critic = _dhgn_loss(ops, depth, tail)
    found = linked_outputs(loss)
    want = 2 * depth + (0 if tail else 2)        # per network: one link per hop, one for the AGG layer when the tail is not fused
    assert len(found) == want, [type(n).__name__ for n, _ in found]
    for n, count in found:
        assert count == 1, (type(n).__name__, count)
    links = [n.y_link for n, _ in found]
    loss.backward()
    torch.cuda.synchronize()
    assert all(l.db is None for l in links)
    grads = [p.grad for p in actor.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)


def test_the_cfg5_attention_agent_offers_no_links(env):
    """the env_3d agent with algo.e3d_comm: attention and algo.e3d_critic: central: its update graph holds _Linear and _GRULayerMulti nodes
    but no ReluLink -- nothing there may be masked by a consumer"""
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    N, T, P = 2, 3, 3
    cfg = baseline_config("cfg5", **{"runtime.num_envs": N, "env.max_steps": T, "env.num_defender": P, "algo.e3d_comm": "attention",
                                     "algo.e3d_features": "pursuit", "algo.e3d_critic": "central"})
    torch.manual_seed(1)
    agent = E3dMAPPO(cfg, N, 1)
    g = torch.Generator().manual_seed(4)
    fa, fc = torch.randn(N, T, P, agent.feat_dim, generator=g).cuda(), torch.randn(N, T, P, agent.critic_feat_dim, generator=g).cuda()
    words = torch.full((N, T, P), (1 << P) - 1, dtype=torch.int64, device="cuda")
    with torch.enable_grad():
        mu, values = agent.sequence_forward(fa, fc, N, T, words=words)
        loss = mu.sum() + values.sum()
    nodes, _ = _graph(loss.grad_fn)
    kinds = {type(n).__name__ for n in nodes}
    assert {"_LinearBackward", "_GRULayerMultiBackward", "_TeamAttentionBackward"} <= kinds, kinds
    assert linked_outputs(loss) == []
    assert all(getattr(n, "x_link", None) is None and getattr(n, "x_links", None) is None for n in nodes)


def test_a_second_reader_of_a_linked_activation_is_found(env):
    """the negative control: a hand-made chain whose linked activation also feeds a sum -- the walk finds two consumers"""
    ops = env.ops
    ops.set_matmul_mode("split_bf16")
    t = cases.make_chain(33)
    L = _leaves("chain", t, frozenset(cases.grad_names("chain", t)))
    link = ops.ReluLink()
    emb = ops.linear(L["m3"], L["Wa"], L["ba"], relu=True, y_link=link)
    y = ops.linear(emb.reshape(33, 3 * E), L["Ws"], L["add"].clone(), consume_addend=True, x_link=link)
    (only,) = linked_outputs(y.sum())
    assert only[1] == 1
    (both,) = linked_outputs(y.sum() + emb.sum())
    assert both[1] == 2
