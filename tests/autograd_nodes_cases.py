"""Case tables, operands and f64 restatements for the autograd nodes of ops.py (_Linear, _SkinnyLinear, _FcraHop, _EncoderTailTrain,
_GRULayer, _GRULayerMulti with _gru_dw_hh, _MsgAgg3, _MsgAgg3Pair) and the ReluLink hand-over between them.  No GPU needed to import.

A restatement is the node's mathematics as a plain torch expression (F.linear, torch.relu, torch.cat, a step-by-step GRU) evaluated
under ordinary torch autograd in whatever dtype / device its operands have.  ReLU's derivative is discontinuous: an activation within
rounding noise of zero may fall on either side in fp32 and f64, which moves a weight gradient by a whole row's contribution.  So
every restatement takes `masks`: None evaluates the plain ReLU network (and reports its own masks); a dict replaces each relu(z) by
z * mask -- the same function wherever the masks agree -- so that gradients are compared under the masks of the forward pass under
test (tests/test_ops_gpu.py::test_fcra_hop_forward_and_backward_match_f64), whose forward is held to the plain network separately and
whose masks may differ from the plain f64 network's in at most MASK_CAP of the elements.

Bound (tests/test_update_parity_gpu.py, tests/test_team_attention_gpu.py::_check): err <= 4 noise + 2e-5 scale per gradient tensor,
noise = the larger distance from f64 of the same restatement evaluated in fp32 on the CPU and (when there is one) on the GPU, scale =
max |f64 tensor|; forward outputs: 2e-5 scale against the plain f64 network.
"""
import itertools

import torch
import torch.nn.functional as F

E = H = 128
GRAD_NOISE_FACTOR, GRAD_REL_FLOOR, FWD_REL = 4.0, 2e-5, 2e-5
MASK_CAP = 1e-3                      # fraction of ReLU decisions that may differ from the plain f64 network's

LINEAR_ROWS = (1, 31, 32, 33, 69)    # around the 32-row tile of k_sb_gemm_n128
THRESHOLD_ROWS = 33
HOP_P, HOP_ROWS = 3, (3, 33, 99)     # R P
GRU_T, GRU_B, GRU_AGENTS = (2, 3), (15, 16, 17), (0, 3)
MSG_R, MSG_P, MSG_K = 5, (3, 8), (0, 33)
LAYOUTS = ("dense", "column_block", "transposed", "off_by_4_bytes", "row_broadcast")


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _n(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


def make_linear(rows, seed=0):
    """relu(x W^T + b), 128 -> 128 (_Linear, a 1-D bias, ReLU)"""
    g = _gen(100 + seed)
    return dict(x=_n(g, rows, E), W=_n(g, E, E, scale=0.2), b=_n(g, E, scale=0.6, shift=0.55), gout=_n(g, rows, E))


def make_linear_addend(rows, seed=0):
    """x W^T + add, 384 -> 128 (_Linear, a full addend as bias, no ReLU)"""
    g = _gen(200 + seed)
    return dict(x=_n(g, rows, 3 * E), W=_n(g, E, 3 * E, scale=0.1), add=_n(g, rows, E), gout=_n(g, rows, E))


def make_linear_nobias(rows, seed=0):
    """x W^T, 128 -> 256 (_Linear, no bias)"""
    g = _gen(300 + seed)
    return dict(x=_n(g, rows, E), W=_n(g, 2 * E, E, scale=0.2), gout=_n(g, rows, 2 * E))


def make_skinny_in(rows, seed=0):
    """x W^T + b, 4 -> 128 (_SkinnyLinear: the position part of the semantic layer)"""
    g = _gen(400 + seed)
    return dict(x=_n(g, rows, 4), W=_n(g, E, 4, scale=0.3), b=_n(g, E, scale=0.2), gout=_n(g, rows, E))


def make_skinny_out(rows, seed=0):
    """x W^T + b, 128 -> 5 (_SkinnyLinear: a head)"""
    g = _gen(500 + seed)
    return dict(x=_n(g, rows, E), W=_n(g, 5, E, scale=0.3), b=_n(g, 5, scale=0.2), gout=_n(g, rows, 5))


def make_chain(rows, seed=0):
    """relu(m3 Wa^T + ba) -> (rows, 384) Ws^T + add: DHGN._after_messages, as two linked _Linear nodes or one _EncoderTailTrain"""
    g = _gen(600 + seed)
    return dict(m3=_n(g, rows, 3, E), Wa=_n(g, E, E, scale=0.1), ba=_n(g, E, scale=0.6, shift=0.55), Ws=_n(g, E, 3 * E, scale=0.1),
                add=_n(g, rows, E), gout=_n(g, rows, E))


def make_hops(R, P=HOP_P, seed=0):
    """two hops of DHGN.fcra: h' = relu([relu(nb Wagg^T + bagg) | h] Wf^T + bf); nb is stored data"""
    g = _gen(700 + seed)
    t = dict(h=_n(g, R, P, E, scale=0.5), gout=_n(g, R, P, E))
    for k in range(2):
        t.update({f"nb{k}": _n(g, R, P, E, scale=0.5), f"Wagg{k}": _n(g, E, E, scale=0.2), f"bagg{k}": _n(g, E, scale=0.6, shift=0.55),
                  f"Wf{k}": _n(g, E, 2 * E, scale=0.15), f"bf{k}": _n(g, E, scale=0.6, shift=0.55)})
    return t


def make_gru(T, B, seed=0, layers=2, tag=""):
    """a two-layer GRU over T steps of B sequences: x (T, B, 128) time-major, h0 (layers, B, 128)"""
    g = _gen(800 + seed)
    t = {f"x{tag}": _n(g, T, B, H), f"h0{tag}": _n(g, layers, B, H, scale=0.5), f"gout{tag}": _n(g, T, B, H)}
    for l in range(layers):
        t.update({f"w_ih{l}{tag}": _n(g, 3 * H, H, scale=0.1), f"w_hh{l}{tag}": _n(g, 3 * H, H, scale=0.1),
                  f"b_ih{l}{tag}": _n(g, 3 * H, scale=0.1), f"b_hh{l}{tag}": _n(g, 3 * H, scale=0.1)})
    return t


def make_gru_multi(T, Bs, seed=0):
    """len(Bs) independent two-layer GRUs (tags _0, _1, ..), each as make_gru"""
    t = {}
    for k, B in enumerate(Bs):
        t.update(make_gru(T, B, seed=10 * seed + k, tag=f"_{k}"))
    return t


def make_hop_gru(episodes, T, P=HOP_P, seed=0):
    """one (last) hop on R = episodes T rows of P agents, its output the input of a two-layer GRU in (episode, step, agent) row order"""
    g = _gen(900 + seed)
    R, B = episodes * T, episodes * P
    t = dict(h=_n(g, R, P, E, scale=0.5), nb0=_n(g, R, P, E, scale=0.5), Wagg0=_n(g, E, E, scale=0.2), bagg0=_n(g, E, scale=0.6, shift=0.55),
             Wf0=_n(g, E, 2 * E, scale=0.15), bf0=_n(g, E, scale=0.6, shift=0.55))
    gru = make_gru(T, B, seed=50 + seed)
    del gru["x"]
    t.update(gru)
    return t


def make_tail_hop(R, P=HOP_P, seed=0):
    """the encoder tail on R P rows, its output the h of one (last) hop"""
    g = _gen(1000 + seed)
    rows = R * P
    return dict(m3=_n(g, rows, 3, E), Wa=_n(g, E, E, scale=0.1), ba=_n(g, E, scale=0.6, shift=0.55), Ws=_n(g, E, 3 * E, scale=0.1),
                add=_n(g, rows, E), nb0=_n(g, R, P, E, scale=0.5), Wagg0=_n(g, E, E, scale=0.2), bagg0=_n(g, E, scale=0.6, shift=0.55),
                Wf0=_n(g, E, 2 * E, scale=0.15), bf0=_n(g, E, scale=0.6, shift=0.55), gout=_n(g, R, P, E))


def make_msg_pair(R, P, K, q_div, seed=0):
    """the operands of ops.msg_agg3_pair_train: p (R, P, 4), e (R, 1, 4), o (R / q_div, K, 4), float adjacencies, three MSG layers"""
    g = _gen(1100 + seed)
    t = dict(p=_n(g, R, P, 4), e=_n(g, R, 1, 4), o=_n(g, R // q_div, K, 4),
             adj_p=(torch.rand(R, P, P, generator=g) < 0.6).float(), adj_e=(torch.rand(R, P, 1, generator=g) < 0.8).float(),
             adj_o=(torch.rand(R, P, K, generator=g) < 0.3).float(),
             W0=_n(g, E, 8, scale=0.3), b0=_n(g, E, scale=0.3, shift=0.2), W1=_n(g, E, 4, scale=0.3), b1=_n(g, E, scale=0.3, shift=0.2),
             W2=_n(g, E, 4, scale=0.3), b2=_n(g, E, scale=0.3, shift=0.2), gout_a=_n(g, R, P, 3, E), gout_c=_n(g, R, P, 3, E))
    return t


# ---- restatements: fn(t, masks) -> (y or tuple of ys, {name: relu decisions}) ------------------------------------------------------
def _relu(z, masks, key, seen):
    """relu(z), or z * masks[key]; records the decisions taken"""
    if masks is None:
        seen[key] = z.detach() > 0
        return torch.relu(z)
    m = masks[key].to(device=z.device).reshape(z.shape)
    seen[key] = m != 0
    return z * m.to(z.dtype)


def ref_linear(t, masks=None):
    seen = {}
    return _relu(F.linear(t["x"], t["W"], t["b"]), masks, "y", seen), seen


def ref_linear_addend(t, masks=None):
    return F.linear(t["x"], t["W"]) + t["add"], {}


def ref_linear_nobias(t, masks=None):
    return F.linear(t["x"], t["W"]), {}


def ref_skinny(t, masks=None):
    return F.linear(t["x"], t["W"], t["b"]), {}


def ref_chain(t, masks=None):
    seen = {}
    emb = _relu(F.linear(t["m3"], t["Wa"], t["ba"]), masks, "emb", seen)
    return F.linear(emb.reshape(emb.shape[0], 3 * E), t["Ws"]) + t["add"], seen


def _hop(t, k, h, masks, seen):
    agg = _relu(F.linear(t[f"nb{k}"], t[f"Wagg{k}"], t[f"bagg{k}"]), masks, f"agg{k}", seen)
    return _relu(F.linear(torch.cat((agg, h), -1), t[f"Wf{k}"], t[f"bf{k}"]), masks, f"y{k}", seen)


def ref_hops(t, masks=None):
    seen = {}
    h = t["h"]
    for k in range(2):
        h = _hop(t, k, h, masks, seen)
    return h, seen


def gru_layer(x, h0, w_ih, w_hh, b_ih, b_hh):
    """torch.nn.GRU's layer, step by step (tests/test_gru_seq_lds_prefetch_gpu.py::_reference): x (T, B, I) -> (T, B, H)"""
    h, hs = h0, []
    for t in range(x.shape[0]):
        gi, gh = F.linear(x[t], w_ih, b_ih), F.linear(h, w_hh, b_hh)
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        hs.append(h)
    return torch.stack(hs)


def time_major(rows, T, B, agents):
    """(T B, C) rows in (episode, step, agent) order (sequence b = episode agents + agent) -> (T, B, C); agents = 0: already time-major"""
    if not agents:
        return rows.reshape(T, B, -1)
    return rows.reshape(B // agents, T, agents, -1).permute(1, 0, 2, 3).reshape(T, B, -1)


def agent_rows(x, agents):
    """inverse of time_major: (T, B, C) -> (T B, C) rows in (episode, step, agent) order"""
    T, B, C = x.shape
    return x.reshape(T, B // agents, agents, C).permute(1, 0, 2, 3).reshape(T * B, C)


def _gru_stack(t, x, tag="", layers=2):
    for l in range(layers):
        x = gru_layer(x, t[f"h0{tag}"][l], t[f"w_ih{l}{tag}"], t[f"w_hh{l}{tag}"], t[f"b_ih{l}{tag}"], t[f"b_hh{l}{tag}"])
    return x


def ref_gru(t, masks=None):
    return _gru_stack(t, t["x"]), {}


def ref_gru_multi(t, masks=None):
    n = sum(1 for k in t if k.startswith("x_"))
    return tuple(_gru_stack(t, t[f"x_{k}"], f"_{k}") for k in range(n)), {}


def ref_hop_gru(t, masks=None):
    seen = {}
    T, B = t["gout"].shape[:2]
    y = _hop(t, 0, t["h"], masks, seen)
    return _gru_stack(t, time_major(y.reshape(-1, E), T, B, y.shape[1])), seen


def ref_tail_hop(t, masks=None):
    seen = {}
    emb = _relu(F.linear(t["m3"], t["Wa"], t["ba"]), masks, "emb", seen)
    h = (F.linear(emb.reshape(emb.shape[0], 3 * E), t["Ws"]) + t["add"]).reshape(t["nb0"].shape)
    return _hop(t, 0, h, masks, seen), seen


# name -> (restatement, tensors that never carry a gradient, the node's inputs (the rest are parameters))
NODES = {
    "linear": (ref_linear, (), ("x",)),
    "linear_addend": (ref_linear_addend, (), ("x", "add")),
    "linear_nobias": (ref_linear_nobias, (), ("x",)),
    "skinny_in": (ref_skinny, (), ("x",)),
    "skinny_out": (ref_skinny, (), ("x",)),
    "chain": (ref_chain, (), ("m3", "add")),
    "hops": (ref_hops, ("nb0", "nb1"), ("h",)),
    "gru": (ref_gru, (), ("x", "h0")),
    "gru_multi": (ref_gru_multi, (), None),
    "hop_gru": (ref_hop_gru, ("nb0",), ("h", "h0")),
    "tail_hop": (ref_tail_hop, ("nb0",), ("m3", "add")),
}


def grad_names(node, t):
    """the tensors of `t` that may require a gradient, in the table's order"""
    stored = NODES[node][1]
    return [k for k in t if not k.startswith("gout") and k not in stored]


def input_names(node, t):
    ins = NODES[node][2]
    if ins is None:      # gru_multi: x_k and h0_k of every network
        return [k for k in grad_names(node, t) if k.startswith(("x_", "h0_"))]
    return list(ins)


def subsets(node, t, chain_split=None):
    """{label: frozenset of tensors requiring a gradient}: all on, each single tensor frozen, inputs only, parameters only, and for a
    chain (chain_split = the producer's tensors) producer wholly frozen / consumer wholly frozen"""
    names = grad_names(node, t)
    ins = [k for k in input_names(node, t) if k in names]
    out = {"all": frozenset(names)}
    for k in names:
        out[f"frozen:{k}"] = frozenset(n for n in names if n != k)
    out["inputs_only"] = frozenset(ins)
    out["parameters_only"] = frozenset(n for n in names if n not in ins)
    if chain_split is not None:
        prod = frozenset(chain_split)
        out["producer_frozen"] = frozenset(n for n in names if n not in prod)
        out["consumer_frozen"] = frozenset(n for n in names if n in prod)
    return out


CHAIN_PRODUCERS = {"chain": ("m3", "Wa", "ba"), "hops": ("h", "Wagg0", "bagg0", "Wf0", "bf0"),
                   "hop_gru": ("h", "Wagg0", "bagg0", "Wf0", "bf0"), "tail_hop": ("m3", "Wa", "ba", "Ws", "add")}


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------
def _gouts(t):
    return [t[k] for k in t if k.startswith("gout")]


def evaluate(node, t, masks=None, dtype=torch.float64, device="cpu"):
    """the restatement and all its gradients under torch autograd -> (outputs tuple, {name: grad}, relu decisions)"""
    fn = NODES[node][0]
    names = grad_names(node, t)
    tt = {k: v.to(device=device, dtype=dtype if v.is_floating_point() else v.dtype) for k, v in t.items()}
    for k in names:
        tt[k] = tt[k].clone().requires_grad_(True)
    y, seen = fn(tt, masks)
    ys = y if isinstance(y, tuple) else (y,)
    loss = sum((a * g).sum() for a, g in zip(ys, _gouts(tt)))
    grads = torch.autograd.grad(loss, [tt[k] for k in names], allow_unused=True)
    return tuple(a.detach() for a in ys), {k: g for k, g in zip(names, grads)}, seen


def mask_mismatch(a, b):
    """(elements whose relu decisions differ, elements) over the masks both dicts hold"""
    bad = tot = 0
    for k in a:
        x, y = a[k].cpu().reshape(-1) != 0, b[k].cpu().reshape(-1) != 0
        bad += int((x != y).sum())
        tot += x.numel()
    return bad, tot


class Reference:
    """f64 gradients of a case under given masks, with the fp32 noise of each tensor and the plain f64 network's forward"""

    def __init__(self, node, t, masks, gpu=False):
        self.plain_y, _, self.plain_masks = evaluate(node, t, None)
        m = {k: v.cpu() for k, v in masks.items()} if masks else None
        self.y, self.grads, _ = evaluate(node, t, m if m else None)
        runs = [evaluate(node, t, m if m else None, torch.float32, "cpu")[1]]
        if gpu:
            runs.append(evaluate(node, t, m if m else None, torch.float32, "cuda")[1])
        self.noise, self.scale = {}, {}
        for k, g in self.grads.items():
            self.noise[k] = max(float((r[k].double().cpu() - g).abs().max()) for r in runs)
            self.scale[k] = float(g.abs().max())
        self.mismatch = mask_mismatch(m, self.plain_masks) if m else (0, 0)

    def bound(self, k):
        return GRAD_NOISE_FACTOR * self.noise[k] + GRAD_REL_FLOOR * self.scale[k]

    def ratio(self, k, grad):
        """|grad - f64| / bound"""
        err = float((grad.detach().double().cpu() - self.grads[k]).abs().max())
        b = self.bound(k)
        return err / b if b > 0 else (0.0 if err == 0 else float("inf"))


# ---- thresholds: (name in ops, the node whose route it selects, the row count (steps for the GRU) it is set to and to one above) ----
def threshold_cases():
    R = THRESHOLD_ROWS
    return [
        ("WGRAD_MIN_ROWS", "linear_nobias", R),
        ("RELU_BWD_MIN_ROWS", "linear", R),
        ("SKINNY_MIN_ROWS", "skinny_in", R),
        ("MASKED_GRAD_MIN_ROWS", "chain", R),
        ("ENCODER_TAIL_TRAIN_MIN_ROWS", "chain", R),
        ("PERSISTENT_GRU_MIN_T", "gru", 2),
    ]


def gru_shapes():
    """(T, sequences, agents): GRU_B sequences, times `agents` where the rows come in (episode, step, agent) order"""
    return [(T, B * max(a, 1), a) for T, B, a in itertools.product(GRU_T, GRU_B, GRU_AGENTS)]
