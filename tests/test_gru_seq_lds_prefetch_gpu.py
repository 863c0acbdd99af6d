"""The split-bf16 GRU sequence backward (csrc/sb_gru_seq.hpp k_gru_seq_bwd_sb) feeds its six per-step inputs through an LDS ring that
LDS-direct loads fill two steps ahead, with hand-counted vmcnt waits.  What that adds to get wrong sits at the ring's edges: sequences
shorter than the pipeline is deep (T = 1, 2, 3), dead rows and tail tiles (B = 1, 15, 16, 17), the benchmark's two mini-batch sizes
(3 280, 3 248), ragged records in one launch, both row orders, both output forms (dnr / full dgh) and launches with and without the
bias gradients.  Every backward output, and the forward's `out` of both routes (k_gru_seq_fwd_sb, k_gru_seq_fwd2) at the same edges,
is held to an f64 torch autograd GRU beside the fp32-route kernels (k_gru_seq_bwd2), with the bound of tests/test_split_bf16_gpu.py::test_split_gru_sequence_matches_f64_beside_the_fp32_kernels; launches repeat bit for bit and a
captured graph replays the eager result.  Reference op: torch.nn.GRU over T steps, DHGN/mappo_parallel.py:397, :432-436."""
import ctypes as C

import pytest
import torch

from tests.helpers import no_gc_during_capture

pytestmark = pytest.mark.gpu

H = 128


def _inputs(T, Bs, agents, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    recs = []
    for B in Bs:
        recs.append(dict(B=B,
                         gi=torch.randn(T * B, 3 * H, device="cuda", generator=gen),       # rows in the launch's gi order
                         w=torch.randn(3 * H, H, device="cuda", generator=gen) * 0.08,
                         b=torch.randn(3 * H, device="cuda", generator=gen) * 0.1,
                         h0=torch.randn(B, H, device="cuda", generator=gen) * 0.5,
                         dout=torch.randn(T, B, H, device="cuda", generator=gen)))
    return recs


def _time_major(rows, T, B, agents):
    """[T B][C] rows in the launch's gi order -> [T][B][C]"""
    if not agents:
        return rows.reshape(T, B, -1)
    return rows.reshape(B // agents, T, agents, -1).permute(1, 0, 2, 3).reshape(T, B, -1)


def _forms(form, bias, k):
    """per record: (full dgh form?, bias gradients requested?); "mixed" alternates both over the records of a launch"""
    if form == "mixed":
        return k % 2 == 1, k % 3 != 1
    return form == "dgh", bias


def _launch(route, T, recs, agents, form, bias, fwd=True):
    """forward (saving the gates) and backward on one route through the C ABI; returns per record the dict of backward outputs"""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    L = ops.load_library()
    f_fwd, f_bwd = ((L.gru_seq_split_fwd_multi, L.gru_seq_split_bwd_multi) if route == "split" else (L.gru_seq_fwd_multi, L.gru_seq_bwd_multi))
    n = len(recs)
    fa, ba = (ops.GruSeqNet * n)(), (ops.GruSeqBwdNet * n)()
    outs = []
    for k, r in enumerate(recs):
        B = r["B"]
        full, wb = _forms(form, bias, k)
        if fwd:
            r["out"] = torch.empty(T, B, H, device="cuda")
            r["save"] = torch.empty(L.gru_seq_save_elems(T, B), device="cuda")
        o = dict(dgi=torch.full((T * B, 3 * H), float("nan"), device="cuda"), dh0=torch.full((B, H), float("nan"), device="cuda"))
        if full:
            o["dgh"] = torch.full((T, B, 3 * H), float("nan"), device="cuda")
        else:
            o["dnr"] = torch.full((T, B, H), float("nan"), device="cuda")
        if wb:
            o["db_ih"] = torch.full((3 * H,), float("nan"), device="cuda")
            o["db_hh"] = torch.full((3 * H,), float("nan"), device="cuda")
            o["_ws"] = torch.empty(L.gru_seq_bwd_workspace(B), dtype=torch.uint8, device="cuda")
        a = fa[k]
        a.gi, a.w_hh, a.b_hh, a.h0, a.out, a.save, a.B = (r["gi"].data_ptr(), r["w"].data_ptr(), r["b"].data_ptr(), r["h0"].data_ptr(),
                                                          r["out"].data_ptr(), r["save"].data_ptr(), B)
        a = ba[k]
        a.dout, a.save, a.out, a.h0, a.w_hh, a.dgi = (r["dout"].data_ptr(), r["save"].data_ptr(), r["out"].data_ptr(), r["h0"].data_ptr(),
                                                      r["w"].data_ptr(), o["dgi"].data_ptr())
        a.dgh = o["dgh"].data_ptr() if full else None
        a.dnr = None if full else o["dnr"].data_ptr()
        a.dh0 = o["dh0"].data_ptr()
        a.db_ih = o["db_ih"].data_ptr() if wb else None
        a.db_hh = o["db_hh"].data_ptr() if wb else None
        a.workspace = o["_ws"].data_ptr() if wb else None
        a.B = B
        outs.append(o)
    Bmax = max(r["B"] for r in recs)
    if fwd:
        ops._check(f_fwd(n, C.cast(fa, C.c_void_p), T, Bmax, H, agents, ops._stream()), "gru_seq forward")
    ops._check(f_bwd(n, C.cast(ba, C.c_void_p), T, Bmax, H, agents, ops._stream()), "gru_seq backward")
    torch.cuda.synchronize()
    return outs


def _reference(T, r, agents):
    """f64 autograd of the recurrence on the same gi: dgi (launch row order), dgh [T][B][3H], dh0, db_ih, db_hh"""
    B = r["B"]
    gi = r["gi"].double().requires_grad_(True)
    w, b = r["w"].double(), r["b"].double().requires_grad_(True)
    h0 = r["h0"].double().requires_grad_(True)
    git = _time_major(gi, T, B, agents)
    h, hs, ghs = h0, [], []
    for t in range(T):
        gh = h @ w.t()
        gh.retain_grad()
        ghs.append(gh)
        g, ghb = git[t], gh + b
        rg = torch.sigmoid(g[:, :H] + ghb[:, :H])
        z = torch.sigmoid(g[:, H:2 * H] + ghb[:, H:2 * H])
        nn = torch.tanh(g[:, 2 * H:] + rg * ghb[:, 2 * H:])
        h = (1 - z) * nn + z * h
        hs.append(h)
    (torch.stack(hs) * r["dout"].double()).sum().backward()
    dgh = torch.stack([g.grad for g in ghs])
    return dict(dgi=gi.grad, dgh=dgh, dnr=dgh[:, :, 2 * H:], dh0=h0.grad, db_ih=gi.grad.sum(0), db_hh=b.grad, out=torch.stack(hs).detach())


def _err(a, ref):
    return float((a.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


SMALL = [(T, [B], 0, "dnr", True) for T in (1, 2, 3, 150) for B in (1, 15, 16, 17)]
SMALL += [(T, [B], 0, "dgh", False) for T in (1, 3) for B in (15, 17)]
LARGE = [(150, [3280], 8, "dgh", True), (150, [3248], 0, "dnr", True), (3, [3280], 0, "dnr", False), (2, [3248], 8, "dgh", True),
         (1, [3280], 0, "dgh", True), (150, [16], 8, "dgh", True), (3, [15], 5, "dgh", False), (2, [17], 17, "dgh", True)]
RAGGED = [(150, [3280, 17, 3248, 1, 16], 0, "mixed", True), (2, [17, 3280, 1], 0, "mixed", True), (3, [3248, 16, 3280], 8, "dgh", True),
          (1, [15, 1, 17], 0, "mixed", True)]


@pytest.mark.parametrize("T,Bs,agents,form,bias", SMALL + LARGE + RAGGED)
def test_split_backward_matches_f64_beside_the_fp32_route(T, Bs, agents, form, bias):
    """every backward output of k_gru_seq_bwd_sb and the forward's `out` (the live rows, time-major) against f64, with the fp32 route's
    error beside it (the bound of test_split_gru_sequence_matches_f64_beside_the_fp32_kernels: e_split <= 2 e_fp32 + 2e-6 and
    e_split < 2e-5, errors relative to the tensor's largest reference magnitude); the fp32 route's `out` on its own below 2e-6"""
    recs = _inputs(T, Bs, agents, 1000 * T + sum(Bs) + agents)
    got = {}
    for route in ("fp32", "split"):
        got[route] = _launch(route, T, recs, agents, form, bias)
        for o, r in zip(got[route], recs):
            o["out"] = r["out"]          # this route's forward output, time-major [T][B][H] (the next launch allocates its own)
    for k, r in enumerate(recs):
        ref = _reference(T, r, agents)
        for nm, a in got["split"][k].items():
            if nm.startswith("_"):
                continue
            assert torch.isfinite(a).all(), (k, nm)
            e_s, e_f = _err(a, ref[nm]), _err(got["fp32"][k][nm], ref[nm])
            print(f"T={T} B={r['B']} agents={agents} record {k} {nm}: split {e_s:.3e} fp32 {e_f:.3e}")
            assert e_s <= 2.0 * e_f + 2e-6, (k, nm, e_s, e_f)
            assert e_s < 2e-5, (k, nm, e_s)
            if nm == "out":              # the fp32 route's forward on its own (the figure of test_split_gru_sequence_matches_f64_.. for `out`)
                assert torch.isfinite(got["fp32"][k][nm]).all(), (k, nm)
                assert e_f < 2e-6, (k, nm, e_f)


@pytest.mark.parametrize("T,Bs,agents,form", [(150, [3280, 17, 3248], 0, "mixed"), (3, [17, 1, 3280], 8, "dgh"), (2, [15], 0, "dnr"), (1, [16, 17], 0, "mixed")])
def test_split_backward_repeats_bit_for_bit(T, Bs, agents, form):
    """three launches on the same saved gates give the same bits in every output"""
    if agents:
        Bs = [b if b % agents == 0 else agents * b for b in Bs]
    recs = _inputs(T, Bs, agents, 7 + T)
    first = _launch("split", T, recs, agents, form, True)
    for _ in range(2):
        again = _launch("split", T, recs, agents, form, True, fwd=False)
        for k, o in enumerate(first):
            for nm, a in o.items():
                if not nm.startswith("_"):
                    assert torch.equal(a, again[k][nm]), (k, nm)


@pytest.mark.parametrize("T,B,agents", [(150, 3280, 8), (3, 17, 0), (2, 16, 8)])
def test_split_backward_through_ops_and_in_a_captured_graph(T, B, agents):
    """ops.gru (two layers, SEQ_MODE split_bf16) against an f64 torch.nn.GRU beside the fp32 route, and the backward launch replayed from
    a captured graph against the eager launch, bit for bit"""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    torch.manual_seed(T + B)
    mod = torch.nn.GRU(H, H, 2).cuda()
    gen = torch.Generator(device="cuda").manual_seed(11)
    n = B // agents if agents else 0
    x = torch.randn(n * T * agents, H, device="cuda", generator=gen) if agents else torch.randn(T, B, H, device="cuda", generator=gen)
    h0 = torch.randn(2, B, H, device="cuda", generator=gen) * 0.5
    gout = torch.randn(T, B, H, device="cuda", generator=gen)
    m64 = torch.nn.GRU(H, H, 2).cuda().double()
    m64.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
    x64, h64 = x.double().requires_grad_(True), h0.double().requires_grad_(True)
    xin = x64.reshape(n, T, agents, H).permute(1, 0, 2, 3).reshape(T, B, H) if agents else x64
    o64, _ = m64(xin, h64)
    (o64 * gout.double()).sum().backward()
    ref = [x64.grad, h64.grad] + [p.grad for p in m64.parameters()]
    names = ["dx", "dh0"] + [k for k, _ in mod.named_parameters()]

    def run(mode):
        old = ops.SEQ_MODE
        try:
            ops.SEQ_MODE = mode
            xs, hs = x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
            mod.zero_grad()
            out, _ = ops.gru(xs, hs, mod, agents=agents, steps=T) if agents else ops.gru(xs, hs, mod)
            (out * gout).sum().backward()
        finally:
            ops.SEQ_MODE = old
        return [xs.grad, hs.grad] + [p.grad.clone() for p in mod.parameters()]

    split, fp32 = run("split_bf16"), run("fp32")
    for nm, a, f, r in zip(names, split, fp32, ref):
        e_s, e_f = _err(a, r), _err(f, r)
        print(f"ops.gru T={T} B={B} agents={agents} {nm}: split {e_s:.3e} fp32 {e_f:.3e}")
        assert e_s <= 2.0 * e_f + 2e-6, (nm, e_s, e_f)
        assert e_s < 2e-5, (nm, e_s)

    # the backward launch alone, eager and replayed from a graph
    recs = _inputs(T, [B, 17 * max(agents, 1)], agents, 3)
    eager = _launch("split", T, recs, agents, "dgh" if agents else "mixed", True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _launch("split", T, recs, agents, "dgh" if agents else "mixed", True, fwd=False)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    holder = {}
    with no_gc_during_capture(), torch.cuda.graph(graph):
        holder["o"] = _launch_captured(T, recs, agents, "dgh" if agents else "mixed")
    for o in holder["o"]:
        for nm, a in o.items():
            if not nm.startswith("_"):
                a.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k, o in enumerate(eager):
        for nm, a in o.items():
            if not nm.startswith("_"):
                assert torch.equal(a, holder["o"][k][nm]), (k, nm)


def _launch_captured(T, recs, agents, form):
    """_launch's backward half without the synchronisation (illegal during capture)"""
    from distributed_multi_agent_reinforcement_learning_amd import ops
    L = ops.load_library()
    n = len(recs)
    ba = (ops.GruSeqBwdNet * n)()
    outs = []
    for k, r in enumerate(recs):
        B = r["B"]
        full, wb = _forms(form, True, k)
        o = dict(dgi=torch.empty(T * B, 3 * H, device="cuda"), dh0=torch.empty(B, H, device="cuda"))
        o["dgh" if full else "dnr"] = torch.empty(T, B, 3 * H if full else H, device="cuda")
        if wb:
            o["db_ih"], o["db_hh"] = torch.empty(3 * H, device="cuda"), torch.empty(3 * H, device="cuda")
            o["_ws"] = torch.empty(L.gru_seq_bwd_workspace(B), dtype=torch.uint8, device="cuda")
        a = ba[k]
        a.dout, a.save, a.out, a.h0, a.w_hh, a.dgi = (r["dout"].data_ptr(), r["save"].data_ptr(), r["out"].data_ptr(), r["h0"].data_ptr(),
                                                      r["w"].data_ptr(), o["dgi"].data_ptr())
        a.dgh = o["dgh"].data_ptr() if full else None
        a.dnr = None if full else o["dnr"].data_ptr()
        a.dh0 = o["dh0"].data_ptr()
        a.db_ih = o["db_ih"].data_ptr() if wb else None
        a.db_hh = o["db_hh"].data_ptr() if wb else None
        a.workspace = o["_ws"].data_ptr() if wb else None
        a.B = B
        outs.append(o)
    ops._check(L.gru_seq_split_bwd_multi(n, C.cast(ba, C.c_void_p), T, max(r["B"] for r in recs), H, agents, ops._stream()), "gru_seq_split_bwd_multi")
    return outs
