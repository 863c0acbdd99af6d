"""ops.encoder_tail (sb_encoder_tail): the rollout encoder's AGG layer and the embedding part of its semantic layer as one launch.
The contract is bit-identity with the two sb_gemm launches it replaces (split_linear(relu=True), then split_linear(addend=out,
out=out)), on every row count around the 32-row tile and with more than two tiles per persistent workgroup, with strided operands, in
a captured graph, and through DHGN.forward_pair."""
import pytest
import torch

from tests.helpers import no_gc_during_capture

pytestmark = pytest.mark.gpu

E = 128


@pytest.fixture()
def split_mode():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    old, old_sw = ops.CELL_MODE, ops.ENCODER_TAIL
    ops.set_cell_mode("split_bf16")
    ops.ENCODER_TAIL = True
    yield ops
    ops.set_cell_mode(old)
    ops.ENCODER_TAIL = old_sw


def make_operands(Rs, seed=0, neg_row=None, zero_addend=False):
    """m3 (Rs, 384), w_agg, b_agg, Ws as the column block [:, 4:] of a (128, 388) matrix, addend (Rs, 128).  The bias is shifted so
    that about a third of the AGG pre-activations are negative (pre-activation ~ N(0.55, 1.28): P(< 0) = 0.33)."""
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + Rs % 997)
    m3 = torch.randn(Rs, 3 * E, device="cuda", generator=g)
    w_agg = torch.randn(E, E, device="cuda", generator=g) * 0.1
    b_agg = torch.randn(E, device="cuda", generator=g) * 0.6 + 0.55
    Ws = (torch.randn(E, 3 * E + 4, device="cuda", generator=g) * 0.1)[:, 4:]
    add = torch.randn(Rs, E, device="cuda", generator=g)
    if neg_row is not None:      # every pre-activation of this row is negative: its embedding is exactly zero
        m3[neg_row] = 0.0
        b_agg = -b_agg.abs() - 0.01
    if zero_addend:
        add[::2] = 0.0
        add[:, ::3] = 0.0
    return m3, w_agg, b_agg, Ws, add


def pair(ops, m3, w_agg, b_agg, Ws, out):
    """today's two launches, accumulating into `out` in place -> (out, emb)"""
    emb = ops.split_linear(m3.reshape(-1, E) if m3.is_contiguous() else m3.contiguous().view(-1, E), w_agg, b_agg, relu=True)
    emb_2d = emb.view(m3.shape[0], 3 * E)
    assert ops.split_linear_ok(emb_2d, Ws, out, out)
    ops.split_linear(emb_2d, Ws, None, False, out=out, addend=out)
    return out, emb


def row_counts():
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    return [1, 15, 16, 17, 31, 32, 33, 69, 64 * cus + 7]


@pytest.mark.parametrize("case", range(9))
def test_encoder_tail_is_bit_identical_to_the_two_launches(split_mode, case):
    ops = split_mode
    Rs = row_counts()[case]
    with torch.no_grad():
        m3, w_agg, b_agg, Ws, add = make_operands(Rs, seed=case)
        ref, emb = pair(ops, m3, w_agg, b_agg, Ws, add.clone())
        frac = float((emb == 0).float().mean())
        assert Rs < 64 or 0.2 < frac < 0.45, frac          # about a third of the pre-activations are negative
        out = add.clone()
        assert ops.encoder_tail_ok(m3, w_agg, b_agg, Ws, out)
        y = ops.encoder_tail(m3, w_agg, b_agg, Ws, out)
        assert y.data_ptr() == out.data_ptr()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize("Rs", [33, 69])
def test_encoder_tail_zero_embedding_row_and_zero_addends(split_mode, Rs):
    ops = split_mode
    with torch.no_grad():
        m3, w_agg, b_agg, Ws, add = make_operands(Rs, seed=3, neg_row=Rs - 2, zero_addend=True)
        ref, emb = pair(ops, m3, w_agg, b_agg, Ws, add.clone())
        assert float(emb.view(Rs, 3 * E)[Rs - 2].abs().max()) == 0.0 and float(emb.abs().max()) > 0.0
        out = add.clone()
        ops.encoder_tail(m3, w_agg, b_agg, Ws, out)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))       # (as bits: the sign of a zero counts)
        assert torch.equal(out[Rs - 2], add[Rs - 2] + 0.0)


@pytest.mark.parametrize("Rs", [17, 69])
def test_encoder_tail_strided_in_place(split_mode, Rs):
    """Y = C = the right-hand column block of an (Rs, 256) matrix (forward_pair at depth > 0), m3 rows 392 floats apart, Ws a column
    block: the left-hand block is left untouched."""
    ops = split_mode
    with torch.no_grad():
        m3, w_agg, b_agg, Ws, add = make_operands(Rs, seed=5)
        assert Ws.stride(0) == 3 * E + 4 and Ws.data_ptr() % 16 == 0
        m3w = torch.randn(Rs, 3 * E + 8, device="cuda")
        m3w[:, 4:4 + 3 * E] = m3
        m3s = m3w[:, 4:4 + 3 * E]
        wide = torch.randn(Rs, 2 * E, device="cuda")
        wide[:, E:] = add
        left0 = wide[:, :E].clone()
        ref, _ = pair(ops, m3, w_agg, b_agg, Ws, add.clone())
        out = wide[:, E:]
        assert ops.encoder_tail_ok(m3s, w_agg, b_agg, Ws, out)
        ops.encoder_tail(m3s, w_agg, b_agg, Ws, out)
        assert torch.equal(wide[:, E:].view(torch.int32), ref.view(torch.int32))
        assert torch.equal(wide[:, :E], left0)


def test_encoder_tail_matches_f64_as_well_as_the_two_launches(split_mode):
    """against an f64 evaluation of the two layers: the bound of test_split_bf16_linear_matches_f64 (twice the error of the fp32
    library evaluation + 1e-6, and 2e-5 of the result's scale), with the two-launch path measured beside it"""
    ops = split_mode
    Rs = 1000
    with torch.no_grad():
        m3, w_agg, b_agg, Ws, add = make_operands(Rs, seed=7)
        emb64 = torch.relu(m3.double().view(-1, E) @ w_agg.double().t() + b_agg.double()).view(Rs, 3 * E)
        ref = emb64 @ Ws.double().t() + add.double()
        emb32 = torch.relu(torch.addmm(b_agg, m3.view(-1, E), w_agg.t())).view(Rs, 3 * E)
        lib = torch.addmm(add, emb32, Ws.t())
        two, _ = pair(ops, m3, w_agg, b_agg, Ws, add.clone())
        out = add.clone()
        ops.encoder_tail(m3, w_agg, b_agg, Ws, out)
        e_lib = float((lib.double() - ref).abs().max())
        e_two, e_one = float((two.double() - ref).abs().max()), float((out.double() - ref).abs().max())
        print(f"max |error| against f64: library fp32 {e_lib:.3e}, two launches {e_two:.3e}, one launch {e_one:.3e}")
        scale = max(1.0, float(ref.abs().max()))
        assert e_two <= 2.0 * e_lib + 1e-6 and e_two < 2e-5 * scale, (e_two, e_lib)
        assert e_one <= 2.0 * e_lib + 1e-6 and e_one < 2e-5 * scale, (e_one, e_lib)


def test_encoder_tail_graph_replay_equals_eager(split_mode):
    ops = split_mode
    Rs = 64 * torch.cuda.get_device_properties(0).multi_processor_count + 7
    with torch.no_grad():
        m3, w_agg, b_agg, Ws, add = make_operands(Rs, seed=9)
        eager = []
        for _ in range(3):
            out = add.clone()
            ops.encoder_tail(m3, w_agg, b_agg, Ws, out)
            eager.append(out)
        assert torch.equal(eager[0].view(torch.int32), eager[1].view(torch.int32)) and torch.equal(eager[0].view(torch.int32), eager[2].view(torch.int32))
        static = add.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.encoder_tail(m3, w_agg, b_agg, Ws, static)       # warm-up on the capture stream (the launch's one-time attribute call)
        torch.cuda.current_stream().wait_stream(s)
        static.copy_(add)
        g = torch.cuda.CUDAGraph()
        with no_gc_during_capture(), torch.cuda.graph(g):
            ops.encoder_tail(m3, w_agg, b_agg, Ws, static)
        static.copy_(add)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static.view(torch.int32), eager[0].view(torch.int32))


@pytest.mark.parametrize("depth", [0, 1])
def test_forward_pair_is_the_same_with_the_switch_on_and_off(split_mode, depth):
    """DHGN.forward_pair on a rollout's own observations and history (5 environments, 8 pursuers): identical embeddings either way"""
    ops = split_mode
    from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
    from distributed_multi_agent_reinforcement_learning_amd.pursuit_env import Pursuit_Env
    from tests.helpers import product_cfg
    cfg = product_cfg(8, 40, 40, T=6, depth=depth, **{"runtime.use_graphs": False, "runtime.seed": 7})
    torch.manual_seed(4)
    agent = MAPPO(cfg, 5, 5, "Worker")
    env = Pursuit_Env(cfg, num_envs=5)
    agent.explore_env(env, 1)                                    # leaves observations and a non-zero history ring in the rollout state
    st = agent._rollout_state(env)
    o = st._obs()
    hops_a, hops_c = st._hops(st.t)
    net = agent.actor.shared_net
    calls = []
    real = ops.encoder_tail

    def counting(*a):
        calls.append(1)
        return real(*a)
    outs = {}
    with torch.no_grad():
        for on in (True, False):
            ops.ENCODER_TAIL = on
            ops.encoder_tail = counting
            try:
                outs[on] = net.forward_pair(o["p_state"], o["e_state"], o["o_state"], o["p_adj"], o["e_adj"], o["o_adj_bits"], hops_a, hops_c,
                                            o["o_kvalid"], 1, None).clone()
            finally:
                ops.encoder_tail = real
            assert len(calls) == 1                               # the fused launch ran with the switch on, and only then
    assert outs[True].shape == (2, 5, 8, E) and float(outs[True].abs().max()) > 0.0
    assert torch.equal(outs[True].view(torch.int32), outs[False].view(torch.int32))


def test_predicate_rejects_what_the_kernel_does_not_cover(split_mode):
    ops = split_mode
    Rs = 40
    m3, w_agg, b_agg, Ws, add = make_operands(Rs, seed=11)
    with torch.no_grad():
        assert ops.encoder_tail_ok(m3, w_agg, b_agg, Ws, add)
        buf = torch.zeros(Rs * 3 * E + 8, device="cuda")
        assert not ops.encoder_tail_ok(buf[1:1 + Rs * 3 * E].view(Rs, 3 * E), w_agg, b_agg, Ws, add)          # m3 4 bytes off alignment
        assert not ops.encoder_tail_ok(torch.zeros(Rs, 3 * E + 2, device="cuda")[:, :3 * E], w_agg, b_agg, Ws, add)   # row stride not a multiple of 4
        assert not ops.encoder_tail_ok(m3, w_agg, b_agg, torch.zeros(E, 3 * E + 3, device="cuda")[:, 3:], add)   # Ws block misaligned
        assert not ops.encoder_tail_ok(m3, w_agg, b_agg, Ws, m3[:, E:2 * E])                                   # Y inside m3
        assert not ops.encoder_tail_ok(m3, w_agg.double(), b_agg, Ws, add)
        assert not ops.encoder_tail_ok(m3, w_agg, None, Ws, add)
        assert not ops.encoder_tail_ok(m3[:, :2 * E], w_agg, b_agg, Ws, add)
        ops.ENCODER_TAIL = False
        assert not ops.encoder_tail_ok(m3, w_agg, b_agg, Ws, add)
        ops.ENCODER_TAIL = True
        ops.set_cell_mode("fp32")
        assert not ops.encoder_tail_ok(m3, w_agg, b_agg, Ws, add)
        ops.set_cell_mode("split_bf16")
    assert not ops.encoder_tail_ok(m3, w_agg, b_agg, Ws, add)                                                  # autograd on
    # the C entry point refuses the same operands instead of launching
    L = ops.load_library()

    def rc(m=m3.data_ptr(), ldx=3 * E, W=Ws.data_ptr()):
        return L.sb_encoder_tail(Rs, m, ldx, w_agg.data_ptr(), b_agg.data_ptr(), W, Ws.stride(0), add.data_ptr(), E, add.data_ptr(), E, None)
    assert rc(m=m3.data_ptr() + 4) != 0 and rc(W=Ws.data_ptr() + 8) != 0 and rc(ldx=3 * E + 2) != 0
