"""ops.fcra_mean / ops.fcra_mean_pair_multi (csrc/mappo_ops.hip k_nbr_mean4, k_nbr_mean<8>, k_nbr_mean<16>) against
tests/nbr_mean_ref.py in f64.

k_nbr_mean4 (E = 128, P <= 8, 16-byte aligned operands) gives a wave per row and launches min(ceil(R / 4), 4096 / jobs) workgroups;
k_nbr_mean<8> / <16> give a workgroup per row and launch min(R, 16384 / jobs).  The row counts here put a few rows -- one partial
workgroup of k_nbr_mean4 -- into the second trip of each grid-stride loop: 16 384 + 5 and 16 384 + 3 rows for one job, 4 096 + 3 for
the four hops of a rollout tick.  P = 9 is the first size past the `P * P <= 64` switch, P = 16 fills the register array.  An operand
4 bytes off the 16-byte boundary must fall back from the wave-per-row kernel and give the same numbers.

Bound, per output element (tests/test_sb_wgrad_pc_gpu.py `_check`): the kernel's error against f64 is at most twice that of
torch.matmul(F.normalize(adj, p=1, dim=-1), z) (+ bias, ReLU) in fp32, plus one fp32 ulp, in units of sum_j |abar_ij| |z_j| + |bias|.
Results go into the left half of a 2E-wide operand whose right half must stay untouched; a joint actor + critic launch equals the
two single launches bit for bit; every launch runs twice for identical bits."""
import numpy as np
import pytest
import torch

from tests import first_gen_cases as cases
from tests import nbr_mean_ref

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
FILL = 7.0


def _ops():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops


def _torch_fp32(z, adj, bias, relu):
    y = torch.matmul(torch.nn.functional.normalize(adj, p=1, dim=-1), z)
    if bias is not None:
        y = y + bias
    return torch.relu(y) if relu else y


def _check(what, got, lib, ref, scale):
    """got, lib: fp32 device tensors; ref, scale: f64 numpy"""
    got, lib = got.cpu().numpy().astype(np.float64), lib.cpu().numpy().astype(np.float64)
    den = np.maximum(scale, 1e-300)
    e, e_lib = float((np.abs(got - ref) / den).max()), float((np.abs(lib - ref) / den).max())
    bound = 2.0 * e_lib + ULP
    print(f"{what}: e_kernel {e:.3e} e_lib {e_lib:.3e} ratio {e / bound:.3f}")
    assert np.isfinite(got).all()
    assert e <= bound, (what, e, e_lib)


def _halves(shape, E):
    """an [agg | h] operand: (..., 2E) filled with FILL, and its left half"""
    cat = torch.full(shape + (2 * E,), FILL, device="cuda")
    return cat, cat[..., :E]


def _history(n, T, P, E, gen, misalign=False):
    """z (n T, P, E) as the kernels may see it: a strided (n, T, P, E) slice of a history buffer (T > 1) or dense (T = 1), optionally
    starting 4 bytes past a 16-byte boundary -> (the tensor to pass, the same values as dense (R, P, E))"""
    if T > 1:
        buf = torch.randn(n, T + 3, P, E, device="cuda", generator=gen)
        z = buf[:, 2:2 + T]
        return z, z.reshape(n * T, P, E)
    flat = torch.randn(n * P * E + 4, device="cuda", generator=gen)
    off = 1 if misalign else 0
    z = flat[off:off + n * P * E].view(n, P, E)
    assert z.data_ptr() % 16 == 4 * off
    return z, z


CASES = [  # P, E, n, T, relu, bias, misaligned
    (8, 128, 5_463, 3, True, True, False),       # k_nbr_mean4, 16 384 + 5 rows
    (5, 128, 16_389, 1, False, False, False),
    (1, 128, 7, 1, False, True, False),
    (8, 64, 2_341, 7, True, True, False),        # k_nbr_mean<8>, 16 384 + 3 rows
    (3, 1024, 8, 5, False, False, False),
    (8, 128, 50, 1, True, True, True),           # misaligned: k_nbr_mean<8> although E = 128, P <= 8
    (9, 64, 2_341, 7, True, False, False),       # k_nbr_mean<16>
    (16, 128, 75, 4, False, True, False),
    (16, 64, 16_387, 1, True, True, False),
]


@pytest.mark.parametrize("P,E,n,T,relu,with_bias,misaligned", CASES)
def test_neighbour_mean_matches_f64(P, E, n, T, relu, with_bias, misaligned):
    ops = _ops()
    R = n * T
    gen = torch.Generator(device="cuda").manual_seed(P * 1000 + E + R)
    z, z_dense = _history(n, T, P, E, gen, misaligned)
    bias = torch.randn(E, device="cuda", generator=gen) if with_bias else None
    adj = cases.nbr_adjacency(R, P, "cuda")
    ones = torch.ones_like(adj)

    def launch():
        cat_b, out_b = _halves((2, R, P), E)
        cat_a, out_a = _halves((R, P), E)
        cat_c, out_c = _halves((R, P), E)
        ops.fcra_mean(z_actor=z, z_critic=z, adj=adj, bias=bias, relu=relu, out=out_b)
        ops.fcra_mean(z_actor=z, adj=adj, bias=bias, relu=relu, out=out_a)
        ops.fcra_mean(z_critic=z, bias=bias, relu=relu, out=out_c)
        torch.cuda.synchronize()
        return cat_b, cat_a, cat_c

    cat_b, cat_a, cat_c = launch()
    for first, second in zip((cat_b, cat_a, cat_c), launch()):
        assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    for cat in (cat_b, cat_a, cat_c):
        assert bool((cat[..., E:] == FILL).all())                                   # the right half of the operand is not touched
    assert torch.equal(cat_b[0, ..., :E].view(torch.int32), cat_a[..., :E].view(torch.int32))     # joint launch = the two single launches
    assert torch.equal(cat_b[1, ..., :E].view(torch.int32), cat_c[..., :E].view(torch.int32))
    zn, bn = z_dense.cpu().numpy(), None if bias is None else bias.cpu().numpy()
    for name, got, a in (("actor", cat_a[..., :E], adj), ("critic", cat_c[..., :E], ones)):
        an = a.cpu().numpy()
        ref, scale = nbr_mean_ref.nbr_mean(zn, an, bn, relu), nbr_mean_ref.scale(zn, an, bn)
        _check(f"P {P} E {E} R {R} T {T} relu {int(relu)} bias {int(with_bias)} {name}", got, _torch_fp32(z_dense, a, bias, relu), ref, scale)
    if bias is None:
        assert not cat_a[0, :, :E].any()                                            # an all-zero adjacency row: exactly 0
    if misaligned:                                                                  # the same numbers as the wave-per-row kernel on an aligned copy
        za = z.clone()
        assert za.data_ptr() % 16 == 0
        al = ops.fcra_mean(z_actor=za, z_critic=za, adj=adj, bias=bias, relu=relu)
        assert torch.equal(al.view(torch.int32), cat_b[..., :E].contiguous().view(torch.int32))


def test_four_hops_in_one_launch():
    """fcra_mean_pair_multi with four jobs: 4096 / 4 workgroups per hop, so at 4 096 + 3 rows every hop's second pass is one partial
    workgroup (three of its four waves have a row).  Each hop against f64, and against the single launch of that hop bit for bit."""
    ops = _ops()
    P, E, R, hops = 8, 128, 4_096 + 3, 4
    gen = torch.Generator(device="cuda").manual_seed(R)
    zas = [torch.randn(R, P, E, device="cuda", generator=gen) for _ in range(hops)]
    zcs = [torch.randn(R, P, E, device="cuda", generator=gen) for _ in range(hops)]
    biases = [torch.randn(E, device="cuda", generator=gen) for _ in range(hops)]
    adj = cases.nbr_adjacency(R, P, "cuda")
    ones = torch.ones_like(adj)

    def launch():
        cats = [_halves((2, R, P), E) for _ in range(hops)]
        ops.fcra_mean_pair_multi(zas, zcs, adj, biases, [o for _, o in cats])
        torch.cuda.synchronize()
        return [c for c, _ in cats]

    cats = launch()
    for first, second in zip(cats, launch()):
        assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    an, on = adj.cpu().numpy(), ones.cpu().numpy()
    for k in range(hops):
        assert bool((cats[k][..., E:] == FILL).all())
        single = ops.fcra_mean(z_actor=zas[k], z_critic=zcs[k], adj=adj, bias=biases[k], relu=True)
        assert torch.equal(single.view(torch.int32), cats[k][..., :E].contiguous().view(torch.int32))
        bn = biases[k].cpu().numpy()
        for name, idx, zt, a_t, a_n in (("actor", 0, zas[k], adj, an), ("critic", 1, zcs[k], ones, on)):
            zn = zt.cpu().numpy()
            _check(f"hop {k} {name}", cats[k][idx, ..., :E], _torch_fp32(zt, a_t, biases[k], True), nbr_mean_ref.nbr_mean(zn, a_n, bn, True),
                   nbr_mean_ref.scale(zn, a_n, bn))
