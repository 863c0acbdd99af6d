"""CPU checks of the f64 restatements the first-generation update kernels are held to (tests/gae_ref.py, sn_power_ref.py,
nbr_mean_ref.py): each against the code it restates, run in f64 -- oracle/model_oracle.py `gae`, torch.nn.utils.spectral_norm's own
hook, and torch.matmul(F.normalize(adj, p=1, dim=-1), z).  Two f64 evaluations of one formula differ by summation order only, so
the tolerance is 1e-12 of each tensor's largest magnitude: seven orders below one fp32 ulp, a wrong formula cannot hide."""
import numpy as np
import pytest
import torch

from oracle import model_oracle as mo
from tests import first_gen_cases as cases
from tests import gae_ref, nbr_mean_ref, sn_power_ref

RTOL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= RTOL * scale, (what, err, scale)


# ---- GAE ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", cases.GAE_MASKS)
@pytest.mark.parametrize("shape", [(7, 13, 4)] + cases.GAE_SHAPES)
def test_gae_restatement_is_the_oracle_in_f64(shape, mask):
    r, v, active = cases.gae_inputs(shape, mask)
    for norm in (True, False):
        adv, vt = gae_ref.gae(r, v, active, 0.99, 0.95, norm)
        adv_o, vt_o = mo.gae(*(torch.from_numpy(x).double() for x in (r, v, active)), 0.99, 0.95, norm)
        _close(adv, adv_o.numpy(), ("adv", norm))
        _close(vt, vt_o.numpy(), ("v_target", norm))
        if norm:
            assert np.all(adv[active == 0] == 0)
    if mask == "none":
        assert not adv.any() and np.array_equal(vt, v[:, :-1].astype(np.float64))


@pytest.mark.parametrize("values", ["shifted", "lamda0", "undiscounted"])
@pytest.mark.parametrize("shape", cases.GAE_SHAPES)
def test_gae_restatement_at_degenerate_values(shape, values):
    gamma, lamda, shift = cases.GAE_VALUES[values]
    r, v, active = cases.gae_inputs(shape, "random", shift)
    for norm in (True, False):
        adv, vt = gae_ref.gae(r, v, active, gamma, lamda, norm)
        adv_o, vt_o = mo.gae(*(torch.from_numpy(x).double() for x in (r, v, active)), gamma, lamda, norm)
        _close(adv, adv_o.numpy(), ("adv", norm))
        _close(vt, vt_o.numpy(), ("v_target", norm))
    if values == "lamda0":     # the one-step advantage
        d = (r.astype(np.float64) + gamma * v[:, 1:].astype(np.float64) - v[:, :-1]) * active
        assert np.array_equal(adv, d)


# ---- spectral normalisation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iter", [0, 1, 3])
@pytest.mark.parametrize("A,H", [(1, 128), (9, 128), (16, 1000)] + cases.SN_SHAPES)
def test_sn_restatement_is_torchs_hook_in_f64(A, H, n_iter):
    W, u, v = cases.sn_inputs(A, H)
    want = cases.sn_torch_hook(W.astype(np.float64), u.astype(np.float64), v.astype(np.float64), 1e-12, n_iter, torch.float64)
    u, v = u.astype(np.float64), v.astype(np.float64)
    for k, (w_t, u_t, v_t) in enumerate(want):
        w, u1, v1 = sn_power_ref.power_iteration(W, u, v, 1e-12, n_iter)
        if n_iter == 0:
            assert np.array_equal(u1, u) and np.array_equal(v1, v)
        u, v = u1, v1
        _close(w, w_t, ("w", k))
        _close(u, u_t, ("u", k))
        _close(v, v_t, ("v", k))


@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("A,H", cases.SN_SHAPES)
def test_sn_restatement_with_both_clamps_binding(A, H, n_iter):
    """W of scale 1e-5 against eps = 1e-3: ||W^T u|| and ||W v|| stay below eps, so both normalisations divide by eps"""
    W, u, v = cases.sn_inputs(A, H, w_scale=1e-5)
    W64, u, v = W.astype(np.float64), u.astype(np.float64), v.astype(np.float64)
    want = cases.sn_torch_hook(W64, u, v, 1e-3, n_iter, torch.float64)
    for k, (w_t, u_t, v_t) in enumerate(want):
        assert np.linalg.norm(W64.T @ u) < 1e-3 and np.linalg.norm(W64 @ (W64.T @ u / 1e-3)) < 1e-3
        w, u, v = sn_power_ref.power_iteration(W, u, v, 1e-3, n_iter)
        assert np.linalg.norm(u) < 1 and np.linalg.norm(v) < 1          # not unit vectors: the clamps bound
        _close(w, w_t, ("w", k))
        _close(u, u_t, ("u", k))
        _close(v, v_t, ("v", k))


# ---- neighbour mean -----------------------------------------------------------------------------------------------------------------------------
NBR_SHAPES = [(8, 128, 6), (15, 128, 18), (4, 128, 30),                                      # tests/test_ops_gpu.py
              (1, 128, 7), (3, 1024, 40), (8, 128, 50), (16, 128, 300), (9, 64, 2_051), (16, 64, 1_027), (8, 128, 4_096 + 3)]
# (the GPU tests' 16 384 + 3 rows differ from these in the row count alone, which the restatement has no branch on, and take over a second here)


@pytest.mark.parametrize("relu,with_bias", [(False, False), (True, True), (False, True)])
@pytest.mark.parametrize("P,E,R", NBR_SHAPES)
def test_nbr_mean_restatement_is_torchs_normalised_matmul_in_f64(P, E, R, relu, with_bias):
    gen = torch.Generator().manual_seed(P + E + R)
    z = torch.randn(R, P, E, generator=gen)
    bias = torch.randn(E, generator=gen) if with_bias else None
    adj = cases.nbr_adjacency(R, P, "cpu")
    assert not adj[0].any() and float(adj[3].abs().sum(-1).max()) < 1e-12 and float(adj[2].min()) < 0 and int((adj[1] != 0).sum()) == P
    for a in (adj, torch.ones_like(adj)):
        want = torch.matmul(torch.nn.functional.normalize(a.double(), p=1, dim=-1), z.double())
        if bias is not None:
            want = want + bias.double()
        want = torch.relu(want) if relu else want
        got = nbr_mean_ref.nbr_mean(z.numpy(), a.numpy(), None if bias is None else bias.numpy(), relu)
        _close(got, want.numpy(), (P, E, R))
        assert np.all(nbr_mean_ref.scale(z.numpy(), a.numpy(), None if bias is None else bias.numpy()) >= np.abs(got) * (1 - 1e-12))
    if bias is None:
        assert not nbr_mean_ref.nbr_mean(z.numpy(), adj.numpy())[0].any()       # an isolated row aggregates to exactly 0
