"""Inputs shared by tests/test_first_gen_refs_cpu.py and the GPU tests of the first-generation update kernels (test_gae_gpu.py,
test_sn_power_gpu.py, test_nbr_mean_gpu.py): the shapes on the kernels' grid edges, the masks and the degenerate values."""
import numpy as np
import torch

# ---- ops.gae_advnorm: one lane per (environment, agent) sequence, 256 workgroups x 256 lanes per pass -----------------------------------
GAE_SHAPES = [(1, 2, 1),        # n - 1 = 1 in the unbiased std
              (3, 1, 5),        # T = 1
              (300, 150, 1),    # P = 1
              (64, 150, 8),
              (65_537, 2, 1),   # one lane into the second pass of the grid
              (8_193, 3, 8)]    # 65 544 sequences: P > 1 in the second pass
GAE_MASKS = ["all", "random", "sequence", "ends", "none"]
GAE_VALUES = {"plain": (0.99, 0.95, 0.0),       # (gamma, lamda, shift of the rewards)
              "shifted": (0.99, 0.95, 1000.0),  # |mean| of the advantages far above their std
              "lamda0": (0.99, 0.0, 0.0),
              "undiscounted": (1.0, 1.0, 0.0)}


def gae_inputs(shape, mask, shift=0.0, seed=0):
    """fp32 numpy (r, v, active): r ~ N(shift, 1), v ~ N(0, 4); mask: all live, 10 % dead at random, the last sequence dead from
    start to end, dead at t = 0 and t = T - 1 only, everything dead"""
    N, T, P = shape
    rng = np.random.default_rng(seed + 7 * N + 3 * T + P)
    r = (rng.standard_normal((N, T, P)) + shift).astype(np.float32)
    v = (rng.standard_normal((N, T + 1, P)) * 2).astype(np.float32)
    active = np.ones((N, T, P), np.float32)
    if mask == "random":
        active = (rng.random((N, T, P)) < 0.9).astype(np.float32)
    elif mask == "sequence":
        active[N - 1, :, P - 1] = 0.0
    elif mask == "ends":
        active[:, 0] = 0.0
        active[:, T - 1] = 0.0
    elif mask == "none":
        active[:] = 0.0
    else:
        assert mask == "all", mask
    return r, v, active


# ---- ops.spectral_norm_weight: columns in steps of 256 (64 per wave), rows in steps of 4 -----------------------------------------------------
SN_SHAPES = [(1, 1), (1, 64), (3, 255), (4, 256), (5, 257), (13, 1000), (16, 1024), (16, 1)]
SN_CALLS = 4


def sn_inputs(A, H, w_scale=1.0, seed=0):
    """fp32 numpy (W, u, v): W ~ N(0, w_scale^2), u and v unit vectors as torch.nn.utils.spectral_norm starts them"""
    rng = np.random.default_rng(seed + 1000 * A + H)
    W = (rng.standard_normal((A, H)) * w_scale).astype(np.float32)
    u, v = rng.standard_normal(A), rng.standard_normal(H)
    return W, (u / np.linalg.norm(u)).astype(np.float32), (v / np.linalg.norm(v)).astype(np.float32)


def sn_torch_hook(W, u, v, eps, n_power_iterations, dtype, calls=SN_CALLS):
    """torch.nn.utils.spectral_norm's own hook on the CPU in `dtype`, `calls` forwards in a row -> [(weight, u, v) after each], numpy.
    n_power_iterations = 0 is the hook of a module in eval mode (the constructor refuses 0)."""
    A, H = W.shape
    lin = torch.nn.utils.spectral_norm(torch.nn.Linear(H, A, bias=False), n_power_iterations=max(n_power_iterations, 1), eps=eps).to(dtype)
    out = []
    with torch.no_grad():
        lin.weight_orig.copy_(torch.from_numpy(W))
        lin.weight_u.copy_(torch.from_numpy(u))
        lin.weight_v.copy_(torch.from_numpy(v))
        if n_power_iterations == 0:
            lin.eval()
        x = torch.zeros(1, H, dtype=dtype)
        for _ in range(calls):
            lin(x)
            out.append(tuple(t.detach().clone().numpy() for t in (lin.weight, lin.weight_u, lin.weight_v)))
    return out


# ---- ops.fcra_mean: adjacency rows every kernel variant has to get right ----------------------------------------------------------------------
NBR_SPECIAL = ("zero", "single", "signed", "tiny")


def nbr_adjacency(R, P, device, seed=0):
    """(R, P, P) fp32 0/1 adjacency (half the edges), with four special rows at the front and, mirrored, at the back (the rows a second
    pass of the grid reaches): all zero (normalize(0) = 0), a single neighbour, general signed weights, and weights whose absolute
    sum is 1e-20 so that F.normalize's 1e-12 clamp binds"""
    gen = torch.Generator(device=device).manual_seed(seed + 131 * R + P)
    adj = (torch.rand(R, P, P, device=device, generator=gen) < 0.5).float()
    signed = torch.rand(P, P, device=device, generator=gen) - 0.3
    signed[0, 0] = -0.5                                             # a negative weight whatever the draw (P = 1: the only one)
    single = torch.roll(torch.eye(P, device=device), 1, dims=1)
    sign = torch.where(torch.rand(P, P, device=device, generator=gen) < 0.5, -1.0, 1.0)
    rows = {"zero": torch.zeros(P, P, device=device), "single": single, "signed": signed, "tiny": sign * (1e-20 / P)}
    for k, name in enumerate(NBR_SPECIAL):
        for r in (k, R - 1 - k):
            if 0 <= r < R:
                adj[r] = rows[name]
    return adj
