"""Inputs shared by tests/test_guidance_ref_cpu.py and tests/test_guidance_gpu.py: small random states of both environments, in the
host order ParticleEnv.reset(init=...) takes, with the cases the lane layout of the guidance kernels can get wrong forced in --
inactive pursuers, an environment whose evader(s) are inactive, two pursuers inside sep_range -- and N = 5 environments, so that the
last wave is partial (8 / 4 environments per wave at PT = 8 / 16)."""
import numpy as np

N = 5
E3D_P = (3, 8, 9)                       # PT 8, PT 8 (full group), PT 16
N2N_PE = ((3, 2), (16, 1), (16, 8))     # PT 8, PT 16, PT 16 with every evader slot in use
KILL_RADIUS = 0.5
E3D_P_VMAX, N2N_P_VMAX = 0.7, 0.3       # the environments' defaults
PARAMS = ((1.0, 2.0, 1.0), (0.0, 2.0, 1.0), (1.0, 2.0, 0.0), (2.5, 3.0, 0.5))   # (lead, sep_range, sep_gain): default, pure pursuit, no
                                                                               # separation, another of each


def _park(row, dims):
    """an inactive agent as the environments leave it: parked at 1000, everything else 0"""
    row[:] = 0.0
    row[:dims] = 1000.0


def e3d_case(P, seed=0):
    """-> (p (N, P, 7), e (N, 7), target (N, 3)) host order: x, y, z, phi, gamma, v, active"""
    rng = np.random.RandomState(100 * P + seed)
    p, e = np.zeros((N, P, 7)), np.zeros((N, 7))
    p[..., :3] = rng.uniform(5, 15, (N, P, 3))
    p[..., 3], p[..., 4], p[..., 5], p[..., 6] = rng.uniform(-np.pi, np.pi, (N, P)), rng.uniform(-1.5, 1.5, (N, P)), rng.uniform(0, 0.7, (N, P)), 1.0
    e[:, :3] = rng.uniform(0, 20, (N, 3))
    e[:, 3], e[:, 4], e[:, 5], e[:, 6] = rng.uniform(-np.pi, np.pi, N), rng.uniform(-1.5, 1.5, N), rng.uniform(0, 1.0, N), 1.0
    for n in (0, N - 1):                 # pursuers 0 and 1 inside sep_range (in the first and in the last, partial, wave)
        p[n, 1, :3] = p[n, 0, :3] + rng.uniform(-0.5, 0.5, 3)
    _park(p[1, 0], 3)                    # forced inactive pursuers: the first and the last slot of a group
    _park(p[3, P - 1], 3)
    p[4, P - 1, :3] = p[4, 0, :3] + 0.3  # ... and an inactive one inside sep_range of an active one: it must not push
    p[4, P - 1, 3:] = 0.0
    _park(e[2], 3)                       # an environment whose evader is inactive
    return p, e, rng.uniform(0, 20, (N, 3))


def n2n_case(P, E, seed=0):
    """-> (p (N, P, 5), e (N, E, 5), target (N, 2)) host order: x, y, phi, v, active"""
    rng = np.random.RandomState(1000 * P + 10 * E + seed)
    p, e = np.zeros((N, P, 5)), np.zeros((N, E, 5))
    p[..., :2] = rng.uniform(4, 16, (N, P, 2))
    p[..., 2], p[..., 3], p[..., 4] = rng.uniform(-np.pi, np.pi, (N, P)), 0.3, 1.0
    e[..., :2] = rng.uniform(0, 20, (N, E, 2))
    e[..., 2], e[..., 3], e[..., 4] = rng.uniform(-np.pi, np.pi, (N, E)), 1.0, 1.0
    for n in (0, N - 1):
        p[n, 1, :2] = p[n, 0, :2] + rng.uniform(-0.5, 0.5, 2)
    _park(p[1, 0], 2)
    _park(p[3, P - 1], 2)
    p[4, P - 1, :2] = p[4, 0, :2] + 0.3
    p[4, P - 1, 2:] = 0.0
    for k in range(E):                   # an environment with no active evader
        _park(e[2, k], 2)
    if E > 1:                            # a parked evader beside active ones: never the nearest
        _park(e[0, 0], 2)
        _park(e[3, E - 1], 2)
    return p, e, rng.uniform(0, 20, (N, 2))


def records(p, e):
    """host order (N, A, C) -> the device records (N, C, A); the env_3d evader (N, 7) stays as it is"""
    p, e = np.asarray(p), np.asarray(e)
    return np.ascontiguousarray(p.transpose(0, 2, 1)), (np.ascontiguousarray(e.transpose(0, 2, 1)) if e.ndim == 3 else e)
