"""Inputs shared by tests/test_e3d_features_ref_cpu.py and tests/test_e3d_features_gpu.py: random states of env_3d as device records,
set the way test_gauss_gpu.test_policy_features_match_numpy sets them (random adjacencies, a quarter of the pursuers inactive) with
positions uniform in the cube and one environment whose evader is inactive; the adjacencies are sparse enough (about one link per
pursuer, three sensors in ten) that the communication graph falls into several components, some without a sensor, so the three evader
models give three different k columns; N = 5 environments, so that the last wave is partial; one
P per lane layout and more (PT 8: 1, 3, 8; PT 16: 9; PT 32: 17; PT 64: 33).  And the chains of the relay test."""
import numpy as np

N = 5
P_CASES = (1, 3, 8, 9, 17, 33)
CFG = dict(p_vmax=0.7, e_vmax=1.0, kill_radius=0.5, max_step=200, p_comm_range=6.0, p_sen_range=3.0)   # ParticleEnv's defaults
MIN_GAP = 1e-9   # the smallest relative gap between two squared team-mate distances the comparison tolerates (see nearest_gap)


def random_case(P, seed=0):
    """-> dict p (N, 7, P), e (N, 7), target (N, 3) f64, time_step (N,) int32, pp_adj (N, P, P), pe_adj (N, P) fp32"""
    rng = np.random.RandomState(1000 * P + seed)
    p, e = np.zeros((N, 7, P)), np.zeros((N, 7))
    p[:, :3] = rng.uniform(0, 20, (N, 3, P))
    p[:, 3], p[:, 4], p[:, 5] = rng.uniform(-np.pi, np.pi, (N, P)), rng.uniform(-1.5, 1.5, (N, P)), rng.uniform(0, 0.7, (N, P))
    p[:, 6] = 1.0
    dead = rng.permutation(N * P)[:(N * P) // 4]                  # a quarter of the pursuers forced inactive, parked as the tick parks them
    for k in dead:
        p[k // P, :, k % P] = (1000.0, 1000.0, 1000.0, 0, 0, 0, 0)
    e[:, :3] = rng.uniform(0, 20, (N, 3))
    e[:, 3], e[:, 4], e[:, 5], e[:, 6] = rng.uniform(-np.pi, np.pi, N), rng.uniform(-1.5, 1.5, N), rng.uniform(0, 1.0, N), 1.0
    e[2] = (1000.0, 1000.0, 1000.0, 0, 0, 0, 0)                   # one environment with the evader inactive
    return dict(p=p, e=e, target=rng.uniform(0, 20, (N, 3)), time_step=rng.randint(0, 200, N).astype(np.int32),
                pp_adj=(rng.uniform(size=(N, P, P)) < min(0.5, 1.2 / P)).astype(np.float32), pe_adj=(rng.uniform(size=(N, P)) < 0.3).astype(np.float32))


def chain_case(P, dead=None, spacing=5.0, comm=6.0, sen=3.0):
    """one environment: P pursuers in a line along x, `spacing` apart, adjacencies as the environment computes them (comm range 6:
    every pursuer hears its two neighbours only; sensing range 3: the evader sits 1 beyond the last pursuer, which alone senses it).
    dead: the index of an inactive pursuer (parked, its adjacency row zero and no column pointing at it)"""
    p, e = np.zeros((1, 7, P)), np.zeros((1, 7))
    p[0, 0] = spacing * np.arange(P)
    p[0, 6] = 1.0
    e[0] = (spacing * (P - 1) + 1.0, 0, 0, 0, 0, 0.5, 1)
    if dead is not None:
        p[0, :, dead] = (1000.0, 1000.0, 1000.0, 0, 0, 0, 0)
    on = p[0, 6] != 0
    d = np.sqrt(((p[0, :3, :, None] - p[0, :3, None, :]) ** 2).sum(0))
    pp = ((d <= comm) & on[:, None] & on[None, :]).astype(np.float32)[None]       # (get_adj_mat: the diagonal is 1 for active pursuers)
    de = np.sqrt(((p[0, :3] - e[0, :3, None]) ** 2).sum(0))
    pe = ((de <= sen) & on).astype(np.float32)[None]
    return dict(p=p, e=e, target=np.full((1, 3), 10.0), time_step=np.array([7], np.int32), pp_adj=pp, pe_adj=pe)
