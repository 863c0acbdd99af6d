"""Inputs shared by tests/test_central_critic_ref_cpu.py and tests/test_central_critic_gpu.py: e3d_features_cases.random_case (a quarter of
the pursuers inactive, so the last slots are empty and the order closes gaps) and an all-active case that fills every one of the P - 1
slots, at one P per unrolled instance and its edges (PT 8: 1, 2, 3, 8; PT 16: 9, 16); and the exact tie.  And the comparisons both files make
of an entry's output: with the specification, and the three identities of the law."""
import numpy as np

from tests import central_critic_ref as cref
from tests import e3d_features_cases as fc
from tests import e3d_features_ref as ref

N = fc.N
CFG = fc.CFG
P_CASES = (1, 2, 3, 8, 9, 16)
random_case = fc.random_case
MIN_GAP = 1e-9   # the smallest relative gap between two consecutive sorted squared team-mate distances the comparison tolerates


def all_active_case(P):
    """random_case's records with every pursuer active and positions uniform in the 20-cube from RandomState(7000 + P)"""
    rng = np.random.RandomState(7000 + P)
    c = fc.random_case(P)
    p = np.zeros((N, 7, P))
    p[:, :3] = rng.uniform(0, 20, (N, 3, P))
    p[:, 3], p[:, 4], p[:, 5] = rng.uniform(-np.pi, np.pi, (N, P)), rng.uniform(-1.5, 1.5, (N, P)), rng.uniform(0, 0.7, (N, P))
    p[:, 6] = 1.0
    return dict(c, p=p)


def case(rows, e_row=(1, 1, 1, 0, 0, 0, 1)):
    """one environment from rows (x, y, z, phi, gamma, v, active), adjacencies all ones"""
    p = np.array(rows, np.float64).T[None]
    P = p.shape[2]
    return dict(p=p, e=np.array(e_row, np.float64)[None], target=np.full((1, 3), 10.0), time_step=np.array([3], np.int32),
                pp_adj=np.ones((1, P, P), np.float32), pe_adj=np.ones((1, P), np.float32))


def tie_case(swap=False):
    """pursuer 0 at (8, 8, 8) and two team-mates at (+-3, 0, 0) from it, told apart by their speeds; swap exchanges their indices;
    a third, farther team-mate follows"""
    plus, minus = [11, 8, 8, 0.5, 0.25, 0.7, 1], [5, 8, 8, -0.5, 0.125, 0.35, 1]
    rows = [[8, 8, 8, 0, 0, 0.1, 1], minus if swap else plus, plus if swap else minus, [8, 12, 8, 1.0, 0, 0.2, 1]]
    return case(rows)


def gap_of(c):
    """the smallest relative gap between two consecutive sorted squared team-mate distances of any row of the case (ref.nearest_gap)"""
    gap, rows = ref.nearest_gap(c["p"])
    assert rows == int((c["p"][:, 6] != 0).sum())      # no row is left out
    return gap


def check_against_ref(got, want, c):
    """rtol = atol = 1e-6 (test_e3d_features_gpu's figures for the pursuit kernel); rows of inactive pursuers and every column the law
    leaves at zero (empty slots, an unknown evader) exact"""
    dead = c["p"][:, 6] == 0
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_allclose(g, w, rtol=1e-6, atol=1e-6)
        assert np.all(g[dead] == 0) and np.all(g[w == 0] == 0)


def identities(actor, critic, pursuit_actor, pursuit_critic, p):
    """the three bit-level identities of the law and the actor rows, on any pair of outputs"""
    N, _, P = p.shape
    assert np.array_equal(actor, pursuit_actor)
    assert np.array_equal(critic[..., :32], pursuit_critic)                            # 1
    for s, col in ((0, 20), (1, 25)):
        if P - 1 > s:
            assert np.array_equal(critic[..., 32 + 8 * s:36 + 8 * s], critic[..., col:col + 4])   # 2
    who = cref.order(p)
    filled = 0
    for n in range(N):
        for i in range(P):
            for s in range(P - 1):
                j = who[n, i, s]
                blk = critic[n, i, 32 + 8 * s:40 + 8 * s]
                if j < 0:
                    assert np.all(blk == 0)
                else:
                    assert np.array_equal(blk[4:8], critic[n, j, 3:7])                  # 3
                    filled += 1
    return filled
