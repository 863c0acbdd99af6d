"""numpy restatement of algo.use_obs_norm (csrc/obs_norm.hpp, e3d_policy_features_norm / e3d_obs_norm_reduce / e3d_obs_norm_update):
the running mean / std normaliser of the env_3d policy features.  The reference ships the class (DHGN/normalization.py
`Normalization` / `RunningMeanStd`) and never applies it to env_3d; this file is the specification, every operation in f64.

State: np.float64 (2, 33): row 0 the actor's features, row 1 the critic's, each n, mean[16], M2[16], all 0 at the start.  It is
frozen during a rollout; the rollout's live rows give, per network and column, c = count, S1 = sum d, S2 = sum d d with
d = (double)x - mean_frozen, and one merge per rollout folds them into the state."""
import numpy as np

COLS = 16
ROW = 1 + 2 * COLS
EPS = 1e-8      # the reference's (normalization.py:33)


def new_state():
    return np.zeros((2, ROW), np.float64)


def split(row):
    """one network's row -> (n, mean[16], M2[16])"""
    return np.float64(row[0]), row[1:1 + COLS], row[1 + COLS:]


def normalise_net(row, x, on, clip):
    """x (..., 16) fp32 raw features of one network -> fp32: n == 0 the identity, else (x - mean) / (sqrt(M2 / n) + 1e-8) clipped to
    +-clip and rounded to fp32; rows with on == 0 (inactive pursuers) stay exactly 0"""
    x = np.asarray(x, np.float32)
    n, mean, M2 = split(row)
    if n == 0.0:
        y = x.copy()
    else:
        den = np.sqrt(M2 / n) + np.float64(EPS)
        v = (x.astype(np.float64) - mean) / den
        y = np.minimum(np.maximum(v, -np.float64(clip)), np.float64(clip)).astype(np.float32)
    return np.where(np.asarray(on)[..., None] != 0, y, np.float32(0.0))


def normalise(state, xa, xc, on, clip):
    """both networks: raw actor / critic features (..., 16) and the pursuers' active flags (...) -> (ya, yc) fp32"""
    return normalise_net(state[0], xa, on, clip), normalise_net(state[1], xc, on, clip)


def terms(row, x, counted):
    """the per-row terms of one network's sums: d (R, 16) f64 over the counted rows (counted != 0), about the row's frozen mean"""
    x = np.asarray(x, np.float32).reshape(-1, COLS)
    keep = np.asarray(counted).reshape(-1) != 0
    return x[keep].astype(np.float64) - split(row)[1]


def sums_net(row, x, counted):
    """-> (33,) f64: c, S1[16], S2[16] of one network over the counted rows"""
    d = terms(row, x, counted)
    return np.concatenate([[np.float64(d.shape[0])], d.sum(0), (d * d).sum(0)])


def sums(state, xa, xc, counted):
    """-> (2, 33) f64 of one batch of raw features; batches (ticks, ranks) add"""
    return np.stack([sums_net(state[0], xa, counted), sums_net(state[1], xc, counted)])


def merge(state, s):
    """folds the totals s (2, 33) of a rollout into the state, in place: per network, C == 0 changes nothing; otherwise
    n' = n + C, delta = A / C, mean' = mean + A / n', M2' = M2 + (Q - A delta) + delta delta (n C / n')"""
    for k in range(2):
        n, mean, M2 = split(state[k])
        C, A, Q = split(np.asarray(s, np.float64)[k])
        if C == 0.0:
            continue
        n1 = n + C
        delta = A / C
        state[k, 1:1 + COLS] = mean + A / n1
        state[k, 1 + COLS:] = M2 + (Q - A * delta) + delta * delta * (n * C / n1)
        state[k, 0] = n1
    return state


def stats(row):
    """-> (mean[16], population std[16]) of one network's row (n > 0)"""
    n, mean, M2 = split(row)
    return mean.copy(), np.sqrt(M2 / n)
