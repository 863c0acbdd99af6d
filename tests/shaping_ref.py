"""numpy restatement of algo.reward_shaping: distance -- potential-based shaping (Ng, Harada and Russell 1999) under the lockstep masks
of the env_3d / env_n2n rollouts (csrc/reward_shaping.hpp, the shaping option of e3d_policy_record / n2n_policy_record, *_shaping_begin).

Records are the device's: p (N, C, P) and e (N, C, E) f64 with the coordinates in the first D rows (D = 2: env_n2n, C = 5; D = 3:
env_3d, C = 7, e given as (N, 7) or (N, 7, 1)) and the active flag in the last row.  Every operation is elementwise f64 in the order
of the header (plain *, +, -, sqrt; squares summed left to right), so the kernels reproduce it bit for bit."""
import math
from fractions import Fraction

import numpy as np


def _e3(e):
    e = np.asarray(e, np.float64)
    return e[:, :, None] if e.ndim == 2 else e


def dims(p):
    """coordinates per position from the record width: 5 rows -> 2 (env_n2n), 7 rows -> 3 (env_3d)"""
    return {5: 2, 7: 3}[p.shape[1]]


def potential(p, e, coef):
    """Phi (N, P) of the state in the records: -coef * min_k |pos_p - pos_k| over the active evaders k; 0 for an inactive pursuer
    and when no evader is active"""
    p, e = np.asarray(p, np.float64), _e3(e)
    D = dims(p)
    p_on, e_on = p[:, -1, :] != 0.0, e[:, -1, :] != 0.0                  # (N, P), (N, E)
    d = p[:, :D, :, None] - e[:, :D, None, :]                            # (N, D, P, E): pos_p - pos_k
    sq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if D == 3:
        sq = sq + d[:, 2] * d[:, 2]
    dist = np.where(e_on[:, None, :], np.sqrt(sq), np.inf)
    any_e = e_on.any(-1)[:, None]
    dmin = np.where(any_e, dist.min(-1), 0.0)
    return np.where(p_on & any_e, -coef * dmin, 0.0)


def within(d, r):
    """d (D, ...), D = 2 or 3 -> `norm(d) <= r` as the environments' range tests evaluate it (numpy's norm of a 2- or 3-vector):
    sqrt(fma(c, c, fma(b, b, a a))) <= r.  numpy has no fma: where the plain sum of squares is within 1e-12 r r of r r -- it differs
    from the chain by a few ulp at most -- the chain is evaluated in rationals, rounded once per fma; elsewhere the plain sum decides."""
    d = np.asarray(d, np.float64)
    sq = (d * d).sum(0)
    out = np.asarray(np.sqrt(sq) <= r)
    for k in zip(*np.nonzero(np.abs(sq - r * r) <= 1e-12 * r * r)):
        s = float(d[0][k]) * float(d[0][k])
        for x in d[1:]:
            s = float(Fraction(float(x[k])) ** 2 + Fraction(s))
        out[k] = math.sqrt(s) <= r
    return out


def ended_after(p, e, target, kill_radius):
    """(N,) the state in the records ends the episode for a reason other than the time limit: no pursuer active, no evader active
    (env_3d: the evader dead), or an evader within the kill radius of the target (get_done of either environment)"""
    p, e, target = np.asarray(p, np.float64), _e3(e), np.asarray(target, np.float64)
    D = dims(p)
    p_on, e_on = p[:, -1, :] != 0.0, e[:, -1, :] != 0.0
    reach = within((e[:, :D, :] - target[:, :, None]).transpose(1, 0, 2), kill_radius)
    return ~p_on.any(-1) | ~e_on.any(-1) | reach.any(-1)


def step(phi, raw, live, done_before, p_after, e_after, ended, coef, gamma):
    """one lockstep tick.  phi (N, P) f64: the carried potential, advanced in place for the environments not done before the step;
    raw (N, P) the tick's reward, live (N, P) 0 / 1, done_before (N,) bool; p_after, e_after: the records after the tick; ended (N,)
    bool: the episode has ended for a reason other than the time limit.
    -> (x, F, phi_next), each (N, P) f64: x = raw + F live is the shaped reward (what RewardScaling receives in place of the raw
    reward), raw itself for environments done before the step; F = gamma phi_next - phi."""
    raw, live = np.asarray(raw, np.float32).astype(np.float64), np.asarray(live, np.float32).astype(np.float64)
    db = np.asarray(done_before, bool)
    phi_state = potential(p_after, e_after, coef)
    p_on = np.asarray(p_after)[:, -1, :] != 0.0
    terminal = ~p_on | np.asarray(ended, bool)[:, None]
    phi_next = np.where(terminal, 0.0, phi_state)
    F = gamma * phi_next - phi
    x = np.where(db[:, None], raw, raw + F * live)
    phi[~db] = phi_state[~db]
    return x, F, phi_next


def buffer_reward(x, live):
    """the buffer's reward row without reward scaling: (float)x * live"""
    return np.asarray(x, np.float64).astype(np.float32) * np.asarray(live, np.float32)


def episode(p, e, raw, done, ended, coef, gamma):
    """whole episodes from recorded states: p (N, T + 1, C, P), e (N, T + 1, C, E) -- index t is the state step t starts from --,
    raw (N, T, P), done and ended (N, T) bool after each step (ended cumulative).  -> dict of phi0 (N, P), and per tick (N, T, P):
    live, x, F, phi_next; (N, T): done_before"""
    N, T, P = raw.shape
    phi = potential(p[:, 0], e[:, 0], coef)                              # shaping_begin
    out = dict(phi0=phi.copy(), live=np.zeros((N, T, P), np.float32), x=np.zeros((N, T, P)), F=np.zeros((N, T, P)),
               phi_next=np.zeros((N, T, P)), done_before=np.zeros((N, T), bool))
    db = np.zeros(N, bool)
    for t in range(T):
        live = ((p[:, t, -1, :] != 0.0) & ~db[:, None]).astype(np.float32)
        x, F, nxt = step(phi, raw[:, t], live, db, p[:, t + 1], e[:, t + 1], ended[:, t], coef, gamma)
        out["live"][:, t], out["x"][:, t], out["F"][:, t], out["phi_next"][:, t], out["done_before"][:, t] = live, x, F, nxt, db
        db = db | np.asarray(done[:, t], bool)
    return out


def telescoped(ep, gamma):
    """per (environment, pursuer): (sum over its live span of gamma^t F_t, gamma^L phi_next(last) - phi0, L); a pursuer's live steps
    are its first L"""
    live = ep["live"] != 0
    L = live.sum(1)                                                      # (N, P)
    N, T, P = live.shape
    assert np.array_equal(live, np.arange(T)[None, :, None] < L[:, None, :])
    g = gamma ** np.arange(T)
    lhs = (g[None, :, None] * ep["F"] * live).sum(1)
    last = np.take_along_axis(ep["phi_next"], np.maximum(L - 1, 0)[:, None, :], 1)[:, 0]
    rhs = np.where(L > 0, gamma ** L * last - ep["phi0"], 0.0)
    return lhs, rhs, L
