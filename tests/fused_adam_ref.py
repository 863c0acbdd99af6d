"""numpy restatement of the fused clip + Adam step of algo.minibatch_steps (csrc/fused_adam.hpp, ops.fused_adam): the two launches of
one optimiser step of the env_3d / env_n2n trainers.  This file is the specification, every operation in f64.

State: np.float64 (6,) = (step, b1t, b2t, norm, coef, skipped): the steps taken, the running products beta1^step and beta2^step, the
gradient norm and the clip coefficient of the last call, and the number of calls skipped for a non-finite norm."""
import math

import numpy as np

STEP, B1T, B2T, NORM, COEF, SKIPPED = range(6)
SKIP = -1.0          # coef of a skipped step
CLIP_EPS = 1e-6      # clip_grad_norm_'s


def new_state():
    return np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0], np.float64)


def grad_sumsq(g):
    """sum g^2, the squares exact in f64 and their sum the exact one rounded once (math.fsum)"""
    g = np.asarray(g, np.float64).ravel()
    return np.float64(math.fsum((g * g).tolist()))


def grad_norm(g):
    """sqrt(grad_sumsq(g)): what launch 1 approximates within n 2^-53"""
    return np.sqrt(grad_sumsq(g))


BLOCKS, THREADS = 256, 256   # launch 1: at most BLOCKS workgroups of THREADS threads, each thread on 16-byte lanes of 4 elements


def grid(n):
    """the workgroups of either launch for n elements"""
    return int(min(max((n // 4 + THREADS - 1) // THREADS, 1), BLOCKS))


def device_sumsq(g):
    """sum g^2 in launch 1's own order, so that sqrt of it is the device's norm bit for bit: every thread adds the four squares of its
    lanes pass by pass of the grid-stride loop (the n % 4 tail elements go to the first threads of workgroup 0), a wave adds its 64
    threads by xor butterflies (32, 16, ..., 1), a workgroup its four waves as (w0 + w1) + (w2 + w3), and the last workgroup adds the
    partials in index order.  The squares are exact in f64, so a fused multiply-add gives the same bits."""
    g = np.asarray(g, np.float32).ravel()
    n, n4 = g.size, g.size // 4
    sq = g.astype(np.float64) ** 2
    blocks = grid(n)
    T = blocks * THREADS
    acc = np.zeros(T, np.float64)
    with np.errstate(all="ignore"):
        for start in range(0, n4, T):
            lanes = sq[4 * start:4 * min(start + T, n4)].reshape(-1, 4)
            for k in range(4):
                acc[:lanes.shape[0]] += lanes[:, k]
        acc[:n - 4 * n4] += sq[4 * n4:]
        w = acc.reshape(-1, 64)
        idx = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            w = w + w[:, idx ^ off]
        w = w[:, 0].reshape(blocks, 4)
        part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
        total = np.float64(0.0)
        for x in part:
            total = total + x
    return total


def advance(state, norm, max_norm, beta1, beta2):
    """the end of launch 1 from the norm, in place: coef = min(1, max_norm / (norm + 1e-6)), exactly 1 when max_norm <= 0; a finite norm
    advances step, b1t, b2t, another one only `skipped`"""
    norm, max_norm = np.float64(norm), np.float64(max_norm)
    state[NORM] = norm
    if not np.isfinite(norm):
        state[COEF] = SKIP
        state[SKIPPED] += 1.0
        return state
    coef = np.float64(1.0)
    if max_norm > 0.0:
        coef = np.minimum(max_norm / (norm + np.float64(CLIP_EPS)), np.float64(1.0))
    state[COEF] = coef
    state[STEP] += 1.0
    state[B1T] *= np.float64(beta1)
    state[B2T] *= np.float64(beta2)
    return state


def rows64(p, g, m, v, state, lr, beta1, beta2, eps):
    """the arithmetic of launch 2 -> (p64, m64, v64), the f64 values before the fp32 stores.  The device's inputs are fp32 arrays (their
    conversion to f64 is exact); f64 arrays are taken as they are, which lets a check chain several steps without the fp32 rounding
    between them.  A skipped step returns its inputs."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    if state[COEF] == SKIP:
        return p.copy(), m.copy(), v.copy()
    lr, beta1, beta2, eps = (np.float64(x) for x in (lr, beta1, beta2, eps))
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        gc = g * state[COEF]
        m64 = beta1 * m + (one - beta1) * gc
        v64 = beta2 * v + ((one - beta2) * gc) * gc
        den = np.sqrt(v64) / np.sqrt(one - state[B2T]) + eps
        p64 = p - lr * ((m64 / (one - state[B1T])) / den)
    return p64, m64, v64


def rows(p, g, m, v, state, lr, beta1, beta2, eps):
    """launch 2 on fp32 arrays -> the new (p, m, v) as fp32 (rows64, then the three stores); a skipped step returns the arrays as they are"""
    p, g, m, v = (np.asarray(x, np.float32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        return tuple(x.astype(np.float32) for x in rows64(p, g, m, v, state, lr, beta1, beta2, eps))


def step(p, g, m, v, state, lr, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, norm=None, f64=False):
    """one whole step -> (p, m, v); state advances in place.  norm: the norm to use in place of grad_norm(g) (the device's read-back,
    which may differ from the exact one in the last bits); f64: rows64's values instead of the fp32 stores"""
    advance(state, grad_norm(g) if norm is None else norm, max_norm, beta1, beta2)
    return (rows64 if f64 else rows)(p, g, m, v, state, lr, beta1, beta2, eps)
