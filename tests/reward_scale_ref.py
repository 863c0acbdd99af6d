"""numpy restatement of algo.use_reward_scaling: the reference's RewardScaling (DHGN/normalization.py:38-52) per environment slot,
under the lockstep masks of the env_n2n / env_3d rollouts (csrc/reward_scale.hpp, the scaling option of n2n_policy_record / e3d_policy_record).

State (N, 1 + 3P) f64: n, mean[P], S[P], R[P] per environment.  Every operation is the reference's, elementwise in f64, so the
results are the reference's bit for bit (tests/golden/reward_scaling.npz)."""
import numpy as np


def new_state(N, P):
    return np.zeros((N, 1 + 3 * P), np.float64)


def reset(state, P):
    """RewardScaling.reset at an episode start: R = 0; n, mean, S persist"""
    state[:, 1 + 2 * P:] = 0.0


def step(state, x, live, done_before, gamma):
    """one lockstep tick: x (N, P) the raw reward, live (N, P) 0 / 1, done_before (N,) bool -> r (N, P) float32 for the buffer.
    Environments done before the step keep their state (the reference's loop has left the episode) and get r = x * live."""
    N, P = x.shape
    x = np.asarray(x, np.float64)
    live = np.asarray(live, np.float32)
    r = x.astype(np.float32) * live
    for e in np.flatnonzero(~np.asarray(done_before, bool)):
        n = state[e, 0] + 1.0
        mean, S, R = state[e, 1:1 + P].copy(), state[e, 1 + P:1 + 2 * P].copy(), state[e, 1 + 2 * P:].copy()
        R = gamma * R + x[e]
        if n == 1.0:           # the reference's first sample: the std is R itself
            mean, std = R, R
        else:
            old = mean
            mean = old + (R - old) / n
            S = S + (R - old) * (R - mean)
            std = np.sqrt(S / n)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = x[e] / (std + 1e-8)
        state[e, 0], state[e, 1:1 + P], state[e, 1 + P:1 + 2 * P], state[e, 1 + 2 * P:] = n, mean, S, R
        r[e] = y.astype(np.float32) * live[e]
    return r


def rollout(state, raw, live, length, gamma):
    """one episode per environment: raw, live (N, T, P), length (N,) = steps before done -> the buffer's r (N, T, P) float32;
    R is reset first, the state advances in place"""
    N, T, P = raw.shape
    reset(state, P)
    out = np.zeros((N, T, P), np.float32)
    for t in range(T):
        out[:, t] = step(state, raw[:, t], live[:, t], t >= np.asarray(length), gamma)
    return out


class Stream:
    """one fixture stream (kind = n2n, e3d or syn) of tests/golden/reward_scaling.npz, cut into its episodes"""

    def __init__(self, gold, kind):
        self.x, self.y, start = gold[kind + "_x"], gold[kind + "_y"], gold[kind + "_start"]
        self.P = self.x.shape[1]
        b = list(np.flatnonzero(start)) + [len(start)]
        self.episodes = [(int(b[i]), int(b[i + 1])) for i in range(len(b) - 1)]
        self.final = np.concatenate(([float(gold[kind + "_n"])], gold[kind + "_mean"], gold[kind + "_S"], gold[kind + "_R"]))
