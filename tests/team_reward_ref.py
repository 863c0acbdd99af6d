"""numpy restatement of algo.team_reward: team reward sharing under the lockstep masks of the env_3d / env_n2n rollouts
(csrc/team_reward.hpp, the team option of e3d_policy_record / n2n_policy_record).

One step of an environment that was not done before it: x_p the raw reward of pursuer p (fp32, widened), live_p its live mask (0 / 1),
s = sum_k x_k live_k added in index order, m_p = (1 - alpha) x_p + (alpha s) live_p.  Every operation is f64 in the order of the
header (plain *, +, -), so the kernels reproduce it bit for bit.  m takes the place of the raw reward in what follows: the buffer's
row (buffer_reward), tests/shaping_ref.step and tests/reward_scale_ref.step (record_step below composes them the way the launch does)."""
import numpy as np

from tests import reward_scale_ref as scale_ref
from tests import shaping_ref


def team_sum(raw, live):
    """s (N,) f64: sum_k x_k live_k, the P terms added one after the other in index order, starting from 0.0"""
    x, lv = np.asarray(raw, np.float32).astype(np.float64), np.asarray(live, np.float32).astype(np.float64)
    s = np.zeros(x.shape[0], np.float64)
    for k in range(x.shape[1]):
        s = s + x[:, k] * lv[:, k]
    return s


def share(raw, live, done_before, alpha):
    """raw, live (N, P), done_before (N,) bool -> m (N, P) f64; environments done before the step keep the raw reward (the launch
    leaves them to its unshared code: their rows are raw * live, and live is 0 there)"""
    x, lv = np.asarray(raw, np.float32).astype(np.float64), np.asarray(live, np.float32).astype(np.float64)
    s = team_sum(raw, live)
    m = (1.0 - alpha) * x + (alpha * s)[:, None] * lv
    return np.where(np.asarray(done_before, bool)[:, None], x, m)


def buffer_reward(m, live):
    """the buffer's reward row without shaping and scaling: (float)m * live"""
    return np.asarray(m, np.float64).astype(np.float32) * np.asarray(live, np.float32)


def record_step(raw, live, done_before, alpha, gamma=None, scale_state=None, phi=None, p_after=None, e_after=None, ended=None, coef=None):
    """the reward row of one record launch with sharing, (N, P) float32.  phi (N, P) f64 (None: no shaping) is the carried potential,
    advanced in place from the records after the tick; scale_state (N, 1 + 3P) f64 (None: no scaling) is the RewardScaling state,
    advanced in place.  m enters the shaping step in place of the raw reward, and the result the scaling step."""
    x = share(raw, live, done_before, alpha)
    if phi is not None:
        x = shaped(phi, x, live, done_before, p_after, e_after, ended, coef, gamma)
    if scale_state is not None:
        return scale_ref.step(scale_state, x, live, done_before, gamma)
    return buffer_reward(x, live)


def shaped(phi, m, live, done_before, p_after, e_after, ended, coef, gamma):
    """shaping_ref.step for an f64 reward m (shaping_ref.step takes the fp32 raw reward and would round m): F and the advance of phi
    are shaping_ref.step's own, x = m + F live as csrc/reward_shaping.hpp adds them, m itself for environments done before the step"""
    _, F, _ = shaping_ref.step(phi, np.zeros(m.shape, np.float32), live, done_before, p_after, e_after, ended, coef, gamma)
    lv = np.asarray(live, np.float32).astype(np.float64)
    return np.where(np.asarray(done_before, bool)[:, None], m, m + F * lv)
