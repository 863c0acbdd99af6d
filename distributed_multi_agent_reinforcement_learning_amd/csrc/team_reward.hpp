// team_reward.hpp -- team reward sharing for one pursuer of one environment, shared by env_3d and env_n2n (algo.team_reward: alpha;
// DESIGN.md section 7j; numpy restatement: tests/team_reward_ref.py).
//
// One step of an environment that was not done before it: x the pursuer's raw reward (fp32, widened), live its live mask (0 / 1),
// s = sum_k x_k live_k over the environment's P pursuers in index order (f64).  The shared reward
//     m = (1 - alpha) x + (alpha s) live
// takes the place of the raw reward in whatever follows in the record launch: the shaping step, the RewardScaling step, the buffer's
// row.  alpha = 0: m is x; alpha = 1: m is s on a live row and 0 on any other.  A weighted sum, not a mean: at alpha = 1 every live
// pursuer sees the team's total.  (A raw reward of -0.0 comes out as +0.0; the environments pay (float)int or 0.f, never -0.0.)
// Plain *, +, - in the order written, so the translation units that include this are built with -ffp-contract=off and reproduce
// numpy bit for bit.
#pragma once

namespace team {

// alpha is a coefficient: a number in [0, 1] (NaN and the infinities fail both comparisons or one of them)
__host__ __device__ inline bool coef_ok(double alpha) { return alpha >= 0.0 && alpha <= 1.0; }

// s: the team's sum of x * live, this pursuer's term included.  Returns m (f64).
__host__ __device__ inline double share(double alpha, double x, double s, double live) { return (1.0 - alpha) * x + (alpha * s) * live; }

}  // namespace team
