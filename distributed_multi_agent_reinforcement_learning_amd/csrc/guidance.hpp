// guidance.hpp -- the scripted lead-pursuit law of one pursuer, shared by env_3d and env_n2n (runtime.guidance_*; DESIGN.md section 7e;
// numpy restatement and authority: tests/guidance_ref.py).  A yardstick policy, not a learner: what a hand-written controller captures
// on the seeds the trainers evaluate on.
//
// Pursuer i (active) against an evader (active; env_n2n: the nearest active one, lowest index on ties):
//   r = e_pos - p_i, d = |r|; e_vel from the evader's heading(s) and speed; t = min(d / p_vmax, lead); aim = r + t e_vel;
//   g = aim / |aim| (0 when |aim| is 0); every active team-mate j != i with 0 < d_ij < sep_range, in index order, adds
//   gain (p_i - p_j) / d_ij (sep_range - d_ij) / sep_range to g; the command is the direction of g (full speed), or HOLD (keep the
//   heading, stop) when g is exactly 0 or the pursuer or the evader is inactive.
// Plain *, +, -, /, sqrt in the order written (sums of squares left to right), so the translation units that include this are built
// with -ffp-contract=off; atan2, cos and sin are the only steps that may differ from numpy, by a few ulp.
#pragma once
#include <math.h>
#include <stdint.h>

namespace guide {

constexpr double PI = 3.14159265358979323846;

__host__ __device__ inline bool param_ok(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }   // finite and >= 0 (nan fails)

// the look-ahead: d / p_vmax, at most `lead` (a nan from 0 / 0 takes the cap)
__host__ __device__ inline double lead_time(double d, double p_vmax, double lead) {
    const double t = d / p_vmax;
    return t < lead ? t : lead;
}

// a / |a|, or 0 when |a| is 0 (az = 0 in the plane: adding 0 * 0 changes no bit of a sum of squares)
__host__ __device__ inline void unit(double ax, double ay, double az, double &gx, double &gy, double &gz) {
    const double n = sqrt(ax * ax + ay * ay + az * az);
    const bool z = n == 0.0;
    gx = z ? 0.0 : ax / n; gy = z ? 0.0 : ay / n; gz = z ? 0.0 : az / n;
}

__host__ __device__ inline bool in_sep(double dij, double sep_range) { return dij > 0.0 && dij < sep_range; }
// one component of the repulsion from team-mate j: diff = p_i - p_j of that component
__host__ __device__ inline double repel(double gain, double diff, double dij, double sep_range) {
    return gain * diff / dij * (sep_range - dij) / sep_range;
}

__host__ __device__ inline double unit_clip(double v) { return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v); }

// env_3d: the command (heading / pi, pitch / (pi / 2), speed) in [-1, 1]^3 that e3d_env_tick takes
__host__ __device__ inline void e3d_command(bool on, double gx, double gy, double gz, double phi, double gamma, double &a0, double &a1, double &a2) {
    if (!on || (gx == 0.0 && gy == 0.0 && gz == 0.0)) {   // hold
        a0 = unit_clip(phi / PI); a1 = unit_clip(gamma / (PI / 2)); a2 = -1.0;
        return;
    }
    a0 = unit_clip(atan2(gy, gx) / PI);
    a1 = unit_clip(atan2(gz, sqrt(gx * gx + gy * gy)) / (PI / 2));
    a2 = 1.0;
}

// env_n2n: bearing b -> the action k in 1..8 whose heading k pi / 4 (the tick turns k pi / 4 > pi into its negative angle) is nearest;
// 0 and -8 map to 8
__host__ __device__ inline int32_t octant(double b) {
    const int k = (int)rint(b / (PI / 4));
    const int m = ((k % 8) + 8) % 8;
    return m == 0 ? 8 : m;
}
__host__ __device__ inline int32_t n2n_command(bool on, double gx, double gy) {
    if (!on || (gx == 0.0 && gy == 0.0)) return 0;   // hold: action 0 stops and keeps the heading
    return octant(atan2(gy, gx));
}

}  // namespace guide
