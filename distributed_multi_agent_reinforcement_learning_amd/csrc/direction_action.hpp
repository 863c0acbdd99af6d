// direction_action.hpp -- the arithmetic of env_3d's direction-vector action head (algo.gauss_squash: direction; DESIGN.md section 7h;
// numpy restatement and specification: tests/direction_ref.py), shared by the rollout head (csrc/gauss_policy.hpp k_gauss_head_ex), the
// imitation launches (csrc/imitation.hpp k_e3d_bc_select, k_bc_loss_gauss) and the host entries of csrc/e3d_env.hip
// (gauss_direction_map_host, e3d_direction_label_host).  The policy's latent action is u = (u_x, u_y, u_z, s); the environment reads
//   a0 = atan2(u_y, u_x) / pi | a1 = atan2(u_z, hypot(u_x, u_y)) / (pi / 2) | a2 = s,   each clamped to [-1, 1],
// in f64 from the fp32 u.  Divisions by the f64 constants, not products with reciprocals: atan2(+0, -1) / pi is exactly 1,
// atan2(-0, -1) / pi exactly -1, atan2(1, 0) / pi exactly 0.5, and u_x = u_y = u_z = 0 gives (0, 0).  The teacher's label of a command
// g = (heading / pi, pitch / (pi / 2), speed) is the unit vector of its angles and the speed, rounded to fp32.  Plain f64 and libm
// calls; no expression here has a product feeding a sum, so contraction cannot change a bit of to_env or label.
#pragma once
#include <math.h>
#include <stdint.h>

namespace diract {

constexpr int LATENT = 4;   // (u_x, u_y, u_z, s)
constexpr int ENV_A = 3;    // (a0, a1, a2)
constexpr double PI = 3.14159265358979323846;
constexpr float HALF_PI_F = 1.57079632679489661923f;

__host__ __device__ inline double clamp1(double x) { return fmin(fmax(x, -1.0), 1.0); }

// u [4] fp32 -> env [3] f64
__host__ __device__ inline void to_env(const float *u, double *env) {
    const double ux = (double)u[0], uy = (double)u[1], uz = (double)u[2];
    env[0] = clamp1(atan2(uy, ux) / PI);
    env[1] = clamp1(atan2(uz, hypot(ux, uy)) / (PI / 2));
    env[2] = clamp1((double)u[3]);
}

// g [3] f64 (a guidance action) -> a_star [4] fp32
__host__ __device__ inline void label(const double *g, float *a_star) {
    const double phi = g[0] * PI, gam = g[1] * PI / 2;
    const double cg = cos(gam);
    a_star[0] = (float)(cg * cos(phi));
    a_star[1] = (float)(cg * sin(phi));
    a_star[2] = (float)sin(gam);
    a_star[3] = (float)g[2];
}

// the angle between m [3] and d [3] in radians, fp32: atan2f(|m x d|, m . d); pi / 2 when |m|^2 is 0 (a mean that points nowhere)
__host__ __device__ inline float angle(const float *m, const float *d) {
#pragma clang fp contract(off)
    if (m[0] * m[0] + m[1] * m[1] + m[2] * m[2] == 0.f) return HALF_PI_F;
    const float cx = m[1] * d[2] - m[2] * d[1], cy = m[2] * d[0] - m[0] * d[2], cz = m[0] * d[1] - m[1] * d[0];
    return atan2f(sqrtf(cx * cx + cy * cy + cz * cz), m[0] * d[0] + m[1] * d[1] + m[2] * d[2]);
}

}  // namespace diract
