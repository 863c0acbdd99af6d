// pursuit_features.hpp -- the arithmetic of env_3d's line-of-sight policy features (algo.e3d_features: pursuit; include/e3d_env.h
// e3d_pursuit_features; numpy restatement and authority: tests/e3d_features_ref.py), shared by the kernel and
// the host entry.  One row = one pursuer i, 32 columns, the same for actor and critic; the two differ in k (who knows where the evader
// is) and in V (which team-mates are visible):
//   0-2 p_i / (W / 2) - 1 | 3-5 u_i | 6 v_i / p_vmax | 7-9 k rh | 10 k d / W | 11-13 k e_vel / e_vmax
//   14 k (-rh . (e_vel - v_i u_i)) / (e_vmax + p_vmax) | 15 k (u_i . rh) | 16 k | 17-19 k (target - e_pos) / W
//   20-24, 25-29 the nearest two of V: (p_j - p_i) / d_ij (0 when d_ij is 0), d_ij / W, kill_radius / max(d_ij, kill_radius)
//   30 |V| / max(P - 1, 1) | 31 time_step / max_step
// with u_i = (cos gamma_i cos phi_i, cos gamma_i sin phi_i, sin gamma_i), r = e_pos - p_i, d = |r|, rh = r / d (0 when d is 0).
// Plain *, +, -, /, sqrt, sin, cos in the order written (sums of squares and dot products x, y, z, left to right), f64, rounded to fp32
// at the store: the translation units that include this are built with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

namespace pfeat {

constexpr int FEAT = 32;

struct Mate { double d2, dx, dy, dz; };   // p_j - p_i and its squared length
// the nearest two of the team-mates added so far, in the order of squared distance; strict <, so the lowest index wins a tie
struct Near { Mate m1, m2; int n; };

__host__ __device__ inline void near_init(Near &s) { s.m1 = Mate{0, 0, 0, 0}; s.m2 = Mate{0, 0, 0, 0}; s.n = 0; }

__host__ __device__ inline double sq3(double dx, double dy, double dz) { return dx * dx + dy * dy + dz * dz; }

// team-mates arrive in index order
__host__ __device__ inline void near_add(Near &s, double dx, double dy, double dz) {
    const Mate c{sq3(dx, dy, dz), dx, dy, dz};
    if (s.n == 0 || c.d2 < s.m1.d2) { s.m2 = s.m1; s.m1 = c; }
    else if (s.n == 1 || c.d2 < s.m2.d2) s.m2 = c;
    s.n++;
}

// what both networks share of a row: the pursuer's own columns, the evader block before k, the clock
struct Common { double own[7], ev[13], clock; };

// p (x, y, z, phi, gamma, v) of the pursuer, e of the evader, t the target
__host__ __device__ inline void common(Common &c, double x, double y, double z, double phi, double gamma, double v, double ex, double ey, double ez,
                                       double ephi, double egam, double evel, double tx, double ty, double tz, double world, double p_vmax,
                                       double e_vmax, int32_t time_step, int32_t max_step) {
    const double half = world / 2, cg = cos(gamma);
    const double ux = cg * cos(phi), uy = cg * sin(phi), uz = sin(gamma);
    c.own[0] = x / half - 1; c.own[1] = y / half - 1; c.own[2] = z / half - 1;
    c.own[3] = ux; c.own[4] = uy; c.own[5] = uz;
    c.own[6] = v / p_vmax;
    const double rx = ex - x, ry = ey - y, rz = ez - z, d = sqrt(sq3(rx, ry, rz));
    const bool z0 = d == 0.0;
    const double hx = z0 ? 0.0 : rx / d, hy = z0 ? 0.0 : ry / d, hz = z0 ? 0.0 : rz / d;
    const double ecg = cos(egam);
    const double vx = evel * ecg * cos(ephi), vy = evel * ecg * sin(ephi), vz = evel * sin(egam);
    const double wx = vx - v * ux, wy = vy - v * uy, wz = vz - v * uz;   // the evader's velocity relative to the pursuer's
    c.ev[0] = hx; c.ev[1] = hy; c.ev[2] = hz;
    c.ev[3] = d / world;
    c.ev[4] = vx / e_vmax; c.ev[5] = vy / e_vmax; c.ev[6] = vz / e_vmax;
    c.ev[7] = (-hx * wx + -hy * wy + -hz * wz) / (e_vmax + p_vmax);       // the closing speed
    c.ev[8] = ux * hx + uy * hy + uz * hz;
    c.ev[9] = 1.0;
    c.ev[10] = (tx - ex) / world; c.ev[11] = (ty - ey) / world; c.ev[12] = (tz - ez) / world;
    c.clock = (double)time_step / (double)max_step;
}

__host__ __device__ inline void mate_block(float *f, bool has, const Mate &m, double world, double kill) {
    if (!has) { f[0] = f[1] = f[2] = f[3] = f[4] = 0.f; return; }
    const double d = sqrt(m.d2);
    const bool z0 = d == 0.0;
    f[0] = (float)(z0 ? 0.0 : m.dx / d); f[1] = (float)(z0 ? 0.0 : m.dy / d); f[2] = (float)(z0 ? 0.0 : m.dz / d);
    f[3] = (float)(d / world);
    f[4] = (float)(kill / (d > kill ? d : kill));
}

// the row of one network: k != 0 where this network knows the evader (k is 0 or 1, so k x is x or 0)
__host__ __device__ inline void row(float *f, const Common &c, bool k, const Near &s, int32_t P, double world, double kill) {
    for (int q = 0; q < 7; q++) f[q] = (float)c.own[q];
    for (int q = 0; q < 13; q++) f[7 + q] = k ? (float)c.ev[q] : 0.f;
    mate_block(f + 20, s.n > 0, s.m1, world, kill);
    mate_block(f + 25, s.n > 1, s.m2, world, kill);
    f[30] = (float)((double)s.n / (double)(P > 2 ? P - 1 : 1));
    f[31] = (float)c.clock;
}

// who hears of a sighting (evader_obs: team): the closure of every pursuer's neighbour mask (bit j of nb[i]: an edge i - j between two
// active pursuers; bit i of nb[i] set) by repeated passes until nothing changes -- the host's form; the kernel doubles paths instead
inline void close_masks(uint64_t *reach, int P) {
    for (bool grew = true; grew;) {
        grew = false;
        for (int i = 0; i < P; i++) {
            uint64_t m = reach[i];
            for (int j = 0; j < P; j++)
                if ((reach[i] >> j) & 1ull) m |= reach[j];
            if (m != reach[i]) { reach[i] = m; grew = true; }
        }
    }
}

}  // namespace pfeat
