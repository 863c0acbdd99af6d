// central_critic.hpp -- the arithmetic of env_3d's centralised critic input (algo.e3d_critic: central; include/e3d_env.h
// e3d_central_features; numpy restatement and authority: tests/central_critic_ref.py), shared by the kernel and
// the host entry.  The critic's row of pursuer i = the 32 columns of pursuit_features.hpp's critic row, then one 8-column slot per
// team-mate, FEAT(P) = 32 + 8 (P - 1) columns in all.  Slot s holds the s-th of V_i, the active j != i, in the order of squared
// distance (strict <: the lowest index first on an exact tie, the rule of pfeat::near_add):
//   0-2 (p_j - p_i) / d_ij (0 when d_ij is 0) | 3 d_ij / W | 4-6 u_j | 7 v_j / p_vmax
// 0-3 are pfeat::mate_block's first four, 4-7 are columns 3-6 of j's own row (pfeat::common), taken as the fp32 values j stores.
// Slots s >= |V_i| are zero; so is the row of an inactive pursuer.  f64, rounded to fp32 at the store, -ffp-contract=off.
#pragma once
#include "pursuit_features.hpp"

namespace ccrit {

constexpr int MATE = 8;     // E3D_CENTRAL_MATE
constexpr int MAX_P = 16;   // E3D_CENTRAL_MAX_P

__host__ __device__ constexpr int feat(int P) { return pfeat::FEAT + MATE * (P - 1); }

// does team-mate j (squared distance dj) sort ahead of team-mate k (dk)?  A slot is addressed by its rank, the count of these
__host__ __device__ inline bool ahead(double dj, int j, double dk, int k) { return dj < dk || (dj == dk && j < k); }

// what a pursuer shares with its team: u_j and v_j / p_vmax, columns 3-6 of its own row as stored
__host__ __device__ inline void share(float *h, const pfeat::Common &c) {
    for (int q = 0; q < 4; q++) h[q] = (float)c.own[3 + q];
}

// one slot: m = p_j - p_i and its squared length, h = share() of team-mate j
__host__ __device__ inline void slot(float *f, const pfeat::Mate &m, const float *h, double world, double kill) {
    float b[5];
    pfeat::mate_block(b, true, m, world, kill);
    for (int q = 0; q < 4; q++) { f[q] = b[q]; f[4 + q] = h[q]; }
}

}  // namespace ccrit
