// obs_norm.hpp -- running mean / std normalisation of the env_3d policy features (algo.use_obs_norm; DESIGN.md section 7a;
// numpy restatement: tests/obs_norm_ref.py).
//
// State per agent, f64, [2][33]: row 0 the actor's features, row 1 the critic's; each row n, mean[16], M2[16], all 0 at the start.
// The statistics are frozen during a rollout: every tick normalises under the same state and adds c, S1 = sum d, S2 = sum d d
// (d = (double)x - mean) of its live rows to per-workgroup slots; once per rollout the sums are merged into the state (Chan's
// parallel update, about the frozen mean).  The eps of the division is the reference's (DHGN/normalization.py:33).  Plain f64 -,
// /, *, +, sqrt in the stated order: the translation units that include this are built with -ffp-contract=off (as for
// reward_scale.hpp), and the header also compiles for the host with a plain C++ compiler, so both reproduce numpy bit for bit.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OBSNORM_HD __host__ __device__
#else
#define OBSNORM_HD
#endif

namespace obsnorm {

constexpr int COLS = 16;             // features per network (e3d_policy_features)
constexpr int ROW = 1 + 2 * COLS;    // n, mean[COLS], M2[COLS]
constexpr double EPS = 1e-8;

// the divisor of a column, std + eps (n > 0)
OBSNORM_HD inline double denom(double n, double M2) { return sqrt(M2 / n) + EPS; }

// x under (mean, den = denom(n, M2)), clipped to [-clip, clip]
OBSNORM_HD inline float apply(float x, double mean, double den, double clip) {
    const double v = ((double)x - mean) / den;
    return (float)(v < -clip ? -clip : (v > clip ? clip : v));
}

// the normalised feature; n == 0 (no rollout merged yet) is the identity
OBSNORM_HD inline float normalise(float x, double n, double mean, double M2, double clip) {
    return n == 0.0 ? x : apply(x, mean, denom(n, M2), clip);
}

// one column's merge of a rollout's totals C = count, A = sum d, Q = sum d d (d about the mean in force) into (mean, M2) of n
// samples; the caller sets n' = n + C afterwards.  C == 0 changes nothing.
OBSNORM_HD inline void merge(double n, double C, double A, double Q, double &mean, double &M2) {
    if (C == 0.0) return;
    const double n1 = n + C, delta = A / C;
    mean = mean + A / n1;
    M2 = M2 + (Q - A * delta) + delta * delta * (n * C / n1);
}

}  // namespace obsnorm
