// ppo_diag.hpp -- the update diagnostics of the PPO loss kernels (algo.update_diagnostics / algo.target_kl; numpy
// restatement: tests/ppo_diag_ref.py).  Eight f64 sums over the live rows (active != 0, each counted once) of a loss call:
//
//   0  1                               the count c
//   1  expm1((double)lr) - (double)lr  the k3 estimator of KL(old || new); in f64, so a small lr does not cancel
//   2  [ratio < 1 - eps or ratio > 1 + eps]   the complement of ppo_elem's `inside`, the same fp32 comparisons
//   3  (double)ent                     the fp32 entropy the row hands to ppo_elem
//   4  (double)v_tgt
//   5  (double)v_tgt * (double)v_tgt
//   6  ((double)v_tgt - (double)v_now)^2
//   7  (double)ratio
//
// lr is the fp32 difference lp_now - lp_old that ppo_elem exponentiates, ratio = expf(lr) its fp32 ratio.  Plain f64 *, +, -, expm1
// in the order written with contraction off, so the host build reproduces the restatement bit for bit.
#pragma once
#include <math.h>

namespace ppodiag {

constexpr int NSUM = 8;

__host__ __device__ inline void row(double (&acc)[NSUM], float lr, float ratio, float ent, float v_now, float v_tgt, float eps) {
#pragma clang fp contract(off)
    const double x = (double)lr, y = (double)v_tgt;
    const double err = y - (double)v_now;
    acc[0] += 1.0;
    acc[1] += expm1(x) - x;
    acc[2] += (ratio < 1.f - eps || ratio > 1.f + eps) ? 1.0 : 0.0;
    acc[3] += (double)ent;
    acc[4] += y;
    acc[5] += y * y;
    acc[6] += err * err;
    acc[7] += (double)ratio;
}

}  // namespace ppodiag
