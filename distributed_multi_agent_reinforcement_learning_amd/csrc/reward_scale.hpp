// reward_scale.hpp -- one step of the reference's RewardScaling (DHGN/normalization.py:38-52) for one pursuer of one environment.
//
// State per environment, f64, [1 + 3P]: n, mean[P], S[P], R[P].  n, mean and S persist over episodes; R, the discounted return,
// is zeroed by the caller at every episode start (RewardScaling.reset).  The step is RunningMeanStd.update (:12-22) on R, then
// x / (std + 1e-8), in the reference's operation order: plain *, +, /, sqrt, so the translation units that include this are built
// with -ffp-contract=off and reproduce numpy bit for bit.  The first sample's quirk is the reference's: at n == 1 the std IS R
// (not 0), so a first reward of -1 is scaled to +1.
#pragma once
#include <math.h>

namespace rscale {

// x: this step's raw reward; n: the sample count INCLUDING this step (the environment's n + 1, shared by its P pursuers);
// mean, S, R: the pursuer's entries, updated in place.  Returns the scaled reward (f64).
__host__ __device__ inline double step(double x, double gamma, double n, double &mean, double &S, double &R) {
    R = gamma * R + x;
    double sd;
    if (n == 1.0) {
        mean = R;
        sd = R;
    } else {
        const double old_mean = mean;
        mean = old_mean + (R - old_mean) / n;
        S = S + (R - old_mean) * (R - mean);
        sd = sqrt(S / n);
    }
    return x / (sd + 1e-8);
}

}  // namespace rscale
