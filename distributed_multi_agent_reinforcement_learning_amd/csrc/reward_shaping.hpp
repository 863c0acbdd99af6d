// reward_shaping.hpp -- potential-based distance shaping (Ng, Harada and Russell 1999) for one pursuer of one environment, shared by
// env_3d and env_n2n (algo.reward_shaping: distance; DESIGN.md sections 7a, 7b; numpy restatement: tests/shaping_ref.py).
//
// Potential of pursuer p in a state: Phi = -coef * min_k |pos_p - pos_k| over the evaders k active in that state, 0 when the pursuer
// is inactive or no evader is active.  State per environment, f64, [P]: Phi of the state the next tick starts from.  A tick's shaped
// reward is x = raw + (gamma * Phi_next - Phi) * live, where Phi_next is the potential of the state after the tick, or 0 when the
// pursuer is inactive after it or its episode ended for a reason other than the time limit (the rule that zeroes the bootstrap
// value).  Plain *, +, -, sqrt in the order written, so the translation units that include this are built with -ffp-contract=off and
// reproduce numpy bit for bit.
#pragma once
#include <math.h>

namespace rshape {

__host__ __device__ inline double dist2(double dx, double dy) { return sqrt(dx * dx + dy * dy); }
__host__ __device__ inline double dist3(double dx, double dy, double dz) { return sqrt(dx * dx + dy * dy + dz * dz); }

// dmin: the distance to the nearest active evader (any: there is one)
__host__ __device__ inline double potential(double coef, bool p_on, bool any, double dmin) { return (p_on && any) ? -coef * dmin : 0.0; }

// phi: the carried potential of the state before the tick, replaced by phi_state, the potential of the state after it (before the
// terminal rule); terminal: the pursuer is inactive after the tick or the episode ended, the time limit excepted.  Returns x (f64).
__host__ __device__ inline double step(double raw, double gamma, double &phi, double phi_state, bool terminal, double live) {
    const double phi_next = terminal ? 0.0 : phi_state;
    const double F = gamma * phi_next - phi;
    phi = phi_state;
    return raw + F * live;
}

}  // namespace rshape
