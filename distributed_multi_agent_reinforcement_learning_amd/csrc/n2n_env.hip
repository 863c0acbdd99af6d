// n2n_env.hip -- batched env_n2n (continuous 2-D pursuit, no obstacles) for MI355X (gfx950).  C ABI: include/n2n_env.h.
// Several environments per wavefront (lane = (environment, agent slot), see k_n2n); the environment's record (5 x (P + E)
// doubles) is contiguous in HBM, every agent lives in its lane's registers, pairwise kill-radius / range tests go through
// wave shuffles.  f64 state like the reference; headings go through
// the device cos/sin (agreement with the reference's libm: <= 1e-9 on positions over an episode, see tests).
// Build with -ffp-contract=off; the only fused multiply-add is the explicit one in norm2 (numpy's 2-vector norm).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "n2n_env.h"
#include "guidance.hpp"
#include "reward_scale.hpp"
#include "reward_shaping.hpp"
#include "rng_replica.hpp"
#include "slsqp_box.hpp"
#include "team_reward.hpp"

namespace {

constexpr int WAVE = 64;
constexpr double PI = 3.14159265358979323846;

__host__ __device__ inline double norm2(double a, double b) { return sqrt(fma(b, b, a * a)); }
// `norm2(a, b) <= r` without the square root: sqrt is correctly rounded and monotonic, so it holds exactly when the squared norm
// (the same fma the norm takes the root of) is <= the largest double t with sqrt(t) <= r, computed once per launch on the host.
// Held by tests/test_particle_config_gpu.py on states whose squared distance is t itself, one double above it, or on the other
// side of it than the unfused sum (tests/particle_config_cases.py): t is not fl(r r) for r = 0.5, the default kill radius.
__device__ __forceinline__ double sq2(double a, double b) { return fma(b, b, a * a); }
double sq_threshold(double r) {
    auto ok = [&](double t) { return sqrt(t) <= r; };
    if (!(r >= 0.0) || !ok(0.0)) return -1.0;  // a squared norm is >= 0: nothing qualifies
    if (std::isinf(r)) return r;
    double t = r * r;
    while (!ok(t)) t = nextafter(t, 0.0);
    for (;;) {
        const double n = nextafter(t, INFINITY);
        if (std::isinf(n) || !ok(n)) break;
        t = n;
    }
    return t;
}
struct N2nThr { double kill, comm, sen; };
__device__ __forceinline__ double sgn(double v) { return (double)((v > 0) - (v < 0)); }

// particle_env.py:41-57 / :78-90 : signed heading change towards the commanded heading a, limited to ang_lmt
__device__ __forceinline__ double turn(double a, double phi, double lim) {
    double sign, delta;
    const double d = fabs(a - phi);
    if (sgn(a * phi) >= 0) { delta = d; sign = sgn(a - phi); }
    else if (d < 2 * PI - d) { delta = d; sign = sgn(a - phi); }
    else { delta = 2 * PI - d; sign = -sgn(a - phi); }
    delta = delta > lim ? lim : (delta < 0 ? 0 : delta);
    return sign * delta;
}
__device__ __forceinline__ double wrap(double phi) { return phi > PI ? phi - 2 * PI : (phi < -PI ? phi + 2 * PI : phi); }

// lane = (environment, agent slot): a group of PT lanes owns one environment (PT = power of two >= max(P, E)), G = 64 / PT
// environments per wavefront, four wavefronts per workgroup.  Slot a holds pursuer a (a < P) AND evader a (a < E) in
// registers; partners are read through wave shuffles inside the group.  (One wavefront per environment left 48 of 64 lanes
// idle at P = 16 and the launch bound by per-wave latency: 9 % of the HBM roofline in round 1.)
constexpr int WPB = 4;

template <int PT, bool TICK>
__global__ __launch_bounds__(WAVE * WPB) void k_n2n(const n2n_config c, const n2n_state st, const int32_t *actions, const double *e_cmd, float *reward,
                                                    uint8_t *active, uint8_t *done, const n2n_obs_out o, const N2nThr th) {
    constexpr int G = WAVE / PT;
    constexpr unsigned long long GM = (PT == 64) ? ~0ull : ((1ull << PT) - 1ull);
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT, base = lane - a;
    const int env = wave * G + g, P = c.P, E = c.E;
    const bool ev = env < st.N, pv = ev && a < P, evv = ev && a < E;
    double px = 0, py = 0, pphi = 0, pvel = 0, pact = 0, ex = 0, ey = 0, ephi = 0, evel = 0, eact = 0;
    double *gp = st.p + (size_t)(ev ? env : 0) * 5 * P, *ge = st.e + (size_t)(ev ? env : 0) * 5 * E;
    if (pv) { px = gp[a]; py = gp[P + a]; pphi = gp[2 * P + a]; pvel = gp[3 * P + a]; pact = gp[4 * P + a]; }
    if (evv) { ex = ge[a]; ey = ge[E + a]; ephi = ge[2 * E + a]; evel = ge[3 * E + a]; eact = ge[4 * E + a]; }
    if (TICK) {
        // Evader.step (:74-99): position with the OLD heading, then the heading turns towards the command
        if (evv && eact != 0.0) {
            const double d = turn(e_cmd[(size_t)env * E + a] * PI, ephi, c.ang_lmt);
            ex += evel * cos(ephi) * c.step_size;
            ey += evel * sin(ephi) * c.step_size;
            ephi = wrap(ephi + d);
        }
        // Pursuer.step (:34-67): the heading turns even when the pursuer is inactive, the position only moves when active
        if (pv) {
            const int a_i = actions[(size_t)env * P + a];
            double v = 0.0;
            if (a_i != 0) {
                v = c.p_vmax;
                double ang = (double)a_i * PI / 4;
                if (ang > PI) ang -= 2 * PI;
                pphi = wrap(pphi + turn(ang, pphi, c.ang_lmt));
            }
            if (pact != 0.0) {
                px += v * cos(pphi) * c.step_size;
                py += v * sin(pphi) * c.step_size;
                pvel = v;
            }
        }
        // reward (:316-334) and update_agent_active (:336-365) are both evaluated on the moved, not yet culled state
        int ce = 0, cp = 0, chit = 0;
        for (int k = 0; k < E; k++) {
            const double kx = __shfl(ex, base + k), ky = __shfl(ey, base + k), ka = __shfl(eact, base + k);
            ce += ka != 0.0 && sq2(px - kx, py - ky) <= th.kill;
        }
        for (int k = 0; k < P; k++) {
            const double kx = __shfl(px, base + k), ky = __shfl(py, base + k), ka = __shfl(pact, base + k);
            cp += ka != 0.0 && sq2(px - kx, py - ky) <= th.kill;
            chit += ka != 0.0 && sq2(ex - kx, ey - ky) <= th.kill;   // the evader of this slot against pursuer k
        }
        const bool p_on = pv && pact != 0.0, e_on = evv && eact != 0.0;
        if (pv) reward[(size_t)env * P + a] = p_on ? (float)(ce - (cp - 1)) : 0.f;
        if (p_on && (cp + ce - 1) != 0) { px = 1000; py = 1000; pphi = 0; pact = 0; }
        if (e_on && chit != 0) { ex = 1000; ey = 1000; ephi = 0; eact = 0; }
        const bool pact_b = pv && pact != 0.0, eact_b = evv && eact != 0.0;
        double tx = 0, ty = 0;
        if (ev) { tx = st.target[2 * env]; ty = st.target[2 * env + 1]; }
        const bool reach = evv && sq2(ex - tx, ey - ty) <= th.kill;  // get_done (:283-304), all evaders
        const int pa = __popcll((__ballot(pact_b) >> base) & GM), ea = __popcll((__ballot(eact_b) >> base) & GM);
        const bool rc = ((__ballot(reach) >> base) & GM) != 0ull;
        if (pv) {
            active[(size_t)env * P + a] = pact_b;
            gp[a] = px; gp[P + a] = py; gp[2 * P + a] = pphi; gp[3 * P + a] = pvel; gp[4 * P + a] = pact;
        }
        if (evv) { ge[a] = ex; ge[E + a] = ey; ge[2 * E + a] = ephi; ge[3 * E + a] = evel; ge[4 * E + a] = eact; }
        if (ev && a == 0) {
            const int t = st.time_step[env] + 1;
            st.time_step[env] = t;
            done[env] = (uint8_t)(rc || pa == 0 || ea == 0 || t >= c.episode_limit);
        }
    }
    // observations (get_team_state rules=False, get_adj_mat :386-397: rows of inactive pursuers are zero)
    if (o.p_state && pv) {
        float *d = o.p_state + (int64_t)env * o.p_state_stride + 3 * a;
        d[0] = (float)px; d[1] = (float)py; d[2] = (float)pphi;
    }
    if (o.e_state && evv) {
        float *d = o.e_state + (int64_t)env * o.e_state_stride + 3 * a;
        d[0] = (float)ex; d[1] = (float)ey; d[2] = (float)ephi;
    }
    if (o.pp_adj)
        for (int k = 0; k < P; k++) {  // row k, column a: the lanes of a group store consecutive floats
            const double kx = __shfl(px, base + k), ky = __shfl(py, base + k), ka = __shfl(pact, base + k);
            if (pv) o.pp_adj[(int64_t)env * o.pp_adj_stride + k * P + a] = (ka != 0.0 && sq2(kx - px, ky - py) <= th.comm) ? 1.f : 0.f;
        }
    if (o.pe_adj)
        for (int k = 0; k < E; k++) {
            const double kx = __shfl(ex, base + k), ky = __shfl(ey, base + k);
            if (pv) o.pe_adj[(int64_t)env * o.pe_adj_stride + a * E + k] = (pact != 0.0 && sq2(px - kx, py - ky) <= th.sen) ? 1.f : 0.f;
        }
}

// the lane layout of the tick and of the policy kernels: PT (group of lanes per environment) and the workgroups covering N environments
int n2n_lanes(const n2n_config *c, int N, int *blocks) {
    const int m = c->P > c->E ? c->P : c->E;
    const int pt = m <= 8 ? 8 : (m <= 16 ? 16 : (m <= 32 ? 32 : 64));
    const int envs_per_block = (WAVE / pt) * WPB;
    *blocks = (N + envs_per_block - 1) / envs_per_block;
    return pt;
}

template <bool TICK>
int launch_n2n(const n2n_config *c, const n2n_state *st, const int32_t *actions, const double *e_cmd, float *reward, uint8_t *active, uint8_t *done,
               const n2n_obs_out &o, hipStream_t s) {
    int blocks;
    const int pt = n2n_lanes(c, st->N, &blocks);
    const N2nThr th{sq_threshold(c->kill_radius), sq_threshold(c->p_comm_range), sq_threshold(c->p_sen_range)};
#define N2N_GO(PT) hipLaunchKernelGGL((k_n2n<PT, TICK>), dim3(blocks), dim3(WAVE * WPB), 0, s, *c, *st, actions, e_cmd, reward, active, done, o, th)
    if (pt == 8) N2N_GO(8); else if (pt == 16) N2N_GO(16); else if (pt == 32) N2N_GO(32); else N2N_GO(64);
#undef N2N_GO
    return (int)hipGetLastError();
}

// ---- MAPPO on env_n2n (n2n_agent.py): the policy's inputs before a tick, the buffer bookkeeping after it ----
// Lane layout of k_n2n: a group of PT lanes per environment, slot a = pursuer a and evader a.  The per-group masks (live pursuers,
// active evaders) are ballots, so the adjacency loops run a uniform trip count over the group's lanes with no shuffles.

template <int PT>
__device__ __forceinline__ unsigned long long group_bits(bool v, int base) {
    constexpr unsigned long long GM = (PT == 64) ? ~0ull : ((1ull << PT) - 1ull);
    return (__ballot(v) >> base) & GM;
}

__device__ __forceinline__ void store4(float *d, bool on, double x, double y, double phi, double v) {
    d[0] = on ? (float)x : 0.f;
    d[1] = on ? (float)y : 0.f;
    d[2] = on ? (float)(v * cos(phi)) : 0.f;
    d[3] = on ? (float)(v * sin(phi)) : 0.f;
}

template <int PT>
__global__ __launch_bounds__(WAVE * WPB) void k_n2n_policy_inputs(const n2n_config c, const n2n_state st, const uint8_t *done_before,
                                                                  const n2n_policy_io io) {
    constexpr int G = WAVE / PT;
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT, base = lane - a;
    const int env = wave * G + g, P = c.P, E = c.E;
    const bool ev = env < st.N, pv = ev && a < P, evv = ev && a < E;
    const double *gp = st.p + (size_t)(ev ? env : 0) * 5 * P, *ge = st.e + (size_t)(ev ? env : 0) * 5 * E;
    const bool db = ev && done_before && done_before[env] != 0;
    const bool live = pv && gp[4 * P + a] != 0.0 && !db;
    const bool e_on = evv && ge[4 * E + a] != 0.0;
    const unsigned long long lm = group_bits<PT>(live, base), em = group_bits<PT>(e_on, base);
    if (pv && io.live) io.live[(int64_t)env * io.live_rs + a] = live ? 1.f : 0.f;
    if (pv && io.p4) store4(io.p4 + (int64_t)env * io.p4_rs + 4 * a, live, gp[a], gp[P + a], gp[2 * P + a], gp[3 * P + a]);
    if (evv && io.e4) store4(io.e4 + (int64_t)env * io.e4_rs + 4 * a, e_on, ge[a], ge[E + a], ge[2 * E + a], ge[3 * E + a]);
    // e_ref: the lowest-index active evader (its lane writes), zeros from slot 0 when none is active
    const int first = em ? __ffsll((long long)em) - 1 : 0;
    if (ev && io.e_ref && a == first)
        store4(io.e_ref + (int64_t)env * io.e_ref_rs, e_on, ge[first], ge[E + first], ge[2 * E + first], ge[3 * E + first]);
    // the actor's adjacencies: entries between live pursuers (pp), between a live pursuer and an active evader (pe)
    if (io.pp_adj)
        for (int k0 = 0; k0 < P * P; k0 += PT) {
            const int k = k0 + a, i = k / P, j = k - i * P;
            if (ev && k < P * P)
                io.pp_adj[(int64_t)env * io.pp_adj_rs + k] = ((lm >> i) & (lm >> j) & 1ull) ? io.pp_in[(int64_t)env * io.pp_in_rs + k] : 0.f;
        }
    if (io.pe_adj)
        for (int k0 = 0; k0 < P * E; k0 += PT) {
            const int k = k0 + a, i = k / E, j = k - i * E;
            if (ev && k < P * E)
                io.pe_adj[(int64_t)env * io.pe_adj_rs + k] = ((lm >> i) & (em >> j) & 1ull) ? io.pe_in[(int64_t)env * io.pe_in_rs + k] : 0.f;
        }
}

// the shaping potential of pursuer a in the current records gp / ge of its environment (p_on: its active flag): the nearest active evader
__device__ __forceinline__ double n2n_potential(const double *gp, const double *ge, int P, int E, int a, bool p_on, double coef) {
    const double px = gp[a], py = gp[P + a];
    double dmin = 0.0;
    bool any = false;
    for (int k = 0; k < E; k++) {
        if (ge[4 * E + k] == 0.0) continue;
        const double d = rshape::dist2(px - ge[k], py - ge[E + k]);
        dmin = (any && dmin < d) ? dmin : d;
        any = true;
    }
    return rshape::potential(coef, p_on, any, dmin);
}

// SCALED: the reward row is the reference's RewardScaling of the raw reward (csrc/reward_scale.hpp) for environments not done before
// the step; rs [N][1 + 3P] (n, mean[P], S[P], R[P]) is read and written once per lane, n by slot 0 after every lane of the group has
// loaded it (one wave, program order).  The return accumulator keeps the raw reward.  SHAPED: potential-based distance shaping
// (csrc/reward_shaping.hpp) goes into the reward row -- and into RewardScaling when SCALED -- once the terminal predicate of v_next is
// known; every lane loads and stores its own phi [N][P] entry once and walks the E evaders itself.  The unshaped instantiations are the
// code they were before SHAPED existed.  TEAM: team reward sharing (csrc/team_reward.hpp) -- m = (1 - alpha) raw + (alpha s) live, s the
// team's f64 sum of raw * live from shuffles in agent order ahead of everything that reads a reward, takes the place of the raw reward
// in the shaping step, the RewardScaling step and the buffer's row of environments not done before the step; acc.ret keeps the raw
// reward.  Every TEAM statement sits under `if (TEAM)` or is `m` where `(double)raw` stood, so the TEAM = false instantiations are the
// instructions they were before it.
template <int PT, bool SCALED, bool SHAPED, bool TEAM>
__global__ __launch_bounds__(WAVE * WPB) void k_n2n_policy_record(const n2n_config c, const n2n_state st, const float *reward, const uint8_t *done,
                                                                  const n2n_record_io io, const n2n_policy_acc acc, const double kill,
                                                                  double *rs, const double gamma, double *phi, const double coef,
                                                                  const double alpha) {
    constexpr int G = WAVE / PT;
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT, base = lane - a;
    const int env = wave * G + g, P = c.P, E = c.E;
    const bool ev = env < st.N, pv = ev && a < P, evv = ev && a < E;
    const double *gp = st.p + (size_t)(ev ? env : 0) * 5 * P, *ge = st.e + (size_t)(ev ? env : 0) * 5 * E;
    const float live = pv ? io.live[(int64_t)env * io.live_rs + a] : 0.f;
    const float raw = pv ? reward[(size_t)env * P + a] : 0.f;
    const float rl = raw * live;
    float rb = rl;  // the buffer's reward
    double m = (double)raw;  // what shaping, scaling and the buffer take for the reward
    if (TEAM) {  // every lane of the wave runs the loop (the trip count is wave-uniform)
        const double xl = (double)raw * (double)live;
        double sd = 0.0;
        for (int k = 0; k < P; k++) sd = sd + __shfl(xl, base + k);
        if (ev && acc.done_before[env] == 0) m = team::share(alpha, (double)raw, sd, (double)live);
        if (!SCALED && !SHAPED) rb = (float)m * live;
    }
    if (SCALED && !SHAPED && pv && acc.done_before[env] == 0) {
        double *q = rs + (size_t)env * (1 + 3 * P);
        const double n = q[0] + 1.0;
        double mean = q[1 + a], S = q[1 + P + a], R = q[1 + 2 * P + a];
        rb = (float)rscale::step(m, gamma, n, mean, S, R) * live;
        q[1 + a] = mean; q[1 + P + a] = S; q[1 + 2 * P + a] = R;
        if (a == 0) q[0] = n;
    }
    if (pv) {
        if (!SHAPED && io.r) io.r[(int64_t)env * io.r_rs + a] = rb;
        if (io.active) io.active[(int64_t)env * io.active_rs + a] = live;
        if (io.v) io.v[(int64_t)env * io.v_rs + a] = io.value[(int64_t)env * io.value_rs + a] * live;
    }
    // the state after the tick (the records): why the episode may have ended, as get_done of the tick evaluates it
    const bool p_on = pv && gp[4 * P + a] != 0.0, e_on = evv && ge[4 * E + a] != 0.0;
    double tx = 0, ty = 0;
    if (ev) { tx = st.target[2 * env]; ty = st.target[2 * env + 1]; }
    const bool reach = evv && sq2(ge[a] - tx, ge[E + a] - ty) <= kill;
    const int pa = __popcll(group_bits<PT>(p_on, base)), ea = __popcll(group_bits<PT>(e_on, base));
    const bool rc = group_bits<PT>(reach, base) != 0ull;
    float s = 0.f;  // the step's team reward, summed in agent order
    for (int k = 0; k < P; k++) s += __shfl(rl, base + k);
    const bool db = ev && acc.done_before[env] != 0;
    const bool ended = ev && (acc.ended[env] != 0 || ((rc || pa == 0 || ea == 0) && !db));
    if (SHAPED && pv) {
        if (!db) {
            double ph = phi[(size_t)env * P + a];
            const double x = rshape::step(m, gamma, ph, n2n_potential(gp, ge, P, E, a, p_on, coef), !p_on || ended, (double)live);
            phi[(size_t)env * P + a] = ph;
            if (SCALED) {
                double *q = rs + (size_t)env * (1 + 3 * P);
                const double n = q[0] + 1.0;
                double mean = q[1 + a], S = q[1 + P + a], R = q[1 + 2 * P + a];
                rb = (float)rscale::step(x, gamma, n, mean, S, R) * live;
                q[1 + a] = mean; q[1 + P + a] = S; q[1 + 2 * P + a] = R;
                if (a == 0) q[0] = n;
            } else {
                rb = (float)x * live;
            }
        }
        if (io.r) io.r[(int64_t)env * io.r_rs + a] = rb;
    }
    if (pv && io.v_next && (!p_on || ended)) io.v_next[(int64_t)env * io.v_next_rs + a] = 0.f;
    if (ev && a == 0) {
        acc.ended[env] = ended;
        if (ea == 0 && !db) acc.captured[env] = 1;
        if (!db) acc.length[env] += 1.f;
        acc.ret[env] += s;
        acc.done_before[env] = db || done[env] != 0;
    }
}

// ---- the reference's evader: eva.e_f (eva.py:36-80), a bounded SLSQP minimisation of obj_func over the heading ----

constexpr double N2N_E_SEN_RANGE = 3.0;  // particle_env.py:114 'e_sen_range' (not a field of n2n_config)

// obj_func (eva.py:60-80) of one evader.  q holds the predicted positions of the n pursuers in sensing range, x at q[k * qs],
// y at q[(P + k) * qs] (LDS on the device, a host array in the CPU path).
template <int PM>
struct N2nObjective {
    double ex, ey, ev, tx, ty;
    int n, P, qs;
    const double *q;
    __host__ __device__ double operator()(const double *b) const {
        const double nx = ex + ev * cos(b[0]), ny = ey + ev * sin(b[0]);
        double d[PM];
#pragma unroll
        for (int k = 0; k < PM; k++) {
            d[k] = INFINITY;
            if (k < n) {
                const double dx = nx - q[k * qs], dy = ny - q[(P + k) * qs];
                d[k] = sqrt(dx * dx + dy * dy);
            }
        }
        slsqp::sort_asc<PM>(d);
        double sdd = 0.0;
#pragma unroll
        for (int k = 0; k < PM; k++)
            if (k < n) sdd = sdd + 0.5 / d[k];
        const double dx = nx - tx, dy = ny - ty;
        return 0.5 * sqrt(dx * dx + dy * dy) + sdd;
    }
};

// e_f for evader a of one environment (records p [5][P], e [5][E]); writes q, returns the normalised heading (0 for an
// inactive evader, which the reference never calls e_f on) and the iterations taken.
template <int PM>
__host__ __device__ inline double n2n_evader_one(const n2n_config &c, const double *p, const double *e, const double *tg, int a,
                                                 double *q, int qs, int *nit) {
    const int P = c.P, E = c.E;
    *nit = 0;
    if (e[4 * E + a] == 0.0) return 0.0;
    const double ex = e[a], ey = e[E + a];
    int n = 0;
    for (int j = 0; j < P; j++) {  // the active pursuers (get_team_state rules=True) inside the evader's sensing range
        if (p[4 * P + j] == 0.0) continue;
        const double dx = ex - p[j], dy = ey - p[P + j];
        if (!(sqrt(dx * dx + dy * dy) <= N2N_E_SEN_RANGE)) continue;
        const double v = p[3 * P + n];  // p_v0[ne]: the speed of the n-th pursuer of the FULL list (eva.py:67)
        q[n * qs] = p[j] + v * cos(p[2 * P + j]);
        q[(P + n) * qs] = p[P + j] + v * sin(p[2 * P + j]);
        n++;
    }
    N2nObjective<PM> fn{ex, ey, e[3 * E + a], tg[0], tg[1], n, P, qs, q};
    double x[1] = {0.0};
    const double lb[1] = {-PI}, ub[1] = {PI};
    *nit = slsqp::minimize<1>(fn, x, lb, ub);
    return x[0] / PI;
}

// one lane per (environment, evader), one wavefront (half of one above 64 KB of LDS) per block; the lane's pursuer
// predictions live in LDS at stride blockDim.x
template <int PM>
__global__ __launch_bounds__(WAVE) void k_n2n_evader(const n2n_config c, const n2n_state st, double *e_cmd, int32_t *nit) {
    extern __shared__ double q_lds[];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= st.N * c.E) return;
    const int env = i / c.E, a = i - env * c.E;
    int it;
    const double cmd = n2n_evader_one<PM>(c, st.p + (size_t)env * 5 * c.P, st.e + (size_t)env * 5 * c.E, st.target + 2 * env, a,
                                          q_lds + threadIdx.x, (int)blockDim.x, &it);
    e_cmd[i] = cmd;
    if (nit) nit[i] = it;
}

int launch_n2n_evader(const n2n_config *c, const n2n_state *st, double *e_cmd, int32_t *nit, hipStream_t s) {
    const long long lanes = (long long)st->N * c->E;
    if (lanes == 0) return 0;
    // 2 P 64 doubles is 65536 bytes at P = N2N_MAX_P = 64, so the 32-lane shape is never taken here (env_3d's, with 3 P, is from P = 43);
    // it stays as the guard it is should N2N_MAX_P grow
    const int tpb = (size_t)2 * c->P * WAVE * sizeof(double) <= 65536 ? WAVE : WAVE / 2;
    const unsigned blocks = (unsigned)((lanes + tpb - 1) / tpb);
    const size_t lds = (size_t)2 * c->P * tpb * sizeof(double);
#define N2N_EV(PM) hipLaunchKernelGGL((k_n2n_evader<PM>), dim3(blocks), dim3(tpb), lds, s, *c, *st, e_cmd, nit)
    if (c->P <= 8) N2N_EV(8); else if (c->P <= 16) N2N_EV(16); else if (c->P <= 32) N2N_EV(32); else N2N_EV(64);
#undef N2N_EV
    return (int)hipGetLastError();
}

template <int PM>
void n2n_evader_host_pm(const n2n_config &c, int N, const double *p, const double *e, const double *tg, double *e_cmd, int32_t *nit) {
    std::vector<double> q((size_t)2 * c.P);
    for (int env = 0; env < N; env++)
        for (int a = 0; a < c.E; a++) {
            int it;
            e_cmd[(size_t)env * c.E + a] = n2n_evader_one<PM>(c, p + (size_t)env * 5 * c.P, e + (size_t)env * 5 * c.E, tg + 2 * env, a,
                                                              q.data(), 1, &it);
            if (nit) nit[(size_t)env * c.E + a] = it;
        }
}

// [N][A][5] host order -> [N][5][A] records
__global__ void k_aos_to_soa(int N, int A, const double *aos, double *soa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * A * 5) return;
    const int n = i / (5 * A), r = i - n * 5 * A, k = r / A, a = r - k * A;
    soa[i] = aos[(size_t)n * 5 * A + a * 5 + k];
}

struct N2nResetter { n2n_config cfg; int N; std::vector<rngrep::NpRandom> rng; };

// false: the placement loop drew N2N_RESET_MAX_DRAWS candidates without seating all n points; it gives up like env_3d's (the
// candidate past the bound is kept, so pts is full and the generator stream up to the bound is the reference's)
bool sample_points(rngrep::NpRandom &g, int n, double lx, double ly, double lo, double hi, std::vector<double> &pts) {
    // gen_init_p_pos / gen_init_e_pos (:239-281): normal(loc, 2, size 2).clip(lo, hi), rejected when < 2 from an earlier point
    pts.clear();
    int draws = 0;
    bool placed = true;
    while ((int)pts.size() < 2 * n) {
        double x = g.normal(lx, 2.0), y = g.normal(ly, 2.0);
        x = x < lo ? lo : (x > hi ? hi : x);
        y = y < lo ? lo : (y > hi ? hi : y);
        bool ok = true;
        if (++draws > N2N_RESET_MAX_DRAWS) placed = false;   // give up: keep this candidate, report the environment
        else for (size_t k = 0; k < pts.size() && ok; k += 2) ok = !(norm2(x - pts[k], y - pts[k + 1]) < 2.0);
        if (ok) { pts.push_back(x); pts.push_back(y); }
    }
    return placed;
}

// phi [N][P] = the shaping potential of the current records (n2n_shaping_begin): the tick's lane layout, one store per lane
template <int PT>
__global__ __launch_bounds__(WAVE * WPB) void k_n2n_shaping_begin(const n2n_config c, const n2n_state st, double *phi, const double coef) {
    constexpr int G = WAVE / PT;
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT;
    const int env = wave * G + g, P = c.P, E = c.E;
    if (env >= st.N || a >= P) return;
    const double *gp = st.p + (size_t)env * 5 * P, *ge = st.e + (size_t)env * 5 * E;
    phi[(size_t)env * P + a] = n2n_potential(gp, ge, P, E, a, gp[4 * P + a] != 0.0, coef);
}

// the scripted pursuers (include/n2n_env.h n2n_pursuer_guidance; csrc/guidance.hpp): the tick's lane layout, slot a = pursuer a and
// evader a in registers.  Every lane walks the E evaders (nearest active one, lowest index on ties) and then its P team-mates, in
// index order, through shuffles inside the group; no LDS, no atomics, one int32 store per lane.  Every lane of the wave runs both
// loops (the trip counts are wave-uniform); only the lanes of real pursuers store.
template <int PT>
__global__ __launch_bounds__(WAVE * WPB) void k_n2n_guidance(const n2n_config c, const n2n_state st, const n2n_guidance_params gp, int32_t *actions) {
    constexpr int G = WAVE / PT;
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT, base = lane - a;
    const int env = wave * G + g, P = c.P, E = c.E;
    const bool ev = env < st.N, pv = ev && a < P, evv = ev && a < E;
    const double *q = st.p + (size_t)(ev ? env : 0) * 5 * P, *ge = st.e + (size_t)(ev ? env : 0) * 5 * E;
    double px = 0, py = 0, pact = 0, ex = 0, ey = 0, ephi = 0, evel = 0, eact = 0;
    if (pv) { px = q[a]; py = q[P + a]; pact = q[4 * P + a]; }
    if (evv) { ex = ge[a]; ey = ge[E + a]; ephi = ge[2 * E + a]; evel = ge[3 * E + a]; eact = ge[4 * E + a]; }
    bool any = false;
    double rx = 0, ry = 0, d = 0, tphi = 0, tvel = 0;   // the chosen evader: r = e_pos - p_i, d = |r|, its heading and speed
    for (int k = 0; k < E; k++) {
        const double kx = __shfl(ex, base + k), ky = __shfl(ey, base + k), kp = __shfl(ephi, base + k), kv = __shfl(evel, base + k);
        const double ka = __shfl(eact, base + k);
        const double dx = kx - px, dy = ky - py, dk = rshape::dist2(dx, dy);
        if (ka != 0.0 && (!any || dk < d)) { any = true; rx = dx; ry = dy; d = dk; tphi = kp; tvel = kv; }
    }
    const double t = guide::lead_time(d, c.p_vmax, gp.lead);
    double gx, gy, gz;
    guide::unit(rx + t * (tvel * cos(tphi)), ry + t * (tvel * sin(tphi)), 0.0, gx, gy, gz);
    for (int k = 0; k < P; k++) {
        const double kx = __shfl(px, base + k), ky = __shfl(py, base + k), ka = __shfl(pact, base + k);
        const double dx = px - kx, dy = py - ky, dij = rshape::dist2(dx, dy);
        if (k != a && ka != 0.0 && guide::in_sep(dij, gp.sep_range)) {
            gx = gx + guide::repel(gp.sep_gain, dx, dij, gp.sep_range);
            gy = gy + guide::repel(gp.sep_gain, dy, dij, gp.sep_range);
        }
    }
    if (pv) actions[(size_t)env * P + a] = guide::n2n_command(pact != 0.0 && any, gx, gy);
}

// n2n_policy_record (include/policy_record.h): the checks, then one launch in the tick's lane layout; an option that is off passes the
// kernel nullptr / 0.0 whatever the record holds
template <bool SCALED, bool SHAPED, bool TEAM>
int n2n_record_launch(const n2n_config *cfg, const n2n_state *st, const float *reward, const uint8_t *done, const n2n_record_io *io,
                      const n2n_policy_acc *acc, const policy_record_opts &o, void *stream) {
    if (!cfg || !st || !reward || !done || !io || !acc || !io->live || (io->v && !io->value)) return N2N_ERR_NULL;
    if (!acc->done_before || !acc->ended || !acc->captured || !acc->ret || !acc->length) return N2N_ERR_NULL;
    const int rc = n2n_config_check(cfg);
    if (rc) return rc;
    if (TEAM && !team::coef_ok(o.alpha)) return N2N_ERR_BAD_CONFIG;
    if (st->N < 1) return 0;
    int blocks;
    const int pt = n2n_lanes(cfg, st->N, &blocks);
    const double kill = sq_threshold(cfg->kill_radius);
    double *rs = SCALED ? o.rs : nullptr, *phi = SHAPED ? o.phi : nullptr;
    const double gamma = SCALED || SHAPED ? o.gamma : 0.0, coef = SHAPED ? o.coef : 0.0, alpha = TEAM ? o.alpha : 0.0;
    hipStream_t s = (hipStream_t)stream;
#define N2N_REC(PT) hipLaunchKernelGGL((k_n2n_policy_record<PT, SCALED, SHAPED, TEAM>), dim3(blocks), dim3(WAVE * WPB), 0, s, *cfg, *st, reward, done, *io, *acc, kill, rs, gamma, phi, coef, alpha)
    if (pt == 8) N2N_REC(8); else if (pt == 16) N2N_REC(16); else if (pt == 32) N2N_REC(32); else N2N_REC(64);
#undef N2N_REC
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int n2n_config_check(const n2n_config *c) {
    if (!c) return N2N_ERR_NULL;
    if (c->P < 1 || c->P > N2N_MAX_P || c->E < 1 || c->E > N2N_MAX_E || c->episode_limit < 1) return N2N_ERR_BAD_CONFIG;
    return 0;
}

int n2n_env_load(const n2n_config *cfg, const n2n_state *st, const double *p, const double *e, const double *target, void *stream) {
    if (!cfg || !st || !p || !e || !target) return N2N_ERR_NULL;
    int rc = n2n_config_check(cfg);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t N = st->N, P = cfg->P, E = cfg->E;
    double *dp = nullptr, *de = nullptr;
    hipError_t err;
#define TRY(x) do { err = (x); if (err != hipSuccess) return (int)err; } while (0)
    TRY(hipMallocAsync((void **)&dp, N * P * 5 * sizeof(double), s));
    TRY(hipMallocAsync((void **)&de, N * E * 5 * sizeof(double), s));
    TRY(hipMemcpyAsync(dp, p, N * P * 5 * sizeof(double), hipMemcpyHostToDevice, s));
    TRY(hipMemcpyAsync(de, e, N * E * 5 * sizeof(double), hipMemcpyHostToDevice, s));
    TRY(hipMemcpyAsync(st->target, target, N * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    TRY(hipMemsetAsync(st->time_step, 0, N * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_aos_to_soa, dim3((unsigned)((N * P * 5 + 255) / 256)), dim3(256), 0, s, (int)N, (int)P, dp, st->p);
    hipLaunchKernelGGL(k_aos_to_soa, dim3((unsigned)((N * E * 5 + 255) / 256)), dim3(256), 0, s, (int)N, (int)E, de, st->e);
    TRY(hipFreeAsync(dp, s));
    TRY(hipFreeAsync(de, s));
#undef TRY
    return (int)hipGetLastError();
}

int n2n_env_observe(const n2n_config *cfg, const n2n_state *st, const n2n_obs_out *out, void *stream) {
    if (!cfg || !st || !out) return N2N_ERR_NULL;
    return launch_n2n<false>(cfg, st, nullptr, nullptr, nullptr, nullptr, nullptr, *out, (hipStream_t)stream);
}

int n2n_env_tick(const n2n_config *cfg, const n2n_state *st, const int32_t *actions, const double *e_cmd, float *reward, uint8_t *active,
                 uint8_t *done, const n2n_obs_out *out, void *stream) {
    if (!cfg || !st || !actions || !e_cmd || !reward || !active || !done) return N2N_ERR_NULL;
    n2n_obs_out o0;
    memset(&o0, 0, sizeof o0);
    return launch_n2n<true>(cfg, st, actions, e_cmd, reward, active, done, out ? *out : o0, (hipStream_t)stream);
}

int n2n_evader_slsqp(const n2n_config *cfg, const n2n_state *st, double *e_cmd, void *stream) {
    return n2n_evader_slsqp_nit(cfg, st, e_cmd, nullptr, stream);
}

int n2n_evader_slsqp_nit(const n2n_config *cfg, const n2n_state *st, double *e_cmd, int32_t *nit, void *stream) {
    if (!cfg || !st || !e_cmd) return N2N_ERR_NULL;
    const int rc = n2n_config_check(cfg);
    if (rc) return rc;
    return launch_n2n_evader(cfg, st, e_cmd, nit, (hipStream_t)stream);
}

int n2n_evader_slsqp_host(const n2n_config *cfg, int32_t N, const double *p, const double *e, const double *target, double *e_cmd,
                          int32_t *nit) {
    if (!cfg || !p || !e || !target || !e_cmd) return N2N_ERR_NULL;
    const int rc = n2n_config_check(cfg);
    if (rc) return rc;
    if (cfg->P <= 8) n2n_evader_host_pm<8>(*cfg, N, p, e, target, e_cmd, nit);
    else if (cfg->P <= 16) n2n_evader_host_pm<16>(*cfg, N, p, e, target, e_cmd, nit);
    else if (cfg->P <= 32) n2n_evader_host_pm<32>(*cfg, N, p, e, target, e_cmd, nit);
    else n2n_evader_host_pm<64>(*cfg, N, p, e, target, e_cmd, nit);
    return 0;
}

int n2n_policy_inputs(const n2n_config *cfg, const n2n_state *st, const uint8_t *done_before, const n2n_policy_io *io, void *stream) {
    if (!cfg || !st || !io || (io->pp_adj && !io->pp_in) || (io->pe_adj && !io->pe_in)) return N2N_ERR_NULL;
    const int rc = n2n_config_check(cfg);
    if (rc) return rc;
    if (st->N < 1) return 0;
    int blocks;
    const int pt = n2n_lanes(cfg, st->N, &blocks);
    hipStream_t s = (hipStream_t)stream;
#define N2N_IN(PT) hipLaunchKernelGGL((k_n2n_policy_inputs<PT>), dim3(blocks), dim3(WAVE * WPB), 0, s, *cfg, *st, done_before, *io)
    if (pt == 8) N2N_IN(8); else if (pt == 16) N2N_IN(16); else if (pt == 32) N2N_IN(32); else N2N_IN(64);
#undef N2N_IN
    return (int)hipGetLastError();
}

int n2n_policy_record(const n2n_config *cfg, const n2n_state *st, const float *reward, const uint8_t *done, const n2n_record_io *io,
                      const n2n_policy_acc *acc, const policy_record_opts *opts, void *stream) {
    const policy_record_opts off = {};
    const policy_record_opts &o = opts ? *opts : off;
    // <SCALED, SHAPED, TEAM>; the cases stand in the order in which the code object has always listed these kernels
    switch ((o.rs ? 1 : 0) | (o.phi ? 2 : 0) | (o.team ? 4 : 0)) {
        case 0: return n2n_record_launch<false, false, false>(cfg, st, reward, done, io, acc, o, stream);
        case 1: return n2n_record_launch<true, false, false>(cfg, st, reward, done, io, acc, o, stream);
        case 3: return n2n_record_launch<true, true, false>(cfg, st, reward, done, io, acc, o, stream);
        case 2: return n2n_record_launch<false, true, false>(cfg, st, reward, done, io, acc, o, stream);
        case 7: return n2n_record_launch<true, true, true>(cfg, st, reward, done, io, acc, o, stream);
        case 6: return n2n_record_launch<false, true, true>(cfg, st, reward, done, io, acc, o, stream);
        case 5: return n2n_record_launch<true, false, true>(cfg, st, reward, done, io, acc, o, stream);
        default: return n2n_record_launch<false, false, true>(cfg, st, reward, done, io, acc, o, stream);
    }
}

int n2n_shaping_begin(const n2n_config *cfg, const n2n_state *st, double *phi, double coef, void *stream) {
    if (!cfg || !st || !phi) return N2N_ERR_NULL;
    const int rc = n2n_config_check(cfg);
    if (rc) return rc;
    if (st->N < 1) return 0;
    int blocks;
    const int pt = n2n_lanes(cfg, st->N, &blocks);
    hipStream_t s = (hipStream_t)stream;
#define N2N_SB(PT) hipLaunchKernelGGL((k_n2n_shaping_begin<PT>), dim3(blocks), dim3(WAVE * WPB), 0, s, *cfg, *st, phi, coef)
    if (pt == 8) N2N_SB(8); else if (pt == 16) N2N_SB(16); else if (pt == 32) N2N_SB(32); else N2N_SB(64);
#undef N2N_SB
    return (int)hipGetLastError();
}

int n2n_pursuer_guidance(const n2n_config *cfg, const n2n_state *st, const n2n_guidance_params *params, int32_t *actions, void *stream) {
    if (!cfg || !st || !params || !actions) return N2N_ERR_NULL;
    const int rc = n2n_config_check(cfg);
    if (rc) return rc;
    if (!guide::param_ok(params->lead) || !guide::param_ok(params->sep_range) || !guide::param_ok(params->sep_gain)) return N2N_ERR_BAD_CONFIG;
    if (st->N < 1) return 0;
    if (!st->p || !st->e) return N2N_ERR_NULL;
    int blocks;
    const int pt = n2n_lanes(cfg, st->N, &blocks);
    hipStream_t s = (hipStream_t)stream;
#define N2N_GD(PT) hipLaunchKernelGGL((k_n2n_guidance<PT>), dim3(blocks), dim3(WAVE * WPB), 0, s, *cfg, *st, *params, actions)
    if (pt == 8) N2N_GD(8); else if (pt == 16) N2N_GD(16); else if (pt == 32) N2N_GD(32); else N2N_GD(64);
#undef N2N_GD
    return (int)hipGetLastError();
}

void *n2n_resetter_create(const n2n_config *cfg, int32_t N, const uint32_t *seeds) {
    if (!cfg || !seeds || N < 1 || n2n_config_check(cfg)) return nullptr;
    N2nResetter *R = new N2nResetter();
    R->cfg = *cfg;
    R->N = N;
    R->rng.resize(N);
    for (int n = 0; n < N; n++) R->rng[n].seed(seeds[n]);
    return R;
}

void n2n_resetter_destroy(void *h) { delete (N2nResetter *)h; }

// Resume support: every environment's generator (rng_replica.hpp ResetterStateHeader, then one NpRandom record each).
static rngrep::ResetterStateHeader n2n_state_header(const N2nResetter &R) {
    return rngrep::ResetterStateHeader{N2N_RESETTER_STATE_TAG, R.N, R.cfg.P, R.cfg.E};
}

int64_t n2n_resetter_state_bytes(void *h) { return h ? rngrep::resetter_state_bytes(((N2nResetter *)h)->N) : 0; }

int n2n_resetter_get_state(void *h, void *out) {
    if (!h || !out) return N2N_ERR_NULL;
    N2nResetter &R = *(N2nResetter *)h;
    rngrep::resetter_state_get(n2n_state_header(R), R.rng.data(), out);
    return 0;
}

int n2n_resetter_set_state(void *h, const void *in) {
    if (!h || !in) return N2N_ERR_NULL;
    N2nResetter &R = *(N2nResetter *)h;
    return rngrep::resetter_state_set(n2n_state_header(R), R.rng.data(), in) ? 0 : N2N_ERR_BAD_STATE;
}

int n2n_resetter_reset(void *h, double *p, double *e, double *target, int32_t n_threads) {
    if (!h || !p || !e || !target) return N2N_ERR_NULL;
    N2nResetter &R = *(N2nResetter *)h;
    const int P = R.cfg.P, E = R.cfg.E;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > R.N) n_threads = R.N;
    std::vector<int> failed(n_threads, 0);
    auto work = [&](int t) {
        std::vector<double> pts;
        for (int n = t; n < R.N; n += n_threads) {
            rngrep::NpRandom &g = R.rng[n];
            const double tx = g.random_sample() * 20, ty = g.random_sample() * 20;  // reset (:200-204)
            target[2 * n] = tx; target[2 * n + 1] = ty;
            if (!sample_points(g, P, 0.0, 0.0, -8.0, 8.0, pts)) failed[t] = 1;
            for (int i = 0; i < P; i++) {
                double *s = p + ((size_t)n * P + i) * 5;
                s[0] = pts[2 * i] + 10; s[1] = pts[2 * i + 1] + 10; s[2] = PI / 4; s[3] = 0.0; s[4] = 1.0;
            }
            if (!sample_points(g, E, 20 - tx, 20 - ty, 0.0, 20.0, pts)) failed[t] = 1;
            for (int i = 0; i < E; i++) {
                double *s = e + ((size_t)n * E + i) * 5;
                s[0] = pts[2 * i]; s[1] = pts[2 * i + 1]; s[2] = PI / 4; s[3] = R.cfg.e_vmax; s[4] = 1.0;
            }
        }
    };
    if (n_threads == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < n_threads; t++) th.emplace_back(work, t);
        for (auto &x : th) x.join();
    }
    for (int t = 0; t < n_threads; t++)
        if (failed[t]) return N2N_ERR_RESET_FAILED;
    return 0;
}

}  // extern "C"
