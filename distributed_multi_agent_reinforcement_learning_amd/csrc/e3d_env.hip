// e3d_env.hip -- batched env_3d (continuous 3-D pursuit, continuous actions) for MI355X (gfx950).  C ABI: include/e3d_env.h.
//
// The environment is tiny (7 (P + 1) + 3 doubles), so a wavefront per environment would leave 56 of 64 lanes idle and the
// launch bound by per-wave latency (that is where the env_n2n kernel sits: 9 % of HBM).  Here lane = (environment, pursuer):
// a group of PT = 8 / 16 / 32 / 64 lanes owns one environment (8 environments per wave for P <= 8), four waves per
// workgroup.  Every lane keeps its pursuer in registers; the evader (one per environment) is replicated in the group's lanes
// and advanced redundantly, so nothing about it needs an exchange; the pairwise kill-radius / range tests read the other
// pursuers through wave shuffles inside the group.  f64 state like the reference; headings go through the device cos/sin
// (agreement with the reference's libm: <= 1e-9 on positions over an episode, see tests).  Build with -ffp-contract=off;
// the only fused multiply-adds are the explicit ones in norm3 (how numpy evaluates the norm of a 3-vector).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "central_critic.hpp"
#include "direction_action.hpp"
#include "e3d_env.h"
#include "guidance.hpp"
#include "obs_norm.hpp"
#include "pursuit_features.hpp"
#include "reward_scale.hpp"
#include "reward_shaping.hpp"
#include "rng_replica.hpp"
#include "slsqp_box.hpp"
#include "team_reward.hpp"

namespace {

constexpr int WAVE = 64, WPB = 4;
constexpr double PI = 3.14159265358979323846;

__host__ __device__ inline double norm3(double a, double b, double c) { return sqrt(fma(c, c, fma(b, b, a * a))); }
// `norm3(..) <= r` without the square root (sqrt is correctly rounded and monotonic): the squared norm -- the same fma chain the
// norm takes the root of -- against the largest double t with sqrt(t) <= r, computed once per launch on the host.
// Held by tests/test_particle_config_gpu.py on states whose squared distance is t itself, one double above it, or on the other
// side of it than the unfused sum (tests/particle_config_cases.py): t is not fl(r r) for r = 0.5, the default kill radius.
__device__ __forceinline__ double sq3(double a, double b, double c) { return fma(c, c, fma(b, b, a * a)); }
double sq_threshold(double r) {
    auto ok = [&](double t) { return sqrt(t) <= r; };
    if (!(r >= 0.0) || !ok(0.0)) return -1.0;
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
struct E3dThr { double kill, comm, sen; };
__device__ __forceinline__ double sgn(double v) { return (double)((v > 0) - (v < 0)); }
__device__ __forceinline__ double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct Agent { double x, y, z, phi, gamma, v, act; };

// particle_env.py:25-55 Point.step
__device__ __forceinline__ void point_step(Agent &s, double a0, double a1, double a2, double v_max, double ang, double vlmt, double h) {
    if (s.act == 0.0) return;
    const double phi = a0 * PI, gamma = a1 * PI / 2, v = (a2 + 1) / 2 * v_max;
    s.gamma += clip(gamma - s.gamma, -ang, ang);
    s.v += clip(v - s.v, -vlmt, vlmt);
    const double d = phi - s.phi, ad = fabs(d);
    double dphi;
    if (sgn(phi * s.phi) >= 0) dphi = clip(d, -ang, ang);
    else if (ad < 2 * PI - ad) dphi = clip(d, -ang, ang);
    else dphi = clip(2 * PI - ad, 0, ang) * -sgn(d);
    s.phi += dphi;
    if (s.phi > PI) s.phi -= 2 * PI; else if (s.phi < -PI) s.phi += 2 * PI;
    s.x += s.v * cos(s.gamma) * cos(phi) * h;
    s.y += s.v * cos(s.gamma) * sin(phi) * h;
    s.z += s.v * sin(s.gamma) * h;
}

template <int PT, bool TICK>
__global__ __launch_bounds__(WAVE * WPB) void k_e3d(const e3d_config c, const e3d_state st, const double *actions, const double *e_cmd, float *reward,
                                                    uint8_t *active, uint8_t *done, const e3d_obs_out o, const E3dThr th) {
    constexpr int G = WAVE / PT;  // environments per wavefront
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT, base = lane - a;  // base: first lane of this lane's group
    const int env = wave * G + g, P = c.P;
    const bool ev = env < st.N, pv = ev && a < P;
    Agent s = {0, 0, 0, 0, 0, 0, 0}, e = {0, 0, 0, 0, 0, 0, 0};
    double tx = 0, ty = 0, tz = 0;
    if (pv) {
        const double *gp = st.p + (size_t)env * 7 * P + a;
        s.x = gp[0]; s.y = gp[P]; s.z = gp[2 * P]; s.phi = gp[3 * P]; s.gamma = gp[4 * P]; s.v = gp[5 * P]; s.act = gp[6 * P];
    }
    if (ev) {
        const double *ge = st.e + (size_t)env * 7;
        e.x = ge[0]; e.y = ge[1]; e.z = ge[2]; e.phi = ge[3]; e.gamma = ge[4]; e.v = ge[5]; e.act = ge[6];
    }
    if (TICK) {
        if (ev) { tx = st.target[3 * env]; ty = st.target[3 * env + 1]; tz = st.target[3 * env + 2]; }
        // evader_step (:354-378): the SLSQP command moves the evader; the reference's driver calls it with the ACTIVE pursuers
        // and cannot when none is left.  Every lane of the group advances its own copy of the evader.
        const bool any_p = (__ballot(pv && s.act != 0.0) >> base) & ((PT == 64) ? ~0ull : ((1ull << PT) - 1ull));
        if (ev && any_p && e.act != 0.0) {
            const double *cm = e_cmd + (size_t)env * 3;
            point_step(e, cm[0], cm[1], cm[2], c.e_vmax, c.ang_lmt, c.v_lmt, c.step_size);
        }
        if (pv) {
            const double *ac = actions + ((size_t)env * P + a) * 3;
            point_step(s, ac[0], ac[1], ac[2], c.p_vmax, c.ang_lmt, c.v_lmt, c.step_size);
        }
        // reward (:267-284) and update_agent_active (:286-326) are both evaluated on the moved, not yet culled state
        int cp = 0;
        for (int k = 0; k < P; k++) {  // wave-uniform trip count; partners through shuffles inside the group
            const double kx = __shfl(s.x, base + k), ky = __shfl(s.y, base + k), kz = __shfl(s.z, base + k), ka = __shfl(s.act, base + k);
            cp += ka != 0.0 && sq3(s.x - kx, s.y - ky, s.z - kz) <= th.kill;
        }
        const bool me = pv && s.act != 0.0;
        const int ce = me && e.act != 0.0 && sq3(s.x - e.x, s.y - e.y, s.z - e.z) <= th.kill;
        const bool e_hit = me && e.act != 0.0 && sq3(e.x - s.x, e.y - s.y, e.z - s.z) <= th.kill;
        const bool pdie = me && (cp + ce - 1) != 0;
        const bool edie = ((__ballot(e_hit) >> base) & ((PT == 64) ? ~0ull : ((1ull << PT) - 1ull))) != 0ull;
        if (pv) reward[(size_t)env * P + a] = me ? (float)(ce - (cp - 1)) : 0.f;
        if (pdie) { s.x = s.y = s.z = 1000; s.phi = s.gamma = s.v = 0; s.act = 0; }
        if (edie) { e.x = e.y = e.z = 1000; e.phi = e.gamma = e.v = 0; e.act = 0; }
        const bool pact = pv && s.act != 0.0;
        const int pa = __popcll((__ballot(pact) >> base) & ((PT == 64) ? ~0ull : ((1ull << PT) - 1ull)));
        if (pv) {
            active[(size_t)env * P + a] = pact;
            double *gp = st.p + (size_t)env * 7 * P + a;
            gp[0] = s.x; gp[P] = s.y; gp[2 * P] = s.z; gp[3 * P] = s.phi; gp[4 * P] = s.gamma; gp[5 * P] = s.v; gp[6 * P] = s.act;
        }
        if (ev && a == 0) {
            double *ge = st.e + (size_t)env * 7;
            ge[0] = e.x; ge[1] = e.y; ge[2] = e.z; ge[3] = e.phi; ge[4] = e.gamma; ge[5] = e.v; ge[6] = e.act;
            const int t = st.time_step[env] + 1;
            st.time_step[env] = t;
            const bool reach = sq3(e.x - tx, e.y - ty, e.z - tz) <= th.kill;   // get_done (:221-241)
            done[env] = (uint8_t)(reach || pa == 0 || e.act == 0.0 || t >= c.max_step);
        }
    }
    // observations (get_team_state rules=False :247-265, get_adj_mat :328-340: rows of inactive pursuers are zero)
    if (o.p_state && pv) {
        float *d = o.p_state + (int64_t)env * o.p_state_stride + a * 6;
        d[0] = (float)s.x; d[1] = (float)s.y; d[2] = (float)s.z; d[3] = (float)s.phi; d[4] = (float)s.gamma; d[5] = (float)s.v;
    }
    if (o.e_state && ev && a == 0) {
        float *d = o.e_state + (int64_t)env * o.e_state_stride;
        d[0] = (float)e.x; d[1] = (float)e.y; d[2] = (float)e.z; d[3] = (float)e.phi; d[4] = (float)e.gamma; d[5] = (float)e.v;
    }
    if (o.pp_adj) {
        for (int k = 0; k < P; k++) {  // row k, column a: the lanes of a group store consecutive floats
            const double kx = __shfl(s.x, base + k), ky = __shfl(s.y, base + k), kz = __shfl(s.z, base + k), ka = __shfl(s.act, base + k);
            if (pv) o.pp_adj[(int64_t)env * o.pp_adj_stride + k * P + a] = (ka != 0.0 && sq3(kx - s.x, ky - s.y, kz - s.z) <= th.comm) ? 1.f : 0.f;
        }
    }
    if (o.pe_adj && pv)
        o.pe_adj[(int64_t)env * o.pe_adj_stride + a] = (s.act != 0.0 && sq3(s.x - e.x, s.y - e.y, s.z - e.z) <= th.sen) ? 1.f : 0.f;
}

// ---- the reference's evader: eva.e_f (eva.py:87-148), a bounded SLSQP minimisation of obj_func (:212-240) ----

constexpr double E3D_E_SEN_RANGE = 3.0;  // particle_env.py:86 'e_sen_range' (not a field of e3d_config)
// obj_func's own Point (eva.py:214-227): ang_lmt pi/4, v_lmt 0.4 and step_size 0.5 are literals there, not the environment's
constexpr double OBJ_ANG_LMT = PI / 4, OBJ_V_LMT = 0.4, OBJ_STEP = 0.5;

// obj_func of one evader.  q holds the predicted positions of the n pursuers in sensing range: x at q[k * qs], y at
// q[(P + k) * qs], z at q[(2P + k) * qs] (LDS on the device, a host array in the CPU path).
template <int PM>
struct E3dObjective {
    double ex, ey, ez, egamma, ev, v_max, tx, ty, tz, kill;
    int n, P, qs;
    const double *q;
    __host__ __device__ double operator()(const double *a) const {
        // Point.step (eva.py:51-84) with the objective's constants: the position moves along the COMMANDED heading phi
        const double phi = a[0] * PI, gamma = a[1] * PI / 2, v = (a[2] + 1) / 2 * v_max;
        const double g = egamma + slsqp::clampd(gamma - egamma, -OBJ_ANG_LMT, OBJ_ANG_LMT);
        const double vv = ev + slsqp::clampd(v - ev, -OBJ_V_LMT, OBJ_V_LMT);
        const double nx = ex + vv * cos(g) * cos(phi) * OBJ_STEP, ny = ey + vv * cos(g) * sin(phi) * OBJ_STEP;
        const double nz = ez + vv * sin(g) * OBJ_STEP;
        double d[PM];
#pragma unroll
        for (int k = 0; k < PM; k++) {
            d[k] = INFINITY;
            if (k < n) {
                const double dx = nx - q[k * qs], dy = ny - q[(P + k) * qs], dz = nz - q[(2 * P + k) * qs];
                d[k] = sqrt(dx * dx + dy * dy + dz * dz);
            }
        }
        slsqp::sort_asc<PM>(d);
        double sdd = 0.0;
#pragma unroll
        for (int k = 0; k < PM; k++)
            if (k < n) sdd = sdd + 1.0 / pow(d[k] / kill, 5.0);
        const double dx = nx - tx, dy = ny - ty, dz = nz - tz;
        return 1.0 * sqrt(dx * dx + dy * dy + dz * dz) + sdd;
    }
};

// e_f for the evader of one environment (records p [7][P], e [7]): cmd [3] in [-1, 1]; zeros when the evader is inactive
// or no pursuer is active (evader_step is not called then, see the tick).  Returns the iterations taken.
template <int PM>
__host__ __device__ inline int e3d_evader_one(const e3d_config &c, const double *p, const double *e, const double *tg, double *q, int qs,
                                              double *cmd) {
    const int P = c.P;
    cmd[0] = cmd[1] = cmd[2] = 0.0;
    if (e[6] == 0.0) return 0;
    const double ex = e[0], ey = e[1], ez = e[2], ephi = e[3], egam = e[4], ev = e[5];
    int n = 0, alive = 0;
    for (int j = 0; j < P; j++) {  // the active pursuers (get_team_state rules=True) inside the evader's sensing range
        if (p[6 * P + j] == 0.0) continue;
        alive++;
        const double dx = ex - p[j], dy = ey - p[P + j], dz = ez - p[2 * P + j];
        if (!(sqrt(dx * dx + dy * dy + dz * dz) <= E3D_E_SEN_RANGE)) continue;
        const double nphi = p[3 * P + j], ngam = p[4 * P + j], nv = p[5 * P + j];
        q[n * qs] = p[j] + nv * cos(nphi) * cos(ngam) * c.step_size;
        q[(P + n) * qs] = p[P + j] + nv * sin(nphi) * cos(ngam) * c.step_size;
        q[(2 * P + n) * qs] = p[2 * P + j] + nv * sin(ngam) * c.step_size;
        n++;
    }
    if (alive == 0) return 0;
    E3dObjective<PM> fn{ex, ey, ez, egam, ev, c.e_vmax, tg[0], tg[1], tg[2], c.kill_radius, n, P, qs, q};
    // bounds from the environment's rate limits (eva.py:130-135), start at the current state (:137-139)
    const double lb[3] = {slsqp::clampd((ephi - c.ang_lmt) / PI, -1, 1), slsqp::clampd((egam - c.ang_lmt) / (PI / 2), -1, 1),
                          slsqp::clampd((ev - c.v_lmt) * 2 - 1, -1, 1)};
    const double ub[3] = {slsqp::clampd((ephi + c.ang_lmt) / PI, -1, 1), slsqp::clampd((egam + c.ang_lmt) / (PI / 2), -1, 1),
                          slsqp::clampd((ev + c.v_lmt) * 2 - 1, -1, 1)};
    double x[3] = {ephi / PI, egam / (PI / 2), ev * 2 - 1};
    const int it = slsqp::minimize<3>(fn, x, lb, ub);
    cmd[0] = x[0]; cmd[1] = x[1]; cmd[2] = x[2];
    return it;
}

// one lane per environment, one wavefront (half of one above 64 KB of LDS) per block; the lane's pursuer predictions
// live in LDS at stride blockDim.x
template <int PM>
__global__ __launch_bounds__(WAVE) void k_e3d_evader(const e3d_config c, const e3d_state st, double *e_cmd, int32_t *nit) {
    extern __shared__ double q_lds[];
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= st.N) return;
    double cmd[3];
    const int it = e3d_evader_one<PM>(c, st.p + (size_t)env * 7 * c.P, st.e + (size_t)env * 7, st.target + 3 * env, q_lds + threadIdx.x,
                                      (int)blockDim.x, cmd);
    e_cmd[3 * env] = cmd[0]; e_cmd[3 * env + 1] = cmd[1]; e_cmd[3 * env + 2] = cmd[2];
    if (nit) nit[env] = it;
}

int launch_e3d_evader(const e3d_config *c, const e3d_state *st, double *e_cmd, int32_t *nit, hipStream_t s) {
    if (st->N == 0) return 0;
    const int tpb = (size_t)3 * c->P * WAVE * sizeof(double) <= 65536 ? WAVE : WAVE / 2;
    const unsigned blocks = (unsigned)((st->N + tpb - 1) / tpb);
    const size_t lds = (size_t)3 * c->P * tpb * sizeof(double);
#define E3D_EV(PM) hipLaunchKernelGGL((k_e3d_evader<PM>), dim3(blocks), dim3(tpb), lds, s, *c, *st, e_cmd, nit)
    if (c->P <= 8) E3D_EV(8); else if (c->P <= 16) E3D_EV(16); else if (c->P <= 32) E3D_EV(32); else E3D_EV(64);
#undef E3D_EV
    return (int)hipGetLastError();
}

template <int PM>
void e3d_evader_host_pm(const e3d_config &c, int N, const double *p, const double *e, const double *tg, double *e_cmd, int32_t *nit) {
    std::vector<double> q((size_t)3 * c.P);
    for (int env = 0; env < N; env++) {
        const int it = e3d_evader_one<PM>(c, p + (size_t)env * 7 * c.P, e + (size_t)env * 7, tg + 3 * env, q.data(), 1, e_cmd + 3 * env);
        if (nit) nit[env] = it;
    }
}

// [N][P][7] host order -> [N][7][P] records
__global__ void k_aos_to_soa7(int N, int A, const double *aos, double *soa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * A * 7) return;
    const int n = i / (7 * A), r = i - n * 7 * A, k = r / A, a = r - k * A;
    soa[i] = aos[(size_t)n * 7 * A + a * 7 + k];
}

// the lane layout of the tick and of the policy kernels: PT (group of lanes per environment) and the workgroups covering N environments
int e3d_lanes(const e3d_config *c, int N, int *blocks) {
    const int pt = c->P <= 8 ? 8 : (c->P <= 16 ? 16 : (c->P <= 32 ? 32 : 64));
    const int envs_per_block = (WAVE / pt) * WPB;
    *blocks = (N + envs_per_block - 1) / envs_per_block;
    return pt;
}

template <bool TICK>
int launch(const e3d_config *c, const e3d_state *st, const double *actions, const double *e_cmd, float *reward, uint8_t *active, uint8_t *done,
           const e3d_obs_out &o, hipStream_t s) {
    int blocks;
    const int pt = e3d_lanes(c, st->N, &blocks);
    const E3dThr th{sq_threshold(c->kill_radius), sq_threshold(c->p_comm_range), sq_threshold(c->p_sen_range)};
#define E3D_GO(PT) hipLaunchKernelGGL((k_e3d<PT, TICK>), dim3(blocks), dim3(WAVE * WPB), 0, s, *c, *st, actions, e_cmd, reward, active, done, o, th)
    if (pt == 8) E3D_GO(8); else if (pt == 16) E3D_GO(16); else if (pt == 32) E3D_GO(32); else E3D_GO(64);
#undef E3D_GO
    return (int)hipGetLastError();
}

// policy features of the trainer (include/e3d_env.h e3d_policy_features): one thread per (environment, pursuer), differences and
// means in f64 on the records, stored as fp32.  The actor sees its sensed evader and its communication neighbours (the observation's
// adjacencies), the critic the whole state.
constexpr int E3D_FEAT = 16;
__global__ __launch_bounds__(256) void k_e3d_features(const e3d_config c, const e3d_state st, const e3d_obs_out o, float *af, float *cf) {
    const int P = c.P;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)st.N * P) return;
    const int env = (int)(idx / P), i = (int)(idx - (int64_t)env * P);
    const double *gp = st.p + (size_t)env * 7 * P, *ge = st.e + (size_t)env * 7;
    float *fa = af + idx * E3D_FEAT, *fc = cf + idx * E3D_FEAT;
    if (gp[6 * P + i] == 0.0) {
        for (int k = 0; k < E3D_FEAT; k++) fa[k] = fc[k] = 0.f;
        return;
    }
    double s[6];
    for (int k = 0; k < 6; k++) s[k] = gp[k * P + i];
    const double pe = (double)o.pe_adj[(int64_t)env * o.pe_adj_stride + i], ae = ge[6];
    const float *pp = o.pp_adj + (int64_t)env * o.pp_adj_stride + (int64_t)i * P;
    double ma[3] = {0, 0, 0}, mc[3] = {0, 0, 0};
    int na = 0, nc = 0;
    for (int j = 0; j < P; j++) {
        if (j == i) continue;
        const bool in_a = pp[j] == 1.f, in_c = gp[6 * P + j] != 0.0;
        if (!in_a && !in_c) continue;
        const double dx = gp[j] - s[0], dy = gp[P + j] - s[1], dz = gp[2 * P + j] - s[2];
        if (in_a) { ma[0] += dx; ma[1] += dy; ma[2] += dz; na++; }
        if (in_c) { mc[0] += dx; mc[1] += dy; mc[2] += dz; nc++; }
    }
    for (int k = 0; k < 6; k++) {
        fa[k] = fc[k] = (float)s[k];
        fa[6 + k] = (float)((ge[k] - s[k]) * pe);
        fc[6 + k] = (float)((ge[k] - s[k]) * ae);
    }
    fa[12] = (float)pe;
    fc[12] = (float)ae;
    for (int k = 0; k < 3; k++) {
        fa[13 + k] = na ? (float)(ma[k] / na) : 0.f;
        fc[13 + k] = nc ? (float)(mc[k] / nc) : 0.f;
    }
}

// ---- algo.use_obs_norm (csrc/obs_norm.hpp; include/e3d_env.h e3d_policy_features_norm) ----
//
// k_e3d_features with the running mean / std normalisation applied to what it stores, and, with ACC, the statistics of the raw
// features of the live rows added to this workgroup's slot.  k_e3d_features itself stays the code it was (the option-off path runs
// it unchanged); the feature expressions below are its expressions in its order, and with n == 0 the outputs are its bits.
//   * threads 0-31 turn the state into mean and std + eps per (network, column) in LDS once per workgroup, so a row does 32
//     subtractions and divisions and no square root;
//   * a row keeps its 2 x 16 fp32 features in registers, stores them normalised as 16-byte lanes;
//   * ACC: the raw features go through LDS transposed -- column k at k * (TPB + 1), so the row-wise stores and the column-wise loads
//     are both free of bank conflicts -- and thread (segment s = t / 32, column k = t % 32) adds d and d d of rows 32 s .. 32 s + 31
//     in row order, then thread k adds the 8 segments in order: a fixed tree, f64, no atomics.  The slot belongs to this workgroup
//     alone and is added to once per launch, so its contents are a sum in tick order.
constexpr int E3D_FN_TPB = 256, E3D_FN_SEG = E3D_FN_TPB / 32, E3D_FN_K = 2 * E3D_FEAT;
constexpr int E3D_SLOT = 2 * obsnorm::ROW;   // f64 per slot: (network, [c, S1[16], S2[16]])

template <bool ACC>
__global__ __launch_bounds__(E3D_FN_TPB) void k_e3d_features_norm(const e3d_config c, const e3d_state st, const e3d_obs_out o, float *af, float *cf,
                                                                   const double *state, const double clipv, const float *live,
                                                                   const int64_t live_rs, double *slots) {
    __shared__ double s_mean[E3D_FN_K], s_den[E3D_FN_K], s_n[2];
    __shared__ float s_x[ACC ? E3D_FN_K * (E3D_FN_TPB + 1) : 1];
    __shared__ float s_live[ACC ? E3D_FN_TPB : 1];
    __shared__ double s_part[ACC ? E3D_FN_SEG * 3 * E3D_FN_K : 1];
    const int P = c.P, t = threadIdx.x;
    if (t < E3D_FN_K) {
        const double *row = state + (t >> 4) * obsnorm::ROW;
        const double n = row[0];
        s_mean[t] = row[1 + (t & 15)];
        s_den[t] = n == 0.0 ? 1.0 : obsnorm::denom(n, row[1 + E3D_FEAT + (t & 15)]);
        if ((t & 15) == 0) s_n[t >> 4] = n;
    }
    const int64_t idx = (int64_t)blockIdx.x * E3D_FN_TPB + t;
    const bool valid = idx < (int64_t)st.N * P;
    float f[E3D_FN_K];   // the raw features: 0-15 the actor's, 16-31 the critic's
#pragma unroll
    for (int k = 0; k < E3D_FN_K; k++) f[k] = 0.f;
    bool on = false, counted = false;
    if (valid) {
        const int env = (int)(idx / P), i = (int)(idx - (int64_t)env * P);
        const double *gp = st.p + (size_t)env * 7 * P, *ge = st.e + (size_t)env * 7;
        on = gp[6 * P + i] != 0.0;
        if (on) {
            double s[6];
#pragma unroll
            for (int k = 0; k < 6; k++) s[k] = gp[k * P + i];
            const double pe = (double)o.pe_adj[(int64_t)env * o.pe_adj_stride + i], ae = ge[6];
            const float *pp = o.pp_adj + (int64_t)env * o.pp_adj_stride + (int64_t)i * P;
            double ma[3] = {0, 0, 0}, mc[3] = {0, 0, 0};
            int na = 0, nc = 0;
            for (int j = 0; j < P; j++) {
                if (j == i) continue;
                const bool in_a = pp[j] == 1.f, in_c = gp[6 * P + j] != 0.0;
                if (!in_a && !in_c) continue;
                const double dx = gp[j] - s[0], dy = gp[P + j] - s[1], dz = gp[2 * P + j] - s[2];
                if (in_a) { ma[0] += dx; ma[1] += dy; ma[2] += dz; na++; }
                if (in_c) { mc[0] += dx; mc[1] += dy; mc[2] += dz; nc++; }
            }
#pragma unroll
            for (int k = 0; k < 6; k++) {
                f[k] = f[E3D_FEAT + k] = (float)s[k];
                f[6 + k] = (float)((ge[k] - s[k]) * pe);
                f[E3D_FEAT + 6 + k] = (float)((ge[k] - s[k]) * ae);
            }
            f[12] = (float)pe;
            f[E3D_FEAT + 12] = (float)ae;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                f[13 + k] = na ? (float)(ma[k] / na) : 0.f;
                f[E3D_FEAT + 13 + k] = nc ? (float)(mc[k] / nc) : 0.f;
            }
            if (ACC) counted = live[(int64_t)env * live_rs + i] != 0.f;
        }
    }
    __syncthreads();   // s_mean, s_den, s_n
    if (valid) {
        float y[E3D_FN_K];
#pragma unroll
        for (int k = 0; k < E3D_FN_K; k++)   // rows of inactive pursuers stay exactly 0: no -mean / std there
            y[k] = (!on || s_n[k >> 4] == 0.0) ? f[k] : obsnorm::apply(f[k], s_mean[k], s_den[k], clipv);
        float4 *da = reinterpret_cast<float4 *>(af + idx * E3D_FEAT), *dc = reinterpret_cast<float4 *>(cf + idx * E3D_FEAT);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            da[q] = make_float4(y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]);
            dc[q] = make_float4(y[E3D_FEAT + 4 * q], y[E3D_FEAT + 4 * q + 1], y[E3D_FEAT + 4 * q + 2], y[E3D_FEAT + 4 * q + 3]);
        }
    }
    if (ACC) {
        s_live[t] = counted ? 1.f : 0.f;
#pragma unroll
        for (int k = 0; k < E3D_FN_K; k++) s_x[k * (E3D_FN_TPB + 1) + t] = f[k];
        __syncthreads();
        const int k = t & 31, seg = t >> 5;
        const double mean = s_mean[k];
        const float *col = s_x + k * (E3D_FN_TPB + 1) + seg * 32;
        double cnt = 0.0, s1 = 0.0, s2 = 0.0;
        for (int r = 0; r < 32; r++) {
            if (s_live[seg * 32 + r] != 0.f) {
                const double d = (double)col[r] - mean;
                cnt += 1.0; s1 += d; s2 += d * d;
            }
        }
        double *part = s_part + (seg * E3D_FN_K + k) * 3;
        part[0] = cnt; part[1] = s1; part[2] = s2;
        __syncthreads();
        if (t < E3D_FN_K) {
            double C = 0.0, A = 0.0, Q = 0.0;
            for (int g = 0; g < E3D_FN_SEG; g++) {
                const double *q = s_part + (g * E3D_FN_K + t) * 3;
                C += q[0]; A += q[1]; Q += q[2];
            }
            double *slot = slots + (size_t)blockIdx.x * E3D_SLOT + (t >> 4) * obsnorm::ROW;
            if ((t & 15) == 0) slot[0] += C;
            slot[1 + (t & 15)] += A;
            slot[1 + E3D_FEAT + (t & 15)] += Q;
        }
    }
}

// sums [2][33] = the slots added in index order (e3d_obs_norm_reduce): one lane per entry
__global__ __launch_bounds__(128) void k_e3d_obs_norm_reduce(const double *slots, const int nslots, double *sums) {
    const int t = threadIdx.x;
    if (t >= E3D_SLOT) return;
    double s = 0.0;
    for (int b = 0; b < nslots; b++) s += slots[(size_t)b * E3D_SLOT + t];
    sums[t] = s;
}

// the merge of the totals into the state (e3d_obs_norm_update; obsnorm::merge), one lane per entry, then the slots are zeroed.  Every
// lane reads what it needs before any lane writes (the lanes of n, mean and M2 of one column read each other's entries).
__global__ __launch_bounds__(128) void k_e3d_obs_norm_update(double *state, const double *sums, double *slots, const int nslots) {
    const int t = threadIdx.x;
    double out = 0.0;
    const bool lane = t < E3D_SLOT;
    if (lane) {
        const int net = t / obsnorm::ROW, j = t - net * obsnorm::ROW, col = j == 0 ? 0 : (j - 1) & 15;
        const double *row = state + net * obsnorm::ROW, *sr = sums + net * obsnorm::ROW;
        const double n = row[0], C = sr[0];
        double mean = row[1 + col], M2 = row[1 + E3D_FEAT + col];
        obsnorm::merge(n, C, sr[1 + col], sr[1 + E3D_FEAT + col], mean, M2);
        out = j == 0 ? n + C : (j <= E3D_FEAT ? mean : M2);
    }
    __syncthreads();
    if (lane) state[t] = out;
    if (slots)
        for (int i = t; i < nslots * E3D_SLOT; i += blockDim.x) slots[i] = 0.0;
}

// the shaping potential of pursuer a of environment env in the current records (p_on, e_on: their active flags)
__device__ __forceinline__ double e3d_potential(const e3d_state &st, int env, int P, int a, bool p_on, bool e_on, double coef) {
    const double *gp = st.p + (size_t)env * 7 * P + a, *ge = st.e + (size_t)env * 7;
    return rshape::potential(coef, p_on, e_on, rshape::dist3(gp[0] - ge[0], gp[P] - ge[1], gp[2 * P] - ge[2]));
}

// MAPPO bookkeeping of one tick (include/e3d_env.h e3d_policy_record): the tick's lane layout, lane = (environment, pursuer).  Every lane
// masks its own buffer entries; the group's flags (pursuers left, evader dead, evader at the target) come from the records after the
// tick, the team reward from shuffles in agent order; slot 0 writes the accumulators after every lane of the group has read them (one
// wave, program order).  SCALED: the reward row is the reference's RewardScaling of the raw reward (csrc/reward_scale.hpp); the state
// rs [N][1 + 3P] is read and written once per lane, n by slot 0.  SHAPED: potential-based distance shaping (csrc/reward_shaping.hpp) goes
// into the reward row -- and into RewardScaling when SCALED -- once the terminal predicate of v_next is known; every lane loads and
// stores its own phi [N][P] entry once.  The unshaped instantiations are the code they were before SHAPED existed.  TEAM: team reward
// sharing (csrc/team_reward.hpp) -- m = (1 - alpha) raw + (alpha s) live, s the team's f64 sum of raw * live from shuffles in agent
// order ahead of everything that reads a reward, takes the place of the raw reward in the shaping step, the RewardScaling step and
// the buffer's row of environments not done before the step; acc.ret keeps the raw reward.  Every TEAM statement sits under
// `if (TEAM)` or is `m` where `(double)raw` stood, so the TEAM = false instantiations are the instructions they were before it.
template <int PT, bool SCALED, bool SHAPED, bool TEAM>
__global__ __launch_bounds__(WAVE * WPB) void k_e3d_policy_record(const e3d_config c, const e3d_state st, const float *reward, const uint8_t *done,
                                                                  const e3d_record_io io, const e3d_policy_acc acc, const double kill,
                                                                  double *rs, const double gamma, double *phi, const double coef,
                                                                  const double alpha) {
    constexpr int G = WAVE / PT;
    constexpr unsigned long long GM = (PT == 64) ? ~0ull : ((1ull << PT) - 1ull);
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT, base = lane - a;
    const int env = wave * G + g, P = c.P;
    const bool ev = env < st.N, pv = ev && a < P;
    const float live = pv ? io.live[(int64_t)env * io.live_rs + a] : 0.f;
    const float raw = pv ? reward[(size_t)env * P + a] : 0.f;
    const float rl = raw * live;
    const bool db = ev && acc.done_before[env] != 0;
    float rb = rl;  // the buffer's reward
    double m = (double)raw;  // what shaping, scaling and the buffer take for the reward
    if (TEAM) {  // every lane of the wave runs the loop (the trip count is wave-uniform)
        const double xl = (double)raw * (double)live;
        double sd = 0.0;
        for (int k = 0; k < P; k++) sd = sd + __shfl(xl, base + k);
        if (!db) m = team::share(alpha, (double)raw, sd, (double)live);
        if (!SCALED && !SHAPED) rb = (float)m * live;
    }
    if (SCALED && !SHAPED && pv && !db) {
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
    const bool p_on = pv && st.p[(size_t)env * 7 * P + 6 * P + a] != 0.0;
    const int pa = __popcll((__ballot(p_on) >> base) & GM);
    bool e_dead = false, reach = false;
    if (ev) {
        const double *ge = st.e + (size_t)env * 7, *tg = st.target + (size_t)env * 3;
        e_dead = ge[6] == 0.0;
        reach = sq3(ge[0] - tg[0], ge[1] - tg[1], ge[2] - tg[2]) <= kill;
    }
    float s = 0.f;  // the step's team reward, summed in agent order
    for (int k = 0; k < P; k++) s += __shfl(rl, base + k);
    const bool ended = ev && (acc.ended[env] != 0 || ((reach || pa == 0 || e_dead) && !db));
    const bool dn = ev && (db || done[env] != 0);
    if (SHAPED && pv) {
        if (!db) {
            double ph = phi[(size_t)env * P + a];
            const double x = rshape::step(m, gamma, ph, e3d_potential(st, env, P, a, p_on, !e_dead, coef), !p_on || ended, (double)live);
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
    if (pv) {
        if (io.v_next && (!p_on || ended)) io.v_next[(int64_t)env * io.v_next_rs + a] = 0.f;
        if (io.live_next) io.live_next[(int64_t)env * io.live_next_rs + a] = (p_on && !dn) ? 1.f : 0.f;
    }
    if (ev && a == 0) {
        acc.ended[env] = ended;
        if (e_dead && !db) acc.captured[env] = 1;
        if (!db) acc.length[env] += 1.f;
        acc.ret[env] += s;
        acc.done_before[env] = dn;
    }
}

// phi [N][P] = the shaping potential of the current records (e3d_shaping_begin): the tick's lane layout, one store per lane
template <int PT>
__global__ __launch_bounds__(WAVE * WPB) void k_e3d_shaping_begin(const e3d_config c, const e3d_state st, double *phi, const double coef) {
    constexpr int G = WAVE / PT;
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT;
    const int env = wave * G + g, P = c.P;
    if (env >= st.N || a >= P) return;
    const bool p_on = st.p[(size_t)env * 7 * P + 6 * P + a] != 0.0, e_on = st.e[(size_t)env * 7 + 6] != 0.0;
    phi[(size_t)env * P + a] = e3d_potential(st, env, P, a, p_on, e_on, coef);
}

// e3d_policy_record (include/policy_record.h): the checks, then one launch in the tick's lane layout; an option that is off passes the
// kernel nullptr / 0.0 whatever the record holds
template <bool SCALED, bool SHAPED, bool TEAM>
int e3d_record_launch(const e3d_config *c, const e3d_state *st, const float *reward, const uint8_t *done, const e3d_record_io *io,
                      const e3d_policy_acc *acc, const policy_record_opts &o, void *stream) {
    if (!c || !st || !reward || !done || !io || !acc || !io->live || (io->v && !io->value)) return E3D_ERR_NULL;
    if (!acc->done_before || !acc->ended || !acc->captured || !acc->ret || !acc->length) return E3D_ERR_NULL;
    const int rc = e3d_config_check(c);
    if (rc) return rc;
    if (TEAM && !team::coef_ok(o.alpha)) return E3D_ERR_BAD_CONFIG;
    if (st->N < 1) return 0;
    int blocks;
    const int pt = e3d_lanes(c, st->N, &blocks);
    const double kill = sq_threshold(c->kill_radius);
    double *rs = SCALED ? o.rs : nullptr, *phi = SHAPED ? o.phi : nullptr;
    const double gamma = SCALED || SHAPED ? o.gamma : 0.0, coef = SHAPED ? o.coef : 0.0, alpha = TEAM ? o.alpha : 0.0;
    hipStream_t s = (hipStream_t)stream;
#define E3D_REC(PT) hipLaunchKernelGGL((k_e3d_policy_record<PT, SCALED, SHAPED, TEAM>), dim3(blocks), dim3(WAVE * WPB), 0, s, *c, *st, reward, done, *io, *acc, kill, rs, gamma, phi, coef, alpha)
    if (pt == 8) E3D_REC(8); else if (pt == 16) E3D_REC(16); else if (pt == 32) E3D_REC(32); else E3D_REC(64);
#undef E3D_REC
    return (int)hipGetLastError();
}

// the scripted pursuers (include/e3d_env.h e3d_pursuer_guidance; csrc/guidance.hpp): the tick's lane layout, lane = (environment,
// pursuer).  Every lane keeps its pursuer and its own copy of the evader in registers and reads its team-mates through shuffles inside
// the group, in index order; no LDS, no atomics, three f64 stores per lane.  Every lane of the wave runs the shuffle loop (the trip
// count is wave-uniform); only the lanes of real pursuers store.
template <int PT>
__global__ __launch_bounds__(WAVE * WPB) void k_e3d_guidance(const e3d_config c, const e3d_state st, const e3d_guidance_params gp, double *actions) {
    constexpr int G = WAVE / PT;
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT, base = lane - a;
    const int env = wave * G + g, P = c.P;
    const bool ev = env < st.N, pv = ev && a < P;
    double x = 0, y = 0, z = 0, phi = 0, gamma = 0, act = 0;
    double ex = 0, ey = 0, ez = 0, ephi = 0, egam = 0, evel = 0, eact = 0;
    if (pv) {
        const double *q = st.p + (size_t)env * 7 * P + a;
        x = q[0]; y = q[P]; z = q[2 * P]; phi = q[3 * P]; gamma = q[4 * P]; act = q[6 * P];
    }
    if (ev) {
        const double *ge = st.e + (size_t)env * 7;
        ex = ge[0]; ey = ge[1]; ez = ge[2]; ephi = ge[3]; egam = ge[4]; evel = ge[5]; eact = ge[6];
    }
    const double rx = ex - x, ry = ey - y, rz = ez - z;
    const double t = guide::lead_time(rshape::dist3(rx, ry, rz), c.p_vmax, gp.lead);
    const double cg = cos(egam);
    double gx, gy, gz;
    guide::unit(rx + t * (evel * cg * cos(ephi)), ry + t * (evel * cg * sin(ephi)), rz + t * (evel * sin(egam)), gx, gy, gz);
    for (int k = 0; k < P; k++) {
        const double kx = __shfl(x, base + k), ky = __shfl(y, base + k), kz = __shfl(z, base + k), ka = __shfl(act, base + k);
        const double dx = x - kx, dy = y - ky, dz = z - kz, dij = rshape::dist3(dx, dy, dz);
        if (k != a && ka != 0.0 && guide::in_sep(dij, gp.sep_range)) {
            gx = gx + guide::repel(gp.sep_gain, dx, dij, gp.sep_range);
            gy = gy + guide::repel(gp.sep_gain, dy, dij, gp.sep_range);
            gz = gz + guide::repel(gp.sep_gain, dz, dij, gp.sep_range);
        }
    }
    if (pv) {
        double a0, a1, a2;
        guide::e3d_command(act != 0.0 && eact != 0.0, gx, gy, gz, phi, gamma, a0, a1, a2);
        double *d = actions + ((size_t)env * P + a) * 3;
        d[0] = a0; d[1] = a1; d[2] = a2;
    }
}

// the line-of-sight policy features (include/e3d_env.h e3d_pursuit_features; csrc/pursuit_features.hpp): the
// tick's lane layout, lane = (environment, pursuer).  A lane keeps its pursuer, its own copy of the evader and of the target and its
// row of pp_adj (one bit per team-mate) in registers; team-mates arrive through shuffles inside the group, in index order, and a
// running (nearest, second) pair per network takes them with strict <: no sort, no LDS, no atomics.  Every lane of the wave runs
// the loops (the trip counts are wave-uniform); only the lanes of real pursuers store, 2 x 8 16-byte stores each.
// TEAM (evader_obs: team): a sighting travels along communication links.  Lane i's neighbour mask is its row OR the transposed bit
// of every team-mate's row, cut to the active pursuers, plus itself; path doubling (reach_i <- OR of reach_j over j in reach_i, LOG2
// rounds of P shuffles of the mask's 32-bit halves) closes it, and the lane knows the evader when its component holds a pursuer
// that senses it (the group's ballot of pe_adj).
template <int PT>
__device__ __forceinline__ uint64_t e3d_shfl_mask(uint64_t m, int src) {
    uint64_t r = (uint32_t)__shfl((int)(uint32_t)m, src);
    if (PT == 64) r |= (uint64_t)(uint32_t)__shfl((int)(uint32_t)(m >> 32), src) << 32;   // (a narrower group has no high half)
    return r;
}

template <int PT, bool TEAM>
__global__ __launch_bounds__(WAVE * WPB) void k_e3d_pursuit(const e3d_config c, const e3d_state st, const e3d_obs_out o, const int sensed,
                                                            float *af, float *cf) {
    constexpr int G = WAVE / PT;
    constexpr int LOG2 = PT == 8 ? 3 : (PT == 16 ? 4 : (PT == 32 ? 5 : 6));
    constexpr uint64_t GM = PT == 64 ? ~0ull : ((1ull << PT) - 1ull);
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT, base = lane - a;
    const int env = wave * G + g, P = c.P;
    const bool ev = env < st.N, pv = ev && a < P;
    double x = 0, y = 0, z = 0, phi = 0, gamma = 0, v = 0, act = 0;
    double e[7] = {0, 0, 0, 0, 0, 0, 0}, tg[3] = {0, 0, 0};
    int32_t ts = 0;
    uint64_t rowm = 0;   // bit j: pp_adj[i][j] == 1
    bool pe = false;
    if (pv) {
        const double *q = st.p + (size_t)env * 7 * P + a;
        x = q[0]; y = q[P]; z = q[2 * P]; phi = q[3 * P]; gamma = q[4 * P]; v = q[5 * P]; act = q[6 * P];
        const float *pp = o.pp_adj + (int64_t)env * o.pp_adj_stride + (int64_t)a * P;
        for (int j = 0; j < P; j++) rowm |= (uint64_t)(pp[j] == 1.f) << j;
        pe = o.pe_adj[(int64_t)env * o.pe_adj_stride + a] == 1.f;
    }
    if (ev) {
        const double *ge = st.e + (size_t)env * 7;
        for (int k = 0; k < 7; k++) e[k] = ge[k];
        for (int k = 0; k < 3; k++) tg[k] = st.target[3 * (size_t)env + k];
        ts = st.time_step[env];
    }
    const bool on = pv && act != 0.0;
    const uint64_t amask = (__ballot(on) >> base) & GM;          // the group's active pursuers
    const uint64_t smask = (__ballot(on && pe) >> base) & GM;    // ... that sense the evader
    pfeat::Near na, nc;
    pfeat::near_init(na);
    pfeat::near_init(nc);
    uint64_t nb = rowm;
    for (int k = 0; k < P; k++) {
        const double kx = __shfl(x, base + k), ky = __shfl(y, base + k), kz = __shfl(z, base + k);
        if (TEAM) nb |= ((e3d_shfl_mask<PT>(rowm, base + k) >> a) & 1ull) << k;   // pp_adj[k][i]
        if (k != a && ((amask >> k) & 1ull)) {
            const double dx = kx - x, dy = ky - y, dz = kz - z;
            pfeat::near_add(nc, dx, dy, dz);
            if ((rowm >> k) & 1ull) pfeat::near_add(na, dx, dy, dz);
        }
    }
    bool ka = sensed ? pe : true;   // sensed | global
    if (TEAM) {
        uint64_t reach = (nb & amask) | (1ull << a);
#pragma unroll 1
        for (int r = 0; r < LOG2; r++) {
            uint64_t m = reach;
            for (int k = 0; k < P; k++) {
                const uint64_t rk = e3d_shfl_mask<PT>(reach, base + k);
                if ((reach >> k) & 1ull) m |= rk;
            }
            reach = m;
        }
        ka = (reach & smask) != 0ull;
    }
    if (!pv) return;   // (after the last shuffle)
    float fa[pfeat::FEAT], fc[pfeat::FEAT];
    if (on) {
        pfeat::Common cm;
        pfeat::common(cm, x, y, z, phi, gamma, v, e[0], e[1], e[2], e[3], e[4], e[5], tg[0], tg[1], tg[2], E3D_WORLD, c.p_vmax, c.e_vmax, ts,
                      c.max_step);
        const bool e_on = e[6] != 0.0;
        pfeat::row(fa, cm, ka && e_on, na, P, E3D_WORLD, c.kill_radius);
        pfeat::row(fc, cm, e_on, nc, P, E3D_WORLD, c.kill_radius);
    } else {
        for (int q = 0; q < pfeat::FEAT; q++) fa[q] = fc[q] = 0.f;
    }
    float4 *da = reinterpret_cast<float4 *>(af + ((size_t)env * P + a) * pfeat::FEAT), *dc = reinterpret_cast<float4 *>(cf + ((size_t)env * P + a) * pfeat::FEAT);
    for (int q = 0; q < pfeat::FEAT / 4; q++) {
        da[q] = make_float4(fa[4 * q], fa[4 * q + 1], fa[4 * q + 2], fa[4 * q + 3]);
        dc[q] = make_float4(fc[4 * q], fc[4 * q + 1], fc[4 * q + 2], fc[4 * q + 3]);
    }
}

// the centralised critic input (include/e3d_env.h e3d_central_features; csrc/central_critic.hpp): k_e3d_pursuit's
// launch -- the same lanes, the same actor rows and the same first 32 critic columns through the same pfeat:: calls -- whose critic
// row goes on with one 8-column slot per active team-mate, nearest first.  PT <= 16, so every loop over the team is unrolled over
// the compile-time PT (lanes past P are inactive, amask masks them) and the squared distances d2[PT] stay in registers: nothing is
// indexed at run time but global memory.  A lane rounds its own u and v / p_vmax to fp32 once and the team reads them through
// shuffles; a team-mate's slot is its rank, the count of the team-mates that sort ahead of it (ccrit::ahead), and its block goes
// straight to that slot as two 16-byte stores, the slots past |V| and the rows of inactive pursuers as zero blocks: no sort, no
// LDS, no atomics, no local row of 32 + 8 (P - 1) floats.  The second pass shuffles the positions again instead of keeping
// 3 PT differences.
template <int PT, bool TEAM>
__global__ __launch_bounds__(WAVE * WPB) void k_e3d_central(const e3d_config c, const e3d_state st, const e3d_obs_out o, const int sensed,
                                                            float *af, float *cf) {
    static_assert(PT <= ccrit::MAX_P, "the team loops are unrolled over PT");
    static_assert(ccrit::MATE == E3D_CENTRAL_MATE && ccrit::MAX_P == E3D_CENTRAL_MAX_P && ccrit::feat(3) == E3D_CENTRAL_FEAT(3), "include/e3d_env.h");
    constexpr int G = WAVE / PT;
    constexpr int LOG2 = PT == 8 ? 3 : 4;
    constexpr uint64_t GM = (1ull << PT) - 1ull;
    const int lane = threadIdx.x & (WAVE - 1), wave = blockIdx.x * WPB + (threadIdx.x >> 6);
    const int g = lane / PT, a = lane - g * PT, base = lane - a;
    const int env = wave * G + g, P = c.P, CF = ccrit::feat(P);
    const bool ev = env < st.N, pv = ev && a < P;
    double x = 0, y = 0, z = 0, phi = 0, gamma = 0, v = 0, act = 0;
    double e[7] = {0, 0, 0, 0, 0, 0, 0}, tg[3] = {0, 0, 0};
    int32_t ts = 0;
    uint64_t rowm = 0;   // bit j: pp_adj[i][j] == 1
    bool pe = false;
    if (pv) {
        const double *q = st.p + (size_t)env * 7 * P + a;
        x = q[0]; y = q[P]; z = q[2 * P]; phi = q[3 * P]; gamma = q[4 * P]; v = q[5 * P]; act = q[6 * P];
        const float *pp = o.pp_adj + (int64_t)env * o.pp_adj_stride + (int64_t)a * P;
        for (int j = 0; j < P; j++) rowm |= (uint64_t)(pp[j] == 1.f) << j;
        pe = o.pe_adj[(int64_t)env * o.pe_adj_stride + a] == 1.f;
    }
    if (ev) {
        const double *ge = st.e + (size_t)env * 7;
        for (int k = 0; k < 7; k++) e[k] = ge[k];
        for (int k = 0; k < 3; k++) tg[k] = st.target[3 * (size_t)env + k];
        ts = st.time_step[env];
    }
    const bool on = pv && act != 0.0;
    const uint64_t amask = (__ballot(on) >> base) & GM;          // the group's active pursuers
    const uint64_t smask = (__ballot(on && pe) >> base) & GM;    // ... that sense the evader
    const uint64_t vm = on ? amask & ~(1ull << a) : 0ull;        // V_i of the critic
    pfeat::Near na, nc;
    pfeat::near_init(na);
    pfeat::near_init(nc);
    uint64_t nb = rowm;
    double d2[PT];
#pragma unroll
    for (int k = 0; k < PT; k++) {
        const double kx = __shfl(x, base + k), ky = __shfl(y, base + k), kz = __shfl(z, base + k);
        if (TEAM) nb |= ((e3d_shfl_mask<PT>(rowm, base + k) >> a) & 1ull) << k;   // pp_adj[k][i]
        const double dx = kx - x, dy = ky - y, dz = kz - z;
        d2[k] = pfeat::sq3(dx, dy, dz);
        if (k != a && ((amask >> k) & 1ull)) {
            pfeat::near_add(nc, dx, dy, dz);
            if ((rowm >> k) & 1ull) pfeat::near_add(na, dx, dy, dz);
        }
    }
    bool ka = sensed ? pe : true;   // sensed | global
    if (TEAM) {
        uint64_t reach = (nb & amask) | (1ull << a);
#pragma unroll 1
        for (int r = 0; r < LOG2; r++) {
            uint64_t m = reach;
            for (int k = 0; k < P; k++) {
                const uint64_t rk = e3d_shfl_mask<PT>(reach, base + k);
                if ((reach >> k) & 1ull) m |= rk;
            }
            reach = m;
        }
        ka = (reach & smask) != 0ull;
    }
    pfeat::Common cm;   // (every lane: the team reads this lane's share below)
    pfeat::common(cm, x, y, z, phi, gamma, v, e[0], e[1], e[2], e[3], e[4], e[5], tg[0], tg[1], tg[2], E3D_WORLD, c.p_vmax, c.e_vmax, ts, c.max_step);
    float h[4];
    ccrit::share(h, cm);
    float *crow = cf + ((size_t)env * P + a) * CF;   // (dereferenced by the lanes of real pursuers only)
    if (pv) {
        float fa[pfeat::FEAT], fc[pfeat::FEAT];
        if (on) {
            const bool e_on = e[6] != 0.0;
            pfeat::row(fa, cm, ka && e_on, na, P, E3D_WORLD, c.kill_radius);
            pfeat::row(fc, cm, e_on, nc, P, E3D_WORLD, c.kill_radius);
        } else {
            for (int q = 0; q < pfeat::FEAT; q++) fa[q] = fc[q] = 0.f;
        }
        float4 *da = reinterpret_cast<float4 *>(af + ((size_t)env * P + a) * pfeat::FEAT), *dc = reinterpret_cast<float4 *>(crow);
        for (int q = 0; q < pfeat::FEAT / 4; q++) {
            da[q] = make_float4(fa[4 * q], fa[4 * q + 1], fa[4 * q + 2], fa[4 * q + 3]);
            dc[q] = make_float4(fc[4 * q], fc[4 * q + 1], fc[4 * q + 2], fc[4 * q + 3]);
        }
    }
#pragma unroll
    for (int k = 0; k < PT; k++) {
        const double kx = __shfl(x, base + k), ky = __shfl(y, base + k), kz = __shfl(z, base + k);
        float hk[4];
        for (int q = 0; q < 4; q++) hk[q] = __shfl(h[q], base + k);
        if ((vm >> k) & 1ull) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < PT; j++)
                if (j != k) rank += (int)(((vm >> j) & 1ull) && ccrit::ahead(d2[j], j, d2[k], k));
            float f[ccrit::MATE];
            ccrit::slot(f, pfeat::Mate{d2[k], kx - x, ky - y, kz - z}, hk, E3D_WORLD, c.kill_radius);
            float4 *d = reinterpret_cast<float4 *>(crow + pfeat::FEAT + ccrit::MATE * rank);
            d[0] = make_float4(f[0], f[1], f[2], f[3]);
            d[1] = make_float4(f[4], f[5], f[6], f[7]);
        }
    }
    if (!pv) return;
    const int nv = __popcll(vm);
#pragma unroll
    for (int s = 0; s < PT - 1; s++)
        if (s >= nv && s < P - 1) {
            float4 *d = reinterpret_cast<float4 *>(crow + pfeat::FEAT + ccrit::MATE * s);
            d[0] = d[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
}

struct E3dResetter { e3d_config cfg; int N; std::vector<rngrep::NpRandom> rng; };

}  // namespace

extern "C" {

int e3d_config_check(const e3d_config *c) {
    if (!c) return E3D_ERR_NULL;
    if (c->P < 1 || c->P > E3D_MAX_P || c->max_step < 1) return E3D_ERR_BAD_CONFIG;
    return 0;
}

int e3d_env_load(const e3d_config *cfg, const e3d_state *st, const double *p, const double *e, const double *target, void *stream) {
    if (!cfg || !st || !p || !e || !target) return E3D_ERR_NULL;
    int rc = e3d_config_check(cfg);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t N = st->N, P = cfg->P;
    double *dp = nullptr;
    hipError_t err;
#define TRY(x) do { err = (x); if (err != hipSuccess) return (int)err; } while (0)
    TRY(hipMallocAsync((void **)&dp, N * P * 7 * sizeof(double), s));
    TRY(hipMemcpyAsync(dp, p, N * P * 7 * sizeof(double), hipMemcpyHostToDevice, s));
    TRY(hipMemcpyAsync(st->e, e, N * 7 * sizeof(double), hipMemcpyHostToDevice, s));
    TRY(hipMemcpyAsync(st->target, target, N * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    TRY(hipMemsetAsync(st->time_step, 0, N * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_aos_to_soa7, dim3((unsigned)((N * P * 7 + 255) / 256)), dim3(256), 0, s, (int)N, (int)P, dp, st->p);
    TRY(hipFreeAsync(dp, s));
#undef TRY
    return (int)hipGetLastError();
}

int e3d_env_observe(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, void *stream) {
    if (!cfg || !st || !out) return E3D_ERR_NULL;
    int rc = e3d_config_check(cfg);
    if (rc) return rc;
    return launch<false>(cfg, st, nullptr, nullptr, nullptr, nullptr, nullptr, *out, (hipStream_t)stream);
}

int e3d_env_tick(const e3d_config *cfg, const e3d_state *st, const double *actions, const double *e_cmd, float *reward, uint8_t *active,
                 uint8_t *done, const e3d_obs_out *out, void *stream) {
    if (!cfg || !st || !actions || !e_cmd || !reward || !active || !done) return E3D_ERR_NULL;
    int rc = e3d_config_check(cfg);
    if (rc) return rc;
    e3d_obs_out o0;
    memset(&o0, 0, sizeof o0);
    return launch<true>(cfg, st, actions, e_cmd, reward, active, done, out ? *out : o0, (hipStream_t)stream);
}

int e3d_policy_features(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, float *actor_feat, float *critic_feat, void *stream) {
    if (!cfg || !st || !out || !out->pp_adj || !out->pe_adj || !actor_feat || !critic_feat) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    const int64_t rows = (int64_t)st->N * cfg->P;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(k_e3d_features, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *cfg, *st, *out, actor_feat, critic_feat);
    return (int)hipGetLastError();
}

int64_t e3d_obs_norm_slots(int64_t rows) { return rows <= 0 ? 0 : (rows + E3D_FN_TPB - 1) / E3D_FN_TPB; }

int e3d_policy_features_norm(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, float *actor_feat, float *critic_feat,
                             const double *norm_state, double clip, const float *live, int64_t live_rs, double *slots, void *stream) {
    if (!cfg || !st || !out || !out->pp_adj || !out->pe_adj || !actor_feat || !critic_feat || !norm_state || (slots && !live)) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    if (!(clip > 0.0) || std::isinf(clip)) return E3D_ERR_BAD_CONFIG;
    const int64_t rows = (int64_t)st->N * cfg->P;
    if (rows == 0) return 0;
    const dim3 grid((unsigned)e3d_obs_norm_slots(rows)), block(E3D_FN_TPB);
    hipStream_t s = (hipStream_t)stream;
    if (slots) hipLaunchKernelGGL(k_e3d_features_norm<true>, grid, block, 0, s, *cfg, *st, *out, actor_feat, critic_feat, norm_state, clip, live, live_rs, slots);
    else hipLaunchKernelGGL(k_e3d_features_norm<false>, grid, block, 0, s, *cfg, *st, *out, actor_feat, critic_feat, norm_state, clip, nullptr, (int64_t)0, nullptr);
    return (int)hipGetLastError();
}

int e3d_obs_norm_reduce(const double *slots, int64_t nslots, double *sums, void *stream) {
    if (!slots || !sums) return E3D_ERR_NULL;
    if (nslots < 0 || nslots > INT32_MAX / E3D_SLOT) return E3D_ERR_BAD_CONFIG;
    hipLaunchKernelGGL(k_e3d_obs_norm_reduce, dim3(1), dim3(128), 0, (hipStream_t)stream, slots, (int)nslots, sums);
    return (int)hipGetLastError();
}

int e3d_obs_norm_update(double *norm_state, const double *sums, double *slots, int64_t nslots, void *stream) {
    if (!norm_state || !sums) return E3D_ERR_NULL;
    if (nslots < 0 || nslots > INT32_MAX / E3D_SLOT) return E3D_ERR_BAD_CONFIG;
    hipLaunchKernelGGL(k_e3d_obs_norm_update, dim3(1), dim3(128), 0, (hipStream_t)stream, norm_state, sums, slots, (int)nslots);
    return (int)hipGetLastError();
}

int e3d_policy_record(const e3d_config *cfg, const e3d_state *st, const float *reward, const uint8_t *done, const e3d_record_io *io,
                      const e3d_policy_acc *acc, const policy_record_opts *opts, void *stream) {
    const policy_record_opts off = {};
    const policy_record_opts &o = opts ? *opts : off;
    // <SCALED, SHAPED, TEAM>; the cases stand in the order in which the code object has always listed these kernels
    switch ((o.rs ? 1 : 0) | (o.phi ? 2 : 0) | (o.team ? 4 : 0)) {
        case 1: return e3d_record_launch<true, false, false>(cfg, st, reward, done, io, acc, o, stream);
        case 0: return e3d_record_launch<false, false, false>(cfg, st, reward, done, io, acc, o, stream);
        case 3: return e3d_record_launch<true, true, false>(cfg, st, reward, done, io, acc, o, stream);
        case 2: return e3d_record_launch<false, true, false>(cfg, st, reward, done, io, acc, o, stream);
        case 7: return e3d_record_launch<true, true, true>(cfg, st, reward, done, io, acc, o, stream);
        case 6: return e3d_record_launch<false, true, true>(cfg, st, reward, done, io, acc, o, stream);
        case 5: return e3d_record_launch<true, false, true>(cfg, st, reward, done, io, acc, o, stream);
        default: return e3d_record_launch<false, false, true>(cfg, st, reward, done, io, acc, o, stream);
    }
}

int e3d_shaping_begin(const e3d_config *cfg, const e3d_state *st, double *phi, double coef, void *stream) {
    if (!cfg || !st || !phi) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    if (st->N < 1) return 0;
    int blocks;
    const int pt = e3d_lanes(cfg, st->N, &blocks);
    hipStream_t s = (hipStream_t)stream;
#define E3D_SB(PT) hipLaunchKernelGGL((k_e3d_shaping_begin<PT>), dim3(blocks), dim3(WAVE * WPB), 0, s, *cfg, *st, phi, coef)
    if (pt == 8) E3D_SB(8); else if (pt == 16) E3D_SB(16); else if (pt == 32) E3D_SB(32); else E3D_SB(64);
#undef E3D_SB
    return (int)hipGetLastError();
}

int e3d_pursuer_guidance(const e3d_config *cfg, const e3d_state *st, const e3d_guidance_params *params, double *actions, void *stream) {
    if (!cfg || !st || !params || !actions) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    if (!guide::param_ok(params->lead) || !guide::param_ok(params->sep_range) || !guide::param_ok(params->sep_gain)) return E3D_ERR_BAD_CONFIG;
    if (st->N < 1) return 0;
    if (!st->p || !st->e) return E3D_ERR_NULL;
    int blocks;
    const int pt = e3d_lanes(cfg, st->N, &blocks);
    hipStream_t s = (hipStream_t)stream;
#define E3D_GD(PT) hipLaunchKernelGGL((k_e3d_guidance<PT>), dim3(blocks), dim3(WAVE * WPB), 0, s, *cfg, *st, *params, actions)
    if (pt == 8) E3D_GD(8); else if (pt == 16) E3D_GD(16); else if (pt == 32) E3D_GD(32); else E3D_GD(64);
#undef E3D_GD
    return (int)hipGetLastError();
}

int e3d_pursuit_features(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, int32_t evader_obs, float *actor_feat,
                         float *critic_feat, void *stream) {
    if (!cfg || !st || !out || !out->pp_adj || !out->pe_adj || !actor_feat || !critic_feat) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    if (evader_obs != E3D_EVADER_OBS_SENSED && evader_obs != E3D_EVADER_OBS_TEAM && evader_obs != E3D_EVADER_OBS_GLOBAL) return E3D_ERR_BAD_CONFIG;
    if (((uintptr_t)actor_feat | (uintptr_t)critic_feat) % 16) return E3D_ERR_BAD_CONFIG;   // the rows are stored as 16-byte lanes
    if (st->N < 1) return 0;
    if (!st->p || !st->e || !st->target || !st->time_step) return E3D_ERR_NULL;
    int blocks;
    const int pt = e3d_lanes(cfg, st->N, &blocks);
    hipStream_t s = (hipStream_t)stream;
    const int sensed = evader_obs == E3D_EVADER_OBS_SENSED;
#define E3D_PF(PT, TEAM) hipLaunchKernelGGL((k_e3d_pursuit<PT, TEAM>), dim3(blocks), dim3(WAVE * WPB), 0, s, *cfg, *st, *out, sensed, actor_feat, critic_feat)
    if (evader_obs == E3D_EVADER_OBS_TEAM) {
        if (pt == 8) E3D_PF(8, true); else if (pt == 16) E3D_PF(16, true); else if (pt == 32) E3D_PF(32, true); else E3D_PF(64, true);
    } else {
        if (pt == 8) E3D_PF(8, false); else if (pt == 16) E3D_PF(16, false); else if (pt == 32) E3D_PF(32, false); else E3D_PF(64, false);
    }
#undef E3D_PF
    return (int)hipGetLastError();
}

int e3d_pursuit_features_host(const e3d_config *cfg, int32_t N, const double *p, const double *e, const double *target, const int32_t *time_step,
                              const float *pp_adj, const float *pe_adj, int32_t evader_obs, float *actor_feat, float *critic_feat) {
    if (!cfg || !p || !e || !target || !time_step || !pp_adj || !pe_adj || !actor_feat || !critic_feat) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    if (evader_obs != E3D_EVADER_OBS_SENSED && evader_obs != E3D_EVADER_OBS_TEAM && evader_obs != E3D_EVADER_OBS_GLOBAL) return E3D_ERR_BAD_CONFIG;
    const int P = cfg->P;
    for (int32_t n = 0; n < N; n++) {
        const double *q = p + (size_t)n * 7 * P, *ge = e + (size_t)n * 7, *tg = target + (size_t)n * 3;
        const float *pp = pp_adj + (size_t)n * P * P, *pe = pe_adj + (size_t)n * P;
        uint64_t amask = 0, smask = 0, reach[E3D_MAX_P];
        for (int i = 0; i < P; i++) {
            if (q[6 * P + i] == 0.0) continue;
            amask |= 1ull << i;
            if (pe[i] == 1.f) smask |= 1ull << i;
        }
        if (evader_obs == E3D_EVADER_OBS_TEAM) {
            for (int i = 0; i < P; i++) {
                uint64_t nb = 0;
                for (int j = 0; j < P; j++) nb |= (uint64_t)(pp[i * P + j] == 1.f || pp[j * P + i] == 1.f) << j;
                reach[i] = ((amask >> i) & 1ull) ? ((nb & amask) | (1ull << i)) : (1ull << i);
            }
            pfeat::close_masks(reach, P);
        }
        for (int i = 0; i < P; i++) {
            float *fa = actor_feat + ((size_t)n * P + i) * pfeat::FEAT, *fc = critic_feat + ((size_t)n * P + i) * pfeat::FEAT;
            if (!((amask >> i) & 1ull)) {
                for (int k = 0; k < pfeat::FEAT; k++) fa[k] = fc[k] = 0.f;
                continue;
            }
            pfeat::Near na, nc;
            pfeat::near_init(na);
            pfeat::near_init(nc);
            for (int j = 0; j < P; j++) {
                if (j == i || !((amask >> j) & 1ull)) continue;
                const double dx = q[j] - q[i], dy = q[P + j] - q[P + i], dz = q[2 * P + j] - q[2 * P + i];
                pfeat::near_add(nc, dx, dy, dz);
                if (pp[i * P + j] == 1.f) pfeat::near_add(na, dx, dy, dz);
            }
            bool ka = true;
            if (evader_obs == E3D_EVADER_OBS_SENSED) ka = pe[i] == 1.f;
            else if (evader_obs == E3D_EVADER_OBS_TEAM) ka = (reach[i] & smask) != 0ull;
            pfeat::Common cm;
            pfeat::common(cm, q[i], q[P + i], q[2 * P + i], q[3 * P + i], q[4 * P + i], q[5 * P + i], ge[0], ge[1], ge[2], ge[3], ge[4], ge[5], tg[0],
                          tg[1], tg[2], E3D_WORLD, cfg->p_vmax, cfg->e_vmax, time_step[n], cfg->max_step);
            const bool e_on = ge[6] != 0.0;
            pfeat::row(fa, cm, ka && e_on, na, P, E3D_WORLD, cfg->kill_radius);
            pfeat::row(fc, cm, e_on, nc, P, E3D_WORLD, cfg->kill_radius);
        }
    }
    return 0;
}

int e3d_central_features(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, int32_t evader_obs, float *actor_feat,
                         float *critic_feat, void *stream) {
    if (!cfg || !st || !out || !out->pp_adj || !out->pe_adj || !actor_feat || !critic_feat) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    if (cfg->P > E3D_CENTRAL_MAX_P) return E3D_ERR_BAD_CONFIG;
    if (evader_obs != E3D_EVADER_OBS_SENSED && evader_obs != E3D_EVADER_OBS_TEAM && evader_obs != E3D_EVADER_OBS_GLOBAL) return E3D_ERR_BAD_CONFIG;
    if (((uintptr_t)actor_feat | (uintptr_t)critic_feat) % 16) return E3D_ERR_BAD_CONFIG;   // the rows are stored as 16-byte lanes
    if (st->N < 1) return 0;
    if (!st->p || !st->e || !st->target || !st->time_step) return E3D_ERR_NULL;
    const int pt = cfg->P <= 8 ? 8 : 16;
    const int envs_per_block = (WAVE / pt) * WPB, blocks = (st->N + envs_per_block - 1) / envs_per_block;
    hipStream_t s = (hipStream_t)stream;
    const int sensed = evader_obs == E3D_EVADER_OBS_SENSED;
#define E3D_CC(PT, TEAM) hipLaunchKernelGGL((k_e3d_central<PT, TEAM>), dim3(blocks), dim3(WAVE * WPB), 0, s, *cfg, *st, *out, sensed, actor_feat, critic_feat)
    if (evader_obs == E3D_EVADER_OBS_TEAM) {
        if (pt == 8) E3D_CC(8, true); else E3D_CC(16, true);
    } else {
        if (pt == 8) E3D_CC(8, false); else E3D_CC(16, false);
    }
#undef E3D_CC
    return (int)hipGetLastError();
}

int e3d_central_features_host(const e3d_config *cfg, int32_t N, const double *p, const double *e, const double *target, const int32_t *time_step,
                              const float *pp_adj, const float *pe_adj, int32_t evader_obs, float *actor_feat, float *critic_feat) {
    if (!cfg || !p || !e || !target || !time_step || !pp_adj || !pe_adj || !actor_feat || !critic_feat) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    if (cfg->P > E3D_CENTRAL_MAX_P) return E3D_ERR_BAD_CONFIG;
    if (evader_obs != E3D_EVADER_OBS_SENSED && evader_obs != E3D_EVADER_OBS_TEAM && evader_obs != E3D_EVADER_OBS_GLOBAL) return E3D_ERR_BAD_CONFIG;
    if (N < 1) return 0;
    const int P = cfg->P, CF = E3D_CENTRAL_FEAT(P);
    // the actor rows and the first 32 critic columns are the pursuit entry's: its dense critic rows, then copied into the wide ones
    std::vector<float> fc32((size_t)N * P * pfeat::FEAT);
    const int rp = e3d_pursuit_features_host(cfg, N, p, e, target, time_step, pp_adj, pe_adj, evader_obs, actor_feat, fc32.data());
    if (rp) return rp;
    for (int32_t n = 0; n < N; n++) {
        const double *q = p + (size_t)n * 7 * P;
        float hs[ccrit::MAX_P][4];   // every pursuer's share, from its own row
        for (int j = 0; j < P; j++)
            for (int k = 0; k < 4; k++) hs[j][k] = fc32[((size_t)n * P + j) * pfeat::FEAT + 3 + k];
        for (int i = 0; i < P; i++) {
            float *fc = critic_feat + ((size_t)n * P + i) * CF;
            for (int k = 0; k < pfeat::FEAT; k++) fc[k] = fc32[((size_t)n * P + i) * pfeat::FEAT + k];
            for (int k = pfeat::FEAT; k < CF; k++) fc[k] = 0.f;
            if (q[6 * P + i] == 0.0) continue;
            pfeat::Mate m[ccrit::MAX_P];
            bool in[ccrit::MAX_P];
            for (int j = 0; j < P; j++) {
                const double dx = q[j] - q[i], dy = q[P + j] - q[P + i], dz = q[2 * P + j] - q[2 * P + i];
                m[j] = pfeat::Mate{pfeat::sq3(dx, dy, dz), dx, dy, dz};
                in[j] = j != i && q[6 * P + j] != 0.0;
            }
            for (int k = 0; k < P; k++) {
                if (!in[k]) continue;
                int rank = 0;
                for (int j = 0; j < P; j++) rank += (int)(j != k && in[j] && ccrit::ahead(m[j].d2, j, m[k].d2, k));
                ccrit::slot(fc + pfeat::FEAT + ccrit::MATE * rank, m[k], hs[k], E3D_WORLD, cfg->kill_radius);
            }
        }
    }
    return 0;
}

int gauss_direction_map_host(int32_t R, const float *u, double *env_action) {
    if (!u || !env_action) return E3D_ERR_NULL;
    if (R < 0) return E3D_ERR_BAD_CONFIG;
    for (int32_t r = 0; r < R; r++) diract::to_env(u + (size_t)r * diract::LATENT, env_action + (size_t)r * diract::ENV_A);
    return 0;
}

int e3d_direction_label_host(int32_t R, const double *g, float *a_star) {
    if (!g || !a_star) return E3D_ERR_NULL;
    if (R < 0) return E3D_ERR_BAD_CONFIG;
    for (int32_t r = 0; r < R; r++) diract::label(g + (size_t)r * diract::ENV_A, a_star + (size_t)r * diract::LATENT);
    return 0;
}

int e3d_evader_slsqp(const e3d_config *cfg, const e3d_state *st, double *e_cmd, void *stream) {
    return e3d_evader_slsqp_nit(cfg, st, e_cmd, nullptr, stream);
}

int e3d_evader_slsqp_nit(const e3d_config *cfg, const e3d_state *st, double *e_cmd, int32_t *nit, void *stream) {
    if (!cfg || !st || !e_cmd) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    return launch_e3d_evader(cfg, st, e_cmd, nit, (hipStream_t)stream);
}

int e3d_evader_slsqp_host(const e3d_config *cfg, int32_t N, const double *p, const double *e, const double *target, double *e_cmd,
                          int32_t *nit) {
    if (!cfg || !p || !e || !target || !e_cmd) return E3D_ERR_NULL;
    const int rc = e3d_config_check(cfg);
    if (rc) return rc;
    if (cfg->P <= 8) e3d_evader_host_pm<8>(*cfg, N, p, e, target, e_cmd, nit);
    else if (cfg->P <= 16) e3d_evader_host_pm<16>(*cfg, N, p, e, target, e_cmd, nit);
    else if (cfg->P <= 32) e3d_evader_host_pm<32>(*cfg, N, p, e, target, e_cmd, nit);
    else e3d_evader_host_pm<64>(*cfg, N, p, e, target, e_cmd, nit);
    return 0;
}

void *e3d_resetter_create(const e3d_config *cfg, int32_t N, const uint32_t *seeds) {
    if (!cfg || !seeds || N < 1 || e3d_config_check(cfg)) return nullptr;
    E3dResetter *R = new E3dResetter();
    R->cfg = *cfg;
    R->N = N;
    R->rng.resize(N);
    for (int n = 0; n < N; n++) R->rng[n].seed(seeds[n]);
    return R;
}

void e3d_resetter_destroy(void *h) { delete (E3dResetter *)h; }

// Resume support: every environment's generator (rng_replica.hpp ResetterStateHeader, then one NpRandom record each; E = 1).
static rngrep::ResetterStateHeader e3d_state_header(const E3dResetter &R) {
    return rngrep::ResetterStateHeader{E3D_RESETTER_STATE_TAG, R.N, R.cfg.P, 1};
}

int64_t e3d_resetter_state_bytes(void *h) { return h ? rngrep::resetter_state_bytes(((E3dResetter *)h)->N) : 0; }

int e3d_resetter_get_state(void *h, void *out) {
    if (!h || !out) return E3D_ERR_NULL;
    E3dResetter &R = *(E3dResetter *)h;
    rngrep::resetter_state_get(e3d_state_header(R), R.rng.data(), out);
    return 0;
}

int e3d_resetter_set_state(void *h, const void *in) {
    if (!h || !in) return E3D_ERR_NULL;
    E3dResetter &R = *(E3dResetter *)h;
    return rngrep::resetter_state_set(e3d_state_header(R), R.rng.data(), in) ? 0 : E3D_ERR_BAD_STATE;
}

int e3d_resetter_reset(void *h, double *p, double *e, double *target, int32_t n_threads) {
    if (!h || !p || !e || !target) return E3D_ERR_NULL;
    E3dResetter &R = *(E3dResetter *)h;
    const int P = R.cfg.P;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > R.N) n_threads = R.N;
    std::vector<int> failed(n_threads, 0);
    auto work = [&](int t) {
        std::vector<double> pts;
        for (int n = t; n < R.N; n += n_threads) {
            rngrep::NpRandom &g = R.rng[n];
            double *tg = target + 3 * (size_t)n;
            for (int k = 0; k < 3; k++) tg[k] = g.random_sample() * 20;   // reset (:138-142)
            // gen_init_p_pos (:151-164): normal(10, 2, size 3).clip(5, 15), rejected when < 4 from an earlier point
            pts.clear();
            int draws = 0;
            while ((int)pts.size() < 3 * P) {
                double q[3];
                for (int k = 0; k < 3; k++) { const double v = g.normal(10.0, 2.0); q[k] = v < 5.0 ? 5.0 : (v > 15.0 ? 15.0 : v); }
                bool ok = true;
                if (++draws > E3D_RESET_MAX_DRAWS) failed[t] = 1;   // give up: keep this candidate, report the environment
                else for (size_t k = 0; k < pts.size() && ok; k += 3) ok = !(norm3(q[0] - pts[k], q[1] - pts[k + 1], q[2] - pts[k + 2]) < 4.0);
                if (ok) { pts.push_back(q[0]); pts.push_back(q[1]); pts.push_back(q[2]); }
            }
            for (int i = 0; i < P; i++) {
                double *s = p + ((size_t)n * P + i) * 7;
                s[0] = pts[3 * i]; s[1] = pts[3 * i + 1]; s[2] = pts[3 * i + 2];
                s[3] = (2 * g.random_sample() - 1) * PI;
                s[4] = (2 * g.random_sample() - 1) * PI / 2;
                s[5] = 0.0; s[6] = 1.0;
            }
            double *s = e + (size_t)n * 7;
            s[0] = 20 - tg[0]; s[1] = 20 - tg[1]; s[2] = 20 - tg[2];
            s[3] = (2 * g.random_sample() - 1) * PI;
            s[4] = (2 * g.random_sample() - 1) * PI / 2;
            s[5] = 0.0; s[6] = 1.0;
        }
    };
    if (n_threads == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < n_threads; t++) th.emplace_back(work, t);
        for (auto &x : th) x.join();
    }
    for (int t = 0; t < n_threads; t++)
        if (failed[t]) return E3D_ERR_RESET_FAILED;
    return 0;
}

}  // extern "C"
