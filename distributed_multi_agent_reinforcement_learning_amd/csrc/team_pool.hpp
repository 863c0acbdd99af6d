// team_pool.hpp -- attention-pooled team context for the critic (`algo.critic_team_pool: attention`): between the GRU features and the
// value head every pursuer's feature gets a permutation-invariant softmax pool over the LIVE team-mates' features added to it (C ABI:
// include/mappo_ops.h team_pool_fwd / team_pool_bwd).  Width 128 only, teams of 1 .. 64.
//
//   a group = the P pursuers of one environment at one step: P consecutive rows f_j, a live flag each; parameters score, gate (128 each)
//   s_j = score . f_j (live j)      w = softmax over the live j (maximum subtracted)      c = sum_live w_j f_j  (nobody live: c = 0)
//   out_i = f_i + gate * c          for EVERY row i of the group
//   backward, G = sum_i g_i, dc = gate * G, a_j = dc . f_j, ds_j = w_j (a_j - dc . c):
//   d f_i = g_i + [i live] (w_i dc + ds_i score)      d score = sum_live ds_j f_j      d gate = G * c
//
// ONE WAVE owns a group: lane l holds features 2 l, 2 l + 1 of every row as a float2 (the layout of fcra_pool.hpp / layer_norm.hpp), so
// the group is PT registers pairs per lane, read from HBM once per direction with every load issued before the first use.  The kernels
// are instantiated per team-size bucket PT in {8, 16, 32, 64}; P is a runtime argument, rows at or above P are loaded clamped to row
// P - 1 and zeroed, so the code is straight-line and every lane stays in every butterfly.
//   scores    a per-lane fmaf, then an xor butterfly: every lane ends with the same bits, and lane j keeps s_j -- the whole softmax of a
//             group (maximum, ONE expf, the division) then runs once, across the lanes of one register
//   live      the group's flags become one 64-bit ballot word in scalar registers: "live?" is a scalar condition, never a lane mask
//   pool      w_j comes back as a scalar (readlane j) and c accumulates over j = 0 .. P - 1 in that order inside the lane
//   backward  recomputes w and c by the forward's own functions (nothing was saved); d score / d gate are kept per lane over all the
//             wave's groups, the four waves are added in wave order through LDS into one partial block of 256 floats per workgroup
//             (d score | d gate) and k_feat_norm_reduce (layer_norm.hpp) adds the blocks in its fixed order.  Up to PT = 32 the
//             group's gradient rows stay in registers next to its features (128 VGPRs of rows); at PT = 64 that would be 256, so the
//             gradient rows are read twice there (once for G, once for d f; the second read is the wave's own 32 KB, from L2).
// Persistent 256-thread workgroups of four waves stride over the groups.  No atomics: two runs give equal bits, and a group's bits
// depend on its own rows and flags only.  Contraction is off where a difference of equal roundings must cancel (s - max, a_j - dc . c).
#pragma once
#include "layer_norm.hpp"

constexpr int TP_E = FA_E;                    // the only width
constexpr int TP_WAVES = FA_WAVES;            // groups in flight per workgroup
constexpr int TP_MAX_P = 64;                  // one ballot word
constexpr int TP_MAX_GRID = FA_MAX_GRID;      // workgroups of the backward = partial blocks in its workspace

__device__ __forceinline__ float tp_lane(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }

// is row j inside every team of the bucket?  (PT > 8: the bucket starts above PT / 2)
template <int PT>
__device__ __forceinline__ bool tp_row(int j, int P) { return (PT > 8 && j <= PT / 2) || j < P; }

// rows 0 .. PT - 1 of a group (base: the lane's pair of row 0), rows >= P clamped for the load and zeroed
template <int PT>
__device__ __forceinline__ void tp_load(const float *base, int64_t ld, int P, float2 (&f)[PT]) {
#pragma unroll
    for (int j = 0; j < PT; j++) {            // (one running address: it stops advancing at row P - 1)
        f[j] = *(const float2 *)base;
        base += tp_row<PT>(j + 1, P) ? ld : 0;
    }
#pragma unroll
    for (int j = 0; j < PT; j++)
        if (!tp_row<PT>(j, P)) f[j] = make_float2(0.f, 0.f);
}

// the live flags of a group (fp32 or uint8, non-zero = live) as one word in scalar registers
__device__ __forceinline__ uint64_t tp_word(const void *live, int live_u8, int64_t at, int P, int l) {
    bool on = false;
    if (l < P) on = live_u8 ? ((const uint8_t *)live)[at + l] != 0 : ((const float *)live)[at + l] != 0.f;
    return __ballot(on);
}

// -> in lane j: w_j, the softmax weight of row j over the live rows (0 for a dead row and for j >= P)
template <int PT>
__device__ __forceinline__ float tp_weights(const float2 (&f)[PT], float2 sc, uint64_t word, int l) {
#pragma clang fp contract(off)
    float sl = 0.f;
#pragma unroll
    for (int j = 0; j < PT; j++) {
        const float s = fn_wave_sum(fmaf(f[j].x, sc.x, f[j].y * sc.y));
        sl = l == j ? s : sl;
    }
    const bool on = (word >> l) & 1;
    float m = on ? sl : -INFINITY;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m = fmaxf(m, __shfl_xor(m, k));
    const float e = on ? expf(sl - m) : 0.f;
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < PT; j++) den += tp_lane(e, j);   // in order of j (dead rows add + 0)
    return on ? e / den : 0.f;
}

// c = sum over the live j, in order, of w_j f_j
template <int PT>
__device__ __forceinline__ float2 tp_context(const float2 (&f)[PT], float wl, uint64_t word) {
    float2 c = make_float2(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < PT; j++) {
        const float wj = tp_lane(wl, j);
        if ((word >> j) & 1) {                // (a scalar condition)
            c.x = fmaf(wj, f[j].x, c.x);
            c.y = fmaf(wj, f[j].y, c.y);
        }
    }
    return c;
}

template <int PT>
FA_KERNEL __launch_bounds__(256) void k_team_pool_fwd(const float *__restrict__ feat, int64_t ldf, const void *__restrict__ live, int live_u8,
                                                       int64_t live_gs, const float *__restrict__ score, const float *__restrict__ gate,
                                                       float *__restrict__ out, int64_t ldo, int64_t G, int P) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's group index stays scalar)
    const float2 sc = *(const float2 *)(score + 2 * l), ga = *(const float2 *)(gate + 2 * l);
    for (int64_t g = (int64_t)blockIdx.x * TP_WAVES + w; g < G; g += (int64_t)gridDim.x * TP_WAVES) {
        float2 f[PT];
        tp_load<PT>(feat + g * P * ldf + 2 * l, ldf, P, f);
        const uint64_t word = tp_word(live, live_u8, g * live_gs, P, l);
        const float2 c = tp_context<PT>(f, tp_weights<PT>(f, sc, word, l), word);
        float *const o = out + g * P * ldo + 2 * l;
#pragma unroll
        for (int j = 0; j < PT; j++)
            if (tp_row<PT>(j, P)) *(float2 *)(o + j * ldo) = make_float2(fmaf(ga.x, c.x, f[j].x), fmaf(ga.y, c.y, f[j].y));
    }
}

// part: [gridDim.x][256] floats, a block = d_score | d_gate.  KEEP: the gradient rows stay in registers (PT <= 32)
template <int PT, bool KEEP>
FA_KERNEL __launch_bounds__(256) void k_team_pool_bwd(const float *__restrict__ feat, int64_t ldf, const void *__restrict__ live, int live_u8,
                                                       int64_t live_gs, const float *__restrict__ score, const float *__restrict__ gate,
                                                       const float *__restrict__ gout, int64_t ldg, float *__restrict__ df, int64_t lddf, int64_t G,
                                                       int P, float *__restrict__ part) {
#pragma clang fp contract(off)
    __shared__ alignas(16) float comb[TP_WAVES][2 * TP_E];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's group index stays scalar)
    const float2 sc = *(const float2 *)(score + 2 * l), ga = *(const float2 *)(gate + 2 * l);
    float2 dsc = make_float2(0.f, 0.f), dga = make_float2(0.f, 0.f);
    for (int64_t g = (int64_t)blockIdx.x * TP_WAVES + w; g < G; g += (int64_t)gridDim.x * TP_WAVES) {
        float2 f[PT], gv[KEEP ? PT : 1];
        const float *const gb = gout + g * P * ldg + 2 * l;
        tp_load<PT>(feat + g * P * ldf + 2 * l, ldf, P, f);
        if constexpr (KEEP) tp_load<PT>(gb, ldg, P, gv);
        const uint64_t word = tp_word(live, live_u8, g * live_gs, P, l);
        float2 gs = make_float2(0.f, 0.f);    // G = the sum of the group's gradient rows, in order
        if constexpr (KEEP) {
#pragma unroll
            for (int j = 0; j < PT; j++) gs.x += gv[KEEP ? j : 0].x, gs.y += gv[KEEP ? j : 0].y;   // (rows >= P are zero)
        } else {
#pragma unroll
            for (int j = 0; j < PT; j++) {
                const float2 v = *(const float2 *)(gb + (tp_row<PT>(j, P) ? j : P - 1) * ldg);
                if (tp_row<PT>(j, P)) gs.x += v.x, gs.y += v.y;
            }
        }
        const float wl = tp_weights<PT>(f, sc, word, l);
        const float2 c = tp_context<PT>(f, wl, word);
        dga.x = fmaf(gs.x, c.x, dga.x);
        dga.y = fmaf(gs.y, c.y, dga.y);
        const float2 dc = make_float2(ga.x * gs.x, ga.y * gs.y);
        const float dcc = fn_wave_sum(fmaf(dc.x, c.x, dc.y * c.y));
        float al = 0.f;                       // lane j: a_j = dc . f_j, by the expression of dc . c (one live row: c == f_j, the difference is 0)
#pragma unroll
        for (int j = 0; j < PT; j++) {
            const float a = fn_wave_sum(fmaf(dc.x, f[j].x, dc.y * f[j].y));
            al = l == j ? a : al;
        }
        const float dsl = (word >> l) & 1 ? wl * (al - dcc) : 0.f;
        float *const d = df + g * P * lddf + 2 * l;
#pragma unroll
        for (int j = 0; j < PT; j++) {
            if (!tp_row<PT>(j, P)) continue;
            float2 v = KEEP ? gv[KEEP ? j : 0] : *(const float2 *)(gb + j * ldg);
            if ((word >> j) & 1) {            // (a scalar condition)
                const float wj = tp_lane(wl, j), dj = tp_lane(dsl, j);
                v.x = fmaf(wj, dc.x, fmaf(dj, sc.x, v.x));
                v.y = fmaf(wj, dc.y, fmaf(dj, sc.y, v.y));
                dsc.x = fmaf(dj, f[j].x, dsc.x);
                dsc.y = fmaf(dj, f[j].y, dsc.y);
            }
            *(float2 *)(d + j * lddf) = v;
        }
    }
    // the four waves in order -> one block per workgroup (every wave arrives here whatever its groups were)
    *(float2 *)(&comb[w][2 * l]) = dsc;
    *(float2 *)(&comb[w][TP_E + 2 * l]) = dga;
    __syncthreads();
    const int t = threadIdx.x;
    part[(size_t)blockIdx.x * (2 * TP_E) + t] = ((comb[0][t] + comb[1][t]) + comb[2][t]) + comb[3][t];
}

// one instantiation per team-size bucket
#define TP_FOR_P(P, CALL) \
    if (P <= 8) CALL(8); \
    else if (P <= 16) CALL(16); \
    else if (P <= 32) CALL(32); \
    else CALL(64);

struct TpArgs {                               // the arguments both directions share
    const float *feat; int64_t ldf; const void *live; int live_u8; int64_t live_gs; const float *score, *gate;
};

inline int launch_team_pool_fwd(const TpArgs &a, float *out, int64_t ldo, int64_t G, int P, int max_blocks, hipStream_t st) {
    const dim3 grid(fa_grid(G, 8, 1 << 16, max_blocks)), block(64 * TP_WAVES);
#define TP_FWD(N) hipLaunchKernelGGL(k_team_pool_fwd<N>, grid, block, 0, st, a.feat, a.ldf, a.live, a.live_u8, a.live_gs, a.score, a.gate, out, ldo, G, P)
    TP_FOR_P(P, TP_FWD)
#undef TP_FWD
    return (int)hipGetLastError();
}

inline int launch_team_pool_bwd(const TpArgs &a, const float *g, int64_t ldg, float *df, int64_t lddf, float *d_score, float *d_gate, int64_t G, int P,
                                float *part, int max_blocks, hipStream_t st) {
    const int B = fa_grid(G, 4, TP_MAX_GRID, max_blocks);
    const dim3 grid(B), block(64 * TP_WAVES);
#define TP_BWD(N) \
    hipLaunchKernelGGL((k_team_pool_bwd<N, (N <= 32)>), grid, block, 0, st, a.feat, a.ldf, a.live, a.live_u8, a.live_gs, a.score, a.gate, g, ldg, df, lddf, G, P, part)
    TP_FOR_P(P, TP_BWD)
#undef TP_BWD
    FnJobs red;                               // the blocks in workgroup order -> d_score (the reduce's first 128 columns), d_gate
    memset(&red, 0, sizeof red);
    red.j[0].d_weight = d_score;
    red.j[0].d_bias = d_gate;
    hipLaunchKernelGGL(k_feat_norm_reduce, dim3(2 * FN_E / FN_RED_COLS, 1), dim3(FN_RED_RUNS * FN_RED_COLS), 0, st, red, (const float *)part, B);
    return (int)hipGetLastError();
}
