// team_pool_heads.hpp -- the critic's team pool with H = 2, 4 or 8 attention heads (`algo.critic_team_pool_heads`; C ABI:
// include/mappo_ops.h team_pool_heads_fwd / team_pool_heads_bwd; DESIGN section 7z').  Width 128 only, teams of 1 .. 64.  H = 1 never
// comes here: it stays on team_pool.hpp, whose loads, flags, buckets and reduce this file reuses.
//
//   D = 128 / H, head h owns features [h D, (h + 1) D); a group = P consecutive rows f_j with a live flag each
//   s_j^h = sum_{u in h} score[u] f_j[u] (live j)      w^h = softmax over the live j of s^h (maximum subtracted)
//   c[u] = sum_live w_j^{h(u)} f_j[u]  (nobody live: 0)      out_i = f_i + gate * c      for EVERY row i of the group
//   backward, G = sum_i g_i, dc = gate * G, a_j^h = sum_{u in h} dc[u] f_j[u], e^h = sum_{u in h} dc[u] c[u], ds_j^h = w_j^h (a_j^h - e^h):
//   d f_i[u] = g_i[u] + [i live] (w_i^{h(u)} dc[u] + ds_i^{h(u)} score[u])     d score[u] = sum_live ds_j^{h(u)} f_j[u]     d gate = G * c
//
// ONE WAVE owns a group and lane l holds features 2 l, 2 l + 1 of every row, as in team_pool.hpp.  What differs:
//   heads     are LANE GROUPS: with LG = 64 / H, lanes [h LG, (h + 1) LG) hold exactly head h's features.  A score is a SEGMENTED
//             all-reduce of log2(LG) stages that never leaves the lane group: quad_perm xor 1, quad_perm xor 2, row_half_mirror,
//             row_mirror (DPP operands of the adds themselves, no LDS crossbar), and for LG = 32 one ds_swizzle xor 16.  3 / 4 / 5
//             stages a row for H = 8 / 4 / 2 against the single-head kernel's 6 bpermute stages; a_j of the backward likewise.
//   softmax   layout (a) of DESIGN 7z': every lane keeps its OWN head's PT scores in registers and runs that head's softmax itself,
//             redundantly within the lane group.  The single-head trick (score j in lane j, weights back as scalars) cannot carry
//             over -- a weight differs between lane groups, so it is a vector register whatever is done -- and dealing a head's rows
//             over its lanes would pay a bpermute per row and lane group to bring w_j (and ds_j) back.  Here no weight ever crosses
//             a lane: PT expf and PT divisions per lane and group, hidden behind the group's 1 KB a row of HBM traffic.
//   sums      the maximum, the denominator and c run over j = 0 .. PT - 1 in that order inside the lane; "live?" stays a scalar
//             condition on the ballot word, so dead rows cost a branch and rows of every lane group agree on it
//   backward  w and c by the forward's own functions; a_j is formed in the store loop and used at once (never kept), so the
//             registers are f (2 PT) + w (PT) + the gradient rows (2 PT, up to PT = 32).  At PT = 64 the gradient rows are read
//             twice, once for G and once for d f (the second read is the wave's own 32 KB, from L2), as in team_pool.hpp: staging
//             them in LDS would take 32 KB a wave, 128 KB a workgroup, and leave one workgroup a CU.
//             d score / d gate per lane over the wave's groups, the four waves in wave order through LDS, one 256-float block per
//             workgroup, k_feat_norm_reduce (layer_norm.hpp) over the blocks.  No atomics.
#pragma once
#include "team_pool.hpp"

template <int CTRL>
__device__ __forceinline__ float tph_dpp(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true)); }

// the sum of x over the lane's group of LG lanes, the same bits in every lane of the group (a + b == b + a in both partners of a stage)
template <int LG>
__device__ __forceinline__ float tph_sum(float x) {
    static_assert(LG == 8 || LG == 16 || LG == 32, "lane groups of 8, 16 or 32");
    x += tph_dpp<0xB1>(x);                    // quad_perm [1, 0, 3, 2]: lane ^ 1
    x += tph_dpp<0x4E>(x);                    // quad_perm [2, 3, 0, 1]: lane ^ 2
    x += tph_dpp<0x141>(x);                   // row_half_mirror: the other quad of the 8
    if constexpr (LG >= 16) x += tph_dpp<0x140>(x);   // row_mirror: the other 8 of the 16
    if constexpr (LG >= 32) x += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), 0x401F));   // bit-mask mode, xor 16 inside the 32
    return x;
}

// -> w[j]: the softmax weight of row j in THIS LANE'S head over the live rows (0 for a dead row and for j >= P)
template <int PT, int LG>
__device__ __forceinline__ void tph_weights(const float2 (&f)[PT], float2 sc, uint64_t word, float (&w)[PT]) {
#pragma clang fp contract(off)
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < PT; j++) {
        w[j] = tph_sum<LG>(fmaf(f[j].x, sc.x, f[j].y * sc.y));
        if ((word >> j) & 1) m = fmaxf(m, w[j]);          // (a scalar condition)
    }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < PT; j++) {            // in order of j
        w[j] = (word >> j) & 1 ? expf(w[j] - m) : 0.f;
        den += w[j];
    }
#pragma unroll
    for (int j = 0; j < PT; j++)
        if ((word >> j) & 1) w[j] = w[j] / den;           // (a live row: den >= 1)
}

// c = sum over the live j, in order, of w_j f_j
template <int PT>
__device__ __forceinline__ float2 tph_context(const float2 (&f)[PT], const float (&w)[PT], uint64_t word) {
    float2 c = make_float2(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < PT; j++)
        if ((word >> j) & 1) {                // (a scalar condition)
            c.x = fmaf(w[j], f[j].x, c.x);
            c.y = fmaf(w[j], f[j].y, c.y);
        }
    return c;
}

template <int PT, int H>
FA_KERNEL __launch_bounds__(256) void k_team_pool_heads_fwd(const float *__restrict__ feat, int64_t ldf, const void *__restrict__ live, int live_u8,
                                                             int64_t live_gs, const float *__restrict__ score, const float *__restrict__ gate,
                                                             float *__restrict__ out, int64_t ldo, int64_t G, int P) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's group index stays scalar)
    const float2 sc = *(const float2 *)(score + 2 * l), ga = *(const float2 *)(gate + 2 * l);
    for (int64_t g = (int64_t)blockIdx.x * TP_WAVES + w; g < G; g += (int64_t)gridDim.x * TP_WAVES) {
        float2 f[PT];
        float wt[PT];
        tp_load<PT>(feat + g * P * ldf + 2 * l, ldf, P, f);
        const uint64_t word = tp_word(live, live_u8, g * live_gs, P, l);
        tph_weights<PT, 64 / H>(f, sc, word, wt);
        const float2 c = tph_context<PT>(f, wt, word);
        float *const o = out + g * P * ldo + 2 * l;
#pragma unroll
        for (int j = 0; j < PT; j++)
            if (tp_row<PT>(j, P)) *(float2 *)(o + j * ldo) = make_float2(fmaf(ga.x, c.x, f[j].x), fmaf(ga.y, c.y, f[j].y));
    }
}

// part: [gridDim.x][256] floats, a block = d_score | d_gate.  KEEP: the gradient rows stay in registers (PT <= 32)
template <int PT, int H, bool KEEP>
FA_KERNEL __launch_bounds__(256) void k_team_pool_heads_bwd(const float *__restrict__ feat, int64_t ldf, const void *__restrict__ live, int live_u8,
                                                             int64_t live_gs, const float *__restrict__ score, const float *__restrict__ gate,
                                                             const float *__restrict__ gout, int64_t ldg, float *__restrict__ df, int64_t lddf,
                                                             int64_t G, int P, float *__restrict__ part) {
#pragma clang fp contract(off)
    constexpr int LG = 64 / H;
    __shared__ alignas(16) float comb[TP_WAVES][2 * TP_E];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's group index stays scalar)
    const float2 sc = *(const float2 *)(score + 2 * l), ga = *(const float2 *)(gate + 2 * l);
    float2 dsc = make_float2(0.f, 0.f), dga = make_float2(0.f, 0.f);
    for (int64_t g = (int64_t)blockIdx.x * TP_WAVES + w; g < G; g += (int64_t)gridDim.x * TP_WAVES) {
        float2 f[PT], gv[KEEP ? PT : 1];
        float wt[PT];
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
        tph_weights<PT, LG>(f, sc, word, wt);
        const float2 c = tph_context<PT>(f, wt, word);
        dga.x = fmaf(gs.x, c.x, dga.x);
        dga.y = fmaf(gs.y, c.y, dga.y);
        const float2 dc = make_float2(ga.x * gs.x, ga.y * gs.y);
        const float e = tph_sum<LG>(fmaf(dc.x, c.x, dc.y * c.y));   // the head's dc . c, by the expression of a_j below
        float *const d = df + g * P * lddf + 2 * l;
#pragma unroll
        for (int j = 0; j < PT; j++) {
            if (!tp_row<PT>(j, P)) continue;
            float2 v = KEEP ? gv[KEEP ? j : 0] : *(const float2 *)(gb + j * ldg);
            if ((word >> j) & 1) {            // (a scalar condition: every lane is in the all-reduce)
                const float a = tph_sum<LG>(fmaf(dc.x, f[j].x, dc.y * f[j].y));
                const float dj = wt[j] * (a - e);          // (one live row: c == f_j, the difference is 0)
                v.x = fmaf(wt[j], dc.x, fmaf(dj, sc.x, v.x));
                v.y = fmaf(wt[j], dc.y, fmaf(dj, sc.y, v.y));
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

inline bool tph_heads_ok(int heads) { return heads == 2 || heads == 4 || heads == 8; }

// one instantiation per (team-size bucket, head count)
template <int H>
inline int launch_team_pool_heads_fwd_h(const TpArgs &a, float *out, int64_t ldo, int64_t G, int P, int max_blocks, hipStream_t st) {
    const dim3 grid(fa_grid(G, 8, 1 << 16, max_blocks)), block(64 * TP_WAVES);
#define TPH_FWD(N) \
    hipLaunchKernelGGL((k_team_pool_heads_fwd<N, H>), grid, block, 0, st, a.feat, a.ldf, a.live, a.live_u8, a.live_gs, a.score, a.gate, out, ldo, G, P)
    TP_FOR_P(P, TPH_FWD)
#undef TPH_FWD
    return (int)hipGetLastError();
}

inline int launch_team_pool_heads_fwd(const TpArgs &a, int heads, float *out, int64_t ldo, int64_t G, int P, int max_blocks, hipStream_t st) {
    if (heads == 2) return launch_team_pool_heads_fwd_h<2>(a, out, ldo, G, P, max_blocks, st);
    if (heads == 4) return launch_team_pool_heads_fwd_h<4>(a, out, ldo, G, P, max_blocks, st);
    return launch_team_pool_heads_fwd_h<8>(a, out, ldo, G, P, max_blocks, st);
}

template <int H>
inline int launch_team_pool_heads_bwd_h(const TpArgs &a, const float *g, int64_t ldg, float *df, int64_t lddf, float *d_score, float *d_gate, int64_t G,
                                        int P, float *part, int max_blocks, hipStream_t st) {
    const int B = fa_grid(G, 4, TP_MAX_GRID, max_blocks);
    const dim3 grid(B), block(64 * TP_WAVES);
#define TPH_BWD(N) \
    hipLaunchKernelGGL((k_team_pool_heads_bwd<N, H, (N <= 32)>), grid, block, 0, st, a.feat, a.ldf, a.live, a.live_u8, a.live_gs, a.score, a.gate, g, ldg, df, \
                       lddf, G, P, part)
    TP_FOR_P(P, TPH_BWD)
#undef TPH_BWD
    FnJobs red;                               // the blocks in workgroup order -> d_score (the reduce's first 128 columns), d_gate
    memset(&red, 0, sizeof red);
    red.j[0].d_weight = d_score;
    red.j[0].d_bias = d_gate;
    hipLaunchKernelGGL(k_feat_norm_reduce, dim3(2 * FN_E / FN_RED_COLS, 1), dim3(FN_RED_RUNS * FN_RED_COLS), 0, st, red, (const float *)part, B);
    return (int)hipGetLastError();
}

inline int launch_team_pool_heads_bwd(const TpArgs &a, int heads, const float *g, int64_t ldg, float *df, int64_t lddf, float *d_score, float *d_gate,
                                      int64_t G, int P, float *part, int max_blocks, hipStream_t st) {
    if (heads == 2) return launch_team_pool_heads_bwd_h<2>(a, g, ldg, df, lddf, d_score, d_gate, G, P, part, max_blocks, st);
    if (heads == 4) return launch_team_pool_heads_bwd_h<4>(a, g, ldg, df, lddf, d_score, d_gate, G, P, part, max_blocks, st);
    return launch_team_pool_heads_bwd_h<8>(a, g, ldg, df, lddf, d_score, d_gate, G, P, part, max_blocks, st);
}
