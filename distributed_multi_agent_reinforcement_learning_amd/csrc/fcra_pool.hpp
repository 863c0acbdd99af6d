// fcra_pool.hpp -- DHGN's MAX-POOL aggregator for the FCRA hops (`algo.fcra_aggregator: pool`): an element-wise maximum over the listed
// team-mates' stored embeddings of one hop in place of the neighbour mean (C ABI: include/mappo_ops.h fcra_pool_fwd_multi / fcra_pool_bwd;
// DESIGN section 7v).  Ours, as csrc/pool_agg.hpp says; no new parameters.
//
//   y_j = W h_j (the caller's GEMM, no bias)        listed j for i: a_ij != 0 (the weight's value is not used)
//   out_i[u] = relu(b[u] + max over listed j of y_j[u])          nothing listed -> relu(b), the convention of csrc/fcra_att.hpp
//   backward, gp_i = [out_i > 0] g_i, j*(i, u) = the first listed j that attains the maximum:
//   dy_j[u] = sum over i with j*(i, u) = j of gp_i[u],   db = sum_i gp_i
//
// The unit of work is a ROW (P vectors of 128 floats); ONE WAVE owns a row, four waves of a persistent 256-thread workgroup stride over the
// rows.  The team size P is a template parameter (1 .. 16), as in fcra_att.hpp: lane l holds features 2 l, 2 l + 1 of all P vectors y_j
// in registers (2 P VGPRs), so y is read from HBM once.  The row's adjacency becomes a P x P BIT MASK in scalar registers: lane q
// compares entry q (+ 64, ..: at most four) with zero and a ballot collects the bits; segment i's P bits are shifted out of it with
// scalar arithmetic, so every "listed?" below is a scalar condition on a compile-time bit and no lane mask is kept per pair.
//   forward   segment i takes a masked maximum over the registers, adds the bias, applies the ReLU and stores through the column stride
//             (2 E: the left half of the hop's [agg | h] operand).  Under ones all P segments share one maximum.
//   backward  recomputes each (i, u) maximum and the index of its first strict improvement from y, reads `out` for the sign only, and
//             forms dy_j in registers with P^2 compare-selects a feature; db is kept per lane over all the wave's rows, the four
//             waves are added in order through LDS into one block per workgroup, k_fcra_pool_reduce adds the blocks in order of workgroup.
// No cross-lane traffic in either direction, no LDS in the forward, no workgroup barrier inside a row loop, no atomics; nothing per pair
// reaches HBM; a row's bits depend on that row's inputs only.
#pragma once
#include "fcra_att.hpp"

struct FpJobs { mo_fcra_pool_job j[MO_FCRA_POOL_MAX_JOBS]; };

constexpr int fp_words(int P) { return (P * P + 63) / 64; }

// the row's adjacency as bits: bit i P + j of the words = [a_ij != 0]; adj_row NULL: ones.  Every lane of the wave calls it.
template <int P>
__device__ __forceinline__ void fp_mask(const float *__restrict__ adj_row, int l, unsigned long long (&bm)[fp_words(P)]) {
#pragma unroll
    for (int c = 0; c < fp_words(P); c++) {
        const int q = 64 * c + l;
        bm[c] = adj_row ? __ballot(q < P * P && adj_row[q] != 0.f) : ~0ull;
    }
}
// segment i's P bits (bit j = listed j): scalar arithmetic on the ballot words
template <int P>
__device__ __forceinline__ uint32_t fp_row(const unsigned long long (&bm)[fp_words(P)], int i) {
    constexpr int NW = fp_words(P);
    const int pos = i * P, wd = pos >> 6, sh = pos & 63;
    unsigned long long lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < NW; c++) {
        if (c == wd) lo = bm[c];
        if (c == wd + 1) hi = bm[c];
    }
    const unsigned long long v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    return (uint32_t)v & ((1u << P) - 1u);
}

// out_i = relu(b + max over listed j of y_j) for the row's P segments; o: the row's first output vector + 2 l
template <int P>
__device__ __forceinline__ void fp_store_out(const float2 (&yv)[P], float2 b2, const float *__restrict__ adj_row, int l, float *__restrict__ o, int64_t ld) {
    if (!adj_row) {                           // ones: one maximum for the P segments
        float mx = yv[0].x, my = yv[0].y;
#pragma unroll
        for (int j = 1; j < P; j++) mx = fmaxf(mx, yv[j].x), my = fmaxf(my, yv[j].y);
        const float2 v = make_float2(fmaxf(b2.x + mx, 0.f), fmaxf(b2.y + my, 0.f));
#pragma unroll 4
        for (int i = 0; i < P; i++) *(float2 *)(o + i * ld) = v;
        return;
    }
    unsigned long long bm[fp_words(P)];
    fp_mask<P>(adj_row, l, bm);
#pragma unroll 1
    for (int i = 0; i < P; i++) {
        const uint32_t row = fp_row<P>(bm, i);
        float mx = -INFINITY, my = -INFINITY;
#pragma unroll
        for (int j = 0; j < P; j++)
            if (row >> j & 1u) mx = fmaxf(mx, yv[j].x), my = fmaxf(my, yv[j].y);
        const float px = row ? b2.x + mx : b2.x, py = row ? b2.y + my : b2.y;      // nothing listed: relu(b)
        *(float2 *)(o + i * ld) = make_float2(fmaxf(px, 0.f), fmaxf(py, 0.f));
    }
}

// grid (row groups, jobs).  A job's actor reads adj, its critic ones; when both read the same y it is loaded once.
template <int P>
FA_KERNEL __launch_bounds__(256) void k_fcra_pool_fwd(FpJobs jobs, int64_t R, const float *__restrict__ adj, int64_t adj_rs, int64_t out_ld) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's row index stays scalar)
    const mo_fcra_pool_job &job = jobs.j[blockIdx.y];
    const float2 b2 = *(const float2 *)(job.bias + 2 * l);
    const bool shared = job.out_actor && job.out_critic && job.y_actor == job.y_critic;
    for (int64_t r = (int64_t)blockIdx.x * FA_WAVES + w; r < R; r += (int64_t)gridDim.x * FA_WAVES) {
        float2 yv[P];
        if (job.out_actor) {
            fa_load<P>(job.y_actor, r, l, yv);
            fp_store_out<P>(yv, b2, adj + r * adj_rs, l, job.out_actor + r * P * out_ld + 2 * l, out_ld);
        }
        if (job.out_critic) {
            if (!shared) fa_load<P>(job.y_critic, r, l, yv);
            fp_store_out<P>(yv, b2, nullptr, l, job.out_critic + r * P * out_ld + 2 * l, out_ld);
        }
    }
}

// dy [R][P][128] dense; part: [gridDim.x][128] floats, a block = db.  adj NULL: ones.
template <int P>
FA_KERNEL __launch_bounds__(256) void k_fcra_pool_bwd(const float *__restrict__ y, const float *__restrict__ adj, int64_t adj_rs,
                                                       const float *__restrict__ out, int64_t out_ld, const float *__restrict__ g, int64_t g_ld,
                                                       int64_t R, float *__restrict__ dy, float *__restrict__ part) {
    __shared__ alignas(16) float comb[FA_WAVES][FA_E];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's row index stays scalar)
    float dbx = 0.f, dby = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * FA_WAVES + w; r < R; r += (int64_t)gridDim.x * FA_WAVES) {
        float2 yv[P], dv[P];
        unsigned long long bm[fp_words(P)];
        fa_load<P>(y, r, l, yv);
        fp_mask<P>(adj ? adj + r * adj_rs : nullptr, l, bm);
#pragma unroll
        for (int j = 0; j < P; j++) dv[j] = make_float2(0.f, 0.f);
        const float *const gr = g + r * P * g_ld + 2 * l, *const orow = out + r * P * out_ld + 2 * l;
        // one segment a trip, not unrolled (the 2 P row offsets of g and out would be loop invariants of the row loop held in scalar
        // registers); the next segment's g and out are fetched a trip ahead
        float2 g2 = *(const float2 *)gr, o2 = *(const float2 *)orow;
#pragma unroll 1
        for (int i = 0; i < P; i++) {
            float2 gn = g2, on = o2;
            if (i + 1 < P) gn = *(const float2 *)(gr + (i + 1) * g_ld), on = *(const float2 *)(orow + (i + 1) * out_ld);
            const float gx = o2.x > 0.f ? g2.x : 0.f, gy = o2.y > 0.f ? g2.y : 0.f;           // gp_i
            dbx += gx;
            dby += gy;
            const uint32_t row = fp_row<P>(bm, i);
            float mx = -INFINITY, my = -INFINITY;
            int jx = -1, jy = -1;             // the first strict improvement: the first listed j that attains the maximum
#pragma unroll
            for (int j = 0; j < P; j++)
                if (row >> j & 1u) {
                    if (yv[j].x > mx) mx = yv[j].x, jx = j;
                    if (yv[j].y > my) my = yv[j].y, jy = j;
                }
#pragma unroll
            for (int j = 0; j < P; j++) {
                dv[j].x += jx == j ? gx : 0.f;
                dv[j].y += jy == j ? gy : 0.f;
            }
            g2 = gn, o2 = on;
        }
        float *const dr = dy + r * P * FA_E + 2 * l;
#pragma unroll
        for (int j = 0; j < P; j++) *(float2 *)(dr + j * FA_E) = dv[j];
    }
    // the four waves in order -> one block per workgroup (every wave arrives here whatever its rows were)
    *(float2 *)(&comb[w][2 * l]) = make_float2(dbx, dby);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < FA_E) part[(size_t)blockIdx.x * FA_E + t] = ((comb[0][t] + comb[1][t]) + comb[2][t]) + comb[3][t];
}

// the partial blocks in order of workgroup -> db [128]
FA_KERNEL __launch_bounds__(128) void k_fcra_pool_reduce(const float *__restrict__ part, int G, float *__restrict__ db) {
    const int t = threadIdx.x;
    float s = 0.f;
    for (int g = 0; g < G; g++) s += part[(size_t)g * FA_E + t];
    db[t] = s;
}

inline int launch_fcra_pool_fwd(const FpJobs &jobs, int n_jobs, int64_t R, int P, const float *adj, int64_t adj_rs, int64_t out_ld, int max_blocks,
                                hipStream_t st) {
    const dim3 grid(fa_grid(R, 8, 1 << 16, max_blocks), n_jobs), block(64 * FA_WAVES);
#define FP_FWD(N) hipLaunchKernelGGL(k_fcra_pool_fwd<N>, grid, block, 0, st, jobs, R, adj, adj_rs, out_ld)
    FA_FOR_P(P, FP_FWD)
#undef FP_FWD
    return (int)hipGetLastError();
}

inline int launch_fcra_pool_bwd(int64_t R, int P, const float *y, const float *adj, int64_t adj_rs, const float *out, int64_t out_ld,
                                const float *g, int64_t g_ld, float *dy, float *db, float *part, int max_blocks, hipStream_t st) {
    const int G = fa_grid(R, 4, FA_MAX_GRID, max_blocks);
    const dim3 grid(G), block(64 * FA_WAVES);
#define FP_BWD(N) hipLaunchKernelGGL(k_fcra_pool_bwd<N>, grid, block, 0, st, y, adj, adj_rs, out, out_ld, g, g_ld, R, dy, part)
    FA_FOR_P(P, FP_BWD)
#undef FP_BWD
    hipLaunchKernelGGL(k_fcra_pool_reduce, dim3(1), dim3(FA_E), 0, st, (const float *)part, G, db);
    return (int)hipGetLastError();
}
