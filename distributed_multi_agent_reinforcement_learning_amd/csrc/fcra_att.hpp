// fcra_att.hpp -- DHGN's ATTENTION aggregator for the FCRA hops (`algo.fcra_aggregator: att`): a softmax over the team-mates' stored
// embeddings of one hop in place of the neighbour mean (C ABI: include/mappo_ops.h fcra_att_fwd_multi / fcra_att_bwd).
//
//   y_j = W h_j (the caller's GEMM, no bias)        s_j = alpha . leaky_relu(y_j + b, 0.01)         one score per (row, j)
//   listed j for i: a_ij != 0      M_i = max over listed j of s_j      u_ij = a_ij exp(s_j - M_i)      w_ij = u_ij / sum_j |u_ij|
//   out_i = relu(b + sum_j w_ij y_j)                nothing listed -> relu(b);  alpha = 0 -> relu(normalize(a, p = 1) @ y + b)
//
// The unit of work is a ROW (one environment or environment-step: P vectors of 128 floats).  ONE WAVE owns a row; four waves of a
// persistent 256-thread workgroup stride over the rows.  Lane l holds features 2 l, 2 l + 1 of all P vectors y_j in registers for
// the whole row (2 P VGPRs), so y is read from HBM once.  Per row:
//   scores   every lane forms its partial of the P dots; a TRANSPOSING butterfly reduces them (step t exchanges half of the live
//            values with lane ^ 2^t and keeps the other half: V - 1 + 6 - log2 V cross-lane moves for V values instead of 6 V; the
//            remaining steps are a plain xor butterfly, so every lane that ends with score j holds the same bits) -> the wave's LDS patch
//   weights  one lane per pair (i, j) (P^2 <= 256: up to four pairs a lane): the lane walks segment i's listed scores for M_i, takes
//            ONE exp, parks u_ij, walks segment i's u for the sum, parks w_ij.  Lanes of one segment walk in the same order: same bits.
//   sums     lanes = features again: out_i = relu(b + sum_j w_ij y_j) as FMAs from registers, w broadcast from LDS.
// No workgroup barrier sits inside the row loop (a wave's LDS operations complete in order), so empty and ragged rows leave no
// lane behind.  Nothing per pair reaches HBM; no atomics; a row's bits depend on that row's inputs only.
//
// The backward saves nothing beyond `out` (read for the sign of pre): s, u, w are recomputed by the same functions.  With
// gp_i = [out_i > 0] g_i, o_i = sum_j w_ij y_j and t_j = sum_i w_ij gp_i (the first half of dy_j, needed anyway) the P^2 dots
// c_ij = gp_i . y_j of the specification are never formed: sum_j' w_ij' c_ij' = gp_i . o_i =: gd_i and sum_i w_ij c_ij = t_j . y_j, so
//   S_j = sum_i ds_ij = t_j . y_j - sum_i |w_ij| gd_i
// costs 2 P dots (two transposing butterflies) instead of P^2.  dy_j = t_j + S_j alpha leaky'(y_j + b); db and d_alpha are kept per
// lane over all the wave's rows, the four waves are added in order through LDS into one partial block per workgroup, and
// k_fcra_att_reduce adds the blocks in order of workgroup.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mappo_ops.h"

constexpr int FA_E = 128;                     // the only width
constexpr int FA_MAX_P = 16;
constexpr int FA_WAVES = 4;                   // rows in flight per workgroup
constexpr int FA_MAX_GRID = 1024;             // workgroups of the backward = partial blocks in its workspace
constexpr float FA_SLOPE = 0.01f;             // LeakyReLU

// The packed fp32 VALU forms stay out of these kernels: a per-kernel target feature, device pass only.
#if defined(__HIP_DEVICE_COMPILE__)
#define FA_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define FA_KERNEL __global__
#endif

// a wave's own LDS: adjacency row, u, w of the P^2 pairs; scores; the backward's gd_i, t_j . y_j and S_j
struct alignas(16) FaPatch {
    float a[FA_MAX_P * FA_MAX_P], u[FA_MAX_P * FA_MAX_P], w[FA_MAX_P * FA_MAX_P];
    float s[FA_MAX_P], gd[FA_MAX_P], ty[FA_MAX_P], S[FA_MAX_P];
};
struct FaJobs { mo_fcra_att_job j[MO_FCRA_ATT_MAX_JOBS]; };

__device__ __forceinline__ void fa_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }   // a wave's LDS operations complete in order
// (slope < 1: the larger of z and slope z is the LeakyReLU; no comparison whose lane mask would be kept from the scores to the last loop)
__device__ __forceinline__ float fa_leaky(float z) { return fmaxf(z, FA_SLOPE * z); }

// V values per lane, summed over the 64 lanes -> the lane's return value is the total of value fa_slot<V>(l)
template <int V>
__device__ __forceinline__ float fa_reduce_t(float (&v)[V], int l) {
    int bit = 1;
#pragma unroll
    for (int h = V / 2; h >= 1; h >>= 1, bit <<= 1) {
        const bool up = (l & bit) != 0;       // this lane keeps the upper half of what is live and hands the lower half over
#pragma unroll
        for (int k = 0; k < h; k++) {
            float lo = v[k], hi = v[k + h];
            asm volatile("" : "+v"(lo), "+v"(hi));   // two plain registers: a select between elements of one array becomes a select of the INDEX and a V-way chain
            v[k] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, bit);
        }
    }
    float x = v[0];
#pragma unroll
    for (int m = V; m < 64; m <<= 1) x += __shfl_xor(x, m);   // a + b == b + a: the same bits in both partners
    return x;
}
// which value a lane ends with: lane bit t chose half t, the most significant index bit first
template <int V>
__device__ __forceinline__ int fa_slot(int l) {
    int j = 0, bit = 1;
#pragma unroll
    for (int h = V / 2; h >= 1; h >>= 1, bit <<= 1)
        if (l & bit) j |= h;
    return j;
}

constexpr int fa_pow2(int p) { return p <= 1 ? 1 : 2 * fa_pow2((p + 1) / 2); }   // the butterfly's width for P values

// The team size P is a template parameter (1 .. 16, one instantiation each): every loop over j is unrolled over exactly P registers and
// every LDS offset is an immediate.  (With P a kernel argument and loops predicated by j < P the compiler kept one lane mask per j in
// scalar registers across the row loop and spilled them.)
template <int P>
__device__ __forceinline__ void fa_load(const float *__restrict__ y, int64_t r, int l, float2 (&yv)[P]) {
    const float *const base = y + r * P * FA_E + 2 * l;
#pragma unroll
    for (int j = 0; j < P; j++) yv[j] = *(const float2 *)(base + j * FA_E);
}

// s_j of the row -> pt.s (visible after the next fa_wave_sync)
template <int P>
__device__ __forceinline__ void fa_scores(const float2 (&yv)[P], float2 b2, float2 al2, int l, FaPatch &pt) {
    constexpr int V = fa_pow2(P);
    float ps[V];
#pragma unroll
    for (int j = 0; j < V; j++) ps[j] = 0.f;
#pragma unroll
    for (int j = 0; j < P; j++) ps[j] = fmaf(al2.y, fa_leaky(yv[j].y + b2.y), al2.x * fa_leaky(yv[j].x + b2.x));
    const float tot = fa_reduce_t<V>(ps, l);
    const int j = fa_slot<V>(l);
    if (l < V && j < P) pt.s[j] = tot;
}

// pt.s and the adjacency row (NULL: ones) -> pt.w, visible on return.  One lane per pair; the patch keeps pair (i, j) at i FA_MAX_P + j,
// so that a segment's weights are whole float4s for the feature lanes.
template <int P>
__device__ __forceinline__ void fa_weights(const float *__restrict__ adj_row, int l, FaPatch &pt) {
#pragma unroll 1
    for (int q = l; q < P * P; q += 64) {
        const int i = q / P;
        pt.a[i * FA_MAX_P + q - i * P] = adj_row ? adj_row[q] : 1.f;
    }
    fa_wave_sync();
#pragma unroll 1
    for (int q = l; q < P * P; q += 64) {
        const int i = q / P, j = q - i * P;
        const float *const ar = pt.a + i * FA_MAX_P;
        float mx = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < P; jj++)
            if (ar[jj] != 0.f) mx = fmaxf(mx, pt.s[jj]);
        pt.u[i * FA_MAX_P + j] = ar[j] != 0.f ? ar[j] * expf(pt.s[j] - mx) : 0.f;
    }
    fa_wave_sync();
#pragma unroll 1
    for (int q = l; q < P * P; q += 64) {
        const int i = q / P, j = q - i * P;
        const float *const ur = pt.u + i * FA_MAX_P;
        float den = 0.f;
#pragma unroll
        for (int jj = 0; jj < P; jj++) den += fabsf(ur[jj]);
        pt.w[i * FA_MAX_P + j] = den > 0.f ? ur[j] / den : 0.f;      // nothing listed: zeros, pre_i = b
    }
    fa_wave_sync();
}

// segment i's weights w_i. -> registers (whole float4s: what lies behind entry P - 1 is not the row's and is never used)
template <int P>
__device__ __forceinline__ void fa_wrow(const FaPatch &pt, int i, float (&wr)[(P + 3) / 4 * 4]) {
#pragma unroll
    for (int c = 0; c < (P + 3) / 4; c++) {
        const float4 t = *(const float4 *)(pt.w + i * FA_MAX_P + 4 * c);
        wr[4 * c] = t.x, wr[4 * c + 1] = t.y, wr[4 * c + 2] = t.z, wr[4 * c + 3] = t.w;
    }
}

// out_i = relu(b + sum_j w_ij y_j) for the row's P segments; o: the row's first output vector + 2 l
template <int P>
__device__ __forceinline__ void fa_store_out(const float2 (&yv)[P], float2 b2, const FaPatch &pt, float *__restrict__ o, int64_t ld) {
#pragma unroll 2
    for (int i = 0; i < P; i++) {
        float wr[(P + 3) / 4 * 4], ax = 0.f, ay = 0.f;
        fa_wrow<P>(pt, i, wr);
#pragma unroll
        for (int j = 0; j < P; j++) {
            ax = fmaf(wr[j], yv[j].x, ax);
            ay = fmaf(wr[j], yv[j].y, ay);
        }
        *(float2 *)(o + i * ld) = make_float2(fmaxf(b2.x + ax, 0.f), fmaxf(b2.y + ay, 0.f));
    }
}

// grid (row groups, jobs).  A job's actor reads adj, its critic ones; when both read the same y the scores are evaluated once.
template <int P>
FA_KERNEL __launch_bounds__(256) void k_fcra_att_fwd(FaJobs jobs, int64_t R, const float *__restrict__ adj, int64_t adj_rs, int64_t out_ld) {
    __shared__ FaPatch patch[FA_WAVES];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's row index stays scalar)
    FaPatch &pt = patch[w];
    const mo_fcra_att_job &job = jobs.j[blockIdx.y];
    const float2 b2 = *(const float2 *)(job.bias + 2 * l), al2 = *(const float2 *)(job.alpha + 2 * l);
    const bool shared = job.out_actor && job.out_critic && job.y_actor == job.y_critic;
    for (int64_t r = (int64_t)blockIdx.x * FA_WAVES + w; r < R; r += (int64_t)gridDim.x * FA_WAVES) {
        float2 yv[P];
        if (job.out_actor) {
            fa_load<P>(job.y_actor, r, l, yv);
            fa_scores<P>(yv, b2, al2, l, pt);
            fa_weights<P>(adj + r * adj_rs, l, pt);
            fa_store_out<P>(yv, b2, pt, job.out_actor + r * P * out_ld + 2 * l, out_ld);
        }
        if (job.out_critic) {
            if (!shared) {
                fa_load<P>(job.y_critic, r, l, yv);
                fa_scores<P>(yv, b2, al2, l, pt);
            }
            fa_weights<P>(nullptr, l, pt);
            fa_store_out<P>(yv, b2, pt, job.out_critic + r * P * out_ld + 2 * l, out_ld);
        }
    }
}

// dy [R][P][128] dense; part: [gridDim.x][256] floats, a block = db [128] | d_alpha [128].  adj NULL: ones.
template <int P>
FA_KERNEL __launch_bounds__(256) void k_fcra_att_bwd(const float *__restrict__ y, const float *__restrict__ adj, int64_t adj_rs,
                                                      const float *__restrict__ bias, const float *__restrict__ alpha, const float *__restrict__ out,
                                                      int64_t out_ld, const float *__restrict__ g, int64_t g_ld, int64_t R, float *__restrict__ dy,
                                                      float *__restrict__ part) {
    constexpr int V = fa_pow2(P);
    __shared__ FaPatch patch[FA_WAVES];
    __shared__ alignas(16) float comb[FA_WAVES][2 * FA_E];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's row index stays scalar)
    FaPatch &pt = patch[w];
    const float2 b2 = *(const float2 *)(bias + 2 * l), al2 = *(const float2 *)(alpha + 2 * l);
    float dbx = 0.f, dby = 0.f, dax = 0.f, day = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * FA_WAVES + w; r < R; r += (int64_t)gridDim.x * FA_WAVES) {
        float2 yv[P], tv[P];
        float pd[V];
        fa_load<P>(y, r, l, yv);
        fa_scores<P>(yv, b2, al2, l, pt);
        fa_weights<P>(adj ? adj + r * adj_rs : nullptr, l, pt);
#pragma unroll
        for (int j = 0; j < P; j++) tv[j] = make_float2(0.f, 0.f);
#pragma unroll
        for (int k = 0; k < V; k++) pd[k] = 0.f;
        const float *const gr = g + r * P * g_ld + 2 * l, *const orow = out + r * P * out_ld + 2 * l;
        // one segment a trip, not unrolled: unrolled, the P^2 LDS offsets and the 2 P row offsets of g and out are loop invariants of the
        // row loop that the compiler keeps in scalar registers, and spills.  The next segment's g and out are fetched a trip ahead.
        float2 g2 = *(const float2 *)gr, o2 = *(const float2 *)orow;
#pragma unroll 1
        for (int i = 0; i < P; i++) {
            float2 gn = g2, on = o2;
            if (i + 1 < P) gn = *(const float2 *)(gr + (i + 1) * g_ld), on = *(const float2 *)(orow + (i + 1) * out_ld);
            const float gx = o2.x > 0.f ? g2.x : 0.f, gy = o2.y > 0.f ? g2.y : 0.f;           // gp_i
            dbx += gx;
            dby += gy;
            float wr[(P + 3) / 4 * 4], ax = 0.f, ay = 0.f;                                     // o_i = sum_j w_ij y_j
            fa_wrow<P>(pt, i, wr);
#pragma unroll
            for (int j = 0; j < P; j++) {
                ax = fmaf(wr[j], yv[j].x, ax);
                ay = fmaf(wr[j], yv[j].y, ay);
                tv[j].x = fmaf(wr[j], gx, tv[j].x);
                tv[j].y = fmaf(wr[j], gy, tv[j].y);
            }
            const float d = fmaf(gy, ay, gx * ax);
#pragma unroll
            for (int k = 0; k + 1 < P; k++) pd[k] = pd[k + 1];   // a shift register: after P trips pd[i] is segment i's (no select by i, no lane masks)
            pd[P - 1] = d;
            g2 = gn, o2 = on;
        }
        const float gd = fa_reduce_t<V>(pd, l);                                                // gd_i = gp_i . o_i
#pragma unroll
        for (int k = 0; k < V; k++) pd[k] = 0.f;
#pragma unroll
        for (int j = 0; j < P; j++) pd[j] = fmaf(tv[j].y, yv[j].y, tv[j].x * yv[j].x);
        const float ty = fa_reduce_t<V>(pd, l);                                                // t_j . y_j
        const int slot = fa_slot<V>(l);
        if (l < V && slot < P) {
            pt.gd[slot] = gd;
            pt.ty[slot] = ty;
        }
        fa_wave_sync();
        if (l < P) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < P; i++) acc = fmaf(fabsf(pt.w[i * FA_MAX_P + l]), pt.gd[i], acc);
            pt.S[l] = pt.ty[l] - acc;
        }
        fa_wave_sync();
        float *const dr = dy + r * P * FA_E + 2 * l;
#pragma unroll
        for (int j = 0; j < P; j++) {
            const float S = pt.S[j], zx = yv[j].x + b2.x, zy = yv[j].y + b2.y;
            const float kx = S * al2.x * (zx > 0.f ? 1.f : FA_SLOPE), ky = S * al2.y * (zy > 0.f ? 1.f : FA_SLOPE);
            *(float2 *)(dr + j * FA_E) = make_float2(tv[j].x + kx, tv[j].y + ky);
            dbx += kx;
            dby += ky;
            dax = fmaf(S, fa_leaky(zx), dax);
            day = fmaf(S, fa_leaky(zy), day);
        }
    }
    // the four waves in order -> one block per workgroup (every wave arrives here whatever its rows were)
    *(float2 *)(&comb[w][2 * l]) = make_float2(dbx, dby);
    *(float2 *)(&comb[w][FA_E + 2 * l]) = make_float2(dax, day);
    __syncthreads();
    const int t = threadIdx.x;
    part[(size_t)blockIdx.x * (2 * FA_E) + t] = ((comb[0][t] + comb[1][t]) + comb[2][t]) + comb[3][t];
}

// the partial blocks in order of workgroup -> db [128], d_alpha [128]
FA_KERNEL __launch_bounds__(256) void k_fcra_att_reduce(const float *__restrict__ part, int G, float *__restrict__ db, float *__restrict__ d_alpha) {
    const int t = threadIdx.x;
    float s = 0.f;
    for (int g = 0; g < G; g++) s += part[(size_t)g * (2 * FA_E) + t];
    if (t < FA_E) db[t] = s;
    else d_alpha[t - FA_E] = s;
}

inline int fa_grid(int64_t R, int per_cu, int cap, int max_blocks) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    int64_t lim = (int64_t)per_cu * cus;
    if (lim > cap) lim = cap;
    if (max_blocks > 0 && lim > max_blocks) lim = max_blocks;
    const int64_t want = (R + FA_WAVES - 1) / FA_WAVES;
    return (int)(want < lim ? want : lim);
}

// one instantiation per team size
#define FA_FOR_P(P, CALL) \
    switch (P) { \
        case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break; \
        case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break; \
        case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break; \
        case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; case 16: CALL(16); break; \
        default: return MO_ERR_BAD_ARG; \
    }

inline int launch_fcra_att_fwd(const FaJobs &jobs, int n_jobs, int64_t R, int P, const float *adj, int64_t adj_rs, int64_t out_ld, int max_blocks,
                               hipStream_t st) {
    const dim3 grid(fa_grid(R, 8, 1 << 16, max_blocks), n_jobs), block(64 * FA_WAVES);
#define FA_FWD(N) hipLaunchKernelGGL(k_fcra_att_fwd<N>, grid, block, 0, st, jobs, R, adj, adj_rs, out_ld)
    FA_FOR_P(P, FA_FWD)
#undef FA_FWD
    return (int)hipGetLastError();
}

inline int launch_fcra_att_bwd(int64_t R, int P, const float *y, const float *adj, int64_t adj_rs, const float *bias, const float *alpha, const float *out,
                               int64_t out_ld, const float *g, int64_t g_ld, float *dy, float *db, float *d_alpha, float *part, int max_blocks,
                               hipStream_t st) {
    const int G = fa_grid(R, 4, FA_MAX_GRID, max_blocks);
    const dim3 grid(G), block(64 * FA_WAVES);
#define FA_BWD(N) hipLaunchKernelGGL(k_fcra_att_bwd<N>, grid, block, 0, st, y, adj, adj_rs, bias, alpha, out, out_ld, g, g_ld, R, dy, part)
    FA_FOR_P(P, FA_BWD)
#undef FA_BWD
    hipLaunchKernelGGL(k_fcra_att_reduce, dim3(1), dim3(2 * FA_E), 0, st, (const float *)part, G, db, d_alpha);
    return (int)hipGetLastError();
}
