// fcra_team.hpp -- the FCRA hop aggregators for LARGE TEAMS (17 .. 64 pursuers; the entry points take 1 .. 64): the attention aggregator
// of fcra_att.hpp and the neighbour mean of fcra_neighbour_mean as a batched small GEMM on the fp32 matrix pipe (C ABI:
// include/mappo_ops.h fcra_team_fwd_multi / fcra_team_bwd).  E = 128 only.
//
//   att    y_j = W h_j (the caller's GEMM)      s_j = alpha . leaky_relu(y_j + b, 0.01)      listed j for i: a_ij != 0
//          u_ij = a_ij exp(s_j - max over listed j of s_j)      w_ij = u_ij / sum_j |u_ij|      out_i = relu(b + sum_j w_ij y_j)
//          nothing listed -> relu(b)
//   mean   w_ij = a_ij / max(sum_j |a_ij|, 1e-12)               out_i = [relu](sum_j w_ij y_j [+ b])        (no alpha; forward only)
//
// Per row the hop is out = Wt (P x P) times Y (P x 128): above 16 pursuers neither 2 P registers of operands per lane nor one lane per
// pair (fcra_att.hpp) are to be had.  Here a ROW is owned by a WORKGROUP of four waves, persistent over the rows:
//   stage    wave v fetches the vectors j = v, v + 4, .. (one 512-byte vector a load, all loads of the row in flight together) into the
//            LDS block Y [16 MT][144] (MT = ceil(P / 16) tiles; rows P .. 16 MT - 1 are zeros) and forms the score partials on the
//            way; fa_reduce_t (fcra_att.hpp) sums the wave's up to 16 scores across the lanes.                     -- lds_barrier --
//   weights  wave v builds the segments i = v, v + 4, ..: lane j holds a_ij and s_j, the maximum and the sum of |u| are xor
//            butterflies (a + b == b + a: every lane ends with the same bits), w_ij goes to the LDS block Wt [16 MT][68]; rows and
//            columns P .. are exact zeros.                                                                         -- lds_barrier --
//   product  v_mfma_f32_16x16x4_f32, fp32 operands (a chain of round-to-nearest FMAs: sb_common.hpp).  Wave v owns features
//            32 v .. 32 v + 31 (two N tiles) for all MT tiles of segments: per K step of four neighbours two B reads and MT A reads
//            (ds_read_b32) feed 2 MT matrix instructions.  The row strides (144 and 68 floats) put the 64 lanes of every such read
//            into 64 different banks.  The epilogue adds the bias, applies the ReLU and stores 64-byte runs.        -- lds_barrier --
// One launch serves several hops x {actor, critic} (grid.y = jobs); a job whose actor and critic read the same vectors stages and
// scores once.  The mean mode reads a (n, T, P, E) history slice in place.
//
// The backward (att) saves nothing beyond `out`: s and w are recomputed by the forward's functions.  With gp_i = [out_i > 0] g_i,
// gd_i = gp_i . (out_i - b) (= gp_i . o_i: gp_i is zero wherever out_i is) and t = Wt^T gp -- the SECOND matrix-pipe product, its A
// operand the weights written transposed, its B operand gp staged like Y --
//   S_j = t_j . y_j - sum_i |w_ij| gd_i            dy_j = t_j + S_j alpha leaky'(y_j + b)
// t stays in the accumulators; t_j . y_j is reduced over the 16 lanes of a tile row and over the four waves in order through LDS.
// db and d_alpha are kept per lane over all the workgroup's rows, combined in a fixed order into one partial block per workgroup, and
// k_fcra_att_reduce (fcra_att.hpp) adds the blocks in order of workgroup.  No atomics; a row's bits depend on that row only.
#pragma once
#include "fcra_att.hpp"
#include "sb_common.hpp"

constexpr int FT_E = FA_E;
constexpr int FT_MAX_P = 64;
constexpr int FT_WAVES = 4;
constexpr int FT_YS = FT_E + 16;              // row stride of the vector blocks: 16 mod 64 banks, four K rows of 16 features never meet
constexpr int FT_WS = FT_MAX_P + 4;           // row stride of the weights: 4 mod 64 banks, 16 segments of four neighbours never meet
constexpr int FT_MAX_GRID = FA_MAX_GRID;      // workgroups of the backward = partial blocks in its workspace
constexpr int FT_LDS_PER_CU = 160 * 1024;
constexpr int64_t FT_MAX_LD = 1 << 20;       // out / g vector strides: a row's offsets are 32-bit

typedef float ft_f32x4 __attribute__((ext_vector_type(4)));

struct FtJobs { mo_fcra_team_job j[MO_FCRA_TEAM_MAX_JOBS]; };

template <int MT>
struct alignas(16) FtLds {
    float y[16 * MT][FT_YS];                  // the row's vectors
    float w[16 * MT][FT_WS];                  // Wt[i][j] (forward) or its transpose (backward)
    float s[FT_MAX_P];
};
template <int MT>
struct alignas(16) FtLdsBwd {
    FtLds<MT> f;
    float g[16 * MT][FT_YS];                  // gp
    float gd[FT_MAX_P], S[FT_MAX_P], ty[FT_WAVES][FT_MAX_P];
    float comb[3][FT_WAVES][FT_E];            // db of the staging lanes | db of the epilogue lanes | d_alpha
};

__device__ __forceinline__ float ft_wave_max(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m));
    return x;
}
__device__ __forceinline__ float ft_wave_sum(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);   // a + b == b + a: the same bits in both partners
    return x;
}

// Row indices of the staging and weight loops: `v` is the wave's index as a VECTOR value (not readfirstlane'd), so that the addresses of
// the up to 16 loads of a loop are one scalar base + a 32-bit lane offset each, not 16 scalar pointers (which were spilled); a row
// index past P - 1 is clamped for the load and the value replaced by zero: straight-line code, every load of the row in flight.
__device__ __forceinline__ float2 ft_load2(const float *__restrict__ base, int i, int P, unsigned ld, int l) {
    const float2 x = *(const float2 *)(base + ((unsigned)min(i, P - 1) * ld + 2u * l));
    return i < P ? x : make_float2(0.f, 0.f);
}

// the vectors j = v, v + 4, .. of one row -> dst (rows P .. 16 MT - 1: zeros); SCORE: s_j -> s (visible after the next barrier)
template <int MT, bool SCORE>
__device__ __forceinline__ void ft_stage(const float *__restrict__ yrow, int P, float2 b2, float2 al2, int v, int l, float (*dst)[FT_YS], float *s) {
    constexpr int NI = 4 * MT, V = fa_pow2(NI);
    float2 x[NI];
#pragma unroll
    for (int it = 0; it < NI; it++) x[it] = ft_load2(yrow, v + 4 * it, P, FT_E, l);
    float ps[V];
#pragma unroll
    for (int k = 0; k < V; k++) ps[k] = 0.f;
#pragma unroll
    for (int it = 0; it < NI; it++) {
        *(float2 *)(&dst[v + 4 * it][2 * l]) = x[it];
        if (SCORE) ps[it] = fmaf(al2.y, fa_leaky(x[it].y + b2.y), al2.x * fa_leaky(x[it].x + b2.x));
    }
    if (SCORE) {
        const float tot = fa_reduce_t<V>(ps, l);
        const int slot = fa_slot<V>(l);
        if (l < V && slot < NI) s[v + 4 * slot] = tot;          // (a score of a padding row is never listed)
    }
}

// s and the adjacency row (NULL: ones) -> the weights of segments i = v, v + 4, ..; lane = neighbour j.  TRANS: w[j][i], else w[i][j].
template <int MT, bool ATT, bool TRANS>
__device__ __forceinline__ void ft_weights(const float *__restrict__ adj_row, int P, int v, int l, float (*wt)[FT_WS], const float *s) {
    constexpr int NI = 4 * MT;
    const float sj = s[l];
    float a[NI];
#pragma unroll
    for (int it = 0; it < NI; it++) {
        const int i = v + 4 * it;
        a[it] = adj_row ? adj_row[(unsigned)(min(i, P - 1) * P + min(l, P - 1))] : 1.f;
        if (i >= P || l >= P) a[it] = 0.f;
    }
#pragma unroll
    for (int it = 0; it < NI; it++) {
        const int i = v + 4 * it;
        float u = a[it], wv;
        if (ATT) {
            const bool listed = u != 0.f;
            const float mx = ft_wave_max(listed ? sj : -INFINITY);
            u = listed ? u * expf(sj - mx) : 0.f;
            const float den = ft_wave_sum(fabsf(u));
            wv = den > 0.f ? u / den : 0.f;                      // nothing listed: zeros, pre_i = b
        } else {
            wv = u / fmaxf(ft_wave_sum(fabsf(u)), 1e-12f);       // F.normalize(adj, p = 1)
        }
        if (TRANS) {
            if (l < 16 * MT) wt[l][i] = wv;
        } else {
            wt[i][l] = wv;
        }
    }
}

// acc[m][n] (16 x 16 tiles: rows 16 m .., features 32 v + 16 n ..) = A [16 MT][4 KT] times B [4 KT][128]
template <int MT>
__device__ __forceinline__ void ft_mma(const float (*A)[FT_WS], const float (*B)[FT_YS], int KT, int v, int l, ft_f32x4 (&acc)[MT][2]) {
    const int c = l & 15, q = l >> 4;
#pragma unroll
    for (int m = 0; m < MT; m++) acc[m][0] = acc[m][1] = ft_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < KT; k++) {
        const float b0 = B[4 * k + q][32 * v + c], b1 = B[4 * k + q][32 * v + 16 + c];
#pragma unroll
        for (int m = 0; m < MT; m++) {
            const float a = A[16 * m + c][4 * k + q];
            acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[m][0], 0, 0, 0);
            acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[m][1], 0, 0, 0);
        }
    }
}

// out_i = act(b + acc): an accumulator register r of lane (q, c) is row 16 m + 4 q + r, feature 32 v + 16 n + c
template <int MT>
__device__ __forceinline__ void ft_store_out(const ft_f32x4 (&acc)[MT][2], const float (&bf)[2], bool relu, int P, int v, int l, float *__restrict__ o,
                                             int64_t ld) {
    const int c = l & 15, q = l >> 4;
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = 16 * m + 4 * q + r;
            if (i < P) {
#pragma unroll
                for (int n = 0; n < 2; n++) {
                    const float pre = bf[n] + acc[m][n][r];
                    o[i * ld + 32 * v + 16 * n + c] = relu ? fmaxf(pre, 0.f) : pre;
                }
            }
        }
}

// grid (persistent workgroups, jobs).  Row r = (r / T, r % T) of a history slice starts at (r / T) es + (r % T) ss.
template <int MT, bool ATT>
FA_KERNEL __launch_bounds__(64 * FT_WAVES) void k_fcra_team_fwd(FtJobs jobs, int64_t R, int P_, int T, int64_t ya_es, int64_t ya_ss, int64_t yc_es,
                                                                  int64_t yc_ss, const float *__restrict__ adj, int64_t adj_rs, int relu, int64_t out_ld) {
    __shared__ FtLds<MT> L;
    const int vv = threadIdx.x >> 6, v = __builtin_amdgcn_readfirstlane(vv), l = threadIdx.x & 63, c = l & 15;
    const mo_fcra_team_job &job = jobs.j[blockIdx.y];
    float2 b2 = make_float2(0.f, 0.f), al2 = b2;
    float bf[2] = {0.f, 0.f};
    if (job.bias) b2 = *(const float2 *)(job.bias + 2 * l), bf[0] = job.bias[32 * v + c], bf[1] = job.bias[32 * v + 16 + c];
    if (ATT) al2 = *(const float2 *)(job.alpha + 2 * l);
    const bool shared = job.out_actor && job.out_critic && job.y_actor == job.y_critic && ya_es == yc_es && ya_ss == yc_ss;
    ft_f32x4 acc[MT][2];
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        int P = P_;
        asm volatile("" : "+s"(P));   // anew every row: the unrolled loops' comparisons with P are no invariants of the row loop to be kept in (and spilled from) scalar registers
        const int64_t n = r / T, t = r - n * T;
        if (job.out_actor) {
            ft_stage<MT, ATT>(job.y_actor + n * ya_es + t * ya_ss, P, b2, al2, vv, l, L.y, L.s);
            lds_barrier();
            ft_weights<MT, ATT, false>(adj + r * adj_rs, P, vv, l, L.w, L.s);
            lds_barrier();
            ft_mma<MT>(L.w, L.y, (P + 3) / 4, v, l, acc);
            ft_store_out<MT>(acc, bf, relu, P, v, l, job.out_actor + r * P * out_ld, out_ld);
            lds_barrier();
        }
        if (job.out_critic) {
            if (!shared) {
                ft_stage<MT, ATT>(job.y_critic + n * yc_es + t * yc_ss, P, b2, al2, vv, l, L.y, L.s);
                lds_barrier();
            }
            ft_weights<MT, ATT, false>(nullptr, P, vv, l, L.w, L.s);
            lds_barrier();
            ft_mma<MT>(L.w, L.y, (P + 3) / 4, v, l, acc);
            ft_store_out<MT>(acc, bf, relu, P, v, l, job.out_critic + r * P * out_ld, out_ld);
            lds_barrier();
        }
    }
}

// dy [R][P][128] dense; part: [gridDim.x][256] floats, a block = db [128] | d_alpha [128].  adj NULL: ones.
template <int MT>
FA_KERNEL __launch_bounds__(64 * FT_WAVES) void k_fcra_team_bwd(const float *__restrict__ y, const float *__restrict__ adj, int64_t adj_rs,
                                                                  const float *__restrict__ bias, const float *__restrict__ alpha,
                                                                  const float *__restrict__ out, int64_t out_ld, const float *__restrict__ g, int64_t g_ld,
                                                                  int64_t R, int P_, float *__restrict__ dy, float *__restrict__ part) {
    constexpr int NI = 4 * MT, V = fa_pow2(NI);
    __shared__ FtLdsBwd<MT> L;
    const int vv = threadIdx.x >> 6, v = __builtin_amdgcn_readfirstlane(vv), l = threadIdx.x & 63, c = l & 15, q = l >> 4;
    const float2 b2 = *(const float2 *)(bias + 2 * l), al2 = *(const float2 *)(alpha + 2 * l);
    float bf[2], af[2], dbk[2] = {0.f, 0.f}, dal[2] = {0.f, 0.f}, dbx = 0.f, dby = 0.f;
#pragma unroll
    for (int n = 0; n < 2; n++) bf[n] = bias[32 * v + 16 * n + c], af[n] = alpha[32 * v + 16 * n + c];
    ft_f32x4 acc[MT][2];
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        int P = P_;
        asm volatile("" : "+s"(P));   // (as in the forward)
        ft_stage<MT, true>(y + r * P * FT_E, P, b2, al2, vv, l, L.f.y, L.f.s);
        {   // gp_i = [out_i > 0] g_i -> L.g; gd_i = gp_i . (out_i - b); db += gp_i
            const float *const gr = g + r * P * g_ld, *const orow = out + r * P * out_ld;
            float2 gv[NI], ov[NI];
#pragma unroll
            for (int it = 0; it < NI; it++) {
                gv[it] = ft_load2(gr, vv + 4 * it, P, (unsigned)g_ld, l), ov[it] = ft_load2(orow, vv + 4 * it, P, (unsigned)out_ld, l);
            }
            float pd[V];
#pragma unroll
            for (int k = 0; k < V; k++) pd[k] = 0.f;
#pragma unroll
            for (int it = 0; it < NI; it++) {
                const float gx = ov[it].x > 0.f ? gv[it].x : 0.f, gy = ov[it].y > 0.f ? gv[it].y : 0.f;
                *(float2 *)(&L.g[vv + 4 * it][2 * l]) = make_float2(gx, gy);
                dbx += gx;
                dby += gy;
                pd[it] = fmaf(gy, ov[it].y - b2.y, gx * (ov[it].x - b2.x));
            }
            const float gd = fa_reduce_t<V>(pd, l);
            const int slot = fa_slot<V>(l);
            if (l < V && slot < NI) L.gd[vv + 4 * slot] = gd;
        }
        lds_barrier();
        ft_weights<MT, true, true>(adj ? adj + r * adj_rs : nullptr, P, vv, l, L.f.w, L.f.s);
        lds_barrier();
        ft_mma<MT>(L.f.w, L.g, (P + 3) / 4, v, l, acc);                                                  // t = Wt^T gp
        // t_j . y_j: this wave's 32 features of every j, the 16 lanes of a tile row, then the four waves in order
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int j = 16 * m + 4 * q + rr;
                float d = fmaf(acc[m][1][rr], L.f.y[j][32 * v + 16 + c], acc[m][0][rr] * L.f.y[j][32 * v + c]);
#pragma unroll
                for (int x = 1; x < 16; x <<= 1) d += __shfl_xor(d, x);
                if (c == 0) L.ty[v][j] = d;
            }
        lds_barrier();
        if (v == 0 && l < P) {
            float s = 0.f;
            for (int i = 0; i < P; i++) s = fmaf(fabsf(L.f.w[l][i]), L.gd[i], s);
            L.S[l] = (((L.ty[0][l] + L.ty[1][l]) + L.ty[2][l]) + L.ty[3][l]) - s;
        }
        lds_barrier();
        float *const dr = dy + r * P * FT_E;
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int j = 16 * m + 4 * q + rr;
                if (j < P) {
                    const float S = L.S[j];
#pragma unroll
                    for (int n = 0; n < 2; n++) {
                        const int f = 32 * v + 16 * n + c;
                        const float z = L.f.y[j][f] + bf[n], k = S * af[n] * (z > 0.f ? 1.f : FA_SLOPE);
                        dr[j * FT_E + f] = acc[m][n][rr] + k;
                        dbk[n] += k;
                        dal[n] = fmaf(S, fa_leaky(z), dal[n]);
                    }
                }
            }
        lds_barrier();
    }
    // one block per workgroup, every addend in a fixed place and order
    *(float2 *)(&L.comb[0][v][2 * l]) = make_float2(dbx, dby);
#pragma unroll
    for (int n = 0; n < 2; n++) L.comb[1][q][32 * v + 16 * n + c] = dbk[n], L.comb[2][q][32 * v + 16 * n + c] = dal[n];
    __syncthreads();
    const int t = threadIdx.x, f = t & (FT_E - 1);
    const float (*const cb)[FT_E] = L.comb[t < FT_E ? 1 : 2];
    float tot = ((cb[0][f] + cb[1][f]) + cb[2][f]) + cb[3][f];
    if (t < FT_E) tot += ((L.comb[0][0][f] + L.comb[0][1][f]) + L.comb[0][2][f]) + L.comb[0][3][f];
    part[(size_t)blockIdx.x * (2 * FT_E) + t] = tot;
}

inline int ft_grid(int64_t R, size_t lds_bytes, int cap, int max_blocks) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    int per_cu = (int)(FT_LDS_PER_CU / lds_bytes);
    if (per_cu > 8) per_cu = 8;
    int64_t lim = (int64_t)per_cu * cus;
    if (lim > cap) lim = cap;
    if (max_blocks > 0 && lim > max_blocks) lim = max_blocks;
    return (int)(R < lim ? R : lim);
}

// one instantiation per number of 16-segment tiles
#define FT_FOR_MT(P, CALL) \
    switch (((P) + 15) / 16) { \
        case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; \
        default: return MO_ERR_BAD_ARG; \
    }

inline int launch_fcra_team_fwd(const FtJobs &jobs, int n_jobs, bool att, int64_t R, int P, int T, int64_t ya_es, int64_t ya_ss, int64_t yc_es,
                                int64_t yc_ss, const float *adj, int64_t adj_rs, int relu, int64_t out_ld, int max_blocks, hipStream_t st) {
    const dim3 block(64 * FT_WAVES);
#define FT_FWD(N) \
    { \
        const dim3 grid(ft_grid(R, sizeof(FtLds<N>), 1 << 16, max_blocks), n_jobs); \
        if (att) hipLaunchKernelGGL((k_fcra_team_fwd<N, true>), grid, block, 0, st, jobs, R, P, T, ya_es, ya_ss, yc_es, yc_ss, adj, adj_rs, relu, out_ld); \
        else hipLaunchKernelGGL((k_fcra_team_fwd<N, false>), grid, block, 0, st, jobs, R, P, T, ya_es, ya_ss, yc_es, yc_ss, adj, adj_rs, relu, out_ld); \
    }
    FT_FOR_MT(P, FT_FWD)
#undef FT_FWD
    return (int)hipGetLastError();
}

inline int launch_fcra_team_bwd(int64_t R, int P, const float *y, const float *adj, int64_t adj_rs, const float *bias, const float *alpha, const float *out,
                                int64_t out_ld, const float *g, int64_t g_ld, float *dy, float *db, float *d_alpha, float *part, int max_blocks,
                                hipStream_t st) {
    int G = 0;
#define FT_BWD(N) \
    { \
        G = ft_grid(R, sizeof(FtLdsBwd<N>), FT_MAX_GRID, max_blocks); \
        hipLaunchKernelGGL(k_fcra_team_bwd<N>, dim3(G), dim3(64 * FT_WAVES), 0, st, y, adj, adj_rs, bias, alpha, out, out_ld, g, g_ld, R, P, dy, part); \
    }
    FT_FOR_MT(P, FT_BWD)
#undef FT_BWD
    hipLaunchKernelGGL(k_fcra_att_reduce, dim3(1), dim3(2 * FA_E), 0, st, (const float *)part, G, db, d_alpha);
    return (int)hipGetLastError();
}
