// layer_norm.hpp -- LayerNorm on the GRU features (`algo.use_layer_norm`): the normalisation the MAPPO recipe puts behind its recurrent
// layer, for actor and critic in ONE launch each way (C ABI: include/mappo_ops.h feat_norm_fwd_multi / feat_norm_bwd_multi; DESIGN
// section 7y).  Width 128 only.
//
//   y = weight (x - mean) / sqrt(var + eps) + bias      mean, var (biased) over the 128 features of a row: torch's F.layer_norm
//   backward, gw = g weight, xh = (x - mean) rstd:      dx = rstd (gw - mean(gw) - xh mean(gw xh)),  d_weight = sum_r g xh,  d_bias = sum_r g
//
// ONE WAVE owns a row: lane l holds features 2 l, 2 l + 1 as a float2, so a 512-byte row is one coalesced load per wave.  Four waves form
// a persistent 256-thread workgroup, the workgroups stride over the rows, grid.y is the job (= network).
//   forward   the mean is an xor butterfly over the 64 lanes (a + b == b + a: every lane ends with the same bits), the variance a second
//             butterfly over the CENTRED values the lanes hold -- two passes over registers, never E[x^2] - mean^2 -- and
//             rstd = 1 / sqrtf(var + eps).  No LDS, no barrier.  The kernel moves 1 KB a row and does nothing else, so what counts is the
//             loads in flight: the row loop is unrolled by FN_U and the FN_U loads of a trip are issued before the first reduction (a row
//             index past R - 1 is replaced by the trip's first row for the load and its store is skipped: straight-line code).  The
//             output goes through a row stride of its own and never in place (in the rollout x is the recurrent state).  Nothing is
//             saved for the backward.
//   backward  recomputes mean and rstd from x by the forward's own function (fn_stats), two more butterflies give mean(gw) and
//             mean(gw xh); d_weight and d_bias are kept per lane over all the wave's rows, the four waves are added in wave order through
//             LDS into one partial block of 256 floats per workgroup, and k_feat_norm_reduce adds the blocks in a fixed order (32 consecutive
//             runs of blocks per column, then the runs in order).
// No atomics: two runs give equal bits, and a row's dx depends on that row only.
#pragma once
#include "fcra_att.hpp"

constexpr int FN_E = FA_E;                    // the only width
constexpr int FN_WAVES = FA_WAVES;            // rows in flight per workgroup and trip of the unrolled loop: FN_WAVES * U
constexpr int FN_U = 4;                       // forward: rows of a wave in flight
constexpr int FN_UB = 2;                      // backward (two loads a row)
constexpr int FN_MAX_GRID = FA_MAX_GRID;      // workgroups of the backward = partial blocks per job in its workspace
constexpr int FN_RED_RUNS = 32, FN_RED_COLS = 32;   // the reduce kernel: consecutive runs of blocks per column, columns per workgroup

struct FnJobs { mo_feat_norm_job j[MO_FEAT_NORM_MAX_JOBS]; };

__device__ __forceinline__ float fn_wave_sum(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);   // a + b == b + a: the same bits in both partners
    return x;
}

// the row's mean and 1 / sqrt(var + eps) and the lane's centred pair; forward and backward call this and nothing else for them
__device__ __forceinline__ void fn_stats(float2 x, float eps, float2 &c, float &rstd) {
    const float mean = fn_wave_sum(x.x + x.y) * (1.f / FN_E);
    c = make_float2(x.x - mean, x.y - mean);
    const float var = fn_wave_sum(fmaf(c.x, c.x, c.y * c.y)) * (1.f / FN_E);
    rstd = 1.f / sqrtf(var + eps);
}

// grid (row groups, jobs)
FA_KERNEL __launch_bounds__(256) void k_feat_norm_fwd(FnJobs jobs, int64_t R, float eps) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's row index stays scalar)
    const mo_feat_norm_job &job = jobs.j[blockIdx.y];
    const float2 w2 = *(const float2 *)(job.weight + 2 * l), b2 = *(const float2 *)(job.bias + 2 * l);
    const float *const x = job.x + 2 * l;
    float *const y = job.y + 2 * l;
    const int64_t ldx = job.ldx, ldy = job.ldy, S = (int64_t)gridDim.x * FN_WAVES;
    for (int64_t r = (int64_t)blockIdx.x * FN_WAVES + w; r < R; r += FN_U * S) {
        float2 xv[FN_U];
#pragma unroll
        for (int u = 0; u < FN_U; u++) {      // all loads of the trip before the first reduction
            const int64_t ru = r + u * S;
            xv[u] = *(const float2 *)(x + (ru < R ? ru : r) * ldx);
        }
#pragma unroll
        for (int u = 0; u < FN_U; u++) {
            const int64_t ru = r + u * S;
            float2 c;
            float rstd;
            fn_stats(xv[u], eps, c, rstd);
            if (ru < R) *(float2 *)(y + ru * ldy) = make_float2(fmaf(c.x * rstd, w2.x, b2.x), fmaf(c.y * rstd, w2.y, b2.y));
        }
    }
}

// grid (row groups, jobs); part: [jobs][gridDim.x][256] floats, a block = d_weight | d_bias
FA_KERNEL __launch_bounds__(256) void k_feat_norm_bwd(FnJobs jobs, int64_t R, float eps, float *__restrict__ part) {
    __shared__ alignas(16) float comb[FN_WAVES][2 * FN_E];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;   // (the wave's row index stays scalar)
    const mo_feat_norm_job &job = jobs.j[blockIdx.y];
    const float2 w2 = *(const float2 *)(job.weight + 2 * l);
    const float *const x = job.x + 2 * l, *const g = job.g + 2 * l;
    float *const dx = job.dx + 2 * l;
    const int64_t ldx = job.ldx, ldg = job.ldg, lddx = job.lddx, S = (int64_t)gridDim.x * FN_WAVES;
    float2 dw = make_float2(0.f, 0.f), db = make_float2(0.f, 0.f);
    for (int64_t r = (int64_t)blockIdx.x * FN_WAVES + w; r < R; r += FN_UB * S) {
        float2 xv[FN_UB], gv[FN_UB];
#pragma unroll
        for (int u = 0; u < FN_UB; u++) {
            const int64_t ru = r + u * S, rc = ru < R ? ru : r;
            xv[u] = *(const float2 *)(x + rc * ldx);
            gv[u] = *(const float2 *)(g + rc * ldg);
        }
#pragma unroll
        for (int u = 0; u < FN_UB; u++) {
            const int64_t ru = r + u * S;
            float2 c;
            float rstd;
            fn_stats(xv[u], eps, c, rstd);
            const float2 xh = make_float2(c.x * rstd, c.y * rstd), gw = make_float2(gv[u].x * w2.x, gv[u].y * w2.y);
            const float m1 = fn_wave_sum(gw.x + gw.y) * (1.f / FN_E);
            const float m2 = fn_wave_sum(fmaf(gw.x, xh.x, gw.y * xh.y)) * (1.f / FN_E);
            if (ru < R) {                     // (a scalar condition: the whole wave takes it or not)
                *(float2 *)(dx + ru * lddx) = make_float2(rstd * ((gw.x - m1) - xh.x * m2), rstd * ((gw.y - m1) - xh.y * m2));
                dw.x = fmaf(gv[u].x, xh.x, dw.x);
                dw.y = fmaf(gv[u].y, xh.y, dw.y);
                db.x += gv[u].x;
                db.y += gv[u].y;
            }
        }
    }
    // the four waves in order -> one block per workgroup (every wave arrives here whatever its rows were)
    *(float2 *)(&comb[w][2 * l]) = dw;
    *(float2 *)(&comb[w][FN_E + 2 * l]) = db;
    __syncthreads();
    const int t = threadIdx.x;
    part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (2 * FN_E) + t] = ((comb[0][t] + comb[1][t]) + comb[2][t]) + comb[3][t];
}

// grid (2 FN_E / FN_RED_COLS, jobs), FN_RED_RUNS x FN_RED_COLS threads: a workgroup owns FN_RED_COLS of the 256 columns; run q adds its
// consecutive share of the job's G blocks in order of workgroup (independent loads, a short chain), thread (0, c) adds the runs in order
// through LDS -> d_weight [128], d_bias [128] (overwritten).  The order is a function of G alone.
FA_KERNEL __launch_bounds__(FN_RED_RUNS * FN_RED_COLS) void k_feat_norm_reduce(FnJobs jobs, const float *__restrict__ part, int G) {
    __shared__ float runs[FN_RED_RUNS][FN_RED_COLS + 1];
    const int c = threadIdx.x % FN_RED_COLS, q = threadIdx.x / FN_RED_COLS, col = blockIdx.x * FN_RED_COLS + c;
    const int per = (G + FN_RED_RUNS - 1) / FN_RED_RUNS, g0 = q * per, g1 = min(G, g0 + per);
    const float *const p = part + (size_t)blockIdx.y * G * (2 * FN_E) + col;
    float s = 0.f;
#pragma unroll 8
    for (int g = g0; g < g1; g++) s += p[(size_t)g * (2 * FN_E)];
    runs[q][c] = s;
    __syncthreads();
    if (q) return;
    float v = runs[0][c];
#pragma unroll
    for (int k = 1; k < FN_RED_RUNS; k++) v += runs[k][c];
    const mo_feat_norm_job &job = jobs.j[blockIdx.y];
    if (col < FN_E) job.d_weight[col] = v;
    else job.d_bias[col - FN_E] = v;
}

inline int launch_feat_norm_fwd(const FnJobs &jobs, int n_jobs, int64_t R, float eps, int max_blocks, hipStream_t st) {
    // (few rows: a workgroup per four rows, the unrolled trips' later rows are skipped; many: the full grid, FN_U rows a wave in flight)
    const dim3 grid(fa_grid(R, 8, 1 << 16, max_blocks), n_jobs), block(64 * FN_WAVES);
    hipLaunchKernelGGL(k_feat_norm_fwd, grid, block, 0, st, jobs, R, eps);
    return (int)hipGetLastError();
}

inline int launch_feat_norm_bwd(const FnJobs &jobs, int n_jobs, int64_t R, float eps, float *part, int max_blocks, hipStream_t st) {
    const int G = fa_grid(R, 4, FN_MAX_GRID, max_blocks);
    hipLaunchKernelGGL(k_feat_norm_bwd, dim3(G, n_jobs), dim3(64 * FN_WAVES), 0, st, jobs, R, eps, part);
    hipLaunchKernelGGL(k_feat_norm_reduce, dim3(2 * FN_E / FN_RED_COLS, n_jobs), dim3(FN_RED_RUNS * FN_RED_COLS), 0, st, jobs, (const float *)part, G);
    return (int)hipGetLastError();
}
