// value_norm.hpp -- algo.use_value_norm of the env_3d / env_n2n trainers: the value targets normalised by running statistics (the
// PopArt-style "ValueNorm" of the public MAPPO implementation; C ABI: include/mappo_ops.h gae_advnorm_vn / value_norm_update /
// value_norm_targets; DESIGN.md sections 7a, 7b; numpy restatement: tests/value_norm_ref.py).  Included once, from
// csrc/mappo_ops.hip after its anonymous namespace: it reuses that file's GAE statistics (GAE_BLOCKS, gae_block_sum, k_gae_center,
// k_gae_std, k_gae_norm).
//
// State: three f64 on the device, (m, q, d) = debiased running mean, running mean of squares and the debiasing term, all 0 at the
// start.  d == 0 is the identity (mean 0, std 1): the scan then takes the stored values as they are and its adv / v_target are
// k_gae_scan's bits (same expressions in the same order; test_value_norm_gpu pins it).  The f64 state arithmetic is written with
// contraction off, so it is the stated expressions rounded operation by operation, as numpy evaluates them.
#pragma once

namespace {

constexpr double VN_VAR_MIN = 1e-2;

// mean and std of the state: (0, 1) before the first update, else m / d and sqrt(max(q / d - mean^2, 1e-2))
__device__ __forceinline__ void vn_stats(const double *__restrict__ st, double &mean, double &sd) {
#pragma clang fp contract(off)
    const double m = st[0], q = st[1], d = st[2];
    if (d == 0.0) { mean = 0.0; sd = 1.0; return; }
    mean = m / d;
    const double var = q / d - mean * mean;
    sd = sqrt(var > VN_VAR_MIN ? var : VN_VAR_MIN);
}

// the masked denormalisation of one stored value: a row the rollout zeroed stays exactly 0 (0 * std + mean would be the mean)
__device__ __forceinline__ float vn_denorm(float x, float mask, bool ident, double mean, double sd) {
#pragma clang fp contract(off)
    if (ident) return x;
    return mask != 0.f ? (float)((double)x * sd + mean) : 0.f;
}

// sum over the workgroup (256 threads) of three f64 values, in a fixed order; valid in thread 0
__device__ __forceinline__ void vn_block_sum3(double &a, double &b, double &c) {
    __shared__ double red[3][4];
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); c += __shfl_xor(c, off); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; red[2][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        c = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    }
}

// k_gae_scan on denormalised values.  v[:, t] of t < T is masked by active[:, t] (the rollout stores value * live there), v[:, T] by
// vmask [N][P], the rollout's bootstrap mask.  Also the sums of the value normaliser over live rows, from the fp32 v_target the
// kernel stores: y, y^2 (exact in f64) and the count, as per-workgroup partials vn_part [3][GAE_BLOCKS].
__global__ __launch_bounds__(256) void k_gae_scan_vn(int N, int T, int P, const float *r, const float *v, const float *active, const float *vmask,
                                                     const double *vn_state, float gamma, float lamda, float *adv, float *v_target, double *stats,
                                                     double *vn_part) {
    double mean, sd;
    vn_stats(vn_state, mean, sd);
    const bool ident = vn_state[2] == 0.0;
    double s = 0.0, s2 = 0.0, y1 = 0.0, y2 = 0.0, cnt = 0.0;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < N * P; idx += gridDim.x * 256) {
        const int n = idx / P, p = idx - n * P;
        float gae = 0.f;
        float vn = vn_denorm(v[((size_t)n * (T + 1) + T) * P + p], vmask[idx], ident, mean, sd);
        for (int t = T - 1; t >= 0; t--) {
            const size_t o = ((size_t)n * T + t) * P + p;
            const float a = active[o];
            const float vt = vn_denorm(v[((size_t)n * (T + 1) + t) * P + p], a, ident, mean, sd);
            float delta = (r[o] + gamma * vn - vt) * a;
            gae = delta + gamma * lamda * gae;
            adv[o] = gae;
            const float y = gae + vt;
            v_target[o] = y;
            s += (double)gae;
            s2 += (double)gae * (double)gae;
            if (a != 0.f) { y1 += (double)y; y2 += (double)y * (double)y; cnt += 1.0; }
            vn = vt;
        }
    }
    gae_block_sum(s, s2);
    vn_block_sum3(y1, y2, cnt);
    if (threadIdx.x == 0) {
        stats[4 + 2 * blockIdx.x] = s; stats[5 + 2 * blockIdx.x] = s2;
        vn_part[blockIdx.x] = y1; vn_part[GAE_BLOCKS + blockIdx.x] = y2; vn_part[2 * GAE_BLOCKS + blockIdx.x] = cnt;
    }
}

// thread 0: k_gae_finalize; threads 1-3: S1, S2, c from the partials, in index order
__global__ void k_gae_finalize_vn(int64_t n, int nblk, double *stats, const double *vn_part, double *sums) {
    if (threadIdx.x == 0) {
        double s = 0.0, s2 = 0.0;
        for (int b = 0; b < nblk; b++) { s += stats[4 + 2 * b]; s2 += stats[5 + 2 * b]; }
        const double mean = s / (double)n;
        const double var = (s2 - (double)n * mean * mean) / (double)(n - 1);  // unbiased, torch.std default (refined by k_gae_center)
        stats[0] = s;
        stats[1] = s2;
        stats[2] = mean;
        stats[3] = sqrt(var > 0.0 ? var : 0.0);
    } else if (threadIdx.x < 4) {
        const int k = threadIdx.x - 1;
        double x = 0.0;
        for (int b = 0; b < nblk; b++) x += vn_part[k * GAE_BLOCKS + b];
        sums[k] = x;
    }
}

// the moving-average step from (S1, S2, c), which may have been summed over ranks; c == 0 changes nothing
__global__ void k_value_norm_update(double *st, const double *sums, double beta) {
#pragma clang fp contract(off)
    const double c = sums[2];
    if (!(c > 0.0)) return;
    const double w = 1.0 - beta;
    st[0] = beta * st[0] + w * (sums[0] / c);
    st[1] = beta * st[1] + w * (sums[1] / c);
    st[2] = beta * st[2] + w;
}

__device__ __forceinline__ float vn_target(float y, float a, double mean, double sd) {
#pragma clang fp contract(off)
    return a != 0.f ? (float)(((double)y - mean) / sd) : 0.f;
}

// out = (y - mean) / std on live entries, 0 elsewhere: n4 16-byte lanes, then the n - 4 n4 tail elements (workgroup 0)
__global__ __launch_bounds__(256) void k_value_norm_targets(int64_t n4, int64_t n, const float *__restrict__ y, const float *__restrict__ active,
                                                            const double *__restrict__ vn_state, float *__restrict__ out) {
    double mean, sd;
    vn_stats(vn_state, mean, sd);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 yy = ((const float4 *)y)[i], a = ((const float4 *)active)[i];
        ((float4 *)out)[i] = make_float4(vn_target(yy.x, a.x, mean, sd), vn_target(yy.y, a.y, mean, sd), vn_target(yy.z, a.z, mean, sd),
                                         vn_target(yy.w, a.w, mean, sd));
    }
    const int64_t i = 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && i < n) out[i] = vn_target(y[i], active[i], mean, sd);
}

}  // namespace

extern "C" {

int64_t gae_advnorm_vn_workspace(void) { return (int64_t)(4 + 5 * GAE_BLOCKS) * sizeof(double); }

int gae_advnorm_vn(int32_t N, int32_t T, int32_t P, const float *r, const float *v, const float *active, const float *vmask,
                   const double *vn_state, float gamma, float lamda, int32_t use_adv_norm, float *adv, float *v_target, double *stats,
                   double *sums, void *stream) {
    if (N < 1 || T < 1 || P < 1 || !r || !v || !active || !vmask || !vn_state || !adv || !v_target || !stats || !sums) return MO_ERR_BAD_ARG;
    if ((int64_t)N * P > INT32_MAX) return MO_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)N * T * P;
    const int64_t seq_blocks = ((int64_t)N * P + 255) / 256, el_blocks = (n + 255) / 256;
    const int g_scan = (int)(seq_blocks < GAE_BLOCKS ? seq_blocks : GAE_BLOCKS), g_el = (int)(el_blocks < GAE_BLOCKS ? el_blocks : GAE_BLOCKS);
    double *vn_part = stats + 4 + 2 * GAE_BLOCKS;
    hipLaunchKernelGGL(k_gae_scan_vn, dim3(g_scan), dim3(256), 0, s, N, T, P, r, v, active, vmask, vn_state, gamma, lamda, adv, v_target, stats,
                       vn_part);
    hipLaunchKernelGGL(k_gae_finalize_vn, dim3(1), dim3(64), 0, s, n, g_scan, stats, vn_part, sums);
    if (use_adv_norm) {
        hipLaunchKernelGGL(k_gae_center, dim3(g_el), dim3(256), 0, s, n, adv, stats);
        hipLaunchKernelGGL(k_gae_std, dim3(1), dim3(1), 0, s, n, g_el, stats);
        hipLaunchKernelGGL(k_gae_norm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, adv, active, stats);
    }
    return (int)hipGetLastError();
}

int value_norm_update(double *vn_state, const double *sums, double beta, void *stream) {
    if (!vn_state || !sums || !(beta > 0.0 && beta < 1.0)) return MO_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_value_norm_update, dim3(1), dim3(1), 0, (hipStream_t)stream, vn_state, sums, beta);
    return (int)hipGetLastError();
}

int value_norm_targets(int64_t n, const float *v_target, const float *active, const double *vn_state, float *out, void *stream) {
    if (n < 0 || !v_target || !active || !vn_state || !out) return MO_ERR_BAD_ARG;
    if (((uintptr_t)v_target | (uintptr_t)active | (uintptr_t)out) & 15) return MO_ERR_BAD_ARG;
    if (n == 0) return 0;
    const int64_t n4 = n / 4, blocks = (n4 + 255) / 256;
    const int grid = (int)(blocks < 1 ? 1 : (blocks < 1024 ? blocks : 1024));
    hipLaunchKernelGGL(k_value_norm_targets, dim3(grid), dim3(256), 0, (hipStream_t)stream, n4, n, v_target, active, vn_state, out);
    return (int)hipGetLastError();
}

}  // extern "C"
