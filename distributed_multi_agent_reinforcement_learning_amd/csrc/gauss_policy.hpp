// gauss_policy.hpp -- the diagonal-Gaussian policy of the env_3d trainer (continuous actions; C ABI: include/mappo_ops.h
// gauss_head_sample / ppo_loss_gauss_fwd_bwd).  Included once, from csrc/mappo_ops.hip after its anonymous namespace: it reuses that
// file's Philox4x32-10 (philox4x32_10), the 16-lane row sum (row16_sum), the wave-local LDS fence (wave_fence), the PPO row
// (ppo_elem, PpoView, PPO_BLOCKS) and the head's feature width (HEAD_H).
#pragma once

namespace {

constexpr int GAUSS_MAX_A = 16;
constexpr float HALF_LN_2PI = 0.91893853320467274178f;   // ln sqrt(2 pi)

// ---- rollout head: a = mu + exp(log_std) z, z ~ N(0, 1) ------------------------------------------------------------------------------
// mu = feat W^T + b as in k_head (16 lanes per row, the A dot products folded with row16_sum, a wave's 64 rows of mu parked in LDS),
// then every lane finishes ONE row: Philox at counter (*counter + r, c2 = j) gives noise block j (dims 4 j .. 4 j + 3), each word mapped
// to u = ((o >> 8) + 1/2) 2^-24 in (0, 1] exactly as the categorical samplers do, and Box-Muller on the pairs (u0, u1), (u2, u3).
// Writes the unclipped sample (the buffer's), its clamp to [-1, 1] in f64 (what e3d_env_tick reads) and log N(a; mu, sigma).  The last
// workgroup out advances the counter by R (the ticket pattern of k_head<true, .>).
template <int AT>
__global__ __launch_bounds__(256) void k_gauss_head(int R, const float *__restrict__ feat, const float *__restrict__ W, const float *__restrict__ b,
                                                    const float *__restrict__ log_std, uint64_t seed, uint64_t *counter, unsigned int *done, int greedy,
                                                    float *__restrict__ action, double *__restrict__ env_action, float *__restrict__ logp) {
    __shared__ float s_y[4][64][AT + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    const int i = lane & 15, g = lane >> 4;
    float w[AT][8];
#pragma unroll
    for (int a = 0; a < AT; a++)
#pragma unroll
        for (int k = 0; k < 8; k++) w[a][k] = W[a * HEAD_H + 8 * i + k];
    const uint64_t offset = *counter;
    float (*sy)[AT + 1] = s_y[wave];
    for (int r0 = (blockIdx.x * 4 + wave) * 64; r0 < R; r0 += nw * 64) {
        float4 fall[16][2];
#pragma unroll
        for (int st = 0; st < 16; st++) {
            const int r = r0 + 4 * st + g;
            fall[st][0] = fall[st][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < R) {
                fall[st][0] = *(const float4 *)(feat + (size_t)r * HEAD_H + 8 * i);
                fall[st][1] = *(const float4 *)(feat + (size_t)r * HEAD_H + 8 * i + 4);
            }
        }
#pragma unroll
        for (int st = 0; st < 16; st++) {
            const int row = 4 * st + g;
            const float4 fa = fall[st][0], fb = fall[st][1];
            float mine = 0.f;
#pragma unroll
            for (int a = 0; a < AT; a++) {
                float sum = fa.x * w[a][0];
                sum = __builtin_fmaf(fa.y, w[a][1], sum); sum = __builtin_fmaf(fa.z, w[a][2], sum); sum = __builtin_fmaf(fa.w, w[a][3], sum);
                sum = __builtin_fmaf(fb.x, w[a][4], sum); sum = __builtin_fmaf(fb.y, w[a][5], sum); sum = __builtin_fmaf(fb.z, w[a][6], sum);
                sum = __builtin_fmaf(fb.w, w[a][7], sum);
                sum = row16_sum(sum);
                mine = i == a ? sum : mine;
            }
            if (i < AT) sy[row][i] = mine;
        }
        wave_fence();
        const int r = r0 + lane;
        if (r < R) {
            float z[AT];
#pragma unroll
            for (int a = 0; a < AT; a++) z[a] = 0.f;
            if (!greedy) {
                const uint64_t ctr = offset + (uint64_t)r;
#pragma unroll
                for (int j = 0; j < (AT + 3) / 4; j++) {
                    uint32_t o[4];
                    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)j, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
                    float u[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) u[k] = ((float)(o[k] >> 8) + 0.5f) * (1.0f / 16777216.0f);   // (0, 1]: log is finite
                    const float ra = sqrtf(-2.f * logf(u[0])), rb = sqrtf(-2.f * logf(u[2]));
                    float sa, ca, sb, cb;
                    sincospif(2.f * u[1], &sa, &ca);   // cos / sin (2 pi u): 2 u is exact
                    sincospif(2.f * u[3], &sb, &cb);
                    const float zz[4] = {ra * ca, ra * sa, rb * cb, rb * sb};
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (4 * j + k < AT) z[4 * j + k] = zz[k];
                }
            }
            float lp = 0.f;
#pragma unroll
            for (int a = 0; a < AT; a++) {
                const float ls = log_std[a];
                const float x = sy[lane][a] + b[a] + expf(ls) * z[a];
                action[(size_t)r * AT + a] = x;
                env_action[(size_t)r * AT + a] = (double)fminf(fmaxf(x, -1.f), 1.f);
                lp += -0.5f * z[a] * z[a] - ls - HALF_LN_2PI;
            }
            logp[r] = lp;
        }
        wave_fence();
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(done, 1u) == gridDim.x - 1) {
            *counter = offset + (uint64_t)R;
            *done = 0u;
            __threadfence();
        }
    }
}

// ---- update: the PPO row of a diagonal Gaussian, forward and gradients in one pass --------------------------------------------------
// Normal(mu, exp(log_std)).log_prob(action).sum(-1) and .entropy().sum(-1) in registers, then ppo_elem (the same tie rules and masked
// means as k_ppo_loss_prob).  g_mu = g_lp (a - mu) / sigma^2 is written in mu's layout (a time-major view); the log_std gradient
// sum_rows g_lp ((a - mu)^2 / sigma^2 - 1) + g_ent and the two loss sums go through f64 per-block partials (wave butterflies, then
// the four waves in a fixed order) that k_ppo_gauss_finish adds in block order: no atomics, the same bits every run.
constexpr int GAUSS_PART = 2 + GAUSS_MAX_A;   // doubles per block: actor sum, critic sum, log_std gradient [A]

__global__ __launch_bounds__(256) void k_ppo_loss_gauss(long n, int A, const float *__restrict__ mu, PpoView mv, const float *__restrict__ log_std,
                                                        const float *__restrict__ action, const float *lp_old, const float *adv, const float *active,
                                                        const float *__restrict__ v_now, PpoView vv, const float *v_old, const float *v_tgt,
                                                        const float *active_sum, float eps, float ent_coef, int value_clip, float *__restrict__ g_mu,
                                                        float *__restrict__ g_v, double *partials) {
    const float inv = 1.f / active_sum[0];
    float ls[GAUSS_MAX_A], iv[GAUSS_MAX_A];
    float ent = 0.f;
#pragma unroll
    for (int k = 0; k < GAUSS_MAX_A; k++) {
        ls[k] = k < A ? log_std[k] : 0.f;
        const float s = expf(ls[k]);
        iv[k] = 1.f / (s * s);
        if (k < A) ent += 0.5f + HALF_LN_2PI + ls[k];
    }
    double acc[GAUSS_PART];
#pragma unroll
    for (int k = 0; k < GAUSS_PART; k++) acc[k] = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long i2 = i % mv.d2, i01 = i / mv.d2, i1 = i01 % mv.d1, i0 = i01 / mv.d1;
        const long mo = i0 * mv.s0 + i1 * mv.s1 + i2 * mv.s2;
        float d[GAUSS_MAX_A];
        float lp = 0.f;
#pragma unroll
        for (int k = 0; k < GAUSS_MAX_A; k++) {
            d[k] = 0.f;
            if (k < A) {
                d[k] = action[i * A + k] - mu[mo + k];
                lp += -(d[k] * d[k]) * iv[k] * 0.5f - ls[k] - HALF_LN_2PI;
            }
        }
        const float act = active[i];
        const float vn = v_now[i0 * vv.s0 + i1 * vv.s1 + i2 * vv.s2];
        const PpoElem e = ppo_elem(lp, ent, lp_old[i], adv[i], act, vn, value_clip ? v_old[i] : 0.f, v_tgt[i], inv, eps, ent_coef, value_clip);
        acc[0] += (double)(e.la * act);
        acc[1] += (double)(e.lc * act);
        g_v[i] = e.g_v;
#pragma unroll
        for (int k = 0; k < GAUSS_MAX_A; k++)
            if (k < A) {
                const float q = d[k] * iv[k];
                g_mu[mo + k] = e.g_lp * q;
                acc[2 + k] += (double)(e.g_lp * (q * d[k] - 1.f) + e.g_ent);
            }
    }
    __shared__ double red[GAUSS_PART][4];
#pragma unroll
    for (int k = 0; k < GAUSS_PART; k++)
        if (k < 2 + A) {   // (A is uniform)
            double s = acc[k];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s;
        }
    __syncthreads();
    if (threadIdx.x < 2 + A) {
        const int k = threadIdx.x;
        partials[(size_t)blockIdx.x * GAUSS_PART + k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
    }
}

// one wave per sum (2 + A workgroups): lane l adds the partials of blocks l, l + 64, .. in order, then a fixed butterfly -- the
// same bits every run, without one lane walking all PPO_BLOCKS partials serially
__global__ __launch_bounds__(64) void k_ppo_gauss_finish(int nblk, const double *partials, const float *active_sum, float *losses,
                                                         float *grad_log_std) {
    const int k = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) s += partials[(size_t)b * GAUSS_PART + k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) {
        if (k < 2) losses[k] = (float)s / active_sum[0];
        else grad_log_std[k - 2] = (float)s;
    }
}

}  // namespace

extern "C" {

int gauss_head_sample(int32_t R, int32_t A, int32_t H, const float *feat, const float *W, const float *b, const float *log_std, uint64_t seed,
                      uint64_t *counter, uint32_t *ticket, int32_t greedy, float *action, double *env_action, float *logp, void *stream) {
    if (R < 0 || A < 1 || A > GAUSS_MAX_A || H != HEAD_H || !feat || !W || !b || !log_std || !counter || !ticket || !action || !env_action || !logp ||
        ((uintptr_t)feat & 15))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int g0 = (R + 255) / 256, grid = g0 < 1024 ? g0 : 1024;   // 4 waves x 64 rows per workgroup step, as head_sample
#define GAUSS_SMP(AT) case AT: hipLaunchKernelGGL((k_gauss_head<AT>), dim3(grid), dim3(256), 0, st, R, feat, W, b, log_std, seed, counter, ticket, \
                                        (int)greedy, action, env_action, logp); break;
    switch (A) {
        GAUSS_SMP(1) GAUSS_SMP(2) GAUSS_SMP(3) GAUSS_SMP(4) GAUSS_SMP(5) GAUSS_SMP(6) GAUSS_SMP(7) GAUSS_SMP(8) GAUSS_SMP(9) GAUSS_SMP(10)
        GAUSS_SMP(11) GAUSS_SMP(12) GAUSS_SMP(13) GAUSS_SMP(14) GAUSS_SMP(15) GAUSS_SMP(16)
    }
#undef GAUSS_SMP
    return (int)hipGetLastError();
}

int64_t ppo_loss_gauss_workspace(void) { return (int64_t)PPO_BLOCKS * GAUSS_PART * sizeof(double); }

int ppo_loss_gauss_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1, int64_t m_s2,
                           const float *log_std, const float *action, const float *logp_old, const float *adv, const float *active,
                           const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                           const float *active_sum, float epsilon, float entropy_coef, int32_t use_value_clip, float *losses, float *grad_values,
                           float *grad_log_std, void *workspace, void *stream) {
    if (n < 1 || A < 1 || A > GAUSS_MAX_A || d1 < 1 || d2 < 1 || (n % (d1 * d2)) || !mu || !grad_mu || !log_std || !action || !logp_old || !adv ||
        !active || !values_now || !v_target || !active_sum || !losses || !grad_values || !grad_log_std || !workspace || (use_value_clip && !values_old))
        return MO_ERR_BAD_ARG;
    long blocks = (n + 255) / 256;
    if (blocks > PPO_BLOCKS) blocks = PPO_BLOCKS;
    const PpoView mv{d1, d2, m_s0, m_s1, m_s2}, vv{d1, d2, v_s0, v_s1, v_s2};
    hipLaunchKernelGGL(k_ppo_loss_gauss, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n, (int)A, mu, mv, log_std, action, logp_old,
                       adv, active, values_now, vv, values_old, v_target, active_sum, epsilon, entropy_coef, (int)use_value_clip, grad_mu, grad_values,
                       (double *)workspace);
    hipLaunchKernelGGL(k_ppo_gauss_finish, dim3(2 + A), dim3(64), 0, (hipStream_t)stream, (int)blocks, (const double *)workspace, active_sum, losses,
                       grad_log_std);
    return (int)hipGetLastError();
}

}  // extern "C"
