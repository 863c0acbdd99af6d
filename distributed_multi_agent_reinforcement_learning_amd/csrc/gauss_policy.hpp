// gauss_policy.hpp -- the diagonal-Gaussian policy of the env_3d trainer (continuous actions; C ABI: include/mappo_ops.h
// gauss_head_sample / ppo_loss_gauss_fwd_bwd, and with a state-dependent log-std / tanh squashing gauss_head_sample_ex /
// ppo_loss_gauss_ex_fwd_bwd).  Included once, from csrc/mappo_ops.hip after its anonymous namespace: it reuses that
// file's Philox4x32-10 (philox4x32_10), the 16-lane row sum (row16_sum), the wave-local LDS fence (wave_fence), the PPO row
// (ppo_elem, PPO_BLOCKS), the steps the strided loss kernels share (PpoView / ppo_row / ppo_offset, ppo_wave_block_sums, ppo_wave_sum, the
// diagnostics' ppo_diag_block_sums / ppo_diag_finish_wave) and the head's feature width (HEAD_H).
#pragma once
#include "direction_action.hpp"

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

// DIAG: the ppodiag::row step of live rows and its partials behind the PPO_BLOCKS x GAUSS_PART loss partials (as k_ppo_loss<DIAG>)
template <bool DIAG>
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
    double dg[ppodiag::NSUM] = {};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const PpoRow row = ppo_row(i, mv);
        const long mo = ppo_offset(row, mv);
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
        const float vn = v_now[ppo_offset(row, vv)];
        float d_lr = 0.f, d_vt = 0.f;
        if (DIAG) { d_lr = lp - lp_old[i]; d_vt = v_tgt[i]; }
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
        if (DIAG && act != 0.f) ppodiag::row(dg, d_lr, expf(d_lr), ent, vn, d_vt, eps);
    }
    ppo_wave_block_sums(acc, 2 + A, partials + (size_t)blockIdx.x * GAUSS_PART);   // (A is uniform)
    if (DIAG) ppo_diag_block_sums(dg, partials + (size_t)PPO_BLOCKS * GAUSS_PART);
}

// one wave per sum (2 + A workgroups, ppo_wave_sum)
__device__ __forceinline__ void ppo_gauss_finish_wave(int k, int nblk, const double *partials, const float *active_sum, float *losses,
                                                      float *grad_log_std) {
    const double s = ppo_wave_sum(nblk, partials, GAUSS_PART, k);
    if (threadIdx.x == 0) {
        if (k < 2) losses[k] = (float)s / active_sum[0];
        else grad_log_std[k - 2] = (float)s;
    }
}

__global__ __launch_bounds__(64) void k_ppo_gauss_finish(int nblk, const double *partials, const float *active_sum, float *losses,
                                                         float *grad_log_std) {
    ppo_gauss_finish_wave(blockIdx.x, nblk, partials, active_sum, losses, grad_log_std);
}

// k_ppo_gauss_finish in the first nsum workgroups, the eight diagnostic sums (ppo_diag_finish_wave) in the eight after them
__global__ __launch_bounds__(64) void k_ppo_gauss_finish_diag(int nsum, int nblk, const double *partials, const float *active_sum, float *losses,
                                                              float *grad_log_std, double *diag) {
    if ((int)blockIdx.x < nsum) ppo_gauss_finish_wave(blockIdx.x, nblk, partials, active_sum, losses, grad_log_std);
    else ppo_diag_finish_wave(blockIdx.x - nsum, nblk, partials + (size_t)PPO_BLOCKS * GAUSS_PART, diag);
}

// ---- state-dependent log-std and tanh squashing (gauss_head_sample_ex / ppo_loss_gauss_ex_fwd_bwd) ---------------------------------
// u = mu + exp(ls) z with ls = clamp(ls_raw, log_std_min, log_std_max); ls_raw = feat W_ls^T + b_ls (state mode) or the log_std vector
// (param mode).  The buffer keeps u in every squash mode; the environment gets clamp(u, -1, 1) (clip) or tanh(u) (tanh) in f64, and the
// tanh log-probability subtracts sum_a c(u_a), c(u) = log(1 - tanh(u)^2) = 2 (ln 2 - u - softplus(-2 u)).  The head and the loss both
// call tanh_log_jac, so the rollout's and the update's correction are the same bits for the same u.
// Direction mode: u = (u_x, u_y, u_z, s) has four dimensions and the environment gets the three commands of
// diract::to_env (csrc/direction_action.hpp): the heading and the pitch of the vector, and s.  The map belongs to the environment: the
// log-probability is the plain Normal one of u, as in clip mode, and the update takes the clip instance of the loss with A = 4.
constexpr int GAUSS_CLIP = 0, GAUSS_TANH = 1, GAUSS_DIRECTION = 2;   // the squash argument of the C entries
constexpr float GAUSS_LN2 = 0.69314718055994530942f;
__device__ __forceinline__ float tanh_log_jac(float u) {
    const float x = -2.f * u;
    return 2.f * (GAUSS_LN2 - u - (fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)))));
}

// The log-std row of the update, shared by k_ppo_loss_gauss_ex, k_bc_loss_gauss and k_ppo_bc_loss_gauss: ls = clamp(ls_raw, lo, hi), and
// torch.clamp's backward -- the gradient w.r.t. ls_raw passes on the closed range [lo, hi] and is 0 outside
__device__ __forceinline__ float gauss_ls_clamp(float ls_raw, float lo, float hi) { return fminf(fmaxf(ls_raw, lo), hi); }
__device__ __forceinline__ bool gauss_ls_pass(float ls_raw, float lo, float hi) { return ls_raw >= lo && ls_raw <= hi; }
// 1 / sigma^2 with sigma = expf(ls), and a dimension's term of the entropy (the PPO launches; k_bc_loss_gauss has its own expf(-2 ls))
__device__ __forceinline__ float gauss_inv_var(float ls) {
    const float s = expf(ls);
    return 1.f / (s * s);
}
__device__ __forceinline__ float gauss_ent_term(float ls) { return 0.5f + HALF_LN_2PI + ls; }

// k_gauss_head with the log-std head folded into the same pass: in state mode a lane holds 2 AT x 8 weights (W's rows, then W_ls's),
// the 2 AT dot products of a row go through row16_sum and LDS like mu's, hence AT <= 8 (2 AT <= 16 lanes of a row).  Same Philox
// layout, expression order and ticket as k_gauss_head.
constexpr int GAUSS_SD_MAX_A = 8;
template <int AT, bool STATE, int MODE>
__global__ __launch_bounds__(256) void k_gauss_head_ex(int R, const float *__restrict__ feat, const float *__restrict__ W, const float *__restrict__ b,
                                                       const float *__restrict__ W_ls, const float *__restrict__ b_ls, const float *__restrict__ log_std,
                                                       float ls_lo, float ls_hi, uint64_t seed, uint64_t *counter, unsigned int *done, int greedy,
                                                       float *__restrict__ action, double *__restrict__ env_action, float *__restrict__ logp) {
    constexpr int NO = STATE ? 2 * AT : AT;   // outputs per row: mu, then ls_raw in state mode
    static_assert(NO <= 16, "one output per lane of a 16-lane row");
    static_assert(MODE != GAUSS_DIRECTION || AT == diract::LATENT, "the direction head has four latent dimensions");
    constexpr bool TANH = MODE == GAUSS_TANH, DIR = MODE == GAUSS_DIRECTION;
    __shared__ float s_y[4][64][NO + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    const int i = lane & 15, g = lane >> 4;
    float w[NO][8];
#pragma unroll
    for (int a = 0; a < NO; a++)
#pragma unroll
        for (int k = 0; k < 8; k++) w[a][k] = a < AT ? W[a * HEAD_H + 8 * i + k] : W_ls[(a - AT) * HEAD_H + 8 * i + k];
    const uint64_t offset = *counter;
    float (*sy)[NO + 1] = s_y[wave];
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
            for (int a = 0; a < NO; a++) {
                float sum = fa.x * w[a][0];
                sum = __builtin_fmaf(fa.y, w[a][1], sum); sum = __builtin_fmaf(fa.z, w[a][2], sum); sum = __builtin_fmaf(fa.w, w[a][3], sum);
                sum = __builtin_fmaf(fb.x, w[a][4], sum); sum = __builtin_fmaf(fb.y, w[a][5], sum); sum = __builtin_fmaf(fb.z, w[a][6], sum);
                sum = __builtin_fmaf(fb.w, w[a][7], sum);
                sum = row16_sum(sum);
                mine = i == a ? sum : mine;
            }
            if (i < NO) sy[row][i] = mine;
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
                    for (int k = 0; k < 4; k++) u[k] = ((float)(o[k] >> 8) + 0.5f) * (1.0f / 16777216.0f);
                    const float ra = sqrtf(-2.f * logf(u[0])), rb = sqrtf(-2.f * logf(u[2]));
                    float sa, ca, sb, cb;
                    sincospif(2.f * u[1], &sa, &ca);
                    sincospif(2.f * u[3], &sb, &cb);
                    const float zz[4] = {ra * ca, ra * sa, rb * cb, rb * sb};
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (4 * j + k < AT) z[4 * j + k] = zz[k];
                }
            }
            float lp = 0.f, jac = 0.f;
            float xs[AT];   // (direction mode only)
#pragma unroll
            for (int a = 0; a < AT; a++) {
                const float ls_raw = STATE ? sy[lane][AT + a] + b_ls[a] : log_std[a];
                const float ls = fminf(fmaxf(ls_raw, ls_lo), ls_hi);
                const float x = sy[lane][a] + b[a] + expf(ls) * z[a];
                action[(size_t)r * AT + a] = x;
                if (DIR) xs[a] = x;
                else env_action[(size_t)r * AT + a] = TANH ? tanh((double)x) : (double)fminf(fmaxf(x, -1.f), 1.f);
                lp += -0.5f * z[a] * z[a] - ls - HALF_LN_2PI;
                if (TANH) jac += tanh_log_jac(x);
            }
            if constexpr (DIR) {   // env_action is (R, 3): the angles of the sampled vector and the speed
                double env[diract::ENV_A];
                diract::to_env(xs, env);
#pragma unroll
                for (int a = 0; a < diract::ENV_A; a++) env_action[(size_t)r * diract::ENV_A + a] = env[a];
            }
            logp[r] = TANH ? lp - jac : lp;
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

// k_ppo_loss_gauss with ls_raw per row (STATE: a strided view like mu's, its gradient written per row in the same layout) or one
// vector (param mode: the gradient summed through the f64 partials as k_ppo_loss_gauss does).  ls = clamp(ls_raw, lo, hi); the
// gradient w.r.t. ls_raw passes on the closed range [lo, hi] and is 0 outside (torch.clamp's backward).  TANH subtracts
// sum_a tanh_log_jac(u_a) from logp_now: no gradient (u is data), but the ratio is 1 where the rollout's policy is the update's.
// AT > 0 fixes the action count (state mode: sigma = exp(ls) and 1 / sigma^2 are per row, so a row pays for AT of them, not for
// GAUSS_MAX_A); AT = 0 takes the runtime A with k_ppo_loss_gauss's loop shape (param mode: sigma is computed once per thread, and
// this shape keeps its bits equal to k_ppo_loss_gauss's).  Same expressions, in the same order, as k_ppo_loss_gauss.
template <int AT, bool STATE, bool TANH, bool DIAG>
__global__ __launch_bounds__(256) void k_ppo_loss_gauss_ex(long n, int A_rt, const float *__restrict__ mu, PpoView mv, const float *__restrict__ ls_raw,
                                                           PpoView lv, float ls_lo, float ls_hi, const float *__restrict__ action, const float *lp_old,
                                                           const float *adv, const float *active, const float *__restrict__ v_now, PpoView vv,
                                                           const float *v_old, const float *v_tgt, const float *active_sum, float eps, float ent_coef,
                                                           int value_clip, float *__restrict__ g_mu, float *__restrict__ g_ls, float *__restrict__ g_v,
                                                           double *partials) {
    constexpr int NA = AT > 0 ? AT : GAUSS_MAX_A;   // register slots
    const int A = AT > 0 ? AT : A_rt;               // (a constant when AT > 0: the k < A guards fold away)
    const float inv = 1.f / active_sum[0];
    float ls[NA], iv[NA];
    bool pass[NA];
    float ent = 0.f;
    if (!STATE) {
#pragma unroll
        for (int k = 0; k < NA; k++) {
            const float lr = k < A ? ls_raw[k] : 0.f;
            ls[k] = gauss_ls_clamp(lr, ls_lo, ls_hi);
            pass[k] = gauss_ls_pass(lr, ls_lo, ls_hi);
            iv[k] = gauss_inv_var(ls[k]);
            if (k < A) ent += gauss_ent_term(ls[k]);
        }
    }
    constexpr int NSUM = STATE ? 2 : 2 + NA;
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; k++) acc[k] = 0.0;
    double dg[ppodiag::NSUM] = {};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const PpoRow row = ppo_row(i, mv);
        const long mo = ppo_offset(row, mv);
        const long lo = STATE ? ppo_offset(row, lv) : 0;
        if (STATE) {
            ent = 0.f;
#pragma unroll
            for (int k = 0; k < NA; k++)
                if (k < A) {
                    const float lr = ls_raw[lo + k];
                    ls[k] = gauss_ls_clamp(lr, ls_lo, ls_hi);
                    pass[k] = gauss_ls_pass(lr, ls_lo, ls_hi);
                    iv[k] = gauss_inv_var(ls[k]);
                    ent += gauss_ent_term(ls[k]);
                }
        }
        float d[NA];
        float lp = 0.f, jac = 0.f;
#pragma unroll
        for (int k = 0; k < NA; k++) {
            d[k] = 0.f;
            if (k < A) {
                const float u = action[i * A + k];
                d[k] = u - mu[mo + k];
                lp += -(d[k] * d[k]) * iv[k] * 0.5f - ls[k] - HALF_LN_2PI;
                if (TANH) jac += tanh_log_jac(u);
            }
        }
        if (TANH) lp -= jac;
        const float act = active[i];
        const float vn = v_now[ppo_offset(row, vv)];
        float d_lr = 0.f, d_vt = 0.f;
        if (DIAG) { d_lr = lp - lp_old[i]; d_vt = v_tgt[i]; }
        const PpoElem e = ppo_elem(lp, ent, lp_old[i], adv[i], act, vn, value_clip ? v_old[i] : 0.f, v_tgt[i], inv, eps, ent_coef, value_clip);
        acc[0] += (double)(e.la * act);
        acc[1] += (double)(e.lc * act);
        g_v[i] = e.g_v;
#pragma unroll
        for (int k = 0; k < NA; k++)
            if (k < A) {
                const float q = d[k] * iv[k];
                g_mu[mo + k] = e.g_lp * q;
                const float gl = e.g_lp * (q * d[k] - 1.f) + e.g_ent;
                if (STATE) g_ls[lo + k] = pass[k] ? gl : 0.f;
                else acc[2 + k] += (double)(pass[k] ? gl : 0.f);
            }
        if (DIAG && act != 0.f) ppodiag::row(dg, d_lr, expf(d_lr), ent, vn, d_vt, eps);
    }
    ppo_wave_block_sums(acc, STATE ? 2 : 2 + A, partials + (size_t)blockIdx.x * GAUSS_PART);   // (A is uniform)
    if (DIAG) ppo_diag_block_sums(dg, partials + (size_t)PPO_BLOCKS * GAUSS_PART);
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
int64_t ppo_loss_gauss_diag_workspace(void) { return (int64_t)PPO_BLOCKS * (GAUSS_PART + ppodiag::NSUM) * sizeof(double); }

// diag == nullptr: the plain launches; else the DIAG instance and the finish with eight more workgroups (two launches either way)
static int ppo_loss_gauss_launch(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                                 int64_t m_s2, const float *log_std, const float *action, const float *logp_old, const float *adv,
                                 const float *active, const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old,
                                 const float *v_target, const float *active_sum, float epsilon, float entropy_coef, int32_t use_value_clip,
                                 float *losses, float *grad_values, float *grad_log_std, void *workspace, double *diag, void *stream) {
    if (n < 1 || A < 1 || A > GAUSS_MAX_A || d1 < 1 || d2 < 1 || (n % (d1 * d2)) || !mu || !grad_mu || !log_std || !action || !logp_old || !adv ||
        !active || !values_now || !v_target || !active_sum || !losses || !grad_values || !grad_log_std || !workspace || (use_value_clip && !values_old))
        return MO_ERR_BAD_ARG;
    long blocks = (n + 255) / 256;
    if (blocks > PPO_BLOCKS) blocks = PPO_BLOCKS;
    const PpoView mv{d1, d2, m_s0, m_s1, m_s2}, vv{d1, d2, v_s0, v_s1, v_s2};
#define GAUSS_LOSS(D) hipLaunchKernelGGL((k_ppo_loss_gauss<D>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n, (int)A, mu, mv, \
                                         log_std, action, logp_old, adv, active, values_now, vv, values_old, v_target, active_sum, epsilon, \
                                         entropy_coef, (int)use_value_clip, grad_mu, grad_values, (double *)workspace)
    if (diag) {
        GAUSS_LOSS(true);
        hipLaunchKernelGGL(k_ppo_gauss_finish_diag, dim3(2 + A + ppodiag::NSUM), dim3(64), 0, (hipStream_t)stream, 2 + (int)A, (int)blocks,
                           (const double *)workspace, active_sum, losses, grad_log_std, diag);
    } else {
        GAUSS_LOSS(false);
        hipLaunchKernelGGL(k_ppo_gauss_finish, dim3(2 + A), dim3(64), 0, (hipStream_t)stream, (int)blocks, (const double *)workspace, active_sum,
                           losses, grad_log_std);
    }
#undef GAUSS_LOSS
    return (int)hipGetLastError();
}

int ppo_loss_gauss_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1, int64_t m_s2,
                           const float *log_std, const float *action, const float *logp_old, const float *adv, const float *active,
                           const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                           const float *active_sum, float epsilon, float entropy_coef, int32_t use_value_clip, float *losses, float *grad_values,
                           float *grad_log_std, void *workspace, void *stream) {
    return ppo_loss_gauss_launch(n, A, mu, grad_mu, d1, d2, m_s0, m_s1, m_s2, log_std, action, logp_old, adv, active, values_now, v_s0, v_s1, v_s2,
                                 values_old, v_target, active_sum, epsilon, entropy_coef, use_value_clip, losses, grad_values, grad_log_std,
                                 workspace, nullptr, stream);
}

int ppo_loss_gauss_fwd_bwd_diag(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                                int64_t m_s2, const float *log_std, const float *action, const float *logp_old, const float *adv,
                                const float *active, const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old,
                                const float *v_target, const float *active_sum, float epsilon, float entropy_coef, int32_t use_value_clip,
                                float *losses, float *grad_values, float *grad_log_std, void *workspace, void *stream, double *diag) {
    if (!diag) return MO_ERR_BAD_ARG;
    return ppo_loss_gauss_launch(n, A, mu, grad_mu, d1, d2, m_s0, m_s1, m_s2, log_std, action, logp_old, adv, active, values_now, v_s0, v_s1, v_s2,
                                 values_old, v_target, active_sum, epsilon, entropy_coef, use_value_clip, losses, grad_values, grad_log_std,
                                 workspace, diag, stream);
}

static bool gauss_ex_bounds_ok(float lo, float hi) { return lo < hi; }   // (NaN fails)

int gauss_head_sample_ex(int32_t R, int32_t A, int32_t H, const float *feat, const float *W, const float *b, const float *W_ls, const float *b_ls,
                         const float *log_std, float log_std_min, float log_std_max, int32_t squash, uint64_t seed, uint64_t *counter,
                         uint32_t *ticket, int32_t greedy, float *action, double *env_action, float *logp, void *stream) {
    const bool state = W_ls != nullptr;
    if (R < 0 || A < 1 || A > (state ? GAUSS_SD_MAX_A : GAUSS_MAX_A) || H != HEAD_H || !feat || !W || !b || state != (b_ls != nullptr) ||
        state == (log_std != nullptr) || (squash != GAUSS_CLIP && squash != GAUSS_TANH && squash != GAUSS_DIRECTION) ||
        (squash == GAUSS_DIRECTION && A != diract::LATENT) || !gauss_ex_bounds_ok(log_std_min, log_std_max) || !counter || !ticket || !action ||
        !env_action || !logp || ((uintptr_t)feat & 15))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int g0 = (R + 255) / 256, grid = g0 < 1024 ? g0 : 1024;
#define GAUSS_EX(AT, S, T) hipLaunchKernelGGL((k_gauss_head_ex<AT, S, T>), dim3(grid), dim3(256), 0, st, R, feat, W, b, W_ls, b_ls, log_std, \
                                              log_std_min, log_std_max, seed, counter, ticket, (int)greedy, action, env_action, logp)
#define GAUSS_EX4(AT) case AT: if (state) { if (squash) GAUSS_EX(AT, true, GAUSS_TANH); else GAUSS_EX(AT, true, GAUSS_CLIP); } \
                               else { if (squash) GAUSS_EX(AT, false, GAUSS_TANH); else GAUSS_EX(AT, false, GAUSS_CLIP); } break;
#define GAUSS_EX2(AT) case AT: if (squash) GAUSS_EX(AT, false, GAUSS_TANH); else GAUSS_EX(AT, false, GAUSS_CLIP); break;
    if (squash == GAUSS_DIRECTION) {   // A is 4: action (R, 4), env_action (R, 3)
        if (state) GAUSS_EX(4, true, GAUSS_DIRECTION);
        else GAUSS_EX(4, false, GAUSS_DIRECTION);
    } else switch (A) {
        GAUSS_EX4(1) GAUSS_EX4(2) GAUSS_EX4(3) GAUSS_EX4(4) GAUSS_EX4(5) GAUSS_EX4(6) GAUSS_EX4(7) GAUSS_EX4(8) GAUSS_EX2(9) GAUSS_EX2(10)
        GAUSS_EX2(11) GAUSS_EX2(12) GAUSS_EX2(13) GAUSS_EX2(14) GAUSS_EX2(15) GAUSS_EX2(16)
    }
#undef GAUSS_EX2
#undef GAUSS_EX4
#undef GAUSS_EX
    return (int)hipGetLastError();
}

int64_t ppo_loss_gauss_ex_workspace(void) { return (int64_t)PPO_BLOCKS * GAUSS_PART * sizeof(double); }

static int ppo_loss_gauss_ex_launch(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                                    int64_t m_s2, const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2,
                                    float log_std_min, float log_std_max, int32_t squash, const float *action, const float *logp_old,
                                    const float *adv, const float *active, const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2,
                                    const float *values_old, const float *v_target, const float *active_sum, float epsilon, float entropy_coef,
                                    int32_t use_value_clip, float *losses, float *grad_values, void *workspace, double *diag, void *stream) {
    if (n < 1 || A < 1 || A > GAUSS_MAX_A || d1 < 1 || d2 < 1 || (n % (d1 * d2)) || !mu || !grad_mu || !ls_raw || !grad_log_std ||
        (squash != GAUSS_CLIP && squash != GAUSS_TANH && squash != GAUSS_DIRECTION) || !gauss_ex_bounds_ok(log_std_min, log_std_max) || !action ||
        !logp_old || !adv || !active || !values_now || !v_target || !active_sum || !losses || !grad_values || !workspace ||
        (use_value_clip && !values_old))
        return MO_ERR_BAD_ARG;
    // direction mode: the action of the MDP is the latent u and the map to the angles is the environment's, so its log-probability has no
    // Jacobian term -- the clip instances
    if (squash == GAUSS_DIRECTION) squash = GAUSS_CLIP;
    const bool state = (l_s0 | l_s1 | l_s2) != 0;
    long blocks = (n + 255) / 256;
    if (blocks > PPO_BLOCKS) blocks = PPO_BLOCKS;
    const PpoView mv{d1, d2, m_s0, m_s1, m_s2}, lv{d1, d2, l_s0, l_s1, l_s2}, vv{d1, d2, v_s0, v_s1, v_s2};
    hipStream_t st = (hipStream_t)stream;
#define GAUSS_LOSS_EXD(AT, S, T, D) hipLaunchKernelGGL((k_ppo_loss_gauss_ex<AT, S, T, D>), dim3((unsigned)blocks), dim3(256), 0, st, (long)n, (int)A, \
                                                       mu, mv, ls_raw, lv, log_std_min, log_std_max, action, logp_old, adv, active, values_now, vv, \
                                                       values_old, v_target, active_sum, epsilon, entropy_coef, (int)use_value_clip, grad_mu, \
                                                       grad_log_std, grad_values, (double *)workspace)
#define GAUSS_LOSS_EX(AT, S, T) do { if (diag) GAUSS_LOSS_EXD(AT, S, T, true); else GAUSS_LOSS_EXD(AT, S, T, false); } while (0)
#define GAUSS_LOSS_EX4(AT) case AT: if (squash) GAUSS_LOSS_EX(AT, true, true); else GAUSS_LOSS_EX(AT, true, false); break;
#define GAUSS_LOSS_EX2(AT) case AT: if (squash) GAUSS_LOSS_EXD(AT, true, true, false); else GAUSS_LOSS_EXD(AT, true, false, false); break;
    // the diagnostics in state mode stop at the action count the state-mode rollout head has (GAUSS_SD_MAX_A): beyond it no policy
    // exists whose update could be diagnosed, and the A = 15 instance would be the one kernel here that needs scratch
    if (diag && state && A > GAUSS_SD_MAX_A) return MO_ERR_BAD_ARG;
    if (!state) {   // param mode: the runtime-A shape of k_ppo_loss_gauss (sigma once per thread)
        if (squash) GAUSS_LOSS_EX(0, false, true);
        else GAUSS_LOSS_EX(0, false, false);
    } else {        // state mode: one instance per action count
        switch (A) {
            GAUSS_LOSS_EX4(1) GAUSS_LOSS_EX4(2) GAUSS_LOSS_EX4(3) GAUSS_LOSS_EX4(4) GAUSS_LOSS_EX4(5) GAUSS_LOSS_EX4(6) GAUSS_LOSS_EX4(7)
            GAUSS_LOSS_EX4(8) GAUSS_LOSS_EX2(9) GAUSS_LOSS_EX2(10) GAUSS_LOSS_EX2(11) GAUSS_LOSS_EX2(12) GAUSS_LOSS_EX2(13) GAUSS_LOSS_EX2(14)
            GAUSS_LOSS_EX2(15) GAUSS_LOSS_EX2(16)
        }
    }
#undef GAUSS_LOSS_EX2
#undef GAUSS_LOSS_EX4
#undef GAUSS_LOSS_EX
#undef GAUSS_LOSS_EXD
    // state mode: the two loss sums only (grad_log_std was written per row); param mode: the A log_std sums as well
    const int nsum = state ? 2 : 2 + A;
    if (diag)
        hipLaunchKernelGGL(k_ppo_gauss_finish_diag, dim3(nsum + ppodiag::NSUM), dim3(64), 0, st, nsum, (int)blocks, (const double *)workspace,
                           active_sum, losses, grad_log_std, diag);
    else
        hipLaunchKernelGGL(k_ppo_gauss_finish, dim3(nsum), dim3(64), 0, st, (int)blocks, (const double *)workspace, active_sum, losses,
                           grad_log_std);
    return (int)hipGetLastError();
}

int ppo_loss_gauss_ex_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1, int64_t m_s2,
                              const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2, float log_std_min,
                              float log_std_max, int32_t squash, const float *action, const float *logp_old, const float *adv, const float *active,
                              const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                              const float *active_sum, float epsilon, float entropy_coef, int32_t use_value_clip, float *losses, float *grad_values,
                              void *workspace, void *stream) {
    return ppo_loss_gauss_ex_launch(n, A, mu, grad_mu, d1, d2, m_s0, m_s1, m_s2, ls_raw, grad_log_std, l_s0, l_s1, l_s2, log_std_min, log_std_max,
                                    squash, action, logp_old, adv, active, values_now, v_s0, v_s1, v_s2, values_old, v_target, active_sum, epsilon,
                                    entropy_coef, use_value_clip, losses, grad_values, workspace, nullptr, stream);
}

int ppo_loss_gauss_ex_fwd_bwd_diag(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                                   int64_t m_s2, const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2,
                                   float log_std_min, float log_std_max, int32_t squash, const float *action, const float *logp_old,
                                   const float *adv, const float *active, const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2,
                                   const float *values_old, const float *v_target, const float *active_sum, float epsilon, float entropy_coef,
                                   int32_t use_value_clip, float *losses, float *grad_values, void *workspace, void *stream, double *diag) {
    if (!diag) return MO_ERR_BAD_ARG;
    return ppo_loss_gauss_ex_launch(n, A, mu, grad_mu, d1, d2, m_s0, m_s1, m_s2, ls_raw, grad_log_std, l_s0, l_s1, l_s2, log_std_min, log_std_max,
                                    squash, action, logp_old, adv, active, values_now, v_s0, v_s1, v_s2, values_old, v_target, active_sum, epsilon,
                                    entropy_coef, use_value_clip, losses, grad_values, workspace, diag, stream);
}

}  // extern "C"
