// imitation.hpp -- the imitation warm start of the env_3d / env_n2n trainers (algo.bc_iterations; imitation.py; DESIGN.md section 7f;
// C ABI: include/mappo_ops.h bc_loss_gauss_fwd_bwd / bc_loss_cat_fwd_bwd / e3d_bc_select / n2n_bc_select; specification:
// tests/imitation_ref.py).  Included once, from csrc/mappo_ops.hip after gauss_policy.hpp: it reuses that file's PPO row (ppo_elem, PPO_BLOCKS,
// ppo_block_sums, ppo_loss_finish_sums), the steps the strided loss kernels share (PpoView / ppo_row / ppo_offset, ppo_wave_block_sums,
// ppo_wave_sum, the categorical row: PPO_MAX_A, P_EPS, cat_clamp / cat_pass) and gauss_policy.hpp's GAUSS_MAX_A,
// log-std clamp and pass rule (gauss_ls_clamp, gauss_ls_pass) and bounds check.
#pragma once

namespace {

// ---- update: Gaussian negative log-likelihood of the teacher's action, forward and gradients in one pass ---------------------------
// Per row: ls = clamp(ls_raw, lo, hi), iv = exp(-2 ls), d = target - mu (dimension 0 taken modulo 2 into [-1, 1) under wrap0),
// la = sum_a 0.5 d^2 iv + (fit_std ? ls : 0); the actor loss is the masked mean of la.  g_mu = -(active / sum active) d iv in mu's layout;
// with fit_std g_ls = (active / sum active) (1 - d^2 iv) on the closed range [lo, hi], 0 outside, per row (STATE) or summed through the
// partials (param mode); without fit_std it is exactly 0.  The critic's lc and g_v are ppo_elem's, and the reduction is
// k_ppo_loss_gauss's (wave butterflies, the four waves in a fixed order, k_bc_gauss_finish in block order), so they carry the bits of
// ppo_loss_gauss on the same inputs.  Sum 2 is sum_rows active sum_a d^2 (bc_action_mse), or with ANGLE (algo.gauss_squash: direction,
// A >= 3) sum_rows active angle(mu[:3], target[:3]) in radians (diract::angle, fp32 per row; bc_angle_deg).  No atomics: the same bits
// every run.
constexpr int BC_GAUSS_PART = 3 + GAUSS_MAX_A;   // doubles per block: actor sum, critic sum, sum d^2 | sum angle, log_std gradient [A]
constexpr int BC_METRIC_SQ = 0, BC_METRIC_ANGLE = 1;   // the metric argument of bc_loss_gauss_ex_fwd_bwd

template <bool STATE, bool ANGLE>
__global__ __launch_bounds__(256) void k_bc_loss_gauss(long n, int A, const float *__restrict__ mu, PpoView mv, const float *__restrict__ ls_raw,
                                                       PpoView lv, float ls_lo, float ls_hi, int fit_std, int wrap0,
                                                       const float *__restrict__ target, const float *active, const float *__restrict__ v_now,
                                                       PpoView vv, const float *v_old, const float *v_tgt, const float *active_sum, float eps,
                                                       int value_clip, float *__restrict__ g_mu, float *__restrict__ g_ls, float *__restrict__ g_v,
                                                       double *partials) {
    const float inv = 1.f / active_sum[0];
    float ls[GAUSS_MAX_A], iv[GAUSS_MAX_A];
    bool pass[GAUSS_MAX_A];
    if (!STATE) {
#pragma unroll
        for (int k = 0; k < GAUSS_MAX_A; k++) {
            const float lr = k < A ? ls_raw[k] : 0.f;
            ls[k] = gauss_ls_clamp(lr, ls_lo, ls_hi);
            pass[k] = gauss_ls_pass(lr, ls_lo, ls_hi);
            iv[k] = expf(-2.f * ls[k]);
        }
    }
    constexpr int NSUM = STATE ? 3 : BC_GAUSS_PART;
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; k++) acc[k] = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const PpoRow row = ppo_row(i, mv);
        const long mo = ppo_offset(row, mv);
        const long lo = STATE ? ppo_offset(row, lv) : 0;
        const float act = active[i];
        const float up = act * inv;
        float la = 0.f, sq = 0.f;
        float m3[3] = {0.f, 0.f, 0.f}, t3[3] = {0.f, 0.f, 0.f};   // (ANGLE only)
#pragma unroll
        for (int k = 0; k < GAUSS_MAX_A; k++)
            if (k < A) {
                float lsk, ivk;
                bool pk;
                if (STATE) {
                    const float lr = ls_raw[lo + k];
                    lsk = gauss_ls_clamp(lr, ls_lo, ls_hi);
                    pk = gauss_ls_pass(lr, ls_lo, ls_hi);
                    ivk = expf(-2.f * lsk);
                } else {
                    lsk = ls[k]; ivk = iv[k]; pk = pass[k];
                }
                float d = target[i * A + k] - mu[mo + k];
                if (ANGLE && k < 3) { m3[k] = mu[mo + k]; t3[k] = target[i * A + k]; }
                if (k == 0 && wrap0) d -= 2.f * floorf((d + 1.f) * 0.5f);   // heading / pi: +-1 are the same heading
                const float dd = d * d;
                la += 0.5f * dd * ivk + (fit_std ? lsk : 0.f);
                sq += dd;
                g_mu[mo + k] = -up * (d * ivk);
                const float gl = (fit_std && pk) ? up * (1.f - dd * ivk) : 0.f;
                if (STATE) g_ls[lo + k] = gl;
                else acc[3 + k] += (double)gl;
            }
        const float vn = v_now[ppo_offset(row, vv)];
        const PpoElem e = ppo_elem(0.f, 0.f, 0.f, 0.f, act, vn, value_clip ? v_old[i] : 0.f, v_tgt[i], inv, eps, 0.f, value_clip);
        acc[0] += (double)(la * act);
        acc[1] += (double)(e.lc * act);
        acc[2] += (double)((ANGLE ? diract::angle(m3, t3) : sq) * act);
        g_v[i] = e.g_v;
    }
    ppo_wave_block_sums(acc, STATE ? 3 : 3 + A, partials + (size_t)blockIdx.x * BC_GAUSS_PART);   // (A is uniform)
}

// one wave per sum (ppo_wave_sum, as k_ppo_gauss_finish).  Sums 0
// and 1 become the two losses, sum 2 and the row count are ADDED to sums[0] / sums[1] (the caller zeroes them once per update; the
// launches of a stream run in order), the sums behind them are the log_std gradient of param mode.
__global__ __launch_bounds__(64) void k_bc_gauss_finish(int nblk, const double *partials, const float *active_sum, float *losses, float *grad_log_std,
                                                        double *sums) {
    const int k = blockIdx.x;
    const double s = ppo_wave_sum(nblk, partials, BC_GAUSS_PART, k);
    if (threadIdx.x == 0) {
        if (k < 2) losses[k] = (float)s / active_sum[0];
        else if (k == 2) {
            if (sums) { sums[0] += s; sums[1] += (double)active_sum[0]; }
        } else grad_log_std[k - 3] = (float)s;
    }
}

// ---- update: cross-entropy of the teacher's label under the policy's probabilities ---------------------------------------------------
// The row of k_ppo_loss_prob -- renormalisation, probs_to_logits' clamp to [P_EPS, 1 - P_EPS], the gather -- with la = -lp, hence
// g_lp = -(active / sum active) and no entropy term; the gradient goes back through the clamp's pass rule and the normalisation as
// there.  The critic's lc and g_v are ppo_elem's and the two loss sums take ppo_block_sums / ppo_loss_finish_sums, so they carry the
// bits of ppo_loss_prob on the same inputs.  The third sum counts the live rows whose argmax over the row as given (lowest index on
// ties) is the label (bc_accuracy).
__global__ __launch_bounds__(256) void k_bc_loss_cat(long n, int A, const float *__restrict__ prob, PpoView pv, const float *__restrict__ label,
                                                     const float *active, const float *__restrict__ v_now, PpoView vv, const float *v_old,
                                                     const float *v_tgt, const float *active_sum, float eps, int value_clip,
                                                     float *__restrict__ g_prob, float *__restrict__ g_v, double *partials) {
    const float inv = 1.f / active_sum[0];
    double sa = 0.0, sc = 0.0;
    double hit[1] = {0.0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const PpoRow row = ppo_row(i, pv);
        const long po = ppo_offset(row, pv);
        float p[PPO_MAX_A];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < PPO_MAX_A; k++) { p[k] = k < A ? prob[po + k] : 0.f; if (k < A) s += p[k]; }
        const int a_idx = (int)label[i];
        int arg = 0;
        float best = p[0];
#pragma unroll
        for (int k = 1; k < PPO_MAX_A; k++)
            if (k < A && p[k] > best) { best = p[k]; arg = k; }
        float lp = 0.f;
#pragma unroll
        for (int k = 0; k < PPO_MAX_A; k++)
            if (k < A) {
                p[k] = p[k] / s;                                              // Categorical.probs
                if (k == a_idx) lp = logf(cat_clamp(p[k]));                   // probs_to_logits, gathered
            }
        const float act = active[i];
        const float up = act * inv;
        const float vn = v_now[ppo_offset(row, vv)];
        const PpoElem e = ppo_elem(0.f, 0.f, 0.f, 0.f, act, vn, value_clip ? v_old[i] : 0.f, v_tgt[i], inv, eps, 0.f, value_clip);
        sa += (double)(-lp * act);
        sc += (double)(e.lc * act);
        if (act != 0.f && arg == a_idx) hit[0] += 1.0;
        g_v[i] = e.g_v;
        float gsel = 0.f, dot = 0.f;                                          // d / d probs[label] (the other entries are 0) and its dot with probs
#pragma unroll
        for (int k = 0; k < PPO_MAX_A; k++)
            if (k < A && k == a_idx) {
                const float c = cat_clamp(p[k]);
                const bool pass = cat_pass(p[k]);
                gsel = pass ? -up / c : 0.f;
                dot = gsel * p[k];
            }
#pragma unroll
        for (int k = 0; k < PPO_MAX_A; k++)
            if (k < A) g_prob[po + k] = ((k == a_idx ? gsel : 0.f) - dot) / s;   // through probs = prob / prob.sum(-1)
    }
    ppo_block_sums(sa, sc, partials);
    ppo_wave_block_sums(hit, 1, partials + 2 * PPO_BLOCKS + blockIdx.x);
}

// workgroup 0: k_ppo_loss_finish; workgroup 1 (launched with sums only): the hit count and the row count, ADDED to sums[0] / sums[1]
__global__ __launch_bounds__(64) void k_bc_cat_finish(int nblk, const double *partials, const float *active_sum, float *losses, double *sums) {
    if (blockIdx.x == 0) { ppo_loss_finish_sums(nblk, partials, active_sum, losses); return; }
    const double s = ppo_wave_sum(nblk, partials + 2 * PPO_BLOCKS, 1, 0);
    if (threadIdx.x == 0) { sums[0] += s; sums[1] += (double)active_sum[0]; }
}

// ---- rollout: the teacher's label into the buffer, the teacher's action over the network's where the environment follows it --------
// One lane per (environment, pursuer).  The label is written for every environment (DAgger labels the learner's own states); nothing
// but row t of a_star (N rows, row_stride floats apart) and the followed rows of the action tensor is touched.
// MODE GAUSS_DIRECTION: the label is the unit vector of the commanded angles and the speed (diract::label), four floats per pursuer.
template <int MODE>
__global__ __launch_bounds__(256) void k_e3d_bc_select(int N, int P, const double *__restrict__ guide, const unsigned char *__restrict__ follow,
                                                       double bound, double *__restrict__ env_action, float *__restrict__ a_star, long row_stride) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * P) return;
    const int env = idx / P, p = idx - env * P;
    const bool f = follow[env] != 0;
    constexpr bool TANH = MODE == GAUSS_TANH, DIR = MODE == GAUSS_DIRECTION;
    float *dst = a_star + (long)env * row_stride + (long)p * (DIR ? diract::LATENT : 3);
    double gs[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double g = guide[(long)idx * 3 + a];
        gs[a] = g;
        if (!DIR) dst[a] = TANH ? (float)atanh(fmin(fmax(g, -bound), bound)) : (float)g;
        if (f) env_action[(long)idx * 3 + a] = g;
    }
    if (DIR) diract::label(gs, dst);
}

__global__ __launch_bounds__(256) void k_n2n_bc_select(int N, int P, const int *__restrict__ guide, const unsigned char *__restrict__ follow,
                                                       int *__restrict__ a_n, float *__restrict__ a_star, long row_stride) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * P) return;
    const int env = idx / P, p = idx - env * P;
    const int k = guide[idx];
    a_star[(long)env * row_stride + p] = (float)k;
    if (follow[env] != 0) a_n[idx] = k;
}

}  // namespace

extern "C" {

int64_t bc_loss_workspace(void) { return (int64_t)PPO_BLOCKS * BC_GAUSS_PART * sizeof(double); }   // (the categorical call needs 3 per block)

int bc_loss_gauss_ex_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                             int64_t m_s2, const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2, float log_std_min,
                             float log_std_max, int32_t fit_std, int32_t wrap0, int32_t metric, const float *target, const float *active,
                             const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                             const float *active_sum, float epsilon, int32_t use_value_clip, float *losses, float *grad_values, double *sums,
                             void *workspace, void *stream) {
    if (n < 1 || A < 1 || A > GAUSS_MAX_A || d1 < 1 || d2 < 1 || (n % (d1 * d2)) || !mu || !grad_mu || !ls_raw || !grad_log_std ||
        !gauss_ex_bounds_ok(log_std_min, log_std_max) || !target || !active || !values_now || !v_target || !active_sum || !losses || !grad_values ||
        !workspace || (use_value_clip && !values_old) || (metric != BC_METRIC_SQ && metric != BC_METRIC_ANGLE) || (metric == BC_METRIC_ANGLE && A < 3))
        return MO_ERR_BAD_ARG;
    if (metric == BC_METRIC_ANGLE) wrap0 = 0;   // a direction vector has no wrapped dimension
    const bool state = (l_s0 | l_s1 | l_s2) != 0;
    long blocks = (n + 255) / 256;
    if (blocks > PPO_BLOCKS) blocks = PPO_BLOCKS;
    const PpoView mv{d1, d2, m_s0, m_s1, m_s2}, lv{d1, d2, l_s0, l_s1, l_s2}, vv{d1, d2, v_s0, v_s1, v_s2};
    hipStream_t st = (hipStream_t)stream;
#define BC_GAUSS(S, M) hipLaunchKernelGGL((k_bc_loss_gauss<S, M>), dim3((unsigned)blocks), dim3(256), 0, st, (long)n, (int)A, mu, mv, ls_raw, lv,  \
                                          log_std_min, log_std_max, (int)(fit_std != 0), (int)(wrap0 != 0), target, active, values_now, vv, values_old, \
                                          v_target, active_sum, epsilon, (int)use_value_clip, grad_mu, grad_log_std, grad_values, (double *)workspace)
    if (metric == BC_METRIC_ANGLE) { if (state) BC_GAUSS(true, true); else BC_GAUSS(false, true); }
    else if (state) BC_GAUSS(true, false);
    else BC_GAUSS(false, false);
#undef BC_GAUSS
    // state mode: the three sums only (grad_log_std was written per row); param mode: the A log_std sums as well
    hipLaunchKernelGGL(k_bc_gauss_finish, dim3(state ? 3 : 3 + A), dim3(64), 0, st, (int)blocks, (const double *)workspace, active_sum, losses,
                       grad_log_std, sums);
    return (int)hipGetLastError();
}

int bc_loss_gauss_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1, int64_t m_s2,
                          const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2, float log_std_min, float log_std_max,
                          int32_t fit_std, int32_t wrap0, const float *target, const float *active, const float *values_now, int64_t v_s0,
                          int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target, const float *active_sum, float epsilon,
                          int32_t use_value_clip, float *losses, float *grad_values, double *sums, void *workspace, void *stream) {
    return bc_loss_gauss_ex_fwd_bwd(n, A, mu, grad_mu, d1, d2, m_s0, m_s1, m_s2, ls_raw, grad_log_std, l_s0, l_s1, l_s2, log_std_min, log_std_max,
                                    fit_std, wrap0, BC_METRIC_SQ, target, active, values_now, v_s0, v_s1, v_s2, values_old, v_target, active_sum,
                                    epsilon, use_value_clip, losses, grad_values, sums, workspace, stream);
}

int bc_loss_cat_fwd_bwd(int64_t n, int32_t A, const float *prob, float *grad_prob, int64_t d1, int64_t d2, int64_t p_s0, int64_t p_s1, int64_t p_s2,
                        const float *label, const float *active, const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2,
                        const float *values_old, const float *v_target, const float *active_sum, float epsilon, int32_t use_value_clip,
                        float *losses, float *grad_values, double *sums, void *workspace, void *stream) {
    if (n < 1 || A < 1 || A > PPO_MAX_A || d1 < 1 || d2 < 1 || (n % (d1 * d2)) || !prob || !grad_prob || !label || !active || !values_now ||
        !v_target || !active_sum || !losses || !grad_values || !workspace || (use_value_clip && !values_old))
        return MO_ERR_BAD_ARG;
    long blocks = (n + 255) / 256;
    if (blocks > PPO_BLOCKS) blocks = PPO_BLOCKS;
    const PpoView pv{d1, d2, p_s0, p_s1, p_s2}, vv{d1, d2, v_s0, v_s1, v_s2};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bc_loss_cat, dim3((unsigned)blocks), dim3(256), 0, st, (long)n, (int)A, prob, pv, label, active, values_now, vv, values_old,
                       v_target, active_sum, epsilon, (int)use_value_clip, grad_prob, grad_values, (double *)workspace);
    hipLaunchKernelGGL(k_bc_cat_finish, dim3(sums ? 2 : 1), dim3(64), 0, st, (int)blocks, (const double *)workspace, active_sum, losses, sums);
    return (int)hipGetLastError();
}

int e3d_bc_select(int32_t N, int32_t P, const double *guide, const uint8_t *follow, int32_t squash, double bound, double *env_action, float *a_star,
                  int64_t row_stride, void *stream) {
    if (N < 0 || P < 1 || (int64_t)N * P > INT32_MAX || !guide || !follow || !env_action || !a_star ||
        (squash != GAUSS_CLIP && squash != GAUSS_TANH && squash != GAUSS_DIRECTION) ||
        row_stride < (int64_t)P * (squash == GAUSS_DIRECTION ? diract::LATENT : 3) || (squash == GAUSS_TANH && !(bound > 0.0 && bound < 1.0)))
        return MO_ERR_BAD_ARG;
    if (N == 0) return 0;
    const unsigned grid = (unsigned)(((int64_t)N * P + 255) / 256);
#define E3D_SEL(M) hipLaunchKernelGGL((k_e3d_bc_select<M>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (int)N, (int)P, guide, follow, bound, env_action, a_star, (long)row_stride)
    if (squash == GAUSS_DIRECTION) E3D_SEL(GAUSS_DIRECTION);   // the label row holds four floats per pursuer; bound is ignored
    else if (squash) E3D_SEL(GAUSS_TANH);
    else E3D_SEL(GAUSS_CLIP);
#undef E3D_SEL
    return (int)hipGetLastError();
}

int n2n_bc_select(int32_t N, int32_t P, const int32_t *guide, const uint8_t *follow, int32_t *a_n, float *a_star, int64_t row_stride, void *stream) {
    if (N < 0 || P < 1 || (int64_t)N * P > INT32_MAX || !guide || !follow || !a_n || !a_star || row_stride < (int64_t)P) return MO_ERR_BAD_ARG;
    if (N == 0) return 0;
    const unsigned grid = (unsigned)(((int64_t)N * P + 255) / 256);
    hipLaunchKernelGGL(k_n2n_bc_select, dim3(grid), dim3(256), 0, (hipStream_t)stream, (int)N, (int)P, guide, follow, a_n, a_star, (long)row_stride);
    return (int)hipGetLastError();
}

}  // extern "C"
