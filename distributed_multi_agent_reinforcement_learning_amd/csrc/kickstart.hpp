// kickstart.hpp -- teacher-regularised PPO of the env_3d / env_n2n trainers (algo.bc_coef; kickstart.py; C ABI:
// include/mappo_ops.h ppo_bc_loss_gauss_fwd_bwd / ppo_bc_loss_cat_fwd_bwd; specification: tests/kickstart_ref.py).  Included once, from
// csrc/mappo_ops.hip after imitation.hpp: it reuses the PPO row (ppo_elem, PPO_BLOCKS, ppo_block_sums), the steps the strided loss
// kernels share (PpoView / ppo_row / ppo_offset, ppo_wave_block_sums, ppo_wave_sum, the categorical row: PPO_MAX_A, P_EPS,
// cat_clamp / cat_pass), the diagnostics (ppodiag, ppo_diag_block_sums, ppo_diag_finish_wave), gauss_policy.hpp's
// GAUSS_MAX_A, log-std row (gauss_ls_clamp / gauss_ls_pass, gauss_inv_var / gauss_ent_term), tanh_log_jac and bounds check, and
// imitation.hpp's metric codes.
#pragma once

namespace {

// ---- Gaussian policy: the PPO row and the imitation row of one sample in one pass ------------------------------------------------------
// Per row mu, ls = clamp(ls_raw, lo, hi) and iv = 1 / exp(ls)^2 are loaded once.  The PPO row is k_ppo_loss_gauss_ex's, expression by
// expression; the imitation row is k_bc_loss_gauss's on the same iv: d* = target - mu (dimension 0 modulo 2 into [-1, 1) under wrap0),
// la_bc = sum_a 0.5 d*^2 iv + (fit_std ? ls : 0).  g_mu = g_mu_ppo + coef g_mu_bc, g_ls = g_ls_ppo + coef g_ls_bc on the closed range
// [lo, hi] (the imitation part exactly 0 without fit_std), per row (STATE) or summed through the partials (param mode); g_v is
// ppo_elem's.  The critic sum takes k_ppo_loss_gauss_ex's reduction (wave butterflies, the four waves in a fixed order, the finish in
// block order), so losses[1] and g_v carry the bits of ppo_loss_gauss_ex on the same inputs.  No atomics: the same bits every run.
// AT > 0 fixes the action count (state mode), AT = 0 takes the runtime A (as k_ppo_loss_gauss_ex).
constexpr int KS_GAUSS_HEAD = 4;                            // doubles per block in front of the log_std sums:
constexpr int KS_GAUSS_PART = KS_GAUSS_HEAD + GAUSS_MAX_A;  // PPO actor sum, critic sum, imitation sum, metric sum, log_std gradient [A]

template <int AT, bool STATE, bool TANH, bool ANGLE, bool DIAG>
__global__ __launch_bounds__(256) void k_ppo_bc_loss_gauss(long n, int A_rt, const float *__restrict__ mu, PpoView mv, const float *__restrict__ ls_raw,
                                                           PpoView lv, float ls_lo, float ls_hi, int fit_std, int wrap0, float coef,
                                                           const float *__restrict__ action, const float *__restrict__ target, const float *lp_old,
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
    constexpr int NSUM = STATE ? KS_GAUSS_HEAD : KS_GAUSS_HEAD + NA;
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
        float d[NA], ds[NA];                                       // action - mu, target - mu
        float lp = 0.f, jac = 0.f, lb = 0.f, sq = 0.f;
        float m3[3] = {0.f, 0.f, 0.f}, t3[3] = {0.f, 0.f, 0.f};   // (ANGLE only)
#pragma unroll
        for (int k = 0; k < NA; k++) {
            d[k] = 0.f; ds[k] = 0.f;
            if (k < A) {
                const float u = action[i * A + k], m = mu[mo + k], t = target[i * A + k];
                d[k] = u - m;
                lp += -(d[k] * d[k]) * iv[k] * 0.5f - ls[k] - HALF_LN_2PI;
                if (TANH) jac += tanh_log_jac(u);
                float r = t - m;
                if (ANGLE && k < 3) { m3[k] = m; t3[k] = t; }
                if (k == 0 && wrap0) r -= 2.f * floorf((r + 1.f) * 0.5f);   // heading / pi: +-1 are the same heading
                ds[k] = r;
                const float dd = r * r;
                lb += 0.5f * dd * iv[k] + (fit_std ? ls[k] : 0.f);
                sq += dd;
            }
        }
        if (TANH) lp -= jac;
        const float act = active[i];
        const float up = act * inv, upc = up * coef;
        const float vn = v_now[ppo_offset(row, vv)];
        float d_lr = 0.f, d_vt = 0.f;
        if (DIAG) { d_lr = lp - lp_old[i]; d_vt = v_tgt[i]; }
        const PpoElem e = ppo_elem(lp, ent, lp_old[i], adv[i], act, vn, value_clip ? v_old[i] : 0.f, v_tgt[i], inv, eps, ent_coef, value_clip);
        acc[0] += (double)(e.la * act);
        acc[1] += (double)(e.lc * act);
        acc[2] += (double)(lb * act);
        acc[3] += (double)((ANGLE ? diract::angle(m3, t3) : sq) * act);
        g_v[i] = e.g_v;
#pragma unroll
        for (int k = 0; k < NA; k++)
            if (k < A) {
                const float q = d[k] * iv[k], qs = ds[k] * iv[k];
                g_mu[mo + k] = e.g_lp * q - upc * qs;
                float gl = e.g_lp * (q * d[k] - 1.f) + e.g_ent;
                if (fit_std) gl += upc * (1.f - qs * ds[k]);
                gl = pass[k] ? gl : 0.f;
                if (STATE) g_ls[lo + k] = gl;
                else acc[KS_GAUSS_HEAD + k] += (double)gl;
            }
        if (DIAG && act != 0.f) ppodiag::row(dg, d_lr, expf(d_lr), ent, vn, d_vt, eps);
    }
    ppo_wave_block_sums(acc, STATE ? KS_GAUSS_HEAD : KS_GAUSS_HEAD + A, partials + (size_t)blockIdx.x * KS_GAUSS_PART);   // (A is uniform)
    if (DIAG) ppo_diag_block_sums(dg, partials + (size_t)PPO_BLOCKS * KS_GAUSS_PART);
}

// Workgroup 0: losses[0] = mean PPO actor loss + coef * mean imitation loss, and the imitation sum ADDED to sums[2]; 1: losses[1] as
// k_ppo_gauss_finish forms it; 2: the metric sum and the row count ADDED to sums[0] / sums[1]; 3 .. nsum - 1: the log_std gradient of
// param mode; the eight after them (diag given): ppo_diag_finish_wave.  sums may be NULL.
__global__ __launch_bounds__(64) void k_ppo_bc_gauss_finish(int nsum, int nblk, const double *partials, const float *active_sum, float coef,
                                                            float *losses, float *grad_log_std, double *sums, double *diag) {
    const int k = blockIdx.x;
    if (k >= nsum) { ppo_diag_finish_wave(k - nsum, nblk, partials + (size_t)PPO_BLOCKS * KS_GAUSS_PART, diag); return; }
    if (k == 0) {
        const double sp = ppo_wave_sum(nblk, partials, KS_GAUSS_PART, 0), sb = ppo_wave_sum(nblk, partials, KS_GAUSS_PART, 2);
        if (threadIdx.x == 0) {
            losses[0] = (float)sp / active_sum[0] + coef * ((float)sb / active_sum[0]);
            if (sums) sums[2] += sb;
        }
        return;
    }
    const double s = ppo_wave_sum(nblk, partials, KS_GAUSS_PART, k == 1 ? 1 : (k == 2 ? 3 : k + 1));
    if (threadIdx.x == 0) {
        if (k == 1) losses[1] = (float)s / active_sum[0];
        else if (k == 2) {
            if (sums) { sums[0] += s; sums[1] += (double)active_sum[0]; }
        } else grad_log_std[k - 3] = (float)s;
    }
}

// ---- Categorical policy: the row of k_ppo_loss_prob and the row of k_bc_loss_cat on one normalised p[] ---------------------------------
// The two gradients with respect to probs are added before the step back through probs = prob / prob.sum(-1), which is linear in them.
// The PPO actor sum and the critic sum take ppo_block_sums and a serial finish in block order, so losses[1] and g_v carry the bits of
// ppo_loss_prob on the same inputs; the imitation sum and the label hits (argmax over the row as given, lowest index on ties) leave
// through partials[2 PPO_BLOCKS + 2 b + {0, 1}], the diagnostics behind them.
constexpr int KS_CAT_PART = 4;   // doubles per block

template <bool DIAG>
__global__ __launch_bounds__(256) void k_ppo_bc_loss_cat(long n, int A, const float *__restrict__ prob, PpoView pv, const float *__restrict__ action,
                                                         const float *__restrict__ label, float coef, const float *lp_old, const float *adv,
                                                         const float *active, const float *__restrict__ v_now, PpoView vv, const float *v_old,
                                                         const float *v_tgt, const float *active_sum, float eps, float ent_coef, int value_clip,
                                                         float *__restrict__ g_prob, float *__restrict__ g_v, double *partials) {
    const float inv = 1.f / active_sum[0];
    double sa = 0.0, sc = 0.0;
    double x[2] = {0.0, 0.0};   // the imitation sum, the label hits
    double dg[ppodiag::NSUM] = {};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const PpoRow row = ppo_row(i, pv);
        const long po = ppo_offset(row, pv);
        float p[PPO_MAX_A], l[PPO_MAX_A];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < PPO_MAX_A; k++) { p[k] = k < A ? prob[po + k] : 0.f; if (k < A) s += p[k]; }
        const int a_idx = (int)action[i], b_idx = (int)label[i];
        int arg = 0;
        float best = p[0];
#pragma unroll
        for (int k = 1; k < PPO_MAX_A; k++)
            if (k < A && p[k] > best) { best = p[k]; arg = k; }
        float lp = 0.f, lpb = 0.f, plp = 0.f;
#pragma unroll
        for (int k = 0; k < PPO_MAX_A; k++)
            if (k < A) {
                p[k] = p[k] / s;                                              // Categorical.probs
                l[k] = logf(cat_clamp(p[k]));                                 // probs_to_logits
                if (k == a_idx) lp = l[k];
                if (k == b_idx) lpb = l[k];
                plp += l[k] * p[k];
            }
        const float act = active[i];
        const float upc = act * inv * coef;
        const float vn = v_now[ppo_offset(row, vv)];
        float d_lr = 0.f, d_vt = 0.f;
        const float d_ent = -plp;
        if (DIAG) { d_lr = lp - lp_old[i]; d_vt = v_tgt[i]; }
        const PpoElem e = ppo_elem(lp, -plp, lp_old[i], adv[i], act, vn, value_clip ? v_old[i] : 0.f, v_tgt[i], inv, eps, ent_coef, value_clip);
        sa += (double)(e.la * act);
        sc += (double)(e.lc * act);
        x[0] += (double)(-lpb * act);
        if (act != 0.f && arg == b_idx) x[1] += 1.0;
        g_v[i] = e.g_v;
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < PPO_MAX_A; k++)
            if (k < A) {
                // d / d logits[k]: log_prob's gather, entropy's logits * probs, and the label's -coef (active / sum active)
                const float c = cat_clamp(p[k]);
                const bool pass = cat_pass(p[k]);
                const float gl = (k == a_idx ? e.g_lp : 0.f) - e.g_ent * p[k] - (k == b_idx ? upc : 0.f);
                l[k] = (pass ? gl / c : 0.f) - e.g_ent * l[k];                    // d / d probs[k]
                dot += l[k] * p[k];
            }
#pragma unroll
        for (int k = 0; k < PPO_MAX_A; k++)
            if (k < A) g_prob[po + k] = (l[k] - dot) / s;                        // through probs = prob / prob.sum(-1)
        if (DIAG && act != 0.f) ppodiag::row(dg, d_lr, expf(d_lr), d_ent, vn, d_vt, eps);
    }
    ppo_block_sums(sa, sc, partials);
    ppo_wave_block_sums(x, 2, partials + 2 * PPO_BLOCKS + 2 * blockIdx.x);
    if (DIAG) ppo_diag_block_sums(dg, partials + KS_CAT_PART * PPO_BLOCKS);
}

// Workgroup 0: the imitation sum by the whole wave, then the two losses (lanes 0 and 1 walk the blocks in order, as k_ppo_loss_finish)
// and the imitation sum ADDED to sums[2]; 1: the hits and the row count ADDED to sums[0] / sums[1]; the eight after them (diag given):
// ppo_diag_finish_wave.  sums may be NULL.
__global__ __launch_bounds__(64) void k_ppo_bc_cat_finish(int nblk, const double *partials, const float *active_sum, float coef, float *losses,
                                                          double *sums, double *diag) {
    if (blockIdx.x >= 2) { ppo_diag_finish_wave(blockIdx.x - 2, nblk, partials + KS_CAT_PART * PPO_BLOCKS, diag); return; }
    if (blockIdx.x == 0) {
        const double b = ppo_wave_sum(nblk, partials + 2 * PPO_BLOCKS, 2, 0);
        if (threadIdx.x < 2) {
            double s = 0.0;
            for (int j = 0; j < nblk; j++) s += partials[2 * j + threadIdx.x];
            if (threadIdx.x == 0) {
                losses[0] = (float)s / active_sum[0] + coef * ((float)b / active_sum[0]);
                if (sums) sums[2] += b;
            } else losses[1] = (float)s / active_sum[0];
        }
        return;
    }
    const double h = ppo_wave_sum(nblk, partials + 2 * PPO_BLOCKS, 2, 1);
    if (threadIdx.x == 0 && sums) { sums[0] += h; sums[1] += (double)active_sum[0]; }
}

static bool ks_coef_ok(float coef) { return coef >= 0.f && coef <= 3.402823466e+38f; }   // finite and >= 0 (NaN fails)

}  // namespace

extern "C" {

// both launches, with or without the diagnostics
int64_t ppo_bc_loss_workspace(void) { return (int64_t)PPO_BLOCKS * (KS_GAUSS_PART + ppodiag::NSUM) * sizeof(double); }

int ppo_bc_loss_gauss_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                              int64_t m_s2, const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2, float log_std_min,
                              float log_std_max, int32_t squash, int32_t fit_std, int32_t wrap0, int32_t metric, const float *action,
                              const float *target, const float *logp_old, const float *adv, const float *active, const float *values_now,
                              int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target, const float *active_sum,
                              float epsilon, float entropy_coef, float coef, int32_t use_value_clip, float *losses, float *grad_values, double *sums,
                              double *diag, void *workspace, void *stream) {
    if (n < 1 || A < 1 || A > GAUSS_MAX_A || d1 < 1 || d2 < 1 || (n % (d1 * d2)) || !mu || !grad_mu || !ls_raw || !grad_log_std ||
        (squash != GAUSS_CLIP && squash != GAUSS_TANH && squash != GAUSS_DIRECTION) || !gauss_ex_bounds_ok(log_std_min, log_std_max) || !action ||
        !target || !logp_old || !adv || !active || !values_now || !v_target || !active_sum || !losses || !grad_values || !workspace ||
        (use_value_clip && !values_old) || (metric != BC_METRIC_SQ && metric != BC_METRIC_ANGLE) || (metric == BC_METRIC_ANGLE && A < 3) ||
        !ks_coef_ok(coef))
        return MO_ERR_BAD_ARG;
    const bool state = (l_s0 | l_s1 | l_s2) != 0;
    // the diagnostics in state mode exist at the two widths an env_3d policy of this feature can have (algo.bc_coef needs env.action_dim 3:
    // three latent dimensions, four in direction mode): one of the runtime-A state instances with DIAG would be the one kernel here that
    // needs scratch (as ppo_loss_gauss_ex_fwd_bwd_diag stops at GAUSS_SD_MAX_A)
    if (diag && state && A != 3 && A != 4) return MO_ERR_BAD_ARG;
    if (squash == GAUSS_DIRECTION) squash = GAUSS_CLIP;   // the clip instances on the four latent dimensions
    if (metric == BC_METRIC_ANGLE) wrap0 = 0;             // a direction vector has no wrapped dimension
    long blocks = (n + 255) / 256;
    if (blocks > PPO_BLOCKS) blocks = PPO_BLOCKS;
    const PpoView mv{d1, d2, m_s0, m_s1, m_s2}, lv{d1, d2, l_s0, l_s1, l_s2}, vv{d1, d2, v_s0, v_s1, v_s2};
    hipStream_t st = (hipStream_t)stream;
#define KS_GAUSS(AT, S, T, M, D) hipLaunchKernelGGL((k_ppo_bc_loss_gauss<AT, S, T, M, D>), dim3((unsigned)blocks), dim3(256), 0, st, (long)n, (int)A, mu, \
                                                    mv, ls_raw, lv, log_std_min, log_std_max, (int)(fit_std != 0), (int)(wrap0 != 0), coef, action, target, \
                                                    logp_old, adv, active, values_now, vv, values_old, v_target, active_sum, epsilon, entropy_coef, \
                                                    (int)use_value_clip, grad_mu, grad_log_std, grad_values, (double *)workspace)
#define KS_GAUSS_D(AT, S, T, M) do { if (diag) KS_GAUSS(AT, S, T, M, true); else KS_GAUSS(AT, S, T, M, false); } while (0)
#define KS_GAUSS_M(AT, S, T) do { if (metric == BC_METRIC_ANGLE) KS_GAUSS_D(AT, S, T, true); else KS_GAUSS_D(AT, S, T, false); } while (0)
#define KS_GAUSS_T(AT, S) do { if (squash) KS_GAUSS_M(AT, S, true); else KS_GAUSS_M(AT, S, false); } while (0)
    // state mode at the two widths a policy of this feature can have fixes the action count; every other call takes the runtime-A shape
    if (state && A == 3) KS_GAUSS_T(3, true);
    else if (state && A == 4) KS_GAUSS_T(4, true);
    else if (!state) KS_GAUSS_T(0, false);
    else if (metric == BC_METRIC_ANGLE) { if (squash) KS_GAUSS(0, true, true, true, false); else KS_GAUSS(0, true, false, true, false); }
    else if (squash) KS_GAUSS(0, true, true, false, false);
    else KS_GAUSS(0, true, false, false, false);
#undef KS_GAUSS_T
#undef KS_GAUSS_M
#undef KS_GAUSS_D
#undef KS_GAUSS
    // state mode: the four sums only (grad_log_std was written per row); param mode: the A log_std sums as well
    const int nsum = state ? 3 : 3 + A;
    hipLaunchKernelGGL(k_ppo_bc_gauss_finish, dim3(nsum + (diag ? ppodiag::NSUM : 0)), dim3(64), 0, st, nsum, (int)blocks,
                       (const double *)workspace, active_sum, coef, losses, grad_log_std, sums, diag);
    return (int)hipGetLastError();
}

int ppo_bc_loss_cat_fwd_bwd(int64_t n, int32_t A, const float *prob, float *grad_prob, int64_t d1, int64_t d2, int64_t p_s0, int64_t p_s1,
                            int64_t p_s2, const float *action, const float *label, const float *logp_old, const float *adv, const float *active,
                            const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                            const float *active_sum, float epsilon, float entropy_coef, float coef, int32_t use_value_clip, float *losses,
                            float *grad_values, double *sums, double *diag, void *workspace, void *stream) {
    if (n < 1 || A < 1 || A > PPO_MAX_A || d1 < 1 || d2 < 1 || (n % (d1 * d2)) || !prob || !grad_prob || !action || !label || !logp_old || !adv ||
        !active || !values_now || !v_target || !active_sum || !losses || !grad_values || !workspace || (use_value_clip && !values_old) ||
        !ks_coef_ok(coef))
        return MO_ERR_BAD_ARG;
    long blocks = (n + 255) / 256;
    if (blocks > PPO_BLOCKS) blocks = PPO_BLOCKS;
    const PpoView pv{d1, d2, p_s0, p_s1, p_s2}, vv{d1, d2, v_s0, v_s1, v_s2};
    hipStream_t st = (hipStream_t)stream;
#define KS_CAT(D) hipLaunchKernelGGL((k_ppo_bc_loss_cat<D>), dim3((unsigned)blocks), dim3(256), 0, st, (long)n, (int)A, prob, pv, action, label, coef, \
                                     logp_old, adv, active, values_now, vv, values_old, v_target, active_sum, epsilon, entropy_coef, \
                                     (int)use_value_clip, grad_prob, grad_values, (double *)workspace)
    if (diag) KS_CAT(true);
    else KS_CAT(false);
#undef KS_CAT
    hipLaunchKernelGGL(k_ppo_bc_cat_finish, dim3(2 + (diag ? ppodiag::NSUM : 0)), dim3(64), 0, st, (int)blocks, (const double *)workspace, active_sum,
                       coef, losses, sums, diag);
    return (int)hipGetLastError();
}

}  // extern "C"
