// mappo_split.hip -- the split-bf16 GEMM (and GRU sequence) kernels of libmappo_ops.so: a second translation unit so that a change
// to these kernels does not recompile csrc/mappo_ops.hip.  C ABI: include/mappo_ops.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "mappo_ops.h"
#include "gru_nets_check.hpp"
#include "sb_gemm.hpp"
#include "sb_encoder_tail.hpp"
#include "sb_encoder_tail_bwd.hpp"
#include "sb_gru_seq.hpp"
#include "gnn_pairs.hpp"
#include "att_agg.hpp"
#include "fcra_att.hpp"
#include "fcra_pool.hpp"
#include "fcra_team.hpp"
#include "layer_norm.hpp"
#include "pool_agg.hpp"
#include "sem_att.hpp"
#include "team_pool.hpp"
#include "team_pool_heads.hpp"

extern "C" {

static int sb_gemm_any(int64_t R, int32_t N, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias, int32_t relu,
                       const float *addend, int64_t lda, float *Y, int64_t ldy, uint8_t *ybits, int64_t ldyb, void *stream) {
    if (R < 0 || !X || !W || !Y || ldx < K || ldw < K || ldy < N || (addend && lda < N)) return MO_ERR_BAD_ARG;
    if ((ldx & 3) || (ldw & 3) || (ldy & 3) || (lda & 3) || ((uintptr_t)X & 15) || ((uintptr_t)W & 15) || ((uintptr_t)Y & 15) || ((uintptr_t)addend & 15) ||
        ((uintptr_t)bias & 15))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (N == 128 && K == 128) return launch_sb_gemm_best<4, 1>(R, X, ldx, W, ldw, bias, addend, lda, Y, ldy, relu, st, ybits, ldyb);
    if (N == 128 && K == 256) return launch_sb_gemm_best<8, 1>(R, X, ldx, W, ldw, bias, addend, lda, Y, ldy, relu, st, ybits, ldyb);
    if (ybits) return MO_ERR_BAD_ARG;      // sign bits: the ReLU layers' shapes (128 outputs from 128 / 256 inputs)
    if (N == 128 && K == 384) return launch_sb_gemm_best<12, 1>(R, X, ldx, W, ldw, bias, addend, lda, Y, ldy, relu, st);
    if (N == 256 && K == 128) return launch_sb_gemm_best<4, 2>(R, X, ldx, W, ldw, bias, addend, lda, Y, ldy, relu, st);
    if (N == 384 && K == 128) return launch_sb_gemm_best<4, 3>(R, X, ldx, W, ldw, bias, addend, lda, Y, ldy, relu, st);
    return MO_ERR_BAD_ARG;
}

int sb_gemm(int64_t R, int32_t N, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias, int32_t relu,
            const float *addend, int64_t lda, float *Y, int64_t ldy, void *stream) {
    return sb_gemm_any(R, N, K, X, ldx, W, ldw, bias, relu, addend, lda, Y, ldy, nullptr, 0, stream);
}

int sb_gemm_signs(int64_t R, int32_t N, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias, int32_t relu,
                  const float *addend, int64_t lda, float *Y, int64_t ldy, uint8_t *y_sign_bits, int64_t ld_bytes, void *stream) {
    if (!y_sign_bits || ld_bytes < N / 8) return MO_ERR_BAD_ARG;
    return sb_gemm_any(R, N, K, X, ldx, W, ldw, bias, relu, addend, lda, Y, ldy, y_sign_bits, ld_bytes, stream);
}

int64_t sb_gemm_masked_workspace(int32_t N) { return N > 0 ? (int64_t)1024 * N * 4 : 0; }   // one row of partial sums per workgroup (<= CUs)

int sb_gemm_masked(int64_t R, int32_t N, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const float *M, int64_t ldm,
                   int32_t mask_cols, float *Y, int64_t ldy, float *colsum, void *workspace, void *stream) {
    if (R < 0 || !X || !W || !M || !Y || !colsum || !workspace || ldx < K || ldw < K || ldy < N || ldm < N) return MO_ERR_BAD_ARG;
    if (mask_cols < 0 || mask_cols > N || (mask_cols & 127)) return MO_ERR_BAD_ARG;
    if ((ldx & 3) || (ldw & 3) || (ldy & 3) || (ldm & 3) || ((uintptr_t)X & 15) || ((uintptr_t)W & 15) || ((uintptr_t)Y & 15) || ((uintptr_t)M & 15) ||
        ((uintptr_t)colsum & 15) || ((uintptr_t)workspace & 15))
        return MO_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (R == 0) return (int)hipMemsetAsync(colsum, 0, (size_t)N * 4, st);
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    if (cus > 512) return MO_ERR_BAD_ARG;          // (the workspace holds 1024 rows: up to two workgroups per CU)
    float *part = (float *)workspace;
    const int mt = mask_cols / 128;
    if (N == 256 && K == 128) return launch_sb_gemm<4, 2, SBG_MASK_OPT_256>(R, X, ldx, W, ldw, nullptr, M, ldm, Y, ldy, 0, st, mt, part, colsum);
    if (N == 384 && K == 128) return launch_sb_gemm<4, 3, SBG_MASK_OPT_384>(R, X, ldx, W, ldw, nullptr, M, ldm, Y, ldy, 0, st, mt, part, colsum);
    if (N == 128 && K == 384) return launch_sb_gemm<12, 1, SBG_MASK_OPT_K384>(R, X, ldx, W, ldw, nullptr, M, ldm, Y, ldy, 0, st, mt, part, colsum);
    return MO_ERR_BAD_ARG;
}

int sb_gemm_masked_bits(int64_t R, int32_t N, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const uint8_t *sign_bits,
                        int64_t ld_bytes, int32_t mask_cols, float *Y, int64_t ldy, float *colsum, void *workspace, void *stream) {
    if (R < 0 || !X || !W || !sign_bits || !Y || !colsum || !workspace || ldx < K || ldw < K || ldy < N || ld_bytes < N / 8) return MO_ERR_BAD_ARG;
    if (mask_cols < 0 || mask_cols > N || (mask_cols & 127)) return MO_ERR_BAD_ARG;
    if ((ldx & 3) || (ldw & 3) || (ldy & 3) || ((uintptr_t)X & 15) || ((uintptr_t)W & 15) || ((uintptr_t)Y & 15) || ((uintptr_t)colsum & 15) ||
        ((uintptr_t)workspace & 15))
        return MO_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (R == 0) return (int)hipMemsetAsync(colsum, 0, (size_t)N * 4, st);
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    if (cus > 512) return MO_ERR_BAD_ARG;
    float *part = (float *)workspace;
    const float *m = (const float *)sign_bits;     // (the kernel reads it as bytes: OPT bit 16)
    const int mt = mask_cols / 128;
    if (N == 256 && K == 128) return launch_sb_gemm<4, 2, SBG_MASK_OPT_256 | 16>(R, X, ldx, W, ldw, nullptr, m, ld_bytes, Y, ldy, 0, st, mt, part, colsum);
    if (N == 384 && K == 128) return launch_sb_gemm<4, 3, SBG_MASK_OPT_384 | 16>(R, X, ldx, W, ldw, nullptr, m, ld_bytes, Y, ldy, 0, st, mt, part, colsum);
    if (N == 128 && K == 384) return launch_sb_gemm<12, 1, SBG_MASK_OPT_K384 | 16>(R, X, ldx, W, ldw, nullptr, m, ld_bytes, Y, ldy, 0, st, mt, part, colsum);
    return MO_ERR_BAD_ARG;
}

int sb_gemm_n128(int64_t R, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias, int32_t relu, const float *addend,
                 int64_t lda, float *Y, int64_t ldy, void *stream) {
    return sb_gemm(R, 128, K, X, ldx, W, ldw, bias, relu, addend, lda, Y, ldy, stream);
}

int sb_encoder_tail(int64_t Rs, const float *m3, int64_t ldx, const float *w_agg, const float *b_agg, const float *Ws, int64_t ldw, const float *C,
                    int64_t ldc, float *Y, int64_t ldy, void *stream) {
    if (Rs < 0 || !m3 || !w_agg || !b_agg || !Ws || !C || !Y || ldx < 384 || ldw < 384 || ldc < 128 || ldy < 128) return MO_ERR_BAD_ARG;
    if ((ldx & 3) || (ldw & 3) || (ldc & 3) || (ldy & 3) || ((uintptr_t)m3 & 15) || ((uintptr_t)w_agg & 15) || ((uintptr_t)b_agg & 15) || ((uintptr_t)Ws & 15) ||
        ((uintptr_t)C & 15) || ((uintptr_t)Y & 15))
        return MO_ERR_BAD_ARG;
    if (Rs == 0) return 0;
    return launch_sb_encoder_tail<false>(Rs, m3, ldx, w_agg, b_agg, Ws, ldw, C, ldc, Y, ldy, (hipStream_t)stream);
}

int sb_encoder_tail_train(int64_t Rs, const float *m3, int64_t ldx, const float *w_agg, const float *b_agg, const float *Ws, int64_t ldw, const float *C,
                          int64_t ldc, float *Y, int64_t ldy, float *emb, int64_t lde, uint8_t *emb_sign_bits, int64_t ld_bytes, void *stream) {
    if (Rs < 0 || !m3 || !w_agg || !b_agg || !Ws || !C || !Y || !emb || !emb_sign_bits || ldx < 384 || ldw < 384 || ldc < 128 || ldy < 128 || lde < 384 ||
        ld_bytes < 48)
        return MO_ERR_BAD_ARG;
    if ((ldx & 3) || (ldw & 3) || (ldc & 3) || (ldy & 3) || (lde & 3) || ((uintptr_t)m3 & 15) || ((uintptr_t)w_agg & 15) || ((uintptr_t)b_agg & 15) ||
        ((uintptr_t)Ws & 15) || ((uintptr_t)C & 15) || ((uintptr_t)Y & 15) || ((uintptr_t)emb & 15))
        return MO_ERR_BAD_ARG;
    if (Rs == 0) return 0;
    return launch_sb_encoder_tail<true>(Rs, m3, ldx, w_agg, b_agg, Ws, ldw, C, ldc, Y, ldy, (hipStream_t)stream, emb, lde, emb_sign_bits, ld_bytes);
}

int64_t sb_encoder_tail_bwd_workspace(void) { return (int64_t)1024 * 384 * 4; }   // one row of partial sums per workgroup (<= CUs)

int sb_encoder_tail_bwd(int64_t Rs, const float *g, int64_t ldg, const float *Ws, int64_t ldw, const float *w_agg, const uint8_t *emb_sign_bits,
                        int64_t ld_bytes, float *ga, int64_t ldga, float *d_m3, int64_t ldd, float *colsum, void *workspace, void *stream) {
    if (Rs < 0 || !g || !Ws || !w_agg || !emb_sign_bits || !ga || !d_m3 || !colsum || !workspace || ldg < 128 || ldw < 384 || ld_bytes < 48 || ldga < 384 ||
        ldd < 384)
        return MO_ERR_BAD_ARG;
    if ((ldg & 3) || (ldw & 3) || (ldga & 3) || (ldd & 3) || ((uintptr_t)g & 15) || ((uintptr_t)Ws & 15) || ((uintptr_t)w_agg & 15) || ((uintptr_t)ga & 15) ||
        ((uintptr_t)d_m3 & 15) || ((uintptr_t)colsum & 15) || ((uintptr_t)workspace & 15))
        return MO_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (Rs == 0) return (int)hipMemsetAsync(colsum, 0, (size_t)384 * 4, st);
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    if (cus > 1024) return MO_ERR_BAD_ARG;         // (the workspace holds 1024 rows)
    return launch_sb_encoder_tail_bwd(Rs, g, ldg, Ws, ldw, w_agg, emb_sign_bits, ld_bytes, ga, ldga, d_m3, ldd, (float *)workspace, colsum, cus, st);
}

// the operands both forward variants of the semantic attention tail share
static bool sem_att_fwd_ok(int64_t Rs, const float *m3, int64_t ldx, const float *w_agg, const float *b_agg, const float *alpha, const float *Ws,
                           int64_t ldw, const float *C, int64_t ldc, const float *Y, int64_t ldy) {
    if (Rs < 0 || !m3 || !w_agg || !b_agg || !alpha || !Ws || !C || !Y || ldx < 384 || ldw < 384 || ldc < 128 || ldy < 128) return false;
    return !((ldx & 3) || (ldw & 3) || (ldc & 3) || (ldy & 3) || ((uintptr_t)m3 & 15) || ((uintptr_t)w_agg & 15) || ((uintptr_t)b_agg & 15) ||
             ((uintptr_t)alpha & 15) || ((uintptr_t)Ws & 15) || ((uintptr_t)C & 15) || ((uintptr_t)Y & 15));
}

int dhgn_sem_att_tail(int64_t Rs, const float *m3, int64_t ldx, const float *w_agg, const float *b_agg, const float *alpha, const float *Ws, int64_t ldw,
                      const float *C, int64_t ldc, float *Y, int64_t ldy, void *stream) {
    if (!sem_att_fwd_ok(Rs, m3, ldx, w_agg, b_agg, alpha, Ws, ldw, C, ldc, Y, ldy)) return MO_ERR_BAD_ARG;
    if (Rs == 0) return 0;
    return launch_sem_att_fwd<false>(Rs, m3, ldx, w_agg, b_agg, alpha, Ws, ldw, C, ldc, Y, ldy, (hipStream_t)stream);
}

int dhgn_sem_att_tail_train(int64_t Rs, const float *m3, int64_t ldx, const float *w_agg, const float *b_agg, const float *alpha, const float *Ws,
                            int64_t ldw, const float *C, int64_t ldc, float *Y, int64_t ldy, float *emb, int64_t lde, uint8_t *emb_sign_bits,
                            int64_t ld_bytes, float *gates, void *stream) {
    if (!sem_att_fwd_ok(Rs, m3, ldx, w_agg, b_agg, alpha, Ws, ldw, C, ldc, Y, ldy) || !emb || !emb_sign_bits || !gates || lde < 384 || (lde & 3) ||
        ld_bytes < 48 || ((uintptr_t)emb & 15) || ((uintptr_t)gates & 3))
        return MO_ERR_BAD_ARG;
    if (Rs == 0) return 0;
    return launch_sem_att_fwd<true>(Rs, m3, ldx, w_agg, b_agg, alpha, Ws, ldw, C, ldc, Y, ldy, (hipStream_t)stream, emb, lde, emb_sign_bits, ld_bytes,
                                    gates);
}

int64_t dhgn_sem_att_tail_bwd_workspace(void) { return (int64_t)SA_MAX_GRID * (384 + 128) * 4; }   // one row of partial sums per workgroup (<= CUs)

int dhgn_sem_att_tail_bwd(int64_t Rs, const float *g, int64_t ldg, const float *Ws, int64_t ldw, const float *w_agg, const float *alpha, const float *emb,
                          int64_t lde, const float *gates, float *ga, int64_t ldga, float *emb_scaled, int64_t ldes, float *d_m3, int64_t ldd,
                          float *colsum, float *d_alpha, void *workspace, void *stream) {
    if (Rs < 0 || !g || !Ws || !w_agg || !alpha || !emb || !gates || !ga || !emb_scaled || !d_m3 || !colsum || !d_alpha || !workspace || ldg < 128 ||
        ldw < 384 || lde < 384 || ldga < 384 || ldes < 384 || ldd < 384)
        return MO_ERR_BAD_ARG;
    if ((ldg & 3) || (ldw & 3) || (lde & 3) || (ldga & 3) || (ldes & 3) || (ldd & 3) || ((uintptr_t)g & 15) || ((uintptr_t)Ws & 15) ||
        ((uintptr_t)w_agg & 15) || ((uintptr_t)alpha & 15) || ((uintptr_t)emb & 15) || ((uintptr_t)gates & 3) || ((uintptr_t)ga & 15) ||
        ((uintptr_t)emb_scaled & 15) || ((uintptr_t)d_m3 & 15) || ((uintptr_t)colsum & 3) || ((uintptr_t)d_alpha & 3) || ((uintptr_t)workspace & 15))
        return MO_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    if (cus > SA_MAX_GRID) return MO_ERR_BAD_ARG;   // (the workspace holds SA_MAX_GRID rows)
    if (Rs == 0) {   // nothing to add up: zero sums from the reduce over no partial rows
        hipLaunchKernelGGL(k_sb_colsum_reduce, dim3(3), dim3(128), 0, st, 0, 384, (const float *)workspace, colsum);
        hipLaunchKernelGGL(k_sb_colsum_reduce, dim3(1), dim3(128), 0, st, 0, 128, (const float *)workspace, d_alpha);
        return (int)hipGetLastError();
    }
    return launch_sem_att_bwd(Rs, g, ldg, Ws, ldw, w_agg, alpha, emb, lde, gates, ga, ldga, emb_scaled, ldes, d_m3, ldd, colsum, d_alpha,
                              (float *)workspace, cus, st);
}

int gru_seq_split_fwd_multi(int32_t n_nets, const mo_gru_seq_net *nets, int32_t T, int32_t B, int32_t H, int32_t gi_agents, void *stream) {
    static_assert(SBR_H == GRU_NETS_H, "gru_nets_check.hpp checks H for these kernels");
    if (!gru_seq_nets_ok(n_nets, nets, T, B, H, gi_agents)) return MO_ERR_BAD_ARG;
    return launch_gru_seq_fwd_sb(n_nets, nets, T, B, gi_agents, (hipStream_t)stream);
}

int gru_seq_split_bwd_multi(int32_t n_nets, const mo_gru_seq_bwd_net *nets, int32_t T, int32_t B, int32_t H, int32_t gi_agents, void *stream) {
    if (!gru_seq_bwd_nets_ok(n_nets, nets, T, B, H, gi_agents)) return MO_ERR_BAD_ARG;
    return launch_gru_seq_bwd_sb(n_nets, nets, T, B, gi_agents, (hipStream_t)stream);
}

// the checks of both gnn_pair_agg entry points -> 0 and the kernels' argument record, or MO_ERR_BAD_ARG
static int gnn_pair_args(int64_t R, int32_t P, int32_t O, int32_t q_div, int32_t middle, int32_t embed, const float *p, const float *e, const float *o,
                         const float *adj_p, const float *adj_e, const void *adj_o, int32_t adj_mode, const float *W1, const float *b1, const float *W2,
                         const float *b2, GpArgs &a) {
    if (R < 0 || P < 1 || P > GP_PMAX || O < 0 || P + 1 + O > GP_KMAX || q_div < 1 || R % q_div != 0 || middle != 128 || embed != 128) return MO_ERR_BAD_ARG;
    if (adj_mode != GP_ADJ_TENSOR && adj_mode != GP_ADJ_ONES && adj_mode != GP_ADJ_BITS) return MO_ERR_BAD_ARG;
    if (!p || !e || (O > 0 && !o) || !W1 || !b1 || !W2 || !b2) return MO_ERR_BAD_ARG;
    if (adj_mode != GP_ADJ_ONES && (!adj_p || !adj_e || (O > 0 && !adj_o))) return MO_ERR_BAD_ARG;
    if (((uintptr_t)p & 15) || ((uintptr_t)e & 15) || ((uintptr_t)o & 15) || ((uintptr_t)W2 & 15) || ((uintptr_t)b2 & 15) || ((uintptr_t)W1 & 3) ||
        ((uintptr_t)b1 & 3) || ((uintptr_t)adj_p & 3) || ((uintptr_t)adj_e & 3) || ((uintptr_t)adj_o & 3))
        return MO_ERR_BAD_ARG;
    a = GpArgs{R, P, O, q_div, adj_mode, MO_ADJ_ROW_WORDS(O), p, e, o, adj_p, adj_e, adj_o, W1, b1, W2, b2};
    return 0;
}

int gnn_pair_agg_fwd(int64_t R, int32_t P, int32_t O, int32_t q_div, int32_t middle, int32_t embed, const float *p, const float *e, const float *o,
                     const float *adj_p, const float *adj_e, const void *adj_o, int32_t adj_mode, const float *W1, const float *b1, const float *W2,
                     const float *b2, float *agg, void *stream) {
    GpArgs a;
    if (gnn_pair_args(R, P, O, q_div, middle, embed, p, e, o, adj_p, adj_e, adj_o, adj_mode, W1, b1, W2, b2, a) || !agg || ((uintptr_t)agg & 15))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    return launch_gnn_pair_fwd(a, agg, (hipStream_t)stream);
}

int64_t gnn_pair_agg_bwd_workspace(int64_t R, int32_t P) {
    return R > 0 && P > 0 ? (int64_t)gp_bwd_grid(R, P) * GP_BLOCK * 4 : 0;
}

int gnn_pair_agg_bwd(int64_t R, int32_t P, int32_t O, int32_t q_div, int32_t middle, int32_t embed, const float *p, const float *e, const float *o,
                     const float *adj_p, const float *adj_e, const void *adj_o, int32_t adj_mode, const float *W1, const float *b1, const float *W2,
                     const float *b2, const float *d_agg, float *dW1, float *db1, float *dW2, float *db2, void *workspace, void *stream) {
    GpArgs a;
    if (gnn_pair_args(R, P, O, q_div, middle, embed, p, e, o, adj_p, adj_e, adj_o, adj_mode, W1, b1, W2, b2, a) || !d_agg || !dW1 || !db1 || !dW2 || !db2 ||
        !workspace || ((uintptr_t)d_agg & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)dW1 & 3) || ((uintptr_t)db1 & 3) || ((uintptr_t)dW2 & 3) ||
        ((uintptr_t)db2 & 3))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    return launch_gnn_pair_bwd(a, d_agg, dW1, db1, dW2, db2, (float *)workspace, (hipStream_t)stream);
}

extern "C++" {   // (templates over the two relation records)
// one relation of the attention / max-pool aggregator as the kernels take it, or not (K = 0: an empty relation, q and adj may be NULL)
static bool agg_alpha_ok(const mo_att_rel &m) { return m.alpha && !((uintptr_t)m.alpha & 3); }
static bool agg_alpha_ok(const mo_msg_rel &) { return true; }
template <class Rel>
static bool att_rel_ok(const Rel &m, int32_t R, int32_t P) {
    if (m.K < 0 || m.K > AA_KMAX || (m.din != 4 && m.din != 8) || m.q_div < 1 || R % m.q_div != 0 || m.adj_mode < 0 || m.adj_mode > 3) return false;
    if (!m.W || !m.b || !agg_alpha_ok(m) || ((uintptr_t)m.W & 15) || ((uintptr_t)m.b & 3)) return false;
    if (m.din == 8 && (!m.e || ((uintptr_t)m.e & 15) || (m.e_rs & 3) || m.e_rs < 4)) return false;
    if (m.adj_mode == MO_ADJ_VALID && (!m.kvalid || ((uintptr_t)m.kvalid & 3))) return false;
    if (m.K == 0) return true;
    if (!m.q || ((uintptr_t)m.q & 15) || (m.q_rs & 3) || m.q_rs < 4 * (int64_t)m.K) return false;
    if (m.adj_mode == MO_ADJ_TENSOR && (!m.adj || ((uintptr_t)m.adj & 3) || m.adj_rs < (int64_t)P * m.K)) return false;
    if (m.adj_mode == MO_ADJ_BITS && (!m.adj || ((uintptr_t)m.adj & 3) || m.adj_rs < (int64_t)P * MO_ADJ_ROW_WORDS(m.K))) return false;
    return true;
}

// the checks common to both entry points -> 0 and the kernels' argument record, or MO_ERR_BAD_ARG
template <class Rel, class Args>
static int att_args(const Rel *rel, int n_rel, int32_t R, int32_t P, int32_t E, const float *p, int64_t p_rs, Args &a) {
    if (!rel || R < 0 || P < 1 || P > AA_PMAX || E != AA_E || !p || ((uintptr_t)p & 15) || (p_rs & 3) || p_rs < 4 * (int64_t)P) return MO_ERR_BAD_ARG;
    int kmax = 4;
    for (int r = 0; r < n_rel; r++) {
        if (!att_rel_ok(rel[r], R, P)) return MO_ERR_BAD_ARG;
        a.rel[r] = rel[r];
        if (rel[r].K > kmax) kmax = rel[r].K;
    }
    for (int r = n_rel; r < 3; r++) a.rel[r] = rel[0];
    a.n_rel = n_rel, a.R = R, a.P = P, a.kc = (kmax + 3) & ~3, a.p_rs = p_rs, a.p = p;
    return 0;
}
}  // extern "C++"

int dhgn_att_agg3_fwd(const mo_att_rel *rel, int32_t R, int32_t P, int32_t E, const float *p, int64_t p_rs, float *out, int64_t out_stride,
                      void *stream) {
    AaArgs a;
    if (att_args(rel, 3, R, P, E, p, p_rs, a) || !out || ((uintptr_t)out & 15) || out_stride < 3 * AA_E || (out_stride & 3)) return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    return launch_att_agg_fwd(a, out, out_stride, (hipStream_t)stream);
}

int64_t dhgn_att_agg_bwd_workspace(int32_t E, int32_t din) {
    return E == AA_E && (din == 4 || din == 8) ? (int64_t)AA_MAX_GRID * 128 * (din + 2) * 4 : 0;
}

int dhgn_att_agg_bwd(int32_t R, int32_t P, int32_t K, int32_t E, int32_t din, const float *p, int64_t p_rs, const float *q, int64_t q_rs,
                     int32_t q_div, const float *e, int64_t e_rs, const void *adj, int64_t adj_rs, int32_t adj_mode, const int32_t *kvalid,
                     const float *W, const float *b, const float *alpha, const float *gout, int64_t gout_stride, float *dW, float *db,
                     float *d_alpha, void *workspace, void *stream) {
    const mo_att_rel rel = {K, din, q_div, adj_mode, q, q_rs, e, e_rs, adj, adj_rs, kvalid, W, b, alpha};
    AaArgs a;
    if (att_args(&rel, 1, R, P, E, p, p_rs, a) || !gout || ((uintptr_t)gout & 7) || gout_stride < AA_E || (gout_stride & 1) || !dW || !db || !d_alpha ||
        !workspace || ((uintptr_t)dW & 3) || ((uintptr_t)db & 3) || ((uintptr_t)d_alpha & 3) || ((uintptr_t)workspace & 15))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    return launch_att_agg_bwd(a, gout, gout_stride, dW, db, d_alpha, (float *)workspace, (hipStream_t)stream);
}

int dhgn_pool_agg3_fwd(const mo_msg_rel *rel, int32_t R, int32_t P, int32_t E, const float *p, int64_t p_rs, float *out, int64_t out_stride,
                       void *stream) {
    PaArgs a;
    if (att_args(rel, 3, R, P, E, p, p_rs, a) || !out || ((uintptr_t)out & 15) || out_stride < 3 * AA_E || (out_stride & 3)) return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    return launch_pool_agg_fwd(a, out, out_stride, (hipStream_t)stream);
}

int64_t dhgn_pool_agg_bwd_workspace(int32_t E, int32_t din) {
    return E == AA_E && (din == 4 || din == 8) ? (int64_t)PA_MAX_GRID * 128 * (din + 1) * 4 : 0;
}

int dhgn_pool_agg_bwd(int32_t R, int32_t P, int32_t K, int32_t E, int32_t din, const float *p, int64_t p_rs, const float *q, int64_t q_rs,
                      int32_t q_div, const float *e, int64_t e_rs, const void *adj, int64_t adj_rs, int32_t adj_mode, const int32_t *kvalid,
                      const float *W, const float *b, const float *gout, int64_t gout_stride, float *dW, float *db, void *workspace,
                      void *stream) {
    const mo_msg_rel rel = {K, din, q_div, adj_mode, q, q_rs, e, e_rs, adj, adj_rs, kvalid, W, b};
    PaArgs a;
    if (att_args(&rel, 1, R, P, E, p, p_rs, a) || !gout || ((uintptr_t)gout & 7) || gout_stride < AA_E || (gout_stride & 1) || !dW || !db ||
        !workspace || ((uintptr_t)dW & 3) || ((uintptr_t)db & 3) || ((uintptr_t)workspace & 15))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    return launch_pool_agg_bwd(a, gout, gout_stride, dW, db, (float *)workspace, (hipStream_t)stream);
}

// alignment of the vectors the lanes read and write as float2
static bool fa_ok8(const void *p) { return p && !((uintptr_t)p & 7); }

int fcra_att_fwd_multi(int32_t n_jobs, const mo_fcra_att_job *jobs, int64_t R, int32_t P, int32_t E, const float *adj, int64_t adj_row_stride,
                       int64_t out_stride, int32_t max_blocks, void *stream) {
    if (n_jobs < 1 || n_jobs > MO_FCRA_ATT_MAX_JOBS || !jobs || R < 0 || P < 1 || P > FA_MAX_P || E != FA_E || out_stride < FA_E || (out_stride & 1) ||
        max_blocks < 0 || ((uintptr_t)adj & 3) || (adj && adj_row_stride < (int64_t)P * P))
        return MO_ERR_BAD_ARG;
    FaJobs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < n_jobs; k++) {
        const mo_fcra_att_job &m = jobs[k];
        if (!fa_ok8(m.bias) || !fa_ok8(m.alpha) || (!m.out_actor && !m.out_critic)) return MO_ERR_BAD_ARG;
        if (m.out_actor && (!adj || !fa_ok8(m.out_actor) || !fa_ok8(m.y_actor))) return MO_ERR_BAD_ARG;
        if (m.out_critic && (!fa_ok8(m.out_critic) || !fa_ok8(m.y_critic))) return MO_ERR_BAD_ARG;
        a.j[k] = m;
    }
    if (R == 0) return 0;
    return launch_fcra_att_fwd(a, n_jobs, R, P, adj, adj_row_stride, out_stride, max_blocks, (hipStream_t)stream);
}

int64_t fcra_att_bwd_workspace(int32_t E, int32_t max_blocks) {
    if (E != FA_E || max_blocks < 0) return 0;
    return (int64_t)(max_blocks > 0 && max_blocks < FA_MAX_GRID ? max_blocks : FA_MAX_GRID) * 2 * FA_E * 4;
}

int fcra_att_bwd(int64_t R, int32_t P, int32_t E, const float *y, const float *adj, int64_t adj_row_stride, const float *bias, const float *alpha,
                 const float *out, int64_t out_stride, const float *g, int64_t g_stride, float *dy, float *db, float *d_alpha, void *workspace,
                 int32_t max_blocks, void *stream) {
    if (R < 0 || P < 1 || P > FA_MAX_P || E != FA_E || out_stride < FA_E || (out_stride & 1) || g_stride < FA_E || (g_stride & 1) || max_blocks < 0 ||
        ((uintptr_t)adj & 3) || (adj && adj_row_stride < (int64_t)P * P))
        return MO_ERR_BAD_ARG;
    if (!fa_ok8(y) || !fa_ok8(bias) || !fa_ok8(alpha) || !fa_ok8(out) || !fa_ok8(g) || !fa_ok8(dy) || !db || !d_alpha || !workspace ||
        ((uintptr_t)db & 3) || ((uintptr_t)d_alpha & 3) || ((uintptr_t)workspace & 15))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    return launch_fcra_att_bwd(R, P, y, adj, adj_row_stride, bias, alpha, out, out_stride, g, g_stride, dy, db, d_alpha, (float *)workspace, max_blocks,
                               (hipStream_t)stream);
}

int fcra_pool_fwd_multi(int32_t n_jobs, const mo_fcra_pool_job *jobs, int64_t R, int32_t P, int32_t E, const float *adj, int64_t adj_row_stride,
                        int64_t out_stride, int32_t max_blocks, void *stream) {
    if (n_jobs < 1 || n_jobs > MO_FCRA_POOL_MAX_JOBS || !jobs || R < 0 || P < 1 || P > FA_MAX_P || E != FA_E || out_stride < FA_E || (out_stride & 1) ||
        max_blocks < 0 || ((uintptr_t)adj & 3) || (adj && adj_row_stride < (int64_t)P * P))
        return MO_ERR_BAD_ARG;
    FpJobs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < n_jobs; k++) {
        const mo_fcra_pool_job &m = jobs[k];
        if (!fa_ok8(m.bias) || (!m.out_actor && !m.out_critic)) return MO_ERR_BAD_ARG;
        if (m.out_actor && (!adj || !fa_ok8(m.out_actor) || !fa_ok8(m.y_actor))) return MO_ERR_BAD_ARG;
        if (m.out_critic && (!fa_ok8(m.out_critic) || !fa_ok8(m.y_critic))) return MO_ERR_BAD_ARG;
        a.j[k] = m;
    }
    if (R == 0) return 0;
    return launch_fcra_pool_fwd(a, n_jobs, R, P, adj, adj_row_stride, out_stride, max_blocks, (hipStream_t)stream);
}

int64_t fcra_pool_bwd_workspace(int32_t E, int32_t max_blocks) {
    if (E != FA_E || max_blocks < 0) return 0;
    return (int64_t)(max_blocks > 0 && max_blocks < FA_MAX_GRID ? max_blocks : FA_MAX_GRID) * FA_E * 4;
}

int fcra_pool_bwd(int64_t R, int32_t P, int32_t E, const float *y, const float *adj, int64_t adj_row_stride, const float *out, int64_t out_stride,
                  const float *g, int64_t g_stride, float *dy, float *db, void *workspace, int32_t max_blocks, void *stream) {
    if (R < 0 || P < 1 || P > FA_MAX_P || E != FA_E || out_stride < FA_E || (out_stride & 1) || g_stride < FA_E || (g_stride & 1) || max_blocks < 0 ||
        ((uintptr_t)adj & 3) || (adj && adj_row_stride < (int64_t)P * P))
        return MO_ERR_BAD_ARG;
    if (!fa_ok8(y) || !fa_ok8(out) || !fa_ok8(g) || !fa_ok8(dy) || !db || !workspace || ((uintptr_t)db & 3) || ((uintptr_t)workspace & 15))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    return launch_fcra_pool_bwd(R, P, y, adj, adj_row_stride, out, out_stride, g, g_stride, dy, db, (float *)workspace, max_blocks, (hipStream_t)stream);
}

// a (T, episode stride, step stride) view whose rows are P dense vectors read as float2
static bool ft_view_ok(int32_t P, int32_t T, int64_t es, int64_t ss) {
    return es >= (int64_t)P * FT_E && !(es & 1) && (T == 1 || (ss >= (int64_t)P * FT_E && !(ss & 1)));
}

int fcra_team_fwd_multi(int32_t n_jobs, const mo_fcra_team_job *jobs, int32_t mode, int64_t R, int32_t P, int32_t E, int32_t T,
                        int64_t ya_episode_stride, int64_t ya_step_stride, int64_t yc_episode_stride, int64_t yc_step_stride, const float *adj,
                        int64_t adj_row_stride, int32_t relu, int64_t out_stride, int32_t max_blocks, void *stream) {
    if (n_jobs < 1 || n_jobs > MO_FCRA_TEAM_MAX_JOBS || !jobs || (mode != MO_FCRA_TEAM_ATT && mode != MO_FCRA_TEAM_MEAN) || R < 0 || P < 1 ||
        P > FT_MAX_P || E != FT_E || T < 1 || out_stride < FT_E || (out_stride & 1) || out_stride > FT_MAX_LD || max_blocks < 0 || ((uintptr_t)adj & 3) ||
        (adj && adj_row_stride < (int64_t)P * P))
        return MO_ERR_BAD_ARG;
    const bool att = mode == MO_FCRA_TEAM_ATT;
    FtJobs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < n_jobs; k++) {
        const mo_fcra_team_job &m = jobs[k];
        if ((att ? !fa_ok8(m.bias) || !fa_ok8(m.alpha) : (m.bias && !fa_ok8(m.bias))) || (!m.out_actor && !m.out_critic)) return MO_ERR_BAD_ARG;
        if (m.out_actor && (!adj || !fa_ok8(m.out_actor) || !fa_ok8(m.y_actor) || !ft_view_ok(P, T, ya_episode_stride, ya_step_stride)))
            return MO_ERR_BAD_ARG;
        if (m.out_critic && (!fa_ok8(m.out_critic) || !fa_ok8(m.y_critic) || !ft_view_ok(P, T, yc_episode_stride, yc_step_stride)))
            return MO_ERR_BAD_ARG;
        a.j[k] = m;
    }
    if (R == 0) return 0;
    return launch_fcra_team_fwd(a, n_jobs, att, R, P, T, ya_episode_stride, ya_step_stride, yc_episode_stride, yc_step_stride, adj, adj_row_stride,
                                att || relu, out_stride, max_blocks, (hipStream_t)stream);
}

int64_t fcra_team_bwd_workspace(int32_t E, int32_t max_blocks) {
    if (E != FT_E || max_blocks < 0) return 0;
    return (int64_t)(max_blocks > 0 && max_blocks < FT_MAX_GRID ? max_blocks : FT_MAX_GRID) * 2 * FT_E * 4;
}

int fcra_team_bwd(int64_t R, int32_t P, int32_t E, const float *y, const float *adj, int64_t adj_row_stride, const float *bias, const float *alpha,
                  const float *out, int64_t out_stride, const float *g, int64_t g_stride, float *dy, float *db, float *d_alpha, void *workspace,
                  int32_t max_blocks, void *stream) {
    if (R < 0 || P < 1 || P > FT_MAX_P || E != FT_E || out_stride < FT_E || (out_stride & 1) || g_stride < FT_E || (g_stride & 1) || out_stride > FT_MAX_LD || g_stride > FT_MAX_LD || max_blocks < 0 ||
        ((uintptr_t)adj & 3) || (adj && adj_row_stride < (int64_t)P * P))
        return MO_ERR_BAD_ARG;
    if (!fa_ok8(y) || !fa_ok8(bias) || !fa_ok8(alpha) || !fa_ok8(out) || !fa_ok8(g) || !fa_ok8(dy) || !db || !d_alpha || !workspace ||
        ((uintptr_t)db & 3) || ((uintptr_t)d_alpha & 3) || ((uintptr_t)workspace & 15))
        return MO_ERR_BAD_ARG;
    if (R == 0) return 0;
    return launch_fcra_team_bwd(R, P, y, adj, adj_row_stride, bias, alpha, out, out_stride, g, g_stride, dy, db, d_alpha, (float *)workspace, max_blocks,
                                (hipStream_t)stream);
}

// rows of FN_E floats ld apart: a stride the float2 lanes can take
static bool fn_ld_ok(int64_t ld) { return ld >= FN_E && !(ld & 1); }
// do R rows from a (ld_a apart) and R rows from b (ld_b apart) share a byte?  (as whole extents: a view inside the other's gaps is refused too)
static bool fn_overlap(const float *a, int64_t ld_a, const float *b, int64_t ld_b, int64_t R) {
    const int64_t rows = R > 0 ? R - 1 : 0;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)(rows * ld_a + FN_E) * 4, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)(rows * ld_b + FN_E) * 4;
    return a0 < b1 && b0 < a1;
}
static bool fn_common_ok(int32_t n_jobs, const mo_feat_norm_job *jobs, int64_t R, int32_t width, float eps, int32_t max_blocks) {
    return n_jobs >= 1 && n_jobs <= MO_FEAT_NORM_MAX_JOBS && jobs && R >= 0 && width == FN_E && isfinite(eps) && eps > 0.f && max_blocks >= 0;
}

int feat_norm_fwd_multi(int32_t n_jobs, const mo_feat_norm_job *jobs, int64_t R, int32_t width, float eps, int32_t max_blocks, void *stream) {
    if (!fn_common_ok(n_jobs, jobs, R, width, eps, max_blocks)) return MO_ERR_BAD_ARG;
    FnJobs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < n_jobs; k++) {
        const mo_feat_norm_job &m = jobs[k];
        if (!fa_ok8(m.x) || !fa_ok8(m.weight) || !fa_ok8(m.bias) || !fa_ok8(m.y) || !fn_ld_ok(m.ldx) || !fn_ld_ok(m.ldy) ||
            fn_overlap(m.x, m.ldx, m.y, m.ldy, R))
            return MO_ERR_BAD_ARG;
        a.j[k] = m;
    }
    if (R == 0) return 0;
    return launch_feat_norm_fwd(a, n_jobs, R, eps, max_blocks, (hipStream_t)stream);
}

int64_t feat_norm_bwd_workspace(int32_t width, int32_t n_jobs, int32_t max_blocks) {
    if (width != FN_E || n_jobs < 1 || n_jobs > MO_FEAT_NORM_MAX_JOBS || max_blocks < 0) return 0;
    return (int64_t)n_jobs * (max_blocks > 0 && max_blocks < FN_MAX_GRID ? max_blocks : FN_MAX_GRID) * 2 * FN_E * 4;
}

int feat_norm_bwd_multi(int32_t n_jobs, const mo_feat_norm_job *jobs, int64_t R, int32_t width, float eps, void *workspace, int32_t max_blocks,
                        void *stream) {
    if (!fn_common_ok(n_jobs, jobs, R, width, eps, max_blocks) || !workspace || ((uintptr_t)workspace & 15)) return MO_ERR_BAD_ARG;
    FnJobs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < n_jobs; k++) {
        const mo_feat_norm_job &m = jobs[k];
        if (!fa_ok8(m.x) || !fa_ok8(m.weight) || !fa_ok8(m.g) || !fa_ok8(m.dx) || !fa_ok8(m.d_weight) || !fa_ok8(m.d_bias) || !fn_ld_ok(m.ldx) ||
            !fn_ld_ok(m.ldg) || !fn_ld_ok(m.lddx) || fn_overlap(m.x, m.ldx, m.dx, m.lddx, R))
            return MO_ERR_BAD_ARG;
        a.j[k] = m;
    }
    if (R == 0) return 0;
    return launch_feat_norm_bwd(a, n_jobs, R, eps, (float *)workspace, max_blocks, (hipStream_t)stream);
}

// the arguments team_pool_fwd and team_pool_bwd share
static bool tp_common_ok(int64_t G, int32_t P, int32_t E, const float *feat, int64_t feat_ld, const void *live, int32_t live_u8, int64_t live_stride,
                         const float *score, const float *gate, int32_t max_blocks) {
    return G >= 0 && P >= 1 && P <= TP_MAX_P && E == TP_E && fa_ok8(feat) && fn_ld_ok(feat_ld) && live && (live_u8 == 1 || (live_u8 == 0 && !((uintptr_t)live & 3))) &&
           live_stride >= P && fa_ok8(score) && fa_ok8(gate) && max_blocks >= 0;
}

int team_pool_fwd(int64_t G, int32_t P, int32_t E, const float *feat, int64_t feat_ld, const void *live, int32_t live_u8, int64_t live_stride,
                  const float *score, const float *gate, float *out, int64_t out_ld, int32_t max_blocks, void *stream) {
    if (!tp_common_ok(G, P, E, feat, feat_ld, live, live_u8, live_stride, score, gate, max_blocks) || !fa_ok8(out) || !fn_ld_ok(out_ld) ||
        fn_overlap(feat, feat_ld, out, out_ld, G * P))
        return MO_ERR_BAD_ARG;
    if (G == 0) return 0;
    const TpArgs a = {feat, feat_ld, live, live_u8, live_stride, score, gate};
    return launch_team_pool_fwd(a, out, out_ld, G, P, max_blocks, (hipStream_t)stream);
}

int64_t team_pool_bwd_workspace(int32_t E, int32_t max_blocks) {
    if (E != TP_E || max_blocks < 0) return 0;
    return (int64_t)(max_blocks > 0 && max_blocks < TP_MAX_GRID ? max_blocks : TP_MAX_GRID) * 2 * TP_E * 4;
}

int team_pool_bwd(int64_t G, int32_t P, int32_t E, const float *feat, int64_t feat_ld, const void *live, int32_t live_u8, int64_t live_stride,
                  const float *score, const float *gate, const float *g, int64_t g_ld, float *d_feat, int64_t d_feat_ld, float *d_score, float *d_gate,
                  void *workspace, int32_t max_blocks, void *stream) {
    if (!tp_common_ok(G, P, E, feat, feat_ld, live, live_u8, live_stride, score, gate, max_blocks) || !fa_ok8(g) || !fn_ld_ok(g_ld) || !fa_ok8(d_feat) ||
        !fn_ld_ok(d_feat_ld) || !fa_ok8(d_score) || !fa_ok8(d_gate) || !workspace || ((uintptr_t)workspace & 15) ||
        fn_overlap(feat, feat_ld, d_feat, d_feat_ld, G * P) || fn_overlap(g, g_ld, d_feat, d_feat_ld, G * P))
        return MO_ERR_BAD_ARG;
    if (G == 0) return 0;
    const TpArgs a = {feat, feat_ld, live, live_u8, live_stride, score, gate};
    return launch_team_pool_bwd(a, g, g_ld, d_feat, d_feat_ld, d_score, d_gate, G, P, (float *)workspace, max_blocks, (hipStream_t)stream);
}


int team_pool_heads_fwd(int64_t G, int32_t P, int32_t E, const float *feat, int64_t feat_ld, const void *live, int32_t live_u8, int64_t live_stride,
                        const float *score, const float *gate, float *out, int64_t out_ld, int32_t heads, int32_t max_blocks, void *stream) {
    if (!tph_heads_ok(heads) || !tp_common_ok(G, P, E, feat, feat_ld, live, live_u8, live_stride, score, gate, max_blocks) || !fa_ok8(out) ||
        !fn_ld_ok(out_ld) || fn_overlap(feat, feat_ld, out, out_ld, G * P))
        return MO_ERR_BAD_ARG;
    if (G == 0) return 0;
    const TpArgs a = {feat, feat_ld, live, live_u8, live_stride, score, gate};
    return launch_team_pool_heads_fwd(a, heads, out, out_ld, G, P, max_blocks, (hipStream_t)stream);
}

int team_pool_heads_bwd(int64_t G, int32_t P, int32_t E, const float *feat, int64_t feat_ld, const void *live, int32_t live_u8, int64_t live_stride,
                        const float *score, const float *gate, const float *g, int64_t g_ld, float *d_feat, int64_t d_feat_ld, float *d_score,
                        float *d_gate, void *workspace, int32_t heads, int32_t max_blocks, void *stream) {
    if (!tph_heads_ok(heads) || !tp_common_ok(G, P, E, feat, feat_ld, live, live_u8, live_stride, score, gate, max_blocks) || !fa_ok8(g) ||
        !fn_ld_ok(g_ld) || !fa_ok8(d_feat) || !fn_ld_ok(d_feat_ld) || !fa_ok8(d_score) || !fa_ok8(d_gate) || !workspace || ((uintptr_t)workspace & 15) ||
        fn_overlap(feat, feat_ld, d_feat, d_feat_ld, G * P) || fn_overlap(g, g_ld, d_feat, d_feat_ld, G * P))
        return MO_ERR_BAD_ARG;
    if (G == 0) return 0;
    const TpArgs a = {feat, feat_ld, live, live_u8, live_stride, score, gate};
    return launch_team_pool_heads_bwd(a, heads, g, g_ld, d_feat, d_feat_ld, d_score, d_gate, G, P, (float *)workspace, max_blocks, (hipStream_t)stream);
}

}  // extern "C"
