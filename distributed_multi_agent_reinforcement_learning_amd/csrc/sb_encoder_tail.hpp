// sb_encoder_tail.hpp -- the rollout encoder's AGG layer and semantic layer as one launch (C ABI: include/mappo_ops.h sb_encoder_tail)
#pragma once
#include <mutex>

#include "sb_common.hpp"

// ---- Y[s] = sum over r of Ws_r relu(W_agg m3[s, r] + b_agg) + C[s]  (k_sb_encoder_tail) -------------------------------------------
// DHGN.forward_pair's encoder tail (reference DHGN/mappo_parallel.py:148-203): the AGG layer (128 <- 128, bias, ReLU) over the three
// relation vectors of a semantic row and the embedding part of the semantic layer (128 <- 384, accumulated onto the position part C,
// which may be Y).  As two k_sb_gemm_n128 launches the (Rs, 384) embedding crosses HBM twice; here it exists 32 rows x 128 units at a
// time, as split pieces in LDS.
// Persistent 512-thread workgroups, 32 semantic rows per tile, three STEPS (relations, in order) per tile; wave w owns units
// 16 w .. 16 w + 15 of both layers.  A step:
//   AGG       acc_a = W_agg x the step's m3 image (4 chunks of 32 inputs, six piece products each in SBG_MMA order, from zero);
//             + bias, max(., 0): per output exactly k_sb_gemm_n128<4,1,0>
//   hand-over the D tile has a lane own units 16 w + 4 gq .. + 3 of row i: split (sb_split2) and written as one half of the 16-byte
//             operand words of the embedding image (chunk w / 2, octet 2 (w & 1) + gq / 2), 8 bytes per piece (as sbr_put4)
//   barrier   (the embedding image is complete; every wave is done reading the m3 image)
//   semantic  acc_s += Ws chunks 4 r .. 4 r + 3 x the embedding image: over a tile acc_s sees chunks 0 .. 11 in the order of
//             k_sb_gemm_n128<12,1,2>, whose epilogue (null bias: + 0.f, + addend, one 16-byte store) follows step 2
//   staging   the m3 rows of step n + 1 (requested a step ago) are split into the m3 image, those of step n + 2 requested: waves 0-3
//             before their semantic phase, waves 4-7 after it (the two waves of a SIMD out of phase, OPT & 2 of k_sb_gemm_n128)
//   barrier   (the m3 image is complete; every wave is done reading the embedding image)
// Every output is therefore bit-identical to the two launches.  The addend rows are requested at the head of the tile.
// Registers: the semantic weights stay resident as pieces (144 per lane).  The AGG weights do not fit beside them (48 registers of
// pieces, or 32 of raw fp32 re-split per chunk: both spill at 256 registers, DESIGN); their pieces live in LDS, written once in the
// prologue, every wave reading back its own 12 KB as A operands per step.
// LDS: 96 KB AGG weight image + 24 KB m3 image + 24 KB embedding image = 144 KB.
constexpr int SBE_IMG = 3 * 4 * 2 * 64;   // uint4 per operand image: [piece][chunk][row half][lane]
constexpr int SBE_WIMG = 8 * 4 * 3 * 64;  // uint4 of the weight image: [wave][chunk][piece][lane]

// SAVE (the update, sb_encoder_tail_train): at the hand-over the lanes that hold the AGG result also store it -- one 16-byte store per lane
// into emb (Rs, 384), row stride lde -- and its sign bits in sb_gemm_signs' layout (bit k of byte j of a relation row: emb[..][8 j + k] > 0;
// 16 bytes per relation, 48 per semantic row, row stride ldb bytes): what the backward (sb_encoder_tail_bwd.hpp) and the weight
// gradients read.  The stores stay in flight across the barriers (lds_barrier); everything else is the rollout's kernel.
template <bool SAVE>
__global__ __launch_bounds__(512) void k_sb_encoder_tail(int64_t Rs, const float *__restrict__ X, int64_t ldx, const float *__restrict__ Wa,
                                                         const float *__restrict__ ba, const float *__restrict__ Ws, int64_t ldw, const float *C,
                                                         int64_t ldc, float *Y, int64_t ldy, float *__restrict__ emb, int64_t lde,
                                                         uint8_t *__restrict__ ebits, int64_t ldb) {
    extern __shared__ uint4 sbe_lds[];                  // [AGG weight image | m3 image | embedding image]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 15, gq = l >> 4;
    uint4 *const wimg = sbe_lds + w * (4 * 3 * 64) + l, *const mimg = sbe_lds + SBE_WIMG, *const eimg = mimg + SBE_IMG;
    {
        const float *rw = Wa + (size_t)(16 * w + i) * 128 + 8 * gq;   // W_agg rows 16 w + i, inputs 32 c + 8 gq .. + 7: this lane's A operands
#pragma unroll
        for (int c = 0; c < 4; c++) {
            uint4 p_[3];
            sb_split8(*(const float4 *)(rw + 32 * c), *(const float4 *)(rw + 32 * c + 4), p_);
#pragma unroll
            for (int p = 0; p < 3; p++) wimg[(c * 3 + p) * 64] = p_[p];
        }
    }
    uint4 ws[12][3];                                    // Ws rows 16 w + i
    {
        const float *rw = Ws + (size_t)(16 * w + i) * ldw + 8 * gq;
#pragma unroll
        for (int c = 0; c < 12; c++) sb_split8(*(const float4 *)(rw + 32 * c), *(const float4 *)(rw + 32 * c + 4), ws[c]);
    }
    const float4 b4 = *(const float4 *)(ba + 16 * w + 4 * gq);
    const int64_t n_t = (Rs + 31) / 32, G = gridDim.x;
    float4 pf[2];
    // wave w stages (chunk w / 2, half w & 1) of a step's image: lane (gq, j) loads inputs 32 c + 8 gq .. of row j of the half
    auto fetch = [&](int64_t t, int r) {
        const int64_t row = t * 32 + (w & 1) * 16 + i;
        pf[0] = pf[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < Rs) {
            const float *src = X + row * ldx + 128 * r + 32 * (w >> 1) + 8 * gq;
            pf[0] = *(const float4 *)src;
            pf[1] = *(const float4 *)(src + 4);
        }
    };
    auto stage = [&]() {
        uint4 p_[3];
        sb_split8(pf[0], pf[1], p_);
#pragma unroll
        for (int p = 0; p < 3; p++) mimg[(p * 8 + w) * 64 + l] = p_[p];
    };
    // this lane's half words of the embedding image: chunk w / 2, octet 2 (w & 1) + gq / 2, column i, half gq & 1
    uint2 *const edst = (uint2 *)eimg + (((w >> 1) * 2) * 64 + ((2 * (w & 1) + (gq >> 1)) << 4) + i) * 2 + (gq & 1);   // + 128: the second row half
    int64_t t = blockIdx.x;
    if (t < n_t) { fetch(t, 0); stage(); fetch(t, 1); }
    lds_barrier();
    for (; t < n_t; t += G) {
        const bool more = t + G < n_t;
        float4 a4[2];
        auto addend = [&]() {
#pragma unroll
            for (int rt = 0; rt < 2; rt++) {
                const int64_t row = t * 32 + rt * 16 + i;
                a4[rt] = row < Rs ? *(const float4 *)(C + row * ldc + 16 * w + 4 * gq) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        if constexpr (!SAVE) addend();   // (SAVE: requested behind step 2's hand-over, in the registers the AGG accumulators release: beside
                                         // the stores' addresses the eight do not fit across a hand-over -- 20 B of scratch wherever else)
        f32x4 acc_s[2];
        acc_s[0] = acc_s[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 3; r++) {
            f32x4 acc_a[2];
            acc_a[0] = acc_a[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#define SBE_MMA(A, pi, pj)                                                                                                                          \
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[pi]), __builtin_bit_cast(bf16x8, b0[pj]), acc[0], 0, 0, 0); \
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[pi]), __builtin_bit_cast(bf16x8, b1[pj]), acc[1], 0, 0, 0);
#define SBE_MMA6(A) SBE_MMA(A, 2, 0) SBE_MMA(A, 0, 2) SBE_MMA(A, 1, 1) SBE_MMA(A, 1, 0) SBE_MMA(A, 0, 1) SBE_MMA(A, 0, 0)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                uint4 a_[3], b0[3], b1[3];
#pragma unroll
                for (int p = 0; p < 3; p++) { a_[p] = wimg[(c * 3 + p) * 64]; b0[p] = mimg[(p * 8 + 2 * c) * 64 + l]; b1[p] = mimg[(p * 8 + 2 * c + 1) * 64 + l]; }
                f32x4(&acc)[2] = acc_a;
                SBE_MMA6(a_)
            }
            // D tile: lane (i, gq), register q -> unit 16 w + 4 gq + q of row i of the half
#pragma unroll
            for (int rt = 0; rt < 2; rt++) {
                float4 v = make_float4(acc_a[rt][0] + b4.x, acc_a[rt][1] + b4.y, acc_a[rt][2] + b4.z, acc_a[rt][3] + b4.w);
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                if constexpr (SAVE) {   // lanes (i, gq) and (i, gq ^ 1) hold the two nibbles of a byte (as k_sb_gemm_n128, OPT & 8)
                    const int64_t row = t * 32 + rt * 16 + i;
                    const unsigned nib = (unsigned)(v.x > 0.f) | ((unsigned)(v.y > 0.f) << 1) | ((unsigned)(v.z > 0.f) << 2) | ((unsigned)(v.w > 0.f) << 3);
                    const unsigned other = (unsigned)__shfl_xor((int)nib, 16);
                    if (row < Rs) {
                        *(float4 *)(emb + row * lde + 128 * r + 16 * w + 4 * gq) = v;
                        if (!(gq & 1)) ebits[row * ldb + 16 * r + 2 * w + (gq >> 1)] = (uint8_t)(nib | (other << 4));
                    }
                }
                uint32_t lo[3], hi[3];
                sb_split2(v.x, v.y, lo[0], lo[1], lo[2]);
                sb_split2(v.z, v.w, hi[0], hi[1], hi[2]);
#pragma unroll
                for (int p = 0; p < 3; p++) edst[p * 8 * 64 * 2 + rt * 128] = make_uint2(lo[p], hi[p]);
            }
            lds_barrier();
            if constexpr (SAVE) if (r == 2) addend();
            auto next_step = [&]() {   // step n + 1 -> the m3 image, step n + 2 requested
                if (r < 2 || more) stage();
                if (r == 0) fetch(t, 2);
                else if (more) fetch(t + G, r - 1);
            };
            if (w < 4) next_step();
#pragma unroll
            for (int c = 0; c < 4; c++) {
                uint4 b0[3], b1[3];
#pragma unroll
                for (int p = 0; p < 3; p++) { b0[p] = eimg[(p * 8 + 2 * c) * 64 + l]; b1[p] = eimg[(p * 8 + 2 * c + 1) * 64 + l]; }
                f32x4(&acc)[2] = acc_s;
                SBE_MMA6(ws[4 * r + c])
            }
#undef SBE_MMA6
#undef SBE_MMA
            if (w >= 4) next_step();
            if (r < 2) lds_barrier();
        }
#pragma unroll
        for (int rt = 0; rt < 2; rt++) {
            const int64_t row = t * 32 + rt * 16 + i;
            if (row < Rs) {
                float4 v = make_float4(acc_s[rt][0] + 0.f, acc_s[rt][1] + 0.f, acc_s[rt][2] + 0.f, acc_s[rt][3] + 0.f);   // (the null bias: -0 -> +0)
                v.x += a4[rt].x; v.y += a4[rt].y; v.z += a4[rt].z; v.w += a4[rt].w;
                *(float4 *)(Y + row * ldy + 16 * w + 4 * gq) = v;
            }
        }
        lds_barrier();
    }
}

template <bool SAVE = false>
int launch_sb_encoder_tail(int64_t Rs, const float *X, int64_t ldx, const float *Wa, const float *ba, const float *Ws, int64_t ldw, const float *C,
                           int64_t ldc, float *Y, int64_t ldy, hipStream_t st, float *emb = nullptr, int64_t lde = 0, uint8_t *ebits = nullptr,
                           int64_t ldb = 0) {
    constexpr int lds = (SBE_WIMG + 2 * SBE_IMG) * 16;
    static std::once_flag once;   // the evaluator's thread may launch concurrently with the trainer's
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_sb_encoder_tail<SAVE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    const int64_t n_t = (Rs + 31) / 32;
    const int grid = n_t < (int64_t)cus ? (int)n_t : cus;
    hipLaunchKernelGGL(k_sb_encoder_tail<SAVE>, dim3(grid), dim3(512), lds, st, Rs, X, ldx, Wa, ba, Ws, ldw, C, ldc, Y, ldy, emb, lde, ebits, ldb);
    return (int)hipGetLastError();
}
