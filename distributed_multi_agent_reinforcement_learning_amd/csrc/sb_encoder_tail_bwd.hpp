// sb_encoder_tail_bwd.hpp -- the update encoder's semantic-layer and AGG-layer input gradients as one launch (C ABI: include/mappo_ops.h
// sb_encoder_tail_bwd); the mirror of csrc/sb_encoder_tail.hpp
#pragma once
#include <mutex>

#include "sb_common.hpp"
#include "sb_encoder_tail.hpp"
#include "sb_gemm.hpp"

// ---- ga[s, r] = (g[s] Ws_r) * relu'(emb[s, r]),  d_m3[s, r] = ga[s, r] W_agg,  column sums of ga  (k_sb_encoder_tail_bwd) -----------
// The backward of DHGN._after_messages' two layers with respect to their inputs.  As two k_sb_gemm_n128 launches (<4,3,20>: the masked
// input gradient of the semantic layer from the sign bits, with the column sums; <4,1,2>: the input gradient of the AGG layer) the
// (Rs, 384) gradient ga is written by the first and read straight back by the second.  It still has to be written once (the AGG weight
// gradient reads it); here the second GEMM takes it from LDS, 32 rows x 128 units at a time.
// Persistent 512-thread workgroups, 32 semantic rows per tile, the g rows of a tile staged ONCE (one 24 KB image) for its three STEPS
// (relations, in order); wave w owns units 16 w .. 16 w + 15 of both results.  A step:
//   semantic^T  acc = Ws_r^T x the g image (4 chunks of 32 outputs of the semantic layer, six piece products each in SBG_MMA order, from
//               zero); the sign bits' nibble keeps or zeroes each of the lane's four; + into the lane's column sums (rows < Rs, in row-half
//               order); one 16-byte store into ga: per output, and per column sum, exactly k_sb_gemm_n128<4,3,20> (same grid, same tile
//               stride, same summation order: the partial rows are its partial rows)
//   hand-over   the lane's four are split (sb_split2) into the ga image as in k_sb_encoder_tail
//   barrier     (the ga image is complete; after step 2 every wave is also done with the g image)
//   AGG^T       acc = W_agg^T x the ga image (4 chunks of 32 units), + 0.f (the null bias), one 16-byte store into d_m3: per output exactly
//               k_sb_gemm_n128<4,1,.> on ga viewed as (3 Rs, 128)
//   staging     step 2 only: the g rows of the next tile (requested a tile ago) are split into the g image, those of the tile after
//               requested: waves 0-3 before their AGG^T phase, waves 4-7 after it
//   barrier     (every wave is done reading the ga image; after step 2 the g image is complete)
// Registers: the three 128 x 128 blocks of Ws^T stay resident as pieces (144 per lane, as <4,3,20> holds them); the W_agg^T pieces live
// in a 96 KB LDS image written once in the prologue.  Both transposes are gathered in the prologue from the weights as stored (Ws may
// be a column block, row stride ldw): no transposed copy is made on the way in.
// LDS: 96 KB W_agg^T image + 24 KB g image + 24 KB ga image = 144 KB.
__global__ __launch_bounds__(512) void k_sb_encoder_tail_bwd(int64_t Rs, const float *__restrict__ G, int64_t ldg, const float *__restrict__ Ws,
                                                             int64_t ldw, const float *__restrict__ Wa, const uint8_t *__restrict__ ebits, int64_t ldb,
                                                             float *__restrict__ GA, int64_t ldga, float *__restrict__ DM, int64_t ldd,
                                                             float *__restrict__ colsum_part) {
    extern __shared__ uint4 sbe_lds[];                  // [W_agg^T image | g image | ga image]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 15, gq = l >> 4;
    uint4 *const wimg = sbe_lds + w * (4 * 3 * 64) + l, *const gimg = sbe_lds + SBE_WIMG, *const aimg = gimg + SBE_IMG;
    {
        const float *cw = Wa + (size_t)(8 * gq) * 128 + 16 * w + i;   // W_agg^T row 16 w + i, inputs 32 c + 8 gq .. + 7 = W_agg[32 c + 8 gq + j][16 w + i]
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float *s = cw + (size_t)(32 * c) * 128;
            uint4 p_[3];
            sb_split8(make_float4(s[0], s[128], s[256], s[384]), make_float4(s[512], s[640], s[768], s[896]), p_);
#pragma unroll
            for (int p = 0; p < 3; p++) wimg[(c * 3 + p) * 64] = p_[p];
        }
    }
    uint4 ws[12][3];                                    // Ws^T rows 128 r + 16 w + i: chunk 4 r + c holds Ws[32 c + 8 gq + j][128 r + 16 w + i]
    {
        const float *cw = Ws + (size_t)(8 * gq) * ldw + 16 * w + i;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float *s = cw + (size_t)(32 * c) * ldw + 128 * r;
                sb_split8(make_float4(s[0], s[ldw], s[2 * ldw], s[3 * ldw]), make_float4(s[4 * ldw], s[5 * ldw], s[6 * ldw], s[7 * ldw]), ws[4 * r + c]);
            }
        }
    }
    const int64_t n_t = (Rs + 31) / 32, G_ = gridDim.x;
    float4 pf[2];
    // wave w stages (chunk w / 2, half w & 1) of a tile's g image: lane (gq, j) loads outputs 32 c + 8 gq .. of row j of the half
    auto fetch = [&](int64_t t) {
        const int64_t row = t * 32 + (w & 1) * 16 + i;
        pf[0] = pf[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < Rs) {
            const float *src = G + row * ldg + 32 * (w >> 1) + 8 * gq;
            pf[0] = *(const float4 *)src;
            pf[1] = *(const float4 *)(src + 4);
        }
    };
    auto stage = [&]() {
        uint4 p_[3];
        sb_split8(pf[0], pf[1], p_);
#pragma unroll
        for (int p = 0; p < 3; p++) gimg[(p * 8 + w) * 64 + l] = p_[p];
    };
    // this lane's half words of the ga image: chunk w / 2, octet 2 (w & 1) + gq / 2, column i, half gq & 1
    uint2 *const adst = (uint2 *)aimg + (((w >> 1) * 2) * 64 + ((2 * (w & 1) + (gq >> 1)) << 4) + i) * 2 + (gq & 1);   // + 128: the second row half
    float4 cs[3];
#pragma unroll
    for (int r = 0; r < 3; r++) cs[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned mbn[2];
    auto mask = [&](int64_t t, int r) {
#pragma unroll
        for (int rt = 0; rt < 2; rt++) {
            const int64_t row = t * 32 + rt * 16 + i;
            mbn[rt] = row < Rs ? (unsigned)ebits[row * ldb + 16 * r + 2 * w + (gq >> 1)] : 255u;
        }
    };
    int64_t t = blockIdx.x;
    if (t < n_t) { fetch(t); stage(); mask(t, 0); }
    if (t + G_ < n_t) fetch(t + G_);
    lds_barrier();
    for (; t < n_t; t += G_) {
        const bool more = t + G_ < n_t;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            // relu' as bits: one byte per half holds this lane's four (a nibble).  The bytes of step n + 1 are requested at the head of step
            // n: a load returns behind every older store of the wave, and the stores just issued are acknowledged late
            unsigned mb[2] = {mbn[0], mbn[1]};
            if (r < 2) mask(t, r + 1);
            else if (more) mask(t + G_, 0);
            f32x4 acc[2];
            acc[0] = acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#define SBE_MMA(A, pi, pj)                                                                                                                          \
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[pi]), __builtin_bit_cast(bf16x8, b0[pj]), acc[0], 0, 0, 0); \
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A[pi]), __builtin_bit_cast(bf16x8, b1[pj]), acc[1], 0, 0, 0);
#define SBE_MMA6(A) SBE_MMA(A, 2, 0) SBE_MMA(A, 0, 2) SBE_MMA(A, 1, 1) SBE_MMA(A, 1, 0) SBE_MMA(A, 0, 1) SBE_MMA(A, 0, 0)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                uint4 b0[3], b1[3];
#pragma unroll
                for (int p = 0; p < 3; p++) { b0[p] = gimg[(p * 8 + 2 * c) * 64 + l]; b1[p] = gimg[(p * 8 + 2 * c + 1) * 64 + l]; }
                SBE_MMA6(ws[4 * r + c])
            }
            // D tile: lane (i, gq), register q -> unit 16 w + 4 gq + q of relation r of row i of the half
#pragma unroll
            for (int rt = 0; rt < 2; rt++) {
                const int64_t row = t * 32 + rt * 16 + i;
                const unsigned m = mb[rt] >> ((gq & 1) * 4);
                float4 v = make_float4(acc[rt][0], acc[rt][1], acc[rt][2], acc[rt][3]);
                v.x = (m & 1u) ? v.x : 0.f; v.y = (m & 2u) ? v.y : 0.f; v.z = (m & 4u) ? v.z : 0.f; v.w = (m & 8u) ? v.w : 0.f;
                if (row < Rs) {
                    cs[r].x += v.x; cs[r].y += v.y; cs[r].z += v.z; cs[r].w += v.w;
                    *(float4 *)(GA + row * ldga + 128 * r + 16 * w + 4 * gq) = v;
                }
                uint32_t lo[3], hi[3];
                sb_split2(v.x, v.y, lo[0], lo[1], lo[2]);
                sb_split2(v.z, v.w, hi[0], hi[1], hi[2]);
#pragma unroll
                for (int p = 0; p < 3; p++) adst[p * 8 * 64 * 2 + rt * 128] = make_uint2(lo[p], hi[p]);
            }
            lds_barrier();
            auto next_tile = [&]() {   // tile n + 1 -> the g image, tile n + 2 requested
                if (more) stage();
                if (t + 2 * G_ < n_t) fetch(t + 2 * G_);
            };
            if (r == 2 && w < 4) next_tile();
            acc[0] = acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                uint4 a_[3], b0[3], b1[3];
#pragma unroll
                for (int p = 0; p < 3; p++) { a_[p] = wimg[(c * 3 + p) * 64]; b0[p] = aimg[(p * 8 + 2 * c) * 64 + l]; b1[p] = aimg[(p * 8 + 2 * c + 1) * 64 + l]; }
                SBE_MMA6(a_)
            }
#undef SBE_MMA6
#undef SBE_MMA
            if (r == 2 && w >= 4) next_tile();
#pragma unroll
            for (int rt = 0; rt < 2; rt++) {
                const int64_t row = t * 32 + rt * 16 + i;
                if (row < Rs)   // (the null bias: -0 -> +0)
                    *(float4 *)(DM + row * ldd + 128 * r + 16 * w + 4 * gq) = make_float4(acc[rt][0] + 0.f, acc[rt][1] + 0.f, acc[rt][2] + 0.f, acc[rt][3] + 0.f);
            }
            lds_barrier();
        }
    }
    // this workgroup's column sums: the 16 row lanes of a column group fold, lane i = 0 stores (as k_sb_gemm_n128, OPT & 4)
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            cs[r].x += __shfl_xor(cs[r].x, m); cs[r].y += __shfl_xor(cs[r].y, m);
            cs[r].z += __shfl_xor(cs[r].z, m); cs[r].w += __shfl_xor(cs[r].w, m);
        }
        if (i == 0) *(float4 *)(colsum_part + (size_t)blockIdx.x * 384 + 128 * r + 16 * w + 4 * gq) = cs[r];
    }
}

// colsum_part: one row of 384 partial sums per workgroup (<= CUs); colsum (384): their sum in workgroup order (k_sb_colsum_reduce)
inline int launch_sb_encoder_tail_bwd(int64_t Rs, const float *G, int64_t ldg, const float *Ws, int64_t ldw, const float *Wa, const uint8_t *ebits,
                                      int64_t ldb, float *GA, int64_t ldga, float *DM, int64_t ldd, float *colsum_part, float *colsum, int cus,
                                      hipStream_t st) {
    constexpr int lds = (SBE_WIMG + 2 * SBE_IMG) * 16;
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_sb_encoder_tail_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    const int64_t n_t = (Rs + 31) / 32;
    const int grid = n_t < (int64_t)cus ? (int)n_t : cus;   // k_sb_gemm_n128<4,3,20>'s grid: its workgroup-to-tile assignment decides the partial sums
    hipLaunchKernelGGL(k_sb_encoder_tail_bwd, dim3(grid), dim3(512), lds, st, Rs, G, ldg, Ws, ldw, Wa, ebits, ldb, GA, ldga, DM, ldd, colsum_part);
    hipLaunchKernelGGL(k_sb_colsum_reduce, dim3(3), dim3(128), 0, st, grid, 384, colsum_part, colsum);
    return (int)hipGetLastError();
}
