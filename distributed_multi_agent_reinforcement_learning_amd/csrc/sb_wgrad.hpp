// sb_wgrad.hpp -- weight gradient C[M][N] = A^T B in fp32 arithmetic on the bf16 matrix pipe (k_sb_wgrad; C ABI: include/mappo_ops.h
// wgrad_split_tn / wgrad_split_tn2; launched from csrc/mappo_ops.hip)
#pragma once
#include "sb_common.hpp"

// ---- weight gradient  C[M][N] = A^T B in the split arithmetic (A [K][M], B [K][N], K ~ 5e5 rows) -------------------------------------
// One workgroup owns the WHOLE M x N output in its accumulators and a contiguous range of the rows (split-K, partials reduced in a fixed
// order afterwards by k_wgrad_reduce).  Rows arrive in chunks of 16 (a "unit" is 4 consecutive rows x 4 consecutive features, one
// 16-byte load per row -- a wave reads 1 KB contiguous pieces of a row), are split into three bf16 pieces and written, per feature and
// piece, as half of a 16-byte LDS word that holds 8 consecutive rows of one feature: exactly the 8 contraction steps a lane feeds to
// v_mfma_f32_32x32x16_bf16 (lane (i, g): tile row/column i, steps 8 g .. 8 g + 7), so an operand is one ds_read_b128 and the
// transposition K-major -> feature-major costs nothing.  Features inside a 64-byte block are XOR-swizzled by (feature / 8) % 4 to spread
// the writes (lane stride 64 bytes) over the banks; readers of 32 consecutive features stay conflict-free.
// Producer / consumer: 12 waves, three per SIMD.  Waves 0-7 (two per SIMD) only read operands from the LDS image and issue MFMAs; waves
// 8-11 (one per SIMD) only load, split and stage.  The image is double-buffered (2 x 48 KB at M + N = 512): the loaders write chunk c + 1
// while the MFMA waves multiply chunk c, one barrier per chunk.  Each loader lane keeps the raw rows of DEPTH chunks in flight (96 KB
// per CU at M + N = 512: 2 units per lane and chunk, 3 chunks; 64 KB at M + N = 256: 1 unit, 4 chunks), so the prefetch depth is not
// paid for out of the MFMA waves' registers.  All 12 waves get the same register allocation: 168 per lane at 3 waves per SIMD; the
// kernels take 107 (128 x 128), 132 (128 x 256, 256 x 128), 148 (384 x 128) and 153 (128 x 384), no scratch
// (hipcc -Rpass-analysis=kernel-resource-usage).
// What a loader wave may issue beside the MFMA waves of its SIMD (stamps in profiles/r20_sb_wgrad_lab.txt): its
// loads, LDS stores and single-rate vector instructions overlap with their MFMAs; packed fp32 instructions (v_pk_add_f32, which the
// compiler's SLP vectoriser makes of the two subtractions of a split) do not -- with them the loader advanced at a fifth of its speed
// while MFMAs were in flight, and a chunk took the MFMA phase PLUS most of the staging.  Hence sb_wg_split2 below.  The prefetch depth,
// a static s_setprio on either role and one MFMA wave per SIMD instead of two did not move the kernel's time and are not here.
// The chunk ranges, the chunk order and the order of the six piece products are those of the 8-wave kernel this replaces: every
// output sees the same sums in the same order, bit for bit.  The K % 16 rows behind the last full chunk are the exception: the last
// workgroup multiplies them in fp32 itself (see sb_wgrad_mma), after its chunks, the same way at every launch.
// Probe hooks and knock-outs: nothing in the product.  tools/microbench/sb_wgrad_lab.hip compiles this header with the hooks defined to
// sum s_memtime cycles per phase and wave, and with SB_WG_KNOCK to leave one side of the pipeline out (timing only).
#ifndef SB_WG_PROBE
#define SB_WG_PROBE_BEGIN
#define SB_WG_PROBE(phase)
#define SB_WG_PROBE_USE(r)
#define SB_WG_PROBE_END(wave, lane)
#endif
#ifndef SB_WG_KNOCK
#define SB_WG_KNOCK 0
#endif
constexpr int SB_WG_MMA_WAVES = 8, SB_WG_LOAD_WAVES = 4, SB_WG_THREADS = 64 * (SB_WG_MMA_WAVES + SB_WG_LOAD_WAVES);

template <int MT, int NT>
struct SbWgCfg {
    static constexpr int M = 128 * MT, N = 128 * NT, COLS = M + N, FQ = COLS / 4;
    static constexpr int CR = 16, NO = 2;                // rows and row octets per chunk
    static constexpr int WGM = MT >= NT ? 4 : 2;         // wave grid WGM x WGN over the output, TM x TN tiles of 32 x 32 per wave
    static constexpr int WGN = 8 / WGM;
    static constexpr int TM = M / 32 / WGM, TN = N / 32 / WGN;
    static constexpr int UNITS = 2 * NO * FQ;            // (row octet, half, feature quad) load units per chunk
    static constexpr int LT = 64 * SB_WG_LOAD_WAVES;     // loader threads
    static constexpr int UL = (UNITS + LT - 1) / LT;     // units per loader thread and chunk (unit = loader thread + LT u)
    static constexpr int DEPTH = UL == 1 ? 4 : 3;        // chunks in flight per loader lane: 16 UL DEPTH registers (4 x 2 spills)
    static constexpr int IMG = 3 * NO * COLS;            // uint4 per LDS image
    static constexpr int LDS_BYTES = 2 * IMG * 16;
};

// sb_split2 for the loader waves: the same operations on the same values, so the same pieces bit for bit, but one of the two
// subtractions of each level passes through an empty asm.  That keeps the SLP vectoriser from pairing them into v_pk_add_f32
// (plus the v_mov that line the pairs up), which does not issue beside the SIMD's MFMAs (see above): 64 v_sub_f32 per chunk and
// lane instead of 32 v_pk_add_f32 + 24 v_mov_b32 took a 16-row chunk of the 512-column kernels from 4 050 to 3 050 cycles.
__device__ __forceinline__ void sb_wg_split2(float x0, float x1, uint32_t &p1, uint32_t &p2, uint32_t &p3) {
    p1 = sb_pk(x0, x1);
    float r0 = x0 - __builtin_bit_cast(float, p1 << 16), r1 = x1 - __builtin_bit_cast(float, p1 & 0xffff0000u);
    asm("" : "+v"(r0));
    p2 = sb_pk(r0, r1);
    float q0 = r0 - __builtin_bit_cast(float, p2 << 16), q1 = r1 - __builtin_bit_cast(float, p2 & 0xffff0000u);
    asm("" : "+v"(q0));
    p3 = sb_pk(q0, q1);
}

// feature f's slot in the LDS image
__device__ __forceinline__ int sb_swz(int f) { return (f & ~3) | ((f & 3) ^ ((f >> 3) & 3)); }

// Loader role (loader wave lw = wave - 8, wave-uniform): fetch rows into registers DEPTH chunks ahead, split them into the image the
// MFMA waves read next.
// The barrier sequence (one before the first chunk, one per chunk, one before the tail) is the MFMA role's.
template <int MT, int NT>
__device__ __forceinline__ void sb_wgrad_loader(int lw, int lane, const float *__restrict__ A, int64_t lda, const float *__restrict__ B, int64_t ldb, int64_t K,
                                                const float *__restrict__ A2, int64_t lda2, int M1, int64_t c_beg, int64_t c_end, bool tail,
                                                uint4 *sb_lds) {
    using C = SbWgCfg<MT, NT>;
    const float *src[C::UL];
    int64_t ld[C::UL];
    bool on[C::UL];
    int row_in_chunk[C::UL], slot2[C::UL], sx[C::UL];
#pragma unroll
    for (int u = 0; u < C::UL; u++) {
        const int unit = 64 * lw + lane + C::LT * u;
        on[u] = (u + 1) * C::LT <= C::UNITS || 64 * lw + C::LT * u < C::UNITS;   // known at compile time or wave-uniform: no divergence
        const int rest = on[u] ? unit / C::FQ : 0, col = on[u] ? 4 * (unit % C::FQ) : 0;   // an idle unit loads unit 0's rows
        row_in_chunk[u] = 4 * rest;                      // = 8 octet + 4 half
        const bool in_a2 = A2 != nullptr && col >= M1 && col < C::M;
        ld[u] = in_a2 ? lda2 : (col < C::M ? lda : ldb);
        src[u] = (in_a2 ? A2 + (col - M1) : (col < C::M ? A + col : B + (col - C::M))) + row_in_chunk[u] * ld[u];
        slot2[u] = 2 * ((rest >> 1) * C::COLS + col) + (rest & 1);   // in 8-byte units
        sx[u] = (col >> 3) & 3;
    }
    // Every fetch is issued, by every lane: past c_end the last chunk is loaded again (and never staged), idle units load unit 0's rows.
    // A load under a branch would make the compiler's s_waitcnt assume it may not have been issued: it then waits for the chunks
    // behind the one being staged too (vmcnt(0..3) instead of vmcnt(4 UL (DEPTH - 1))), and the prefetch depth collapses.
    constexpr int D = C::DEPTH;
    float4 raw[D][C::UL][4];
    auto fetch = [&](float4 (&r)[C::UL][4], int64_t c) {
        c = c < c_end ? c : c_end - 1;
#pragma unroll
        for (int u = 0; u < C::UL; u++) {
            const float *p = src[u] + c * C::CR * ld[u];
#pragma unroll
            for (int j = 0; j < 4; j++) r[u][j] = *(const float4 *)(p + j * ld[u]);
        }
    };
    // registers -> three bf16 pieces -> LDS image
    auto stage = [&](const float4 (&r)[C::UL][4], uint4 *img) {
        uint2 *img2 = (uint2 *)img;
        if constexpr (SB_WG_KNOCK == 2) {                // no splits, no LDS stores: the loads are only waited for
#pragma unroll
            for (int u = 0; u < C::UL; u++)
#pragma unroll
                for (int j = 0; j < 4; j++) asm volatile("" ::"v"(r[u][j].x), "v"(r[u][j].y), "v"(r[u][j].z), "v"(r[u][j].w));
            return;
        }
#pragma unroll
        for (int u = 0; u < C::UL; u++) {
            if (!on[u]) continue;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                uint32_t p[3][2];
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const float4 &v0 = r[u][2 * q], &v1 = r[u][2 * q + 1];
                    const float x0 = t == 0 ? v0.x : t == 1 ? v0.y : t == 2 ? v0.z : v0.w;
                    const float x1 = t == 0 ? v1.x : t == 1 ? v1.y : t == 2 ? v1.z : v1.w;
                    sb_wg_split2(x0, x1, p[0][q], p[1][q], p[2][q]);
                }
#pragma unroll
                for (int s = 0; s < 3; s++) {
                    if constexpr (SB_WG_KNOCK == 3) asm volatile("" ::"v"(p[s][0]), "v"(p[s][1]));   // splits, no LDS stores
                    else img2[2 * s * C::NO * C::COLS + slot2[u] + 2 * (t ^ sx[u])] = make_uint2(p[s][0], p[s][1]);
                }
            }
        }
    };
    SB_WG_PROBE_BEGIN
    if (c_beg < c_end) {
#pragma unroll
        for (int d = 0; d < D; d++) fetch(raw[d], c_beg + d);
        // issue order as in the loop, so that the loop is entered with the same loads outstanding in the same order as its back edge
        // (the s_waitcnt pass merges the two: a reordered prologue made the first step of every D drain all loads)
        __builtin_amdgcn_sched_barrier(0);
        stage(raw[0], sb_lds);
        __builtin_amdgcn_sched_barrier(0);
        fetch(raw[0], c_beg + D);
    }
    lds_barrier();
    SB_WG_PROBE(0)
    // invariant at the top of step c: image (c - c_beg) % 2 holds chunk c; raw[(c + k - c_beg) % D] holds chunk c + k, k = 1 .. D
    for (int64_t c = c_beg; c < c_end; c += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const int64_t cc = c + d;
            if (cc >= c_end) break;
            SB_WG_PROBE_USE(raw[(d + 1) % D])
            SB_WG_PROBE(4)
            // at cc = c_end - 1 this stages a copy of the last chunk into the image nobody reads again (no branch: see fetch)
            stage(raw[(d + 1) % D], sb_lds + ((cc + 1 - c_beg) & 1) * C::IMG);
            SB_WG_PROBE(1)
            fetch(raw[(d + 1) % D], cc + 1 + D);
            SB_WG_PROBE(2)
            lds_barrier();
            SB_WG_PROBE(3)
        }
    }
    SB_WG_PROBE_END(SB_WG_MMA_WAVES + lw, lane)
    if (tail) {                                          // the K % 16 rows after the last full chunk, zero-filled: raw fp32, [row][COLS] over image 0
        const int64_t r0 = (K / C::CR) * C::CR;
        float4 *rawf = (float4 *)sb_lds;                 // 64 COLS of the image's 96 COLS bytes; every MFMA wave is past its last chunk here
#pragma unroll
        for (int u = 0; u < C::UL; u++) {
            if (!on[u]) continue;
            const int unit = 64 * lw + lane + C::LT * u, col = 4 * (unit % C::FQ);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = row_in_chunk[u] + j;
                rawf[(row * C::COLS + col) >> 2] = r0 + row < K ? *(const float4 *)(src[u] + (r0 + j) * ld[u]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        lds_barrier();
    }
}

// MFMA role (waves 0-7): wave (wm, wn) of a WGM x WGN grid owns TM x TN tiles of 32 x 32; its partial tile goes to `part` [blockIdx.x][M][N].
template <int MT, int NT>
__device__ __forceinline__ void sb_wgrad_mma(int wave, int lane, int64_t c_beg, int64_t c_end, bool tail, const uint4 *sb_lds, float *__restrict__ part) {
    using C = SbWgCfg<MT, NT>;
    const int i = lane & 31, g = lane >> 5;
    const int wm = wave / C::WGN, wn = wave % C::WGN;
    f32x16 acc[C::TM][C::TN];
#pragma unroll
    for (int a = 0; a < C::TM; a++)
#pragma unroll
        for (int b = 0; b < C::TN; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;
    auto multiply = [&](const uint4 *buf) {
        const uint4 *img = buf + g * C::COLS;
        constexpr int PS = C::NO * C::COLS;              // piece stride
        if constexpr (C::TN <= C::TM) {                  // the narrower side's operands stay in registers across the other's tiles
            uint4 b[C::TN][3];
#pragma unroll
            for (int nt = 0; nt < C::TN; nt++) {
                const int f = sb_swz(C::M + 32 * (wn * C::TN + nt) + i);
#pragma unroll
                for (int s = 0; s < 3; s++) b[nt][s] = img[s * PS + f];
            }
#pragma unroll
            for (int mt = 0; mt < C::TM; mt++) {
                const int f = sb_swz(32 * (wm * C::TM + mt) + i);
                uint4 a[3];
#pragma unroll
                for (int s = 0; s < 3; s++) a[s] = img[s * PS + f];
#pragma unroll
                for (int nt = 0; nt < C::TN; nt++) acc[mt][nt] = sb_mma6_32(a, b[nt], acc[mt][nt]);
            }
        } else {
            uint4 a[C::TM][3];
#pragma unroll
            for (int mt = 0; mt < C::TM; mt++) {
                const int f = sb_swz(32 * (wm * C::TM + mt) + i);
#pragma unroll
                for (int s = 0; s < 3; s++) a[mt][s] = img[s * PS + f];
            }
#pragma unroll
            for (int nt = 0; nt < C::TN; nt++) {
                const int f = sb_swz(C::M + 32 * (wn * C::TN + nt) + i);
                uint4 b[3];
#pragma unroll
                for (int s = 0; s < 3; s++) b[s] = img[s * PS + f];
#pragma unroll
                for (int mt = 0; mt < C::TM; mt++) acc[mt][nt] = sb_mma6_32(a[mt], b, acc[mt][nt]);
            }
        }
    };
    SB_WG_PROBE_BEGIN
    lds_barrier();
    SB_WG_PROBE(0)
    for (int64_t c = c_beg; c < c_end; c++) {
        if constexpr (SB_WG_KNOCK != 1) multiply(sb_lds + ((c - c_beg) & 1) * C::IMG);
        SB_WG_PROBE(1)
        lds_barrier();
        SB_WG_PROBE(3)
    }
    SB_WG_PROBE_END(wave, lane)
    if (tail) {
        // The tail rows are multiplied in fp32 itself (v_mfma_f32_32x32x2_f32: a chain of round-to-nearest multiply-adds; lane (i, g)
        // feeds tile row / column i of row 2 s + g), not as piece products: a product of fewer than 16 rows, which is a tail alone,
        // then meets the K 2^-24 bound of an fp32 dot product, which the bf16 instruction's truncated accumulation misses at K = 1
        // (DESIGN.md section 3.7).  The benchmark's row counts are multiples of 16 and never come here.
        lds_barrier();
        const float *rawf = (const float *)sb_lds;
#pragma unroll 1
        for (int s = 0; s < C::CR / 2; s++) {
            const float *row = rawf + (2 * s + g) * C::COLS;
            float b[C::TN];
#pragma unroll
            for (int nt = 0; nt < C::TN; nt++) b[nt] = row[C::M + 32 * (wn * C::TN + nt) + i];
#pragma unroll
            for (int mt = 0; mt < C::TM; mt++) {
                const float a = row[32 * (wm * C::TM + mt) + i];
#pragma unroll
                for (int nt = 0; nt < C::TN; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[nt], acc[mt][nt], 0, 0, 0);
            }
        }
    }
    // D tile (32 x 32): lane (i, g), register r -> row 8 (r / 4) + 4 g + r % 4 (the A operand's tile row: an M index), column i
    float *po = part + (size_t)blockIdx.x * C::M * C::N + (size_t)(32 * wm * C::TM + 4 * g) * C::N + 32 * wn * C::TN + i;
#pragma unroll
    for (int mt = 0; mt < C::TM; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++)
#pragma unroll
            for (int nt = 0; nt < C::TN; nt++) po[(size_t)(32 * mt + 8 * (r / 4) + (r % 4)) * C::N + 32 * nt] = acc[mt][nt][r];
}

// A may come in two column blocks (A2 != nullptr: columns M1 .. M - 1 from A2, row stride lda2): the GRU's dW_hh = [dr dz | dnr]^T h_prev
// takes (dr, dz) from dgi and dnr from its own tensor in ONE pass over h_prev.  Launch: SB_WG_THREADS threads, SbWgCfg::LDS_BYTES.
template <int MT, int NT>
__global__ __launch_bounds__(SB_WG_THREADS) void k_sb_wgrad(const float *__restrict__ A, int64_t lda, const float *__restrict__ B, int64_t ldb, int64_t K,
                                                            float *__restrict__ part, const float *__restrict__ A2, int64_t lda2, int M1) {
    using C = SbWgCfg<MT, NT>;
    static_assert(C::WGM * C::WGN == SB_WG_MMA_WAVES && C::TM * C::WGM * 32 == C::M && C::TN * C::WGN * 32 == C::N, "tiling");
    extern __shared__ uint4 sb_lds[];                    // [buffer][piece][octet][feature slot] x 16 bytes
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the role branch is a scalar branch
    const int64_t chunks = K / C::CR;                    // full chunks; the K % 16 tail rows are the last workgroup's epilogue
    const int64_t c_beg = chunks * blockIdx.x / gridDim.x, c_end = chunks * (blockIdx.x + 1) / gridDim.x;
    const bool tail = blockIdx.x == gridDim.x - 1 && (K % C::CR);
    if (wave >= SB_WG_MMA_WAVES)
        sb_wgrad_loader<MT, NT>(wave - SB_WG_MMA_WAVES, threadIdx.x & 63, A, lda, B, ldb, K, A2, lda2, M1, c_beg, c_end, tail, sb_lds);
    else
        sb_wgrad_mma<MT, NT>(wave, threadIdx.x & 63, c_beg, c_end, tail, sb_lds, part);
}
