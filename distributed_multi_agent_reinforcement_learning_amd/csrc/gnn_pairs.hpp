// gnn_pairs.hpp -- the GnnExtractor encoder's per-pair MLP and its adjacency-weighted sum as one launch each way
// (C ABI: include/mappo_ops.h gnn_pair_agg_fwd / gnn_pair_agg_bwd).
//
//   x_ij  = [state_j - state_i (4), one-hot(type of j) (3)]          entity j of row r: P pursuers, the evader, O obstacles of row r / q_div
//   h1_ij = relu(W1 x_ij + b1),  h2_ij = relu(W2 h1_ij + b2)         W1 [128][7], W2 [128][128]
//   agg[r, i] = sum over j of (adj_ij / max(sum_j |adj_ij|, 1e-12)) h2_ij
//
// A SEGMENT is one (r, i); persistent 512-thread workgroups take segments blockIdx.x, + gridDim.x, ..  Per segment:
//   list     the lanes compact the j with adj_ij != 0, in order of j, into LDS (ballot + popcount per wave, wave offsets through LDS):
//            relative state, adjacency value and j of each listed pair.  The critic (ones) lists all K.  sum |adj| is reduced in a fixed
//            order beside it.  Every thread passes every barrier whatever the list's length.
//   tile     TILE listed pairs.  Layer 1 is VALU: a lane makes 8 consecutive units of one pair (four fmaf onto W1[:, 4 + type] + b1, ReLU),
//            splits them (sb_split8) and writes one 16-byte B-operand word per piece into the h1 image [piece][chunk][subtile][lane].
//            Layer 2: wave w owns units 16 w .. 16 w + 15, W2's rows as A-operand pieces in 48 registers for the whole launch (as the GRU
//            kernels hold W_hh: the image is then the only LDS traffic of the matrix phase, which that traffic already bounds -- a wave
//            reads 48 B of image per MFMA -- and the backward needs the 96 KB for its four images); per 16-pair subtile 4 chunks x six piece products (sb_mma6_hl).  The D tile has lane (n, gq) own units
//            16 w + 4 gq .. + 3 of pair n: + b2, ReLU, x weight in registers, then the 16 pairs are added across lanes (xor 1, 2, 4, 8) and
//            the subtiles and tiles of the segment in order.  Subtiles past the end of the list are skipped (wave-uniform); pairs past
//            the end inside a subtile are computed on zeros with weight 0.
// No (pairs, .) tensor reaches HBM, no atomics; a segment's bits depend on its own inputs only.
//
// The backward saves nothing: it rebuilds the list and h1 / z2 per 32-pair tile with the functions of the forward (gp_h1, sb_mma6_hl in
// the same chunk order), so the ReLU masks are the forward's.  Layout in LDS (96 KB of images + 28 KB of lists and tables):
//   h1 image   pair-major  [piece][chunk][subtile][lane]   B operand of z2 = W2 h1; its leading piece is the mask [z1 > 0] of g1
//   h1T image  unit-major  [piece][column tile][lane]      B operand of dW2 += g2^T h1 (contraction over the tile's 32 pairs); made by the VALU
//                                                          a second time in this order (5 flops a value) instead of a transpose through LDS
//   g2 image   pair-major  [piece][chunk][subtile][lane]   B operand of g1 = (W2^T) g2; written from the D tile as 8-byte half words
//   g2T image  unit-major  [piece][wave][lane]             A operand of dW2: wave w's own 16 units, written as single bf16, wave-private
// W2 is held in BOTH orientations in registers, so neither costs LDS: rows 16 w .. of W2 as pieces (48) for z2, rows 16 w .. of W2^T as
// fp32 (32), split once per tile for g1 (as pieces too the kernel spills at 256 registers).
// dW1 += g1^T [x | 0] is one more product over the tile's pairs: g1^T overwrites the wave's g2T words (already in registers), x^T is a
// 3 KB image that wave 0 makes beside h1.  dW2 (8 column tiles), dW1 (one tile) and db2 stay in
// registers over all the workgroup's tiles; one partial block per workgroup, k_gnn_pair_reduce adds the blocks in order of workgroup.
// db1 is the sum of dW1's three one-hot columns (every pair has exactly one type).
#pragma once
#include <mutex>

#include "sb_common.hpp"

constexpr int GP_KMAX = 1024;                 // listed pairs of a segment (K = P + 1 + O <= GP_KMAX)
constexpr int GP_PMAX = 64;
constexpr int GP_LISTS = GP_KMAX + GP_KMAX / 2 + 8;              // uint4: rel [KMAX] float4 | a [KMAX] float | j [KMAX] int | wcnt [2][8] | wsum [8]
constexpr int GP_BLOCK = 128 * 128 + 128 * 7 + 128;              // floats of a backward partial block: dW2 | dW1 | db2
constexpr int GP_MAX_GRID = 512;
constexpr int GP_ADJ_TENSOR = 0, GP_ADJ_ONES = 1, GP_ADJ_BITS = 3;   // (MO_ADJ_*)

// The packed fp32 VALU forms stay out of these kernels (they run beside MFMAs): a per-kernel target feature, device pass only.
#if defined(__HIP_DEVICE_COMPILE__)
#define GP_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define GP_KERNEL __global__
#endif

struct GpArgs {
    int64_t R;
    int32_t P, O, q_div, mode, rw;
    const float *p, *e, *o, *adj_p, *adj_e;
    const void *adj_o;
    const float *W1, *b1, *W2, *b2;
};

// one unit of layer 1: the SAME expression wherever h1 is made, so that every copy of a value has the same bits
__device__ __forceinline__ float gp_h1(const float4 &w, float tb, const float4 &x) {
    return fmaxf(fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, fmaf(w.x, x.x, tb)))), 0.f);
}
__device__ __forceinline__ float gp_pick(const float4 &tb, int type) { return type == 0 ? tb.x : (type == 1 ? tb.y : tb.z); }
__device__ __forceinline__ int gp_type(int j, int P) { return j < P ? 0 : (j == P ? 1 : 2); }

// sum over the 16 lanes of a D-tile row group (lanes that differ in l & 15), the same order in every lane
__device__ __forceinline__ float gp_sum16(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// the pair list of segment (r, pi) -> count; denom = max(sum |adj|, 1e-12).  All 512 threads call it; ends with a barrier.
__device__ __forceinline__ int gp_build_list(const GpArgs &a, int64_t r, int pi, uint4 *lds, float &denom) {
    float4 *l_rel = (float4 *)lds;
    float *l_a = (float *)(lds + GP_KMAX);
    int *l_j = (int *)(lds + GP_KMAX + GP_KMAX / 4);
    int *wcnt = (int *)(lds + GP_KMAX + GP_KMAX / 2);
    float *wsum = (float *)(lds + GP_KMAX + GP_KMAX / 2 + 4);
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, P = a.P, O = a.O, K = P + 1 + O;
    const int64_t ri = r * P + pi;
    const float4 si = *(const float4 *)(a.p + ri * 4);
    float asum = 0.f;
    int base = 0, it = 0;
    for (int j0 = 0; j0 < K; j0 += 512, it ^= 1) {
        const int j = j0 + tid, jo = j - P - 1;
        float av = 0.f;
        if (j < K) {
            if (a.mode == GP_ADJ_ONES) av = 1.f;
            else if (j < P) av = a.adj_p[ri * P + j];
            else if (j == P) av = a.adj_e[ri];
            else if (a.mode == GP_ADJ_BITS) av = (float)((((const uint32_t *)a.adj_o)[ri * a.rw + (jo >> 5)] >> (jo & 31)) & 1u);
            else av = ((const float *)a.adj_o)[ri * O + jo];
        }
        asum += fabsf(av);
        const bool nz = av != 0.f;
        const unsigned long long bal = __ballot(nz);
        const int pre = __popcll(bal & ((1ull << l) - 1ull));
        if (l == 0) wcnt[it * 8 + w] = __popcll(bal);
        lds_barrier();
        int off = base;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int c = wcnt[it * 8 + k];
            off += k < w ? c : 0;
            base += c;
        }
        if (nz) {
            const float *sp = j < P ? a.p + (r * P + j) * 4 : (j == P ? a.e + r * 4 : a.o + ((r / a.q_div) * O + jo) * 4);
            const float4 sj = *(const float4 *)sp;
            const int pos = off + pre;
            l_rel[pos] = make_float4(sj.x - si.x, sj.y - si.y, sj.z - si.z, sj.w - si.w);
            l_a[pos] = av;
            l_j[pos] = j;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) asum += __shfl_xor(asum, m);
    if (l == 0) wsum[w] = asum;
    lds_barrier();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; k++) s += wsum[k];
    denom = fmaxf(s, 1e-12f);
    return base;
}

// listed pair `pos` of a segment with `cnt` pairs: relative state, type, weight (zeros, an obstacle, 0 past the end)
__device__ __forceinline__ void gp_pair(const uint4 *lds, int pos, int cnt, int P, float4 &x, int &type) {
    const bool ok = pos < cnt;
    x = ok ? ((const float4 *)lds)[pos] : make_float4(0.f, 0.f, 0.f, 0.f);
    type = ok ? gp_type(((const int *)(lds + GP_KMAX + GP_KMAX / 4))[pos], P) : 2;
}
__device__ __forceinline__ float gp_weight(const uint4 *lds, int pos, int cnt, float denom) {
    return pos < cnt ? ((const float *)(lds + GP_KMAX))[pos] / denom : 0.f;
}

// this lane's A operands of the layer-2 product: rows 16 w + n of W2, contraction steps 32 c + 8 gq .. + 7
__device__ __forceinline__ void gp_load_w2(const float *__restrict__ W2, int w, int n, int gq, uint4 (&out)[4][3]) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float *rw = W2 + (size_t)(16 * w + n) * 128 + 32 * c + 8 * gq;
        sb_split8(*(const float4 *)rw, *(const float4 *)(rw + 4), out[c]);
    }
}

// z2 - b2 of one 16-pair subtile: W2 rows (A, registers) x h1 image (B), chunks in order
template <int NS>
__device__ __forceinline__ f32x4 gp_z2(const uint4 (&w2)[4][3], const uint4 *img, int s, int l) {
    f32x4 hi = {0.f, 0.f, 0.f, 0.f}, lo = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        uint4 b[3];
#pragma unroll
        for (int p = 0; p < 3; p++) b[p] = img[((p * 4 + c) * NS + s) * 64 + l];
        sb_mma6_hl(w2[c], b, hi, lo);
    }
    return hi + lo;
}

GP_KERNEL __launch_bounds__(512) void k_gnn_pair_fwd(GpArgs a, float *__restrict__ agg) {
    extern __shared__ uint4 gp_lds[];                   // [lists | h1 image (64 pairs)]
    uint4 *const img = gp_lds + GP_LISTS;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, gq = l >> 4, P = a.P, c1 = w & 3;
    uint4 w2[4][3];
    gp_load_w2(a.W2, w, n, gq, w2);
    const float4 b2v = *(const float4 *)(a.b2 + 16 * w + 4 * gq);
    float4 w1[8], tb[8];                                // layer 1, units 32 c1 + 8 gq + e
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float *rw = a.W1 + (32 * c1 + 8 * gq + e) * 7;
        const float b = a.b1[32 * c1 + 8 * gq + e];
        w1[e] = make_float4(rw[0], rw[1], rw[2], rw[3]);
        tb[e] = make_float4(rw[4] + b, rw[5] + b, rw[6] + b, 0.f);
    }
    const int64_t n_seg = a.R * P;
    for (int64_t seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        float denom;
        const int cnt = gp_build_list(a, seg / P, (int)(seg % P), gp_lds, denom);
        f32x4 out = {0.f, 0.f, 0.f, 0.f};
        for (int t0 = 0; t0 < cnt; t0 += 64) {
            const int live = (cnt - t0 + 15) >> 4;      // subtiles with a listed pair (of 4)
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int s = (w >> 2) * 2 + k;
                if (s < live) {
                    float4 x;
                    int type;
                    gp_pair(gp_lds, t0 + 16 * s + n, cnt, P, x, type);
                    float h[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) h[e] = gp_h1(w1[e], gp_pick(tb[e], type), x);
                    uint4 p_[3];
                    sb_split8(make_float4(h[0], h[1], h[2], h[3]), make_float4(h[4], h[5], h[6], h[7]), p_);
#pragma unroll
                    for (int p = 0; p < 3; p++) img[((p * 4 + c1) * 4 + s) * 64 + l] = p_[p];
                }
            }
            lds_barrier();
            for (int s = 0; s < 4 && s < live; s++) {
                const f32x4 z = gp_z2<4>(w2, img, s, l);
                const float wt = gp_weight(gp_lds, t0 + 16 * s + n, cnt, denom);
                out[0] += gp_sum16(fmaxf(z[0] + b2v.x, 0.f) * wt);
                out[1] += gp_sum16(fmaxf(z[1] + b2v.y, 0.f) * wt);
                out[2] += gp_sum16(fmaxf(z[2] + b2v.z, 0.f) * wt);
                out[3] += gp_sum16(fmaxf(z[3] + b2v.w, 0.f) * wt);
            }
            lds_barrier();
        }
        if (n == 0) *(float4 *)(agg + seg * 128 + 16 * w + 4 * gq) = make_float4(out[0], out[1], out[2], out[3]);
        lds_barrier();                                  // (the lists are free)
    }
}

constexpr int GP_BIMG = 3 * 4 * 2 * 64;                 // uint4 of each of the backward's four images (32 pairs x 128 units x 3 pieces)

GP_KERNEL __launch_bounds__(512) void k_gnn_pair_bwd(GpArgs a, const float *__restrict__ d_agg, float *__restrict__ part) {
    extern __shared__ uint4 gp_lds[];                   // [lists | W1 table | h1 image | h1T image | g2 image | g2T / g1T image | xT image]
    float4 *const tabw = (float4 *)(gp_lds + GP_LISTS), *const tabb = tabw + 128;
    uint4 *const h1i = gp_lds + GP_LISTS + 256, *const h1t = h1i + GP_BIMG, *const g2i = h1t + GP_BIMG, *const g2t = g2i + GP_BIMG, *const xti = g2t + GP_BIMG;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, n = l & 15, gq = l >> 4, P = a.P, c1 = w & 3, s1 = w >> 2;
    uint4 w2[4][3];
    gp_load_w2(a.W2, w, n, gq, w2);
    float4 w2t[4][2];                                   // rows 16 w + n of W2^T, steps 32 c + 8 gq .. + 7, as fp32: split once per tile (16 registers less)
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float *cw = a.W2 + (size_t)(32 * c + 8 * gq) * 128 + 16 * w + n;
        w2t[c][0] = make_float4(cw[0], cw[128], cw[256], cw[384]);
        w2t[c][1] = make_float4(cw[512], cw[640], cw[768], cw[896]);
    }
    if (tid < 128) {
        const float *rw = a.W1 + tid * 7;
        const float b = a.b1[tid];
        tabw[tid] = make_float4(rw[0], rw[1], rw[2], rw[3]);
        tabb[tid] = make_float4(rw[4] + b, rw[5] + b, rw[6] + b, 0.f);
    }                                                   // (visible after the first list's barriers)
    // where this lane's D-tile units 16 w + 4 gq .. + 3 of pair n sit in a pair-major image: chunk w / 2, octet 2 (w & 1) + gq / 2, half gq & 1
    const int dhalf = (((w >> 1) * 2) * 64 + ((2 * (w & 1) + (gq >> 1)) << 4) + n) * 2 + (gq & 1);   // uint2 index at piece 0, subtile 0
    f32x4 dw2[8];
#pragma unroll
    for (int ct = 0; ct < 8; ct++) dw2[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 dw1 = {0.f, 0.f, 0.f, 0.f};                   // rows 16 w + 4 gq + q, column n (< 7) of dW1
    float db2[4] = {0.f, 0.f, 0.f, 0.f};
    float *const blk = part + (size_t)blockIdx.x * GP_BLOCK;   // (taken here: at the end the argument block is out of reach without a spill)
    const int64_t n_seg = a.R * P;
    for (int64_t seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
        float denom;
        const int cnt = gp_build_list(a, seg / P, (int)(seg % P), gp_lds, denom);
        for (int t0 = 0; t0 < cnt; t0 += 32) {
            {   // h1, pair-major: pair 16 s1 + n, units 32 c1 + 8 gq + e
                float4 x;
                int type;
                gp_pair(gp_lds, t0 + 16 * s1 + n, cnt, P, x, type);
                float h[8];
#pragma unroll
                for (int e = 0; e < 8; e++) h[e] = gp_h1(tabw[32 * c1 + 8 * gq + e], gp_pick(tabb[32 * c1 + 8 * gq + e], type), x);
                uint4 p_[3];
                sb_split8(make_float4(h[0], h[1], h[2], h[3]), make_float4(h[4], h[5], h[6], h[7]), p_);
#pragma unroll
                for (int p = 0; p < 3; p++) h1i[((p * 4 + c1) * 2 + s1) * 64 + l] = p_[p];
            }
            {   // h1, unit-major: unit 16 w + n, pairs 8 gq + e
                const float4 uw = tabw[16 * w + n], ub = tabb[16 * w + n];
                float h[8];
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    float4 x;
                    int type;
                    gp_pair(gp_lds, t0 + 8 * gq + e, cnt, P, x, type);
                    h[e] = gp_h1(uw, gp_pick(ub, type), x);
                }
                uint4 p_[3];
                sb_split8(make_float4(h[0], h[1], h[2], h[3]), make_float4(h[4], h[5], h[6], h[7]), p_);
#pragma unroll
                for (int p = 0; p < 3; p++) h1t[(p * 8 + w) * 64 + l] = p_[p];
            }
            if (w == 0) {   // x^T, unit-major: feature n (7 .. 15: zero columns), pairs 8 gq + e
                float h[8];
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    float4 x;
                    int type;
                    gp_pair(gp_lds, t0 + 8 * gq + e, cnt, P, x, type);
                    h[e] = n == 0 ? x.x : n == 1 ? x.y : n == 2 ? x.z : n == 3 ? x.w : (n - 4 == type ? 1.f : 0.f);
                }
                uint4 p_[3];
                sb_split8(make_float4(h[0], h[1], h[2], h[3]), make_float4(h[4], h[5], h[6], h[7]), p_);
#pragma unroll
                for (int p = 0; p < 3; p++) xti[p * 64 + l] = p_[p];
            }
            const float4 dav = *(const float4 *)(d_agg + seg * 128 + 16 * w + 4 * gq);   // (per tile: four registers less across the phases)
            lds_barrier();
#pragma unroll 1
            for (int s = 0; s < 2; s++) {               // g2 = w d_agg [z2 > 0] of pair 16 s + n, units 16 w + 4 gq + q
                const f32x4 z = gp_z2<2>(w2, h1i, s, l);
                const float4 b2v = *(const float4 *)(a.b2 + 16 * w + 4 * gq);   // (per use: registers)
                const float wt = gp_weight(gp_lds, t0 + 16 * s + n, cnt, denom);
                float g[4];
                g[0] = z[0] + b2v.x > 0.f ? wt * dav.x : 0.f;
                g[1] = z[1] + b2v.y > 0.f ? wt * dav.y : 0.f;
                g[2] = z[2] + b2v.z > 0.f ? wt * dav.z : 0.f;
                g[3] = z[3] + b2v.w > 0.f ? wt * dav.w : 0.f;
#pragma unroll
                for (int q = 0; q < 4; q++) db2[q] += g[q];
                uint32_t lo[3], hi[3];
                sb_split2(g[0], g[1], lo[0], lo[1], lo[2]);
                sb_split2(g[2], g[3], hi[0], hi[1], hi[2]);
                const int pp = 16 * s + n;              // the pair as a contraction step of dW2: octet pp / 8, element pp % 8
                uint16_t *const row = (uint16_t *)(g2t + w * 64 + (pp >> 3) * 16 + 4 * gq) + (pp & 7);   // + 8 q: unit 4 gq + q;  + 4096 p: piece p
#define GP_PUT(p)                                                                                  \
                ((uint2 *)g2i)[dhalf + ((p) * 4 * 2 + s) * 128] = make_uint2(lo[p], hi[p]);        \
                row[4096 * (p)] = (uint16_t)lo[p], row[4096 * (p) + 8] = (uint16_t)(lo[p] >> 16); \
                row[4096 * (p) + 16] = (uint16_t)hi[p], row[4096 * (p) + 24] = (uint16_t)(hi[p] >> 16);
                GP_PUT(0) GP_PUT(1) GP_PUT(2)
#undef GP_PUT
            }
            lds_barrier();
            {   // dW2[16 w .., 16 ct ..] += g2^T h1 over the tile's 32 pairs
                uint4 ga[3];
#pragma unroll
                for (int p = 0; p < 3; p++) ga[p] = g2t[(p * 8 + w) * 64 + l];
#pragma unroll
                for (int ct = 0; ct < 8; ct++) {
                    uint4 b[3];
#pragma unroll
                    for (int p = 0; p < 3; p++) b[p] = h1t[(p * 8 + ct) * 64 + l];
                    dw2[ct] = sb_mma6(ga, b, dw2[ct]);
                }
            }
            uint4 w2p[4][3];
#pragma unroll
            for (int c = 0; c < 4; c++) sb_split8(w2t[c][0], w2t[c][1], w2p[c]);
#pragma unroll 1
            for (int s = 0; s < 2; s++) {               // g1 = (W2^T g2) [z1 > 0] of pair 16 s + n, units 16 w + 4 gq + q
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    uint4 b[3];
#pragma unroll
                    for (int p = 0; p < 3; p++) b[p] = g2i[((p * 4 + c) * 2 + s) * 64 + l];
                    acc = sb_mma6(w2p[c], b, acc);
                }
                const uint2 m = ((const uint2 *)h1i)[dhalf + s * 128];   // the leading pieces of h1: nonzero where z1 > 0
                const float g1[4] = {(m.x & 0xffffu) ? acc[0] : 0.f, (m.x >> 16) ? acc[1] : 0.f, (m.y & 0xffffu) ? acc[2] : 0.f, (m.y >> 16) ? acc[3] : 0.f};
                // g1^T over the wave's own g2T words (read into registers above): the A operand of dW1 += g1^T x
                uint32_t lo[3], hi[3];
                sb_split2(g1[0], g1[1], lo[0], lo[1], lo[2]);
                sb_split2(g1[2], g1[3], hi[0], hi[1], hi[2]);
                const int pp = 16 * s + n;
                uint16_t *const row = (uint16_t *)(g2t + w * 64 + (pp >> 3) * 16 + 4 * gq) + (pp & 7);
#define GP_PUT(p)                                                                                  \
                row[4096 * (p)] = (uint16_t)lo[p], row[4096 * (p) + 8] = (uint16_t)(lo[p] >> 16); \
                row[4096 * (p) + 16] = (uint16_t)hi[p], row[4096 * (p) + 24] = (uint16_t)(hi[p] >> 16);
                GP_PUT(0) GP_PUT(1) GP_PUT(2)
#undef GP_PUT
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (a wave's LDS operations complete in order: its own words, no barrier)
            {
                uint4 ga[3], b[3];
#pragma unroll
                for (int p = 0; p < 3; p++) { ga[p] = g2t[(p * 8 + w) * 64 + l]; b[p] = xti[p * 64 + l]; }
                dw1 = sb_mma6(ga, b, dw1);
            }
            lds_barrier();
        }
        lds_barrier();                                  // (the lists are free)
    }
#pragma unroll
    for (int ct = 0; ct < 8; ct++)
#pragma unroll
        for (int q = 0; q < 4; q++) blk[(16 * w + 4 * gq + q) * 128 + 16 * ct + n] = dw2[ct][q];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (n < 7) blk[128 * 128 + (16 * w + 4 * gq + q) * 7 + n] = dw1[q];
        const float v = gp_sum16(db2[q]);
        if (n == 0) blk[128 * 128 + 128 * 7 + 16 * w + 4 * gq + q] = v;
    }
}

// the partial blocks in order of workgroup -> dW2 [128][128], dW1 [128][7], db2 [128], db1 [128] = dW1's three one-hot columns
GP_KERNEL __launch_bounds__(256) void k_gnn_pair_reduce(const float *__restrict__ part, int G, float *__restrict__ dW1, float *__restrict__ db1,
                                                         float *__restrict__ dW2, float *__restrict__ db2) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= GP_BLOCK + 128) return;
    const bool bias1 = idx >= GP_BLOCK;                 // db1[k]: the three one-hot columns of dW1's row k, each added in order of workgroup
    const int at = bias1 ? 128 * 128 + (idx - GP_BLOCK) * 7 + 4 : idx;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int g = 0; g < G; g++) {
        const float *b = part + (size_t)g * GP_BLOCK + at;
        s0 += b[0];
        if (bias1) { s1 += b[1]; s2 += b[2]; }
    }
    if (bias1) db1[idx - GP_BLOCK] = (s0 + s1) + s2;
    else if (idx < 128 * 128) dW2[idx] = s0;
    else if (idx < 128 * 128 + 128 * 7) dW1[idx - 128 * 128] = s0;
    else db2[idx - 128 * 128 - 128 * 7] = s0;
}

inline int gp_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    return cus;
}
inline int gp_bwd_grid(int64_t R, int32_t P) {
    const int64_t n_seg = R * P;
    const int cap = gp_cus() < GP_MAX_GRID ? gp_cus() : GP_MAX_GRID;
    return n_seg < cap ? (int)n_seg : cap;
}

inline int launch_gnn_pair_fwd(const GpArgs &a, float *agg, hipStream_t st) {
    constexpr int lds = (GP_LISTS + 3 * 4 * 4 * 64) * 16;
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_gnn_pair_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    const int64_t n_seg = a.R * a.P, cap = 2 * (int64_t)gp_cus();   // (segments differ in length: two shares per CU even them out)
    hipLaunchKernelGGL(k_gnn_pair_fwd, dim3((unsigned)(n_seg < cap ? n_seg : cap)), dim3(512), lds, st, a, agg);
    return (int)hipGetLastError();
}

inline int launch_gnn_pair_bwd(const GpArgs &a, const float *d_agg, float *dW1, float *db1, float *dW2, float *db2, float *part, hipStream_t st) {
    constexpr int lds = (GP_LISTS + 256 + 4 * GP_BIMG + 3 * 64) * 16;
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_gnn_pair_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    const int G = gp_bwd_grid(a.R, a.P);
    hipLaunchKernelGGL(k_gnn_pair_bwd, dim3(G), dim3(512), lds, st, a, d_agg, part);
    hipLaunchKernelGGL(k_gnn_pair_reduce, dim3((GP_BLOCK + 128 + 255) / 256), dim3(256), 0, st, (const float *)part, G, dW1, db1, dW2, db2);
    return (int)hipGetLastError();
}
