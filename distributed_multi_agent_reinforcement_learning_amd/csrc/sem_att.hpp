// sem_att.hpp -- DHGN's semantic-level ATTENTION aggregator (`algo.semantic_level_aggregator: att`): the encoder tail with a
// softmax over the three relations between the AGG layer and the semantic layer, one launch forward and one backward (C ABI:
// include/mappo_ops.h dhgn_sem_att_*).  Ours: the reference sketched the branch and left it commented out.
#pragma once
#include <mutex>

#include "sb_common.hpp"
#include "sb_encoder_tail.hpp"
#include "sb_gemm.hpp"

// ---- emb_r = relu(W_agg m3[s, r] + b_agg), s_r = alpha . emb_r, g = 3 softmax(s), Y[s] = C[s] + sum over r of g_r Ws_r emb_r  (k_sem_att_fwd)
// The step structure is k_sb_encoder_tail's (csrc/sb_encoder_tail.hpp): persistent 512-thread workgroups, a tile of semantic rows,
// three STEPS (relations) per tile, wave w owning units 16 w .. 16 w + 15 of both layers, the W_agg pieces in a 96 KB LDS image, the
// Ws pieces resident in registers, the embedding handed from the AGG accumulators to the semantic product as split pieces in LDS.
// What the softmax changes: no gated product is final before all three scores are known, so every relation keeps a semantic
// accumulator of its own (acc_s[r]) and the gates meet them in the epilogue:
//   AGG       as k_sb_encoder_tail; + bias, max(., 0)
//   score     while the result is in registers: the lane's four units times its four alpha (fp32 FMAs), folded over the four column
//             groups of the wave (two __shfl_xor), one float per (relation, row, wave) into a 1.5 KB LDS exchange
//   hand-over, barrier, semantic (acc_s[r] from zero: Ws chunks 4 r .. 4 r + 3 x the embedding image), staging, barrier: as the mean tail
//   epilogue  behind step 2: every lane adds the eight waves' partial scores of its rows in wave order (the same sum in every wave),
//             M = max, e_r = exp(s_r - M), g_r = 3 e_r / (e_0 + e_1 + e_2), Y = fma(g_2, acc_2, fma(g_1, acc_1, g_0 acc_0)) + C
// alpha = 0: every score is 0, e_r = 1, g_r = 3 / 3 = 1 exactly.
// The tile is SA_ROWS = 16 rows, half the mean tail's: three accumulator pairs beside the 144 registers of Ws pieces did not fit in 256
// registers at 32 rows (scratch), one row half per tile does -- the B operands of the second half go, and each accumulator
// is four registers.  The price: the W_agg image is read back from LDS once per 16 rows instead of once per 32.
// SAVE (the update): emb, its sign bits (sb_gemm_signs' layout, as k_sb_encoder_tail<true>) and the gates (Rs, 3) are stored.
constexpr int SA_NH = 1;                        // row halves (16 rows each) per tile
constexpr int SA_ROWS = 16 * SA_NH;
constexpr int SA_IMG = 3 * 4 * SA_NH * 64;      // uint4 per operand image: [piece][chunk][row half][lane]
constexpr int SA_SC = 3 * SA_ROWS * 8;          // floats of the score exchange: [relation][row][wave]
constexpr int SA_LDS = (SBE_WIMG + 2 * SA_IMG) * 16 + SA_SC * 4;

// the eight waves' partials of (relation r, row) in wave order
__device__ __forceinline__ float sa_fold8(const float *sc, int r, int row) {
    const float4 a = *(const float4 *)(sc + (r * SA_ROWS + row) * 8), b = *(const float4 *)(sc + (r * SA_ROWS + row) * 8 + 4);
    return ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
}
// a lane's value summed over the four column groups gq of its wave (every lane gets the sum)
__device__ __forceinline__ float sa_fold_gq(float v) {
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

template <bool SAVE>
__global__ __launch_bounds__(512) void k_sem_att_fwd(int64_t Rs, const float *__restrict__ X, int64_t ldx, const float *__restrict__ Wa,
                                                     const float *__restrict__ ba, const float *__restrict__ al, const float *__restrict__ Ws,
                                                     int64_t ldw, const float *C, int64_t ldc, float *Y, int64_t ldy, float *__restrict__ emb,
                                                     int64_t lde, uint8_t *__restrict__ ebits, int64_t ldb, float *__restrict__ gates) {
    extern __shared__ uint4 sa_lds[];                   // [AGG weight image | m3 image | embedding image | score exchange]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 15, gq = l >> 4;
    uint4 *const wimg = sa_lds + w * (4 * 3 * 64) + l, *const mimg = sa_lds + SBE_WIMG, *const eimg = mimg + SA_IMG;
    float *const sc = (float *)(eimg + SA_IMG);
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
    const float4 b4 = *(const float4 *)(ba + 16 * w + 4 * gq), al4 = *(const float4 *)(al + 16 * w + 4 * gq);
    const int64_t n_t = (Rs + SA_ROWS - 1) / SA_ROWS, G = gridDim.x;
    float4 pf[2];
    // wave w < 4 SA_NH stages (chunk w / SA_NH, half w % SA_NH) of a step's image: lane (gq, j) loads inputs 32 c + 8 gq .. of row j of the half
    const bool stager = w < 4 * SA_NH;
    auto fetch = [&](int64_t t, int r) {
        const int64_t row = t * SA_ROWS + (w % SA_NH) * 16 + i;
        pf[0] = pf[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (stager && row < Rs) {
            const float *src = X + row * ldx + 128 * r + 32 * (w / SA_NH) + 8 * gq;
            pf[0] = *(const float4 *)src;
            pf[1] = *(const float4 *)(src + 4);
        }
    };
    auto stage = [&]() {
        if (!stager) return;
        uint4 p_[3];
        sb_split8(pf[0], pf[1], p_);
#pragma unroll
        for (int p = 0; p < 3; p++) mimg[(p * 4 * SA_NH + w) * 64 + l] = p_[p];
    };
    // this lane's half words of the embedding image: chunk w / 2, octet 2 (w & 1) + gq / 2, column i, half gq & 1 (+ 128 per row half)
    uint2 *const edst = (uint2 *)eimg + (((w >> 1) * SA_NH) * 64 + ((2 * (w & 1) + (gq >> 1)) << 4) + i) * 2 + (gq & 1);
    int64_t t = blockIdx.x;
    if (t < n_t) { fetch(t, 0); stage(); fetch(t, 1); }
    lds_barrier();
    for (; t < n_t; t += G) {
        const bool more = t + G < n_t;
        f32x4 acc_s[3][SA_NH];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            f32x4 acc_a[SA_NH];
#pragma unroll
            for (int h = 0; h < SA_NH; h++) acc_a[h] = acc_s[r][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                uint4 a_[3], b_[SA_NH][3];
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    a_[p] = wimg[(c * 3 + p) * 64];
#pragma unroll
                    for (int h = 0; h < SA_NH; h++) b_[h][p] = mimg[(p * 4 * SA_NH + SA_NH * c + h) * 64 + l];
                }
#pragma unroll
                for (int h = 0; h < SA_NH; h++) acc_a[h] = sb_mma6(a_, b_[h], acc_a[h]);
            }
            // D tile: lane (i, gq), register q -> unit 16 w + 4 gq + q of row i of the half
#pragma unroll
            for (int h = 0; h < SA_NH; h++) {
                float4 v = make_float4(acc_a[h][0] + b4.x, acc_a[h][1] + b4.y, acc_a[h][2] + b4.z, acc_a[h][3] + b4.w);
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                const float sp = sa_fold_gq(fmaf(al4.w, v.w, fmaf(al4.z, v.z, fmaf(al4.y, v.y, al4.x * v.x))));
                if (gq == 0) sc[(r * SA_ROWS + h * 16 + i) * 8 + w] = sp;
                if constexpr (SAVE) {   // lanes (i, gq) and (i, gq ^ 1) hold the two nibbles of a byte (as k_sb_encoder_tail<true>)
                    const int64_t row = t * SA_ROWS + h * 16 + i;
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
                for (int p = 0; p < 3; p++) edst[p * 4 * SA_NH * 64 * 2 + h * 128] = make_uint2(lo[p], hi[p]);
            }
            lds_barrier();   // (the embedding image and this step's scores are complete; every wave is done reading the m3 image)
            auto next_step = [&]() {   // step n + 1 -> the m3 image, step n + 2 requested
                if (r < 2 || more) stage();
                if (r == 0) fetch(t, 2);
                else if (more) fetch(t + G, r - 1);
            };
            if (w < 4) next_step();
#pragma unroll
            for (int c = 0; c < 4; c++) {
                uint4 b_[SA_NH][3];
#pragma unroll
                for (int p = 0; p < 3; p++) {
#pragma unroll
                    for (int h = 0; h < SA_NH; h++) b_[h][p] = eimg[(p * 4 * SA_NH + SA_NH * c + h) * 64 + l];
                }
#pragma unroll
                for (int h = 0; h < SA_NH; h++) acc_s[r][h] = sb_mma6(ws[4 * r + c], b_[h], acc_s[r][h]);
            }
            if (w >= 4) next_step();
            if (r < 2) lds_barrier();   // (the m3 image is complete; every wave is done reading the embedding image)
        }
#pragma unroll
        for (int h = 0; h < SA_NH; h++) {
            const int64_t row = t * SA_ROWS + h * 16 + i;
            const float s0 = sa_fold8(sc, 0, h * 16 + i), s1 = sa_fold8(sc, 1, h * 16 + i), s2 = sa_fold8(sc, 2, h * 16 + i);
            const float M = fmaxf(fmaxf(s0, s1), s2);
            const float e0 = expf(s0 - M), e1 = expf(s1 - M), e2 = expf(s2 - M), den = (e0 + e1) + e2;
            const float g0 = 3.f * e0 / den, g1 = 3.f * e1 / den, g2 = 3.f * e2 / den;
            if (row < Rs) {
                const float4 a4 = *(const float4 *)(C + row * ldc + 16 * w + 4 * gq);
                float4 v;
                v.x = fmaf(g2, acc_s[2][h][0], fmaf(g1, acc_s[1][h][0], g0 * acc_s[0][h][0])) + a4.x;
                v.y = fmaf(g2, acc_s[2][h][1], fmaf(g1, acc_s[1][h][1], g0 * acc_s[0][h][1])) + a4.y;
                v.z = fmaf(g2, acc_s[2][h][2], fmaf(g1, acc_s[1][h][2], g0 * acc_s[0][h][2])) + a4.z;
                v.w = fmaf(g2, acc_s[2][h][3], fmaf(g1, acc_s[1][h][3], g0 * acc_s[0][h][3])) + a4.w;
                *(float4 *)(Y + row * ldy + 16 * w + 4 * gq) = v;
                if constexpr (SAVE) {
                    if (w == 0 && gq == 0) { gates[row * 3] = g0; gates[row * 3 + 1] = g1; gates[row * 3 + 2] = g2; }
                }
            }
        }
        lds_barrier();   // (every wave is done reading the scores and the embedding image)
    }
}

template <bool SAVE>
int launch_sem_att_fwd(int64_t Rs, const float *X, int64_t ldx, const float *Wa, const float *ba, const float *al, const float *Ws, int64_t ldw,
                       const float *C, int64_t ldc, float *Y, int64_t ldy, hipStream_t st, float *emb = nullptr, int64_t lde = 0,
                       uint8_t *ebits = nullptr, int64_t ldb = 0, float *gates = nullptr) {
    static std::once_flag once;   // the evaluator's thread may launch concurrently with the trainer's
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_sem_att_fwd<SAVE>, hipFuncAttributeMaxDynamicSharedMemorySize, SA_LDS); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    const int64_t n_t = (Rs + SA_ROWS - 1) / SA_ROWS;
    const int grid = n_t < (int64_t)cus ? (int)n_t : cus;
    hipLaunchKernelGGL(k_sem_att_fwd<SAVE>, dim3(grid), dim3(512), SA_LDS, st, Rs, X, ldx, Wa, ba, al, Ws, ldw, C, ldc, Y, ldy, emb, lde, ebits, ldb,
                       gates);
    return (int)hipGetLastError();
}

// ---- the backward: for g = d Y[s], t_r = Ws_r^T g, c_r = t_r . emb_r, ds_r = g_r (c_r - sum_q (g_q / 3) c_q),
//      ga_r = [emb_r > 0] (g_r t_r + ds_r alpha), d_m3[s, r] = W_agg^T ga_r, es_r = g_r emb_r; column sums of ga, d_alpha = sum ds_r emb_r
// k_sb_encoder_tail_bwd's structure (csrc/sb_encoder_tail_bwd.hpp: the three blocks of Ws^T resident as pieces, the W_agg^T pieces in
// a 96 KB LDS image, the g rows of a tile staged once, ga handed to the AGG^T product in LDS), with the softmax's backward between
// the two products.  c_r couples the three relations, so a tile first takes all three t_r (one accumulator each):
//   semantic^T  t_r = Ws_r^T x the g image, r = 0, 1, 2
//   row dots    the lane's four of t_r times its four of the saved emb_r, folded over the wave's column groups, one float per
//               (relation, row, wave) into the 1.5 KB LDS exchange; barrier; every lane adds the eight partials of its row in wave order
//   per r       d emb = fma(ds_r, alpha, g_r t_r), masked by emb_r > 0 (the values are at hand: emb is read again for d_alpha and es, so
//               the sign bits the forward saves are not read here), + into the column sums, ga and es stored, the four split into the
//               ga image; barrier; AGG^T = W_agg^T x the ga image, + 0.f, d_m3 stored; barrier
// d_alpha and the column sums leave as one row of partial sums per workgroup, added in workgroup order by k_sb_colsum_reduce: no atomics.
// Rows past Rs carry zero gates and a zero emb: they add nothing and store nothing.
__global__ __launch_bounds__(512) void k_sem_att_bwd(int64_t Rs, const float *__restrict__ G, int64_t ldg, const float *__restrict__ Ws, int64_t ldw,
                                                     const float *__restrict__ Wa, const float *__restrict__ al, const float *__restrict__ emb,
                                                     int64_t lde, const float *__restrict__ gates, float *__restrict__ GA, int64_t ldga,
                                                     float *__restrict__ ES, int64_t ldes, float *__restrict__ DM, int64_t ldd,
                                                     float *__restrict__ cs_part, float *__restrict__ da_part) {
    extern __shared__ uint4 sa_lds[];                   // [W_agg^T image | g image | ga image | row-dot exchange | running sums]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 15, gq = l >> 4;
    uint4 *const wimg = sa_lds + w * (4 * 3 * 64) + l, *const gimg = sa_lds + SBE_WIMG, *const aimg = gimg + SA_IMG;
    float *const cx = (float *)(aimg + SA_IMG);
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
    const float4 al4 = *(const float4 *)(al + 16 * w + 4 * gq);
    const int64_t n_t = (Rs + SA_ROWS - 1) / SA_ROWS, G_ = gridDim.x;
    float4 pf[2];
    const bool stager = w < 4 * SA_NH;   // wave w stages (chunk w / SA_NH, half w % SA_NH) of a tile's g image
    auto fetch = [&](int64_t t) {
        const int64_t row = t * SA_ROWS + (w % SA_NH) * 16 + i;
        pf[0] = pf[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (stager && row < Rs) {
            const float *src = G + row * ldg + 32 * (w / SA_NH) + 8 * gq;
            pf[0] = *(const float4 *)src;
            pf[1] = *(const float4 *)(src + 4);
        }
    };
    auto stage = [&]() {
        if (!stager) return;
        uint4 p_[3];
        sb_split8(pf[0], pf[1], p_);
#pragma unroll
        for (int p = 0; p < 3; p++) gimg[(p * 4 * SA_NH + w) * 64 + l] = p_[p];
    };
    uint2 *const adst = (uint2 *)aimg + (((w >> 1) * SA_NH) * 64 + ((2 * (w & 1) + (gq >> 1)) << 4) + i) * 2 + (gq & 1);
    // the lane's running sums (column sums of ga per relation, d_alpha) live in LDS slots of its own, [slot][thread]: beside the three
    // accumulators they do not fit in registers; lane-private, so no barrier guards them
    float4 *const lacc = (float4 *)(cx + SA_SC) + tid;
#pragma unroll
    for (int k = 0; k < 4; k++) lacc[k * 512] = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t t = blockIdx.x;
    if (t < n_t) { fetch(t); stage(); }
    lds_barrier();
    for (; t < n_t; t += G_) {
        const bool more = t + G_ < n_t;
        f32x4 tr[3][SA_NH];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int h = 0; h < SA_NH; h++) tr[r][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                uint4 b_[SA_NH][3];
#pragma unroll
                for (int p = 0; p < 3; p++) {
#pragma unroll
                    for (int h = 0; h < SA_NH; h++) b_[h][p] = gimg[(p * 4 * SA_NH + SA_NH * c + h) * 64 + l];
                }
#pragma unroll
                for (int h = 0; h < SA_NH; h++) tr[r][h] = sb_mma6(ws[4 * r + c], b_[h], tr[r][h]);
            }
            // D tile: lane (i, gq), register q -> unit 16 w + 4 gq + q of relation r of row i of the half
#pragma unroll
            for (int h = 0; h < SA_NH; h++) {
                const int64_t row = t * SA_ROWS + h * 16 + i;
                const float4 e4 = row < Rs ? *(const float4 *)(emb + row * lde + 128 * r + 16 * w + 4 * gq) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float cp = sa_fold_gq(fmaf(tr[r][h][3], e4.w, fmaf(tr[r][h][2], e4.z, fmaf(tr[r][h][1], e4.y, tr[r][h][0] * e4.x))));
                if (gq == 0) cx[(r * SA_ROWS + h * 16 + i) * 8 + w] = cp;
            }
        }
        lds_barrier();   // (the row dots are complete)
        float gt[3][SA_NH], ds[3][SA_NH];
#pragma unroll
        for (int h = 0; h < SA_NH; h++) {
            const int64_t row = t * SA_ROWS + h * 16 + i;
            const float c0 = sa_fold8(cx, 0, h * 16 + i), c1 = sa_fold8(cx, 1, h * 16 + i), c2 = sa_fold8(cx, 2, h * 16 + i);
#pragma unroll
            for (int r = 0; r < 3; r++) gt[r][h] = row < Rs ? gates[row * 3 + r] : 0.f;
            // beta_q = g_q / 3 by division: a gate of exactly 3 (the other scores far below) gives beta = 1, cbar = c and ds = 0 exactly,
            // where a multiplication by 1 / 3 leaves a rounding of c that the gate then triples
            const float cbar = fmaf(gt[2][h] / 3.f, c2, fmaf(gt[1][h] / 3.f, c1, (gt[0][h] / 3.f) * c0));
            ds[0][h] = gt[0][h] * (c0 - cbar); ds[1][h] = gt[1][h] * (c1 - cbar); ds[2][h] = gt[2][h] * (c2 - cbar);
        }
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int h = 0; h < SA_NH; h++) {
                const int64_t row = t * SA_ROWS + h * 16 + i;
                const float g_ = gt[r][h], d_ = ds[r][h];
                float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < Rs) e4 = *(const float4 *)(emb + row * lde + 128 * r + 16 * w + 4 * gq);
                float4 v = make_float4(fmaf(d_, al4.x, g_ * tr[r][h][0]), fmaf(d_, al4.y, g_ * tr[r][h][1]), fmaf(d_, al4.z, g_ * tr[r][h][2]),
                                       fmaf(d_, al4.w, g_ * tr[r][h][3]));
                v.x = e4.x > 0.f ? v.x : 0.f; v.y = e4.y > 0.f ? v.y : 0.f; v.z = e4.z > 0.f ? v.z : 0.f; v.w = e4.w > 0.f ? v.w : 0.f;
                if (row < Rs) {
                    float4 cs = lacc[r * 512], da = lacc[3 * 512];
                    cs.x += v.x; cs.y += v.y; cs.z += v.z; cs.w += v.w;
                    da.x = fmaf(d_, e4.x, da.x); da.y = fmaf(d_, e4.y, da.y); da.z = fmaf(d_, e4.z, da.z); da.w = fmaf(d_, e4.w, da.w);
                    lacc[r * 512] = cs; lacc[3 * 512] = da;
                    *(float4 *)(GA + row * ldga + 128 * r + 16 * w + 4 * gq) = v;
                    *(float4 *)(ES + row * ldes + 128 * r + 16 * w + 4 * gq) = make_float4(g_ * e4.x, g_ * e4.y, g_ * e4.z, g_ * e4.w);
                }
                uint32_t lo[3], hi[3];
                sb_split2(v.x, v.y, lo[0], lo[1], lo[2]);
                sb_split2(v.z, v.w, hi[0], hi[1], hi[2]);
#pragma unroll
                for (int p = 0; p < 3; p++) adst[p * 4 * SA_NH * 64 * 2 + h * 128] = make_uint2(lo[p], hi[p]);
            }
            lds_barrier();   // (the ga image is complete; after step 2 every wave is also done with the g image and the row dots)
            if (r == 2 && more) fetch(t + G_);   // the next tile's g rows, requested where the fewest registers are live: under the last AGG^T product
            f32x4 acc[SA_NH];
#pragma unroll
            for (int h = 0; h < SA_NH; h++) acc[h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                uint4 a_[3], b_[SA_NH][3];
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    a_[p] = wimg[(c * 3 + p) * 64];
#pragma unroll
                    for (int h = 0; h < SA_NH; h++) b_[h][p] = aimg[(p * 4 * SA_NH + SA_NH * c + h) * 64 + l];
                }
#pragma unroll
                for (int h = 0; h < SA_NH; h++) acc[h] = sb_mma6(a_, b_[h], acc[h]);
            }
            if (r == 2 && more) stage();         // (every wave is behind step 2's hand-over barrier: done with the g image)
#pragma unroll
            for (int h = 0; h < SA_NH; h++) {
                const int64_t row = t * SA_ROWS + h * 16 + i;
                if (row < Rs)   // (the null bias: -0 -> +0)
                    *(float4 *)(DM + row * ldd + 128 * r + 16 * w + 4 * gq) = make_float4(acc[h][0] + 0.f, acc[h][1] + 0.f, acc[h][2] + 0.f, acc[h][3] + 0.f);
            }
            lds_barrier();   // (every wave is done reading the ga image; after step 2 the g image is complete)
        }
    }
    // this workgroup's partial sums: the 16 row lanes of a column group fold, lane i = 0 stores
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float4 s = lacc[k * 512];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            s.x += __shfl_xor(s.x, m); s.y += __shfl_xor(s.y, m); s.z += __shfl_xor(s.z, m); s.w += __shfl_xor(s.w, m);
        }
        if (i == 0) *(float4 *)((k < 3 ? cs_part + (size_t)blockIdx.x * 384 + 128 * k : da_part + (size_t)blockIdx.x * 128) + 16 * w + 4 * gq) = s;
    }
}

constexpr int SA_LDS_BWD = SA_LDS + 4 * 512 * 16;   // + the lanes' running sums
constexpr int SA_MAX_GRID = 1024;   // rows of partial sums the workspace holds (one workgroup per CU)

// workspace: [SA_MAX_GRID][384] column-sum partials, then [SA_MAX_GRID][128] d_alpha partials
inline int launch_sem_att_bwd(int64_t Rs, const float *G, int64_t ldg, const float *Ws, int64_t ldw, const float *Wa, const float *al, const float *emb,
                              int64_t lde, const float *gates, float *GA, int64_t ldga, float *ES, int64_t ldes, float *DM, int64_t ldd, float *colsum,
                              float *d_alpha, float *workspace, int cus, hipStream_t st) {
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_sem_att_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, SA_LDS_BWD); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    const int64_t n_t = (Rs + SA_ROWS - 1) / SA_ROWS;
    const int grid = n_t < (int64_t)cus ? (int)n_t : cus;
    float *cs_part = workspace, *da_part = workspace + (size_t)SA_MAX_GRID * 384;
    hipLaunchKernelGGL(k_sem_att_bwd, dim3(grid), dim3(512), SA_LDS_BWD, st, Rs, G, ldg, Ws, ldw, Wa, al, emb, lde, gates, GA, ldga, ES, ldes, DM, ldd, cs_part,
                       da_part);
    hipLaunchKernelGGL(k_sb_colsum_reduce, dim3(3), dim3(128), 0, st, grid, 384, cs_part, colsum);
    hipLaunchKernelGGL(k_sb_colsum_reduce, dim3(1), dim3(128), 0, st, grid, 128, da_part, d_alpha);
    return (int)hipGetLastError();
}
