// att_agg.hpp -- DHGN's vertex-level ATTENTION aggregator (`algo.vertex_level_aggregator: att`): the relation message and a softmax over
// the listed neighbours as one launch each way (C ABI: include/mappo_ops.h dhgn_att_agg3_fwd / dhgn_att_agg_bwd).
//
//   x_ij = p_i - q_j  (din 8: [p_i - q_j, p_i - e])        m_ij = relu(W x_ij + b)        s_ij = alpha . m_ij
//   listed j: a_ij != 0      M_i = max over listed j of s_ij      u_ij = a_ij exp(s_ij - M_i)
//   out_i = sum_j u_ij m_ij / sum_j |u_ij|                 nothing listed -> exact zeros;  alpha = 0 -> the mean path's numbers
//
// A SEGMENT is one (relation, row, pursuer).  ONE WAVE owns a segment from its list to its output row: four waves of a persistent
// 256-thread workgroup stride over the segments (relation-major, so every wave walks all relations), everything a segment needs sits
// in that wave's own LDS region, and the only workgroup barrier is the one behind the table staged at the start.  Per segment:
//   list     the lanes compact the j with a_ij != 0, in order of j (ballot + popcount), into the wave's LDS: x = p_i - q_j and a_ij.
//            The p_i - e half of the defender relation does not depend on j: the unit lanes fold it into a per-segment bias
//            tb = b + W[:, 4:8] (p_i - e) once, so a pair costs four fused multiply-adds a unit in both passes.
//   pass A   lanes = listed pairs (chunks of 64, x in registers): a lane walks the 128 units with W[:, :4], tb and alpha broadcast from
//            LDS and accumulates s_ij on its own; s is parked in the list, then ONE max and ONE sum across lanes (xor butterflies: the
//            same bits in every lane), and u_ij overwrites a_ij.
//   pass B   lanes = units (2 l, 2 l + 1; their rows of W, b in registers while the relation lasts): the lane walks the list with x_j
//            and u_j broadcast from LDS, evaluates m again and accumulates u_j m; one 512-byte row per wave is stored.
// Both passes evaluate z through aa_z on the same bits (W from the table / registers, tb from the unit lanes), so m and the ReLU
// decision agree; no per-pair cross-lane reduction exists.  Nothing per pair reaches HBM, no atomics; a segment's bits depend on its
// own inputs only.
//
// The backward saves nothing: pass A also forms c_j = g . m_j beside s_j, then w_j = u_j / sum |u|, g . out_i = sum_j w_j c_j and
// ds_j = w_j c_j - |w_j| (g . out_i); pass B accumulates dW, db, d_alpha of the lane's two units in registers over all the wave's
// segments (dm_j = [z_j > 0] (w_j g + ds_j alpha)).  The four waves are added in order through LDS into one partial block per
// workgroup; k_att_agg_reduce adds the blocks in order of workgroup.
#pragma once
#include <math.h>
#include <mutex>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mappo_ops.h"

constexpr int AA_E = 128;                     // the only width
constexpr int AA_KMAX = 1024, AA_PMAX = 64;
constexpr int AA_WAVES = 4;                   // segments in flight per workgroup
constexpr int AA_MAX_GRID = 1024;             // workgroups of the backward = partial blocks in its workspace
constexpr int AA_TABLE = 3 * 128 * 5;         // floats: W[:, :4] as float4 [3][128] | alpha [3][128]

// The packed fp32 VALU forms stay out of these kernels: a per-kernel target feature, device pass only.
#if defined(__HIP_DEVICE_COMPILE__)
#define AA_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define AA_KERNEL __global__
#endif

struct AaArgs {
    mo_att_rel rel[3];
    int32_t n_rel, R, P, kc;                  // kc: list capacity of a wave (the largest K, a multiple of 4)
    int64_t p_rs;
    const float *p;
};

__device__ __forceinline__ void aa_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }   // a wave's LDS operations complete in order
// one pre-activation: the SAME expression in both passes, forward and backward
__device__ __forceinline__ float aa_z(const float4 &w, float tb, const float4 &x) {
    return fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, fmaf(w.x, x.x, tb))));
}
__device__ __forceinline__ float aa_wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float aa_wave_sum(float v) {   // a + b == b + a: every lane ends with the same bits
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <class Rel>   // mo_att_rel, or mo_msg_rel (csrc/pool_agg.hpp)
__device__ __forceinline__ float aa_adj(const Rel &m, int64_t r, int i, int j, int kv) {
    if (m.adj_mode == MO_ADJ_TENSOR) return ((const float *)m.adj)[r * m.adj_rs + (int64_t)i * m.K + j];
    if (m.adj_mode == MO_ADJ_BITS)
        return (float)((((const uint32_t *)m.adj)[r * m.adj_rs + (int64_t)i * MO_ADJ_ROW_WORDS(m.K) + (j >> 5)] >> (j & 31)) & 1u);
    return j < kv ? 1.f : 0.f;                // MO_ADJ_ONES (kv = K), MO_ADJ_VALID
}

// the table both kernels stage once: W[:, :4] and alpha of every relation, then the workgroup's only barrier before the segments
__device__ __forceinline__ void aa_stage(const AaArgs &a, float4 *tW, float *tA) {
    for (int idx = threadIdx.x; idx < a.n_rel * 128; idx += blockDim.x) {
        const mo_att_rel &m = a.rel[idx >> 7];
        tW[idx] = *(const float4 *)(m.W + (idx & 127) * m.din);
        tA[idx] = m.alpha[idx & 127];
    }
    __syncthreads();
}

// the pair list of segment (r, i) in order of j -> count.  pi = p[r, i].  Every lane of the wave calls it.
__device__ __forceinline__ int aa_build_list(const mo_att_rel &m, const float *__restrict__ p, int64_t p_rs, int64_t r, int i, int l, float4 *lx,
                                             float *la, float4 &pi) {
    pi = *(const float4 *)(p + r * p_rs + 4 * i);
    const int K = m.K;
    const int64_t qr = r / m.q_div;
    const int kv = m.adj_mode == MO_ADJ_VALID ? m.kvalid[qr] : K;
    const float *qrow = m.q + qr * m.q_rs;
    int cnt = 0;
    for (int j0 = 0; j0 < K; j0 += 64) {
        const int j = j0 + l;
        const float av = j < K ? aa_adj(m, r, i, j, kv) : 0.f;
        const bool nz = av != 0.f;
        const unsigned long long bal = __ballot(nz);
        if (nz) {
            const int pos = cnt + __popcll(bal & ((1ull << l) - 1ull));
            const float4 qj = *(const float4 *)(qrow + 4 * j);
            lx[pos] = make_float4(pi.x - qj.x, pi.y - qj.y, pi.z - qj.z, pi.w - qj.w);
            la[pos] = av;
        }
        cnt += __popcll(bal);
    }
    return cnt;
}

// rows 2 l and 2 l + 1 of a relation's layer, held by the unit lanes while the relation lasts
struct AaUnit {
    float4 w0, w1, we0, we1;
    float b0, b1, al0, al1;
};
__device__ __forceinline__ AaUnit aa_load_unit(const mo_att_rel &m, int l) {
    AaUnit u;
    const float *r0 = m.W + (2 * l) * m.din, *r1 = r0 + m.din;
    u.w0 = *(const float4 *)r0;
    u.w1 = *(const float4 *)r1;
    u.we0 = u.we1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m.din == 8) {
        u.we0 = *(const float4 *)(r0 + 4);
        u.we1 = *(const float4 *)(r1 + 4);
    }
    u.b0 = m.b[2 * l];
    u.b1 = m.b[2 * l + 1];
    u.al0 = m.alpha[2 * l];
    u.al1 = m.alpha[2 * l + 1];
    return u;
}
// the per-segment bias of the lane's two units -> the wave's table (read by pass A) and registers (pass B): the same bits
__device__ __forceinline__ void aa_segment_bias(const mo_att_rel &m, const AaUnit &u, int64_t r, const float4 &pi, int l, float *tbs, float4 &pe,
                                                float &tb0, float &tb1) {
    tb0 = u.b0;
    tb1 = u.b1;
    pe = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m.din == 8) {
        const float4 e4 = *(const float4 *)(m.e + r * m.e_rs);
        pe = make_float4(pi.x - e4.x, pi.y - e4.y, pi.z - e4.z, pi.w - e4.w);
        tb0 = aa_z(u.we0, u.b0, pe);
        tb1 = aa_z(u.we1, u.b1, pe);
    }
    *(float2 *)(tbs + 2 * l) = make_float2(tb0, tb1);
}

AA_KERNEL __launch_bounds__(256) void k_att_agg_fwd(AaArgs a, float *__restrict__ out, int64_t out_stride) {
    extern __shared__ float4 aa_lds[];        // [table | per wave: x [kc] float4 | a -> u [kc] | s [kc] | tb [128]]
    float4 *const tW = aa_lds;
    float *const tA = (float *)(aa_lds + 3 * 128);
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, kc = a.kc;
    float *const priv = (float *)aa_lds + AA_TABLE + w * (6 * kc + 128);
    float4 *const lx = (float4 *)priv;
    float *const la = priv + 4 * kc, *const ls = la + kc, *const tbs = ls + kc;
    aa_stage(a, tW, tA);
    const int64_t RP = (int64_t)a.R * a.P, n_seg = RP * a.n_rel;
    int cur = -1;
    AaUnit un;
    for (int64_t seg = (int64_t)blockIdx.x * AA_WAVES + w; seg < n_seg; seg += (int64_t)gridDim.x * AA_WAVES) {
        const int rel = (int)(seg / RP);
        const int64_t ri = seg - rel * RP, r = ri / a.P;
        const int i = (int)(ri - r * a.P);
        const mo_att_rel &m = a.rel[rel];
        if (rel != cur) {
            un = aa_load_unit(m, l);
            cur = rel;
        }
        float4 pi, pe;
        const int cnt = aa_build_list(m, a.p, a.p_rs, r, i, l, lx, la, pi);
        float *const o = out + ri * out_stride + rel * AA_E + 2 * l;
        if (cnt == 0) {                       // (wave-uniform) nothing listed: exact zeros
            *(float2 *)o = make_float2(0.f, 0.f);
            continue;
        }
        float tb0, tb1;
        aa_segment_bias(m, un, r, pi, l, tbs, pe, tb0, tb1);
        aa_wave_sync();
        const float4 *const rW = tW + rel * 128;
        const float *const rA = tA + rel * 128;
        // pass A: lanes = pairs
        float mx = -INFINITY;
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            const int j = j0 + l;
            if (j < cnt) {
                const float4 x = lx[j];
                float s = 0.f;
#pragma unroll 8
                for (int u = 0; u < AA_E; u++) s = fmaf(rA[u], fmaxf(aa_z(rW[u], tbs[u], x), 0.f), s);
                ls[j] = s;
                mx = fmaxf(mx, s);
            }
        }
        mx = aa_wave_max(mx);
        float sum = 0.f;
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            const int j = j0 + l;
            if (j < cnt) {
                const float u = la[j] * expf(ls[j] - mx);
                la[j] = u;
                sum += fabsf(u);
            }
        }
        sum = aa_wave_sum(sum);
        aa_wave_sync();
        // pass B: lanes = units
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 4
        for (int j = 0; j < cnt; j++) {
            const float4 x = lx[j];
            const float u = la[j];
            acc0 = fmaf(u, fmaxf(aa_z(un.w0, tb0, x), 0.f), acc0);
            acc1 = fmaf(u, fmaxf(aa_z(un.w1, tb1, x), 0.f), acc1);
        }
        *(float2 *)o = make_float2(acc0 / sum, acc1 / sum);
        aa_wave_sync();                       // (the list is free)
    }
}

// one relation (a.n_rel == 1).  part: [gridDim.x][128 (din + 2)] floats, a block = dW [128][din] | db [128] | d_alpha [128]
AA_KERNEL __launch_bounds__(256) void k_att_agg_bwd(AaArgs a, const float *__restrict__ gout, int64_t g_stride, float *__restrict__ part) {
    extern __shared__ float4 aa_lds[];        // [table | per wave: x [kc] float4 | a -> w [kc] | s -> ds [kc] | c [kc] | tb [128] | g [128]]
    float4 *const tW = aa_lds;
    float *const tA = (float *)(aa_lds + 3 * 128);
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, kc = a.kc;
    float *const priv = (float *)aa_lds + AA_TABLE + w * (7 * kc + 256);
    float4 *const lx = (float4 *)priv;
    float *const la = priv + 4 * kc, *const ls = la + kc, *const lc = ls + kc, *const tbs = lc + kc, *const gs = tbs + 128;
    aa_stage(a, tW, tA);
    const mo_att_rel &m = a.rel[0];
    const int din = m.din;
    const AaUnit un = aa_load_unit(m, l);
    float4 dw0 = make_float4(0.f, 0.f, 0.f, 0.f), dw1 = dw0, dwe0 = dw0, dwe1 = dw0;
    float db0 = 0.f, db1 = 0.f, da0 = 0.f, da1 = 0.f;
    const int64_t n_seg = (int64_t)a.R * a.P;
    for (int64_t ri = (int64_t)blockIdx.x * AA_WAVES + w; ri < n_seg; ri += (int64_t)gridDim.x * AA_WAVES) {
        const int64_t r = ri / a.P;
        const int i = (int)(ri - r * a.P);
        float4 pi, pe;
        const int cnt = aa_build_list(m, a.p, a.p_rs, r, i, l, lx, la, pi);
        if (cnt == 0) continue;               // (wave-uniform) no pair, no gradient
        float tb0, tb1;
        aa_segment_bias(m, un, r, pi, l, tbs, pe, tb0, tb1);
        const float2 g2 = *(const float2 *)(gout + ri * g_stride + 2 * l);
        *(float2 *)(gs + 2 * l) = g2;
        aa_wave_sync();
        // pass A: s_j and c_j = g . m_j side by side
        float mx = -INFINITY;
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            const int j = j0 + l;
            if (j < cnt) {
                const float4 x = lx[j];
                float s = 0.f, c = 0.f;
#pragma unroll 8
                for (int u = 0; u < AA_E; u++) {
                    const float mv = fmaxf(aa_z(tW[u], tbs[u], x), 0.f);
                    s = fmaf(tA[u], mv, s);
                    c = fmaf(gs[u], mv, c);
                }
                ls[j] = s;
                lc[j] = c;
                mx = fmaxf(mx, s);
            }
        }
        mx = aa_wave_max(mx);
        float sum = 0.f;
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            const int j = j0 + l;
            if (j < cnt) {
                const float u = la[j] * expf(ls[j] - mx);
                la[j] = u;
                sum += fabsf(u);
            }
        }
        sum = aa_wave_sum(sum);
        float gd = 0.f;                       // g . out_i = sum_j w_j c_j
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            const int j = j0 + l;
            if (j < cnt) {
                const float wj = la[j] / sum;
                la[j] = wj;
                gd = fmaf(wj, lc[j], gd);
            }
        }
        gd = aa_wave_sum(gd);
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            const int j = j0 + l;
            if (j < cnt) {
                const float wj = la[j];
                ls[j] = fmaf(wj, lc[j], -fabsf(wj) * gd);
            }
        }
        aa_wave_sync();
        // pass B: lanes = units
        float sd0 = 0.f, sd1 = 0.f;           // sum_j dm_j of this segment (db, and the p_i - e columns of dW)
#pragma unroll 2
        for (int j = 0; j < cnt; j++) {
            const float4 x = lx[j];
            const float wj = la[j], ds = ls[j];
            const float z0 = aa_z(un.w0, tb0, x), z1 = aa_z(un.w1, tb1, x);
            const float dm0 = z0 > 0.f ? fmaf(ds, un.al0, wj * g2.x) : 0.f;
            const float dm1 = z1 > 0.f ? fmaf(ds, un.al1, wj * g2.y) : 0.f;
            da0 = fmaf(ds, fmaxf(z0, 0.f), da0);
            da1 = fmaf(ds, fmaxf(z1, 0.f), da1);
            sd0 += dm0;
            sd1 += dm1;
            dw0.x = fmaf(dm0, x.x, dw0.x); dw0.y = fmaf(dm0, x.y, dw0.y); dw0.z = fmaf(dm0, x.z, dw0.z); dw0.w = fmaf(dm0, x.w, dw0.w);
            dw1.x = fmaf(dm1, x.x, dw1.x); dw1.y = fmaf(dm1, x.y, dw1.y); dw1.z = fmaf(dm1, x.z, dw1.z); dw1.w = fmaf(dm1, x.w, dw1.w);
        }
        db0 += sd0;
        db1 += sd1;
        if (din == 8) {
            dwe0.x = fmaf(sd0, pe.x, dwe0.x); dwe0.y = fmaf(sd0, pe.y, dwe0.y); dwe0.z = fmaf(sd0, pe.z, dwe0.z); dwe0.w = fmaf(sd0, pe.w, dwe0.w);
            dwe1.x = fmaf(sd1, pe.x, dwe1.x); dwe1.y = fmaf(sd1, pe.y, dwe1.y); dwe1.z = fmaf(sd1, pe.z, dwe1.z); dwe1.w = fmaf(sd1, pe.w, dwe1.w);
        }
        aa_wave_sync();                       // (the list is free)
    }
    // the four waves in order -> one block per workgroup (every wave arrives here whatever its segments were)
    const int BL = 128 * (din + 2);
    float *const comb = (float *)aa_lds;      // [4][BL]; the table and the lists are done with
    __syncthreads();
    {
        float *const c = comb + w * BL;
        *(float4 *)(c + (2 * l) * din) = dw0;
        *(float4 *)(c + (2 * l + 1) * din) = dw1;
        if (din == 8) {
            *(float4 *)(c + (2 * l) * din + 4) = dwe0;
            *(float4 *)(c + (2 * l + 1) * din + 4) = dwe1;
        }
        *(float2 *)(c + 128 * din + 2 * l) = make_float2(db0, db1);
        *(float2 *)(c + 128 * din + 128 + 2 * l) = make_float2(da0, da1);
    }
    __syncthreads();
    float *const blk = part + (size_t)blockIdx.x * BL;
    for (int idx = tid; idx < BL; idx += 256) blk[idx] = ((comb[idx] + comb[BL + idx]) + comb[2 * BL + idx]) + comb[3 * BL + idx];
}

// the partial blocks in order of workgroup -> dW [128][din], db [128], d_alpha [128]
AA_KERNEL __launch_bounds__(256) void k_att_agg_reduce(const float *__restrict__ part, int G, int din, float *__restrict__ dW, float *__restrict__ db,
                                                        float *__restrict__ d_alpha) {
    const int BL = 128 * (din + 2), idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= BL) return;
    float s = 0.f;
    for (int g = 0; g < G; g++) s += part[(size_t)g * BL + idx];
    if (idx < 128 * din) dW[idx] = s;
    else if (idx < 128 * din + 128) db[idx - 128 * din] = s;
    else d_alpha[idx - 128 * din - 128] = s;
}

inline int aa_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    return cus;
}
inline int aa_lds_fwd(int kc) { return (AA_TABLE + AA_WAVES * (6 * kc + 128)) * 4; }
inline int aa_lds_bwd(int kc) {
    const int lists = (AA_TABLE + AA_WAVES * (7 * kc + 256)) * 4, comb = AA_WAVES * 128 * 10 * 4;
    return lists > comb ? lists : comb;
}
inline int aa_bwd_grid(int64_t n_seg) {
    int64_t cap = 2 * (int64_t)aa_cus();
    if (cap > AA_MAX_GRID) cap = AA_MAX_GRID;
    const int64_t want = (n_seg + AA_WAVES - 1) / AA_WAVES;
    return (int)(want < cap ? want : cap);
}

inline int launch_att_agg_fwd(const AaArgs &a, float *out, int64_t out_stride, hipStream_t st) {
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_att_agg_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, aa_lds_fwd(AA_KMAX)); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    const int64_t n_seg = (int64_t)a.R * a.P * a.n_rel, want = (n_seg + AA_WAVES - 1) / AA_WAVES, cap = 4 * (int64_t)aa_cus();
    hipLaunchKernelGGL(k_att_agg_fwd, dim3((unsigned)(want < cap ? want : cap)), dim3(64 * AA_WAVES), aa_lds_fwd(a.kc), st, a, out, out_stride);
    return (int)hipGetLastError();
}

inline int launch_att_agg_bwd(const AaArgs &a, const float *gout, int64_t g_stride, float *dW, float *db, float *d_alpha, float *part, hipStream_t st) {
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_att_agg_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, aa_lds_bwd(AA_KMAX)); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    const int G = aa_bwd_grid((int64_t)a.R * a.P), din = a.rel[0].din;
    hipLaunchKernelGGL(k_att_agg_bwd, dim3(G), dim3(64 * AA_WAVES), aa_lds_bwd(a.kc), st, a, gout, g_stride, part);
    hipLaunchKernelGGL(k_att_agg_reduce, dim3((128 * (din + 2) + 255) / 256), dim3(256), 0, st, (const float *)part, G, din, dW, db, d_alpha);
    return (int)hipGetLastError();
}
