// pool_agg.hpp -- DHGN's vertex-level MAX-POOL aggregator (`algo.vertex_level_aggregator: pool`): the relation message and an element-wise
// maximum over the listed neighbours as one launch each way (C ABI: include/mappo_ops.h dhgn_pool_agg3_fwd / dhgn_pool_agg_bwd).
// Ours: the reference's `pool` branch (CustomMaxPool) takes the arg-max over the feature axis and cannot be ported; this is the
// GraphSAGE max-pool aggregator with the AGG layer kept linear behind the maximum (no new parameters).
//
//   x_ij = p_i - q_j  (din 8: [p_i - q_j, p_i - e])        z_ij = W x_ij + b        listed j: a_ij != 0 (the weight's value is not used)
//   out_i[u] = relu(max over listed j of z_ij[u])           nothing listed -> exact zeros     (max_j relu(z_j) = relu(max_j z_j): ONE ReLU)
//   backward, g = d out_i: for every unit with out_i[u] > 0, j*(u) = the first listed j (list order) that attains the maximum:
//   dW[u, :] += g[u] x_{i j*(u)},  db[u] += g[u];  a unit whose maximum is not positive gets nothing.
//
// A SEGMENT is one (relation, row, pursuer).  ONE WAVE owns a segment from its list to its output row; four waves of a persistent
// 256-thread workgroup stride over the segments relation-major, as csrc/att_agg.hpp does, each with its own LDS region sized by the
// launch's largest K.  Per segment:
//   list     the lanes compact the j with a_ij != 0, in order of j (ballot + popcount), into the wave's LDS as x = p_i - q_j; under the
//            all-ones and valid masks nothing is compacted, the first kv differences are written where they belong.  The p_i - e half of
//            the defender relation does not depend on j: it is folded into a per-segment bias tb = b + W[:, 4:8] (p_i - e).
//   walk     lanes = units (2 l, 2 l + 1; their rows of W, b in registers while the relation lasts): x_j is broadcast from LDS, a pair
//            costs four fused multiply-adds and one max a unit on the PRE-activation; the ReLU is applied once, one 512-byte row stored.
// The forward is that one pass: no score pass, no butterflies, no staged table and so NO workgroup barrier at all (the unit lanes read
// their rows of W from global memory once per relation).  z is evaluated on the differences, never as W p_i - min_j W q_j, which cancels
// in fp32 when positions are large and differences small.
//
// The backward saves nothing: it walks the same list through the same aa_z, so its maximum has the forward's bits, and keeps per unit the
// index of the first strict improvement; x_{j*} is read back from LDS at a lane-varying address.  dW[2][din], db[2] stay in the lane's
// registers over all the wave's segments; the four waves are added in order through LDS into one partial block per workgroup and
// k_pool_agg_reduce adds the blocks in order of workgroup.  No atomics, nothing per pair in HBM; a segment's bits depend on its own inputs only.
// The P segments of a critic row each walk the row's obstacle list themselves: a shared walk was not built.
#pragma once
#include "att_agg.hpp"

constexpr int PA_WAVES = AA_WAVES, PA_MAX_GRID = AA_MAX_GRID;

struct PaArgs {
    mo_msg_rel rel[3];
    int32_t n_rel, R, P, kc;                  // kc: list capacity of a wave (the largest K, a multiple of 4)
    int64_t p_rs;
    const float *p;
};

// the differences x = p_i - q_j of segment (r, i)'s listed pairs in order of j -> count.  Every lane of the wave calls it.
__device__ __forceinline__ int pa_build_list(const mo_msg_rel &m, const float *__restrict__ p, int64_t p_rs, int64_t r, int i, int l, float4 *lx,
                                             float4 &pi) {
    pi = *(const float4 *)(p + r * p_rs + 4 * i);
    const int K = m.K;
    const int64_t qr = r / m.q_div;
    const float *qrow = m.q + qr * m.q_rs;
    if (m.adj_mode == MO_ADJ_ONES || m.adj_mode == MO_ADJ_VALID) {   // (uniform) the first kv pairs, nothing to compact
        int kv = K;
        if (m.adj_mode == MO_ADJ_VALID) {
            kv = m.kvalid[qr];
            kv = kv < 0 ? 0 : (kv > K ? K : kv);
        }
        for (int j = l; j < kv; j += 64) {
            const float4 qj = *(const float4 *)(qrow + 4 * j);
            lx[j] = make_float4(pi.x - qj.x, pi.y - qj.y, pi.z - qj.z, pi.w - qj.w);
        }
        return kv;
    }
    int cnt = 0;
    for (int j0 = 0; j0 < K; j0 += 64) {
        const int j = j0 + l;
        const bool nz = j < K && aa_adj(m, r, i, j, K) != 0.f;
        const unsigned long long bal = __ballot(nz);
        if (nz) {
            const float4 qj = *(const float4 *)(qrow + 4 * j);
            lx[cnt + __popcll(bal & ((1ull << l) - 1ull))] = make_float4(pi.x - qj.x, pi.y - qj.y, pi.z - qj.z, pi.w - qj.w);
        }
        cnt += __popcll(bal);
    }
    return cnt;
}

// rows 2 l and 2 l + 1 of a relation's layer, held by the unit lanes while the relation lasts
struct PaUnit {
    float4 w0, w1, we0, we1;
    float b0, b1;
};
__device__ __forceinline__ PaUnit pa_load_unit(const mo_msg_rel &m, int l) {
    PaUnit u;
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
    return u;
}
// the per-segment bias of the lane's two units: the same expression forward and backward
__device__ __forceinline__ void pa_segment_bias(const mo_msg_rel &m, const PaUnit &u, int64_t r, const float4 &pi, float4 &pe, float &tb0, float &tb1) {
    tb0 = u.b0;
    tb1 = u.b1;
    pe = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m.din == 8) {
        const float4 e4 = *(const float4 *)(m.e + r * m.e_rs);
        pe = make_float4(pi.x - e4.x, pi.y - e4.y, pi.z - e4.z, pi.w - e4.w);
        tb0 = aa_z(u.we0, u.b0, pe);
        tb1 = aa_z(u.we1, u.b1, pe);
    }
}

AA_KERNEL __launch_bounds__(256) void k_pool_agg_fwd(PaArgs a, float *__restrict__ out, int64_t out_stride) {
    extern __shared__ float4 pa_lds[];        // per wave: x [kc] float4
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    float4 *const lx = pa_lds + w * a.kc;
    const int64_t RP = (int64_t)a.R * a.P, n_seg = RP * a.n_rel;
    int cur = -1;
    PaUnit un;
    for (int64_t seg = (int64_t)blockIdx.x * PA_WAVES + w; seg < n_seg; seg += (int64_t)gridDim.x * PA_WAVES) {
        const int rel = (int)(seg / RP);
        const int64_t ri = seg - rel * RP, r = ri / a.P;
        const int i = (int)(ri - r * a.P);
        const mo_msg_rel &m = a.rel[rel];
        if (rel != cur) {
            un = pa_load_unit(m, l);
            cur = rel;
        }
        float4 pi, pe;
        const int cnt = pa_build_list(m, a.p, a.p_rs, r, i, l, lx, pi);
        float tb0, tb1;
        pa_segment_bias(m, un, r, pi, pe, tb0, tb1);
        aa_wave_sync();
        float mx0 = -INFINITY, mx1 = -INFINITY;   // nothing listed: relu(-inf) = exact zeros
#pragma unroll 4
        for (int j = 0; j < cnt; j++) {
            const float4 x = lx[j];
            mx0 = fmaxf(mx0, aa_z(un.w0, tb0, x));
            mx1 = fmaxf(mx1, aa_z(un.w1, tb1, x));
        }
        *(float2 *)(out + ri * out_stride + rel * AA_E + 2 * l) = make_float2(fmaxf(mx0, 0.f), fmaxf(mx1, 0.f));
        aa_wave_sync();                       // (the list is free)
    }
}

__device__ __forceinline__ void pa_fma4(float4 &acc, float s, const float4 &x) {
    acc.x = fmaf(s, x.x, acc.x); acc.y = fmaf(s, x.y, acc.y); acc.z = fmaf(s, x.z, acc.z); acc.w = fmaf(s, x.w, acc.w);
}

// one relation (a.n_rel == 1).  part: [gridDim.x][128 (din + 1)] floats, a block = dW [128][din] | db [128]
AA_KERNEL __launch_bounds__(256) void k_pool_agg_bwd(PaArgs a, const float *__restrict__ gout, int64_t g_stride, float *__restrict__ part) {
    extern __shared__ float4 pa_lds[];        // per wave: x [kc] float4; afterwards [4][BL] floats
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    float4 *const lx = pa_lds + w * a.kc;
    const mo_msg_rel &m = a.rel[0];
    const int din = m.din;
    const PaUnit un = pa_load_unit(m, l);
    float4 dw0 = make_float4(0.f, 0.f, 0.f, 0.f), dw1 = dw0, dwe0 = dw0, dwe1 = dw0;
    float db0 = 0.f, db1 = 0.f;
    const int64_t n_seg = (int64_t)a.R * a.P;
    for (int64_t ri = (int64_t)blockIdx.x * PA_WAVES + w; ri < n_seg; ri += (int64_t)gridDim.x * PA_WAVES) {
        const int64_t r = ri / a.P;
        const int i = (int)(ri - r * a.P);
        float4 pi, pe;
        const int cnt = pa_build_list(m, a.p, a.p_rs, r, i, l, lx, pi);
        if (cnt == 0) continue;               // (wave-uniform) no pair, no gradient
        float tb0, tb1;
        pa_segment_bias(m, un, r, pi, pe, tb0, tb1);
        const float2 g2 = *(const float2 *)(gout + ri * g_stride + 2 * l);
        aa_wave_sync();
        float mx0 = -INFINITY, mx1 = -INFINITY;
        int j0 = 0, j1 = 0;                   // the first strict improvement: the first j that attains the maximum
#pragma unroll 4
        for (int j = 0; j < cnt; j++) {
            const float4 x = lx[j];
            const float z0 = aa_z(un.w0, tb0, x), z1 = aa_z(un.w1, tb1, x);
            if (z0 > mx0) mx0 = z0, j0 = j;
            if (z1 > mx1) mx1 = z1, j1 = j;
        }
        const float d0 = mx0 > 0.f ? g2.x : 0.f, d1 = mx1 > 0.f ? g2.y : 0.f;
        const float4 x0 = lx[j0], x1 = lx[j1];       // (j0, j1 < cnt: entries of this segment's list whatever the maximum was)
        pa_fma4(dw0, d0, x0);
        pa_fma4(dw1, d1, x1);
        db0 += d0;
        db1 += d1;
        if (din == 8) {
            pa_fma4(dwe0, d0, pe);
            pa_fma4(dwe1, d1, pe);
        }
        aa_wave_sync();                       // (the list is free)
    }
    // the four waves in order -> one block per workgroup (every wave arrives here whatever its segments were)
    const int BL = 128 * (din + 1);
    float *const comb = (float *)pa_lds;      // [4][BL]; the lists are done with
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
    }
    __syncthreads();
    float *const blk = part + (size_t)blockIdx.x * BL;
    for (int idx = tid; idx < BL; idx += 256) blk[idx] = ((comb[idx] + comb[BL + idx]) + comb[2 * BL + idx]) + comb[3 * BL + idx];
}

// the partial blocks in order of workgroup -> dW [128][din], db [128]
AA_KERNEL __launch_bounds__(256) void k_pool_agg_reduce(const float *__restrict__ part, int G, int din, float *__restrict__ dW, float *__restrict__ db) {
    const int BL = 128 * (din + 1), idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= BL) return;
    float s = 0.f;
    for (int g = 0; g < G; g++) s += part[(size_t)g * BL + idx];
    if (idx < 128 * din) dW[idx] = s;
    else db[idx - 128 * din] = s;
}

inline int pa_lds_fwd(int kc) { return PA_WAVES * kc * 16; }
inline int pa_lds_bwd(int kc) {
    const int lists = PA_WAVES * kc * 16, comb = PA_WAVES * 128 * 9 * 4;
    return lists > comb ? lists : comb;
}

inline int launch_pool_agg_fwd(const PaArgs &a, float *out, int64_t out_stride, hipStream_t st) {
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_pool_agg_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, pa_lds_fwd(AA_KMAX)); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    const int64_t n_seg = (int64_t)a.R * a.P * a.n_rel, want = (n_seg + PA_WAVES - 1) / PA_WAVES, cap = 8 * (int64_t)aa_cus();
    hipLaunchKernelGGL(k_pool_agg_fwd, dim3((unsigned)(want < cap ? want : cap)), dim3(64 * PA_WAVES), pa_lds_fwd(a.kc), st, a, out, out_stride);
    return (int)hipGetLastError();
}

inline int launch_pool_agg_bwd(const PaArgs &a, const float *gout, int64_t g_stride, float *dW, float *db, float *part, hipStream_t st) {
    static std::once_flag once;
    static hipError_t attr_rc = hipSuccess;
    std::call_once(once, [] { attr_rc = hipFuncSetAttribute((const void *)k_pool_agg_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, pa_lds_bwd(AA_KMAX)); });
    if (attr_rc != hipSuccess) return (int)attr_rc;
    const int G = aa_bwd_grid((int64_t)a.R * a.P), din = a.rel[0].din;
    hipLaunchKernelGGL(k_pool_agg_bwd, dim3(G), dim3(64 * PA_WAVES), pa_lds_bwd(a.kc), st, a, gout, g_stride, part);
    hipLaunchKernelGGL(k_pool_agg_reduce, dim3((128 * (din + 1) + 255) / 256), dim3(256), 0, st, (const float *)part, G, din, dW, db);
    return (int)hipGetLastError();
}
