// Phase stamps of the split-bf16 GRU sequence backward (csrc/sb_gru_seq.hpp k_gru_seq_bwd_sb): a copy of the kernel's step with
// s_memtime stamps between its phases, in the two forms of its input path -- RING = false: the six float4 inputs of step t - 1 loaded
// into registers during step t (the kernel before the ring); RING = true: the product kernel's LDS ring filled by LDS-direct loads two
// steps ahead.  The grouped update launch of the benchmark (18 records of 3 280 sequences + 2 of 3 248, T = 150, dnr form, bias sums):
// 4 096 workgroups.  Prints per wave of one mid-grid workgroup the cycles per step spent in each phase, and the launch time.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I distributed_multi_agent_reinforcement_learning_amd/csrc \
//         tools/microbench/gru_seq_bwd_lab.hip -o tools/microbench/gru_seq_bwd_lab
#include "sb_gru_seq.hpp"

#include <cstdio>
#include <vector>

__device__ unsigned long long sbr_stamps[8][8];

#define STAMP(k)                                             \
    {                                                        \
        const unsigned long long now_ = __builtin_readcyclecounter(); \
        acc[k] += now_ - last;                               \
        last = now_;                                         \
    }

template <bool RING>
__global__ __launch_bounds__(512) void k_lab(int T, int Bmax, SbGruBwdNets nets, int gi_agents) {
    const mo_gru_seq_bwd_net &net = nets.n[blockIdx.y];
    const int B = net.B > 0 ? net.B : Bmax;
    if ((int)blockIdx.x * SBR_RB >= B) return;
    const float *__restrict__ dout = net.dout, *__restrict__ save = net.save, *__restrict__ out = net.out, *__restrict__ h0 = net.h0,
                *__restrict__ w_hh = net.w_hh;
    float *__restrict__ dgi = net.dgi, *__restrict__ dgh = net.dgh, *__restrict__ dnr_out = net.dnr, *__restrict__ dh0 = net.dh0;
    extern __shared__ uint4 sbr_lds[];
    constexpr int IMG = 3 * 12 * 64;
    uint4 *const sbr_gimg = sbr_lds + (RING ? SBR_RING_SLOTS * 8 * 64 : 0);
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, i = l & 15, gq = l >> 4;
    const int b0 = blockIdx.x * SBR_RB;
    uint4 wt[12][3];
#pragma unroll
    for (int c = 0; c < 12; c++) {
        const float *col = w_hh + (size_t)(32 * c + 8 * gq) * SBR_H + 16 * w + i;
        const float4 u = make_float4(col[0], col[SBR_H], col[2 * SBR_H], col[3 * SBR_H]);
        const float4 v = make_float4(col[4 * SBR_H], col[5 * SBR_H], col[6 * SBR_H], col[7 * SBR_H]);
        sb_split8(u, v, wt[c]);
    }
    const int row = i, u0 = 16 * w + 4 * gq;
    const bool live = b0 + row < B;
    const size_t nblk = (size_t)(B + SBR_RB - 1) / SBR_RB;
    const float4 *sv = (const float4 *)save + (size_t)blockIdx.x * 4 * 512 + tid;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 sb_r = zero4, sb_z = zero4, sb_n = zero4, sb_nr = zero4;
    float4 dcarry = zero4;
    float4 pr, pz, pn, phn, php, pdo;
    auto prefetch = [&](int t) {
        pr = pz = pn = phn = php = pdo = zero4;
        if (live) {
            const float4 *s4 = sv + (size_t)t * nblk * 4 * 512;
            pr = s4[0]; pz = s4[512]; pn = s4[1024]; phn = s4[1536];
            const size_t o = (size_t)(b0 + row) * SBR_H + u0;
            php = *(const float4 *)(t > 0 ? out + (size_t)(t - 1) * B * SBR_H + o : h0 + o);
            pdo = *(const float4 *)(dout + (size_t)t * B * SBR_H + o);
        }
    };
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const uint32_t ring0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)sbr_lds + wu * SBR_RING_SLOTS * 1024;
    const float4 *ring = (const float4 *)sbr_lds + wu * SBR_RING_SLOTS * 64 + l;
    const size_t orow = (size_t)(live ? b0 + row : b0) * SBR_H + u0;
    auto fetch_hn = [&](int t) { sbr_glds16(sv + (size_t)(t > 0 ? t : 0) * nblk * 4 * 512 + 1536, ring0 + 10 * 1024, true); };
    auto fetch5 = [&](int t, int par) {
        const int tc = t > 0 ? t : 0;
        const float4 *s4 = sv + (size_t)tc * nblk * 4 * 512;
        const uint32_t dst = ring0 + par * 5 * 1024;
        sbr_glds16(s4, dst, false); sbr_glds16(s4 + 512, dst + 1024, false); sbr_glds16(s4 + 1024, dst + 2048, false);
        sbr_glds16(tc > 0 ? out + (size_t)(tc - 1) * B * SBR_H + orow : h0 + orow, dst + 3072, false);
        sbr_glds16(dout + (size_t)tc * B * SBR_H + orow, dst + 4096, false);
    };
    if constexpr (RING) {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        fetch_hn(T - 1); fetch5(T - 1, 0); fetch5(T - 2, 1);
        asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    } else {
        prefetch(T - 1);
    }
    int buf = 0, par = 0;
    unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
    const unsigned long long begin = __builtin_readcyclecounter();
    unsigned long long last = begin;
    for (int t = T - 1; t >= 0; t--) {
        float4 dr, dz, dn, dnr, dhz;
        {
            float4 r, z, n, hn, hp, dO;
            if constexpr (RING) {
                r = ring[(par * 5 + 0) * 64]; z = ring[(par * 5 + 1) * 64]; n = ring[(par * 5 + 2) * 64]; hp = ring[(par * 5 + 3) * 64];
                dO = ring[(par * 5 + 4) * 64]; hn = ring[10 * 64];
                fetch_hn(t - 1);
                fetch5(t - 2, par);
                if (!live) r = z = n = hp = dO = hn = zero4;
            } else {
                r = pr; z = pz; n = pn; hn = phn; hp = php; dO = pdo;
                // every prefetched register is needed here: the wait for the loads issued one step ago
                asm volatile("" ::"v"(r.x), "v"(z.x), "v"(n.x), "v"(hn.x), "v"(hp.x), "v"(dO.x), "v"(r.w), "v"(z.w), "v"(n.w), "v"(hn.w), "v"(hp.w), "v"(dO.w));
            }
            STAMP(0)   // RING: read-back from LDS and issue of the loads; else: wait for the prefetched registers
#define SBR_ONE(f)                                               \
            {                                                    \
                const float dh = dO.f + dcarry.f;                \
                dn.f = dh * (1.f - z.f) * (1.f - n.f * n.f);     \
                dz.f = dh * (hp.f - n.f) * z.f * (1.f - z.f);    \
                dr.f = dn.f * hn.f * r.f * (1.f - r.f);          \
                dnr.f = dn.f * r.f;                              \
                dhz.f = dh * z.f;                                \
            }
            SBR_ONE(x) SBR_ONE(y) SBR_ONE(z) SBR_ONE(w)
#undef SBR_ONE
            asm volatile("" ::"v"(dr.x), "v"(dz.x), "v"(dnr.x), "v"(dhz.x), "v"(dr.w), "v"(dz.w), "v"(dnr.w), "v"(dhz.w));
        }
        STAMP(1)       // gate math
        par ^= 1;
        if constexpr (!RING)
            if (t > 0) prefetch(t - 1);
        uint4 *gb = sbr_gimg + buf * IMG;
        sbr_put4(gb, 12, u0, row, dr);
        sbr_put4(gb, 12, SBR_H + u0, row, dz);
        sbr_put4(gb, 12, 2 * SBR_H + u0, row, dnr);
        if (live) {
            float *g = dgi + sbr_gi_row(b0 + row, t, T, B, gi_agents) * 3 * SBR_H + u0;
            *(float4 *)g = dr; *(float4 *)(g + SBR_H) = dz; *(float4 *)(g + 2 * SBR_H) = dn;
            const size_t tb = (size_t)t * B + b0 + row;
            if (dgh) {
                float *h = dgh + tb * 3 * SBR_H + u0;
                *(float4 *)h = dr; *(float4 *)(h + SBR_H) = dz; *(float4 *)(h + 2 * SBR_H) = dnr;
            } else {
                *(float4 *)(dnr_out + tb * SBR_H + u0) = dnr;
            }
#define SBR_ACC(S, V) S.x += V.x; S.y += V.y; S.z += V.z; S.w += V.w;
            SBR_ACC(sb_r, dr) SBR_ACC(sb_z, dz) SBR_ACC(sb_n, dn) SBR_ACC(sb_nr, dnr)
#undef SBR_ACC
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        STAMP(2)       // (register form: issue of the loads,) splits, image writes, store issue
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        STAMP(3)       // barrier
        const uint4 *tb = gb + l;
        f32x4 hi0 = {0.f, 0.f, 0.f, 0.f}, hi1 = hi0, lo0 = hi0, lo1 = hi0, lo2 = hi0;
#pragma unroll
        for (int c = 0; c < 12; c++) {
            uint4 b[3];
#pragma unroll
            for (int p = 0; p < 3; p++) b[p] = tb[(p * 12 + c) * 64];
#define SBR_MMA(pi, pj, ACC) ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wt[c][pi]), __builtin_bit_cast(bf16x8, b[pj]), ACC, 0, 0, 0);
            if (c & 1) { SBR_MMA(2, 0, lo0) SBR_MMA(0, 2, lo1) SBR_MMA(1, 1, lo2) SBR_MMA(0, 0, hi1) SBR_MMA(1, 0, lo0) SBR_MMA(0, 1, lo1) }
            else       { SBR_MMA(2, 0, lo2) SBR_MMA(0, 2, lo0) SBR_MMA(1, 1, lo1) SBR_MMA(0, 0, hi0) SBR_MMA(1, 0, lo2) SBR_MMA(0, 1, lo0) }
#undef SBR_MMA
        }
        const f32x4 s = (hi0 + hi1) + ((lo0 + lo1) + lo2);
        dcarry.x = dhz.x + s[0]; dcarry.y = dhz.y + s[1]; dcarry.z = dhz.z + s[2]; dcarry.w = dhz.w + s[3];
        asm volatile("" ::"v"(dcarry.x), "v"(dcarry.y), "v"(dcarry.z), "v"(dcarry.w));
        buf ^= 1;
        STAMP(4)       // matrix phase
        if constexpr (RING) {
            if (dgh) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
            STAMP(5)   // RING: the counted wait for the next step's inputs
        }
    }
    const unsigned long long end = __builtin_readcyclecounter();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (live) *(float4 *)(dh0 + (size_t)(b0 + row) * SBR_H + u0) = make_float4(dcarry.x + sb_r.x, dcarry.y + sb_z.y, dcarry.z + sb_n.z, dcarry.w + sb_nr.w);
    if (l == 0 && blockIdx.x == 100 && blockIdx.y == 10) {
        for (int k = 0; k < 6; k++) sbr_stamps[w][k] = acc[k];
        sbr_stamps[w][6] = end - begin;
    }
}

template <bool RING>
static void run(const char *name, int n, const mo_gru_seq_bwd_net *nets, int T, int Bmax) {
    const int lds = (RING ? SBR_RING_SLOTS * 8 * 1024 : 0) + 2 * 3 * 12 * 64 * 16;
    if (hipFuncSetAttribute((const void *)k_lab<RING>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) { printf("%s: LDS size refused\n", name); exit(2); }
    SbGruBwdNets a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < n; k++) a.n[k] = nets[k];
    const int nblk = (Bmax + SBR_RB - 1) / SBR_RB;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int it = 0; it < 2; it++) hipLaunchKernelGGL(k_lab<RING>, dim3(nblk, n), dim3(512), lds, 0, T, Bmax, a, 0);
    (void)hipEventRecord(e0, 0);
    for (int it = 0; it < 5; it++) hipLaunchKernelGGL(k_lab<RING>, dim3(nblk, n), dim3(512), lds, 0, T, Bmax, a, 0);
    (void)hipEventRecord(e1, 0);
    if (hipEventSynchronize(e1) != hipSuccess) { printf("%s: launch failed\n", name); exit(3); }
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    printf("%s: %.2f ms per launch (stamped build), %d workgroups, T = %d\n", name, ms / 5, nblk * n, T);
    unsigned long long st[8][8];
    (void)hipMemcpyFromSymbol(st, HIP_SYMBOL(sbr_stamps), sizeof st);
    for (int w = 0; w < 8; w++)
        printf("  wave %d, cycles per step: %s %.0f | gate math %.0f | split, image, store issue %.0f | barrier %.0f | matrix phase %.0f | counted wait %.0f | whole step %.0f\n", w,
               RING ? "read-back + load issue" : "wait for the prefetched registers", st[w][0] / (double)T, st[w][1] / (double)T, st[w][2] / (double)T, st[w][3] / (double)T,
               st[w][4] / (double)T, st[w][5] / (double)T, st[w][6] / (double)T);
}

int main() {
    const int T = 150, n = 20;
    std::vector<mo_gru_seq_bwd_net> nets(n);
    for (int k = 0; k < n; k++) {
        const int B = k < 18 ? 3280 : 3248;
        const size_t nblk = (B + 15) / 16, tbh = (size_t)T * B * 128 * 4;
        const size_t sz[9] = {tbh, T * nblk * 4 * 512 * 16, tbh, (size_t)B * 128 * 4, 384 * 128 * 4, tbh * 3, tbh, (size_t)B * 128 * 4, nblk * 4 * 128 * 4};
        void *p[9];
        for (int j = 0; j < 9; j++) {
            if (hipMalloc(&p[j], sz[j]) != hipSuccess) { printf("out of memory\n"); return 1; }
            (void)hipMemset(p[j], 0x3c, sz[j]);   // every float 0.0115: finite gates and gradients
        }
        nets[k] = mo_gru_seq_bwd_net{(const float *)p[0], (const float *)p[1], (const float *)p[2], (const float *)p[3], (const float *)p[4], (float *)p[5], nullptr,
                                     (float *)p[6], (float *)p[7], nullptr, nullptr, p[8], B, 0};
    }
    (void)hipDeviceSynchronize();
    run<false>("register prefetch, one step ahead", n, nets.data(), T, 3280);
    run<true>("LDS ring, two steps ahead", n, nets.data(), T, 3280);
    return 0;
}
