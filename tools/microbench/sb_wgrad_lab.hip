// sb_wgrad_lab.hip -- phase lab of the weight-gradient kernel k_sb_wgrad.  It compiles the PRODUCT header (csrc/sb_wgrad.hpp), not a
// copy: the header's probe hooks are defined here, so what is stamped is what ships.  Results: profiles/r20_sb_wgrad_lab.txt,
// DESIGN.md section 11.  (The 8-wave kernel's lab, with its clock figures, is in this file's history: profiles/r03_split_bf16_lab.txt.)
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I distributed_multi_agent_reinforcement_learning_amd/csrc [-DSB_LAB_STAMPS] [-DSB_WG_KNOCK=n]
//         tools/microbench/sb_wgrad_lab.hip -o tools/microbench/sb_wgrad_lab_x
//   SB_LAB_STAMPS   per-wave s_memtime sums of the phases of a chunk, workgroup SB_LAB_WG (mid-grid), printed per wave.  Reading the
//                   counter waits for the wave's LDS operations too (lgkmcnt), so a stamp behind LDS stores or reads includes their
//                   completion; a stamped build runs 1-3 % slower and is for the split of a chunk, not for its length.
//   SB_WG_KNOCK     1 the MFMA waves skip the multiply (loader side alone), 2 the loaders neither split nor store (MFMA side alone on a
//                   stale image, HBM stream kept), 3 the loaders split but do not store.  Knock-outs compute garbage: timing only.
// Every run prints, per shape, the time of the kernel alone (no reduction) and an FNV-1a hash of the 256 partial tiles, which two builds
// that claim the same sums in the same order must share.
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef SB_LAB_STAMPS
#ifndef SB_LAB_WG
#define SB_LAB_WG 131
#endif
constexpr int SB_LAB_PHASES = 5;
__device__ unsigned long long sb_lab_cycles[12][SB_LAB_PHASES + 2];   // [wave][phase], then the whole role in cycles and in 100 MHz ticks
struct SbLabProbe {
    uint64_t first, last, rt, acc[SB_LAB_PHASES];
};
#define SB_WG_PROBE_BEGIN                                                   \
    SbLabProbe sb_probe = {};                                               \
    sb_probe.first = sb_probe.last = __builtin_amdgcn_s_memtime();          \
    sb_probe.rt = __builtin_amdgcn_s_memrealtime();
// phase 0 restarts the clock (the prologue is not a chunk)
#define SB_WG_PROBE(phase)                                                  \
    {                                                                       \
        const uint64_t sb_t = __builtin_amdgcn_s_memtime();                 \
        if ((phase) != 0) sb_probe.acc[phase] += sb_t - sb_probe.last;      \
        sb_probe.last = sb_t;                                               \
    }
// the wave's loads of this chunk have landed (the compiler puts the s_waitcnt vmcnt in front of the first use)
#define SB_WG_PROBE_USE(r)                                                                                                   \
    for (auto &sb_u : r)                                                                                                     \
        for (auto &sb_v : sb_u) asm volatile("" ::"v"(sb_v.x), "v"(sb_v.y), "v"(sb_v.z), "v"(sb_v.w));
#define SB_WG_PROBE_END(wave, lane)                                                                           \
    if (blockIdx.x == SB_LAB_WG && (lane) == 0) {                                                             \
        for (int sb_p = 0; sb_p < SB_LAB_PHASES; sb_p++) sb_lab_cycles[wave][sb_p] = sb_probe.acc[sb_p];      \
        sb_lab_cycles[wave][SB_LAB_PHASES] = __builtin_amdgcn_s_memtime() - sb_probe.first;                   \
        sb_lab_cycles[wave][SB_LAB_PHASES + 1] = __builtin_amdgcn_s_memrealtime() - sb_probe.rt;              \
    }
#endif

#include "sb_wgrad.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define LAB_CHECK(x)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) {                                                             \
            fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);     \
            exit(1);                                                                        \
        }                                                                                   \
    } while (0)

constexpr int LAB_WGS = 256;

template <int MT, int NT>
void run(int64_t K, int reps) {
    using C = SbWgCfg<MT, NT>;
    float *A, *B, *part;
    const size_t part_n = (size_t)LAB_WGS * C::M * C::N;
    LAB_CHECK(hipMalloc(&A, (size_t)K * C::M * 4));
    LAB_CHECK(hipMalloc(&B, (size_t)K * C::N * 4));
    LAB_CHECK(hipMalloc(&part, part_n * 4));
    {
        std::vector<float> h((size_t)K * (C::M > C::N ? C::M : C::N));
        uint32_t s = 12345u + 977u * MT + NT;
        for (auto &v : h) {
            s = s * 1664525u + 1013904223u;
            v = (float)(int32_t)s * (1.0f / 2147483648.0f) * (1.0f + (float)((s >> 7) & 15));   // |v| < 16, full mantissas
        }
        LAB_CHECK(hipMemcpy(A, h.data(), (size_t)K * C::M * 4, hipMemcpyHostToDevice));
        for (auto &v : h) v = -0.75f * v + 0.125f;
        LAB_CHECK(hipMemcpy(B, h.data(), (size_t)K * C::N * 4, hipMemcpyHostToDevice));
    }
    LAB_CHECK(hipFuncSetAttribute((const void *)k_sb_wgrad<MT, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
    auto launch = [&] {
        hipLaunchKernelGGL((k_sb_wgrad<MT, NT>), dim3(LAB_WGS), dim3(SB_WG_THREADS), C::LDS_BYTES, 0, A, (int64_t)C::M, B, (int64_t)C::N, K, part,
                           (const float *)nullptr, (int64_t)0, 0);
    };
    hipEvent_t e0, e1;
    LAB_CHECK(hipEventCreate(&e0));
    LAB_CHECK(hipEventCreate(&e1));
    for (int w = 0; w < reps; w++) launch();             // warm clock: as many launches as are timed
    LAB_CHECK(hipEventRecord(e0, 0));
    for (int w = 0; w < reps; w++) launch();
    LAB_CHECK(hipEventRecord(e1, 0));
    LAB_CHECK(hipEventSynchronize(e1));
    LAB_CHECK(hipGetLastError());
    float ms;
    LAB_CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<uint32_t> hp(part_n);
    LAB_CHECK(hipMemcpy(hp.data(), part, part_n * 4, hipMemcpyDeviceToHost));
    uint64_t hash = 1469598103934665603ull;
    for (uint32_t w : hp) hash = (hash ^ w) * 1099511628211ull;
    const double us = ms / reps * 1e3;
    const int64_t chunks = K / C::CR / LAB_WGS;
    printf("knock %d  <%d,%d> %3d x %3d  K %8lld: %7.1f us per launch  %5.2f TB/s  %6.3f us per chunk  partials %016llx\n", SB_WG_KNOCK, MT, NT, C::M,
           C::N, (long long)K, us, (double)K * C::COLS * 4.0 / us / 1e6, us / chunks, (unsigned long long)hash);
#ifdef SB_LAB_STAMPS
    unsigned long long hc[12][SB_LAB_PHASES + 2];
    LAB_CHECK(hipMemcpyFromSymbol(hc, HIP_SYMBOL(sb_lab_cycles), sizeof(hc)));
    printf("  workgroup %d, %lld chunks; cycles per chunk.  MFMA waves: multiply | - | barrier | -.  loaders: stage (splits + stores landed) | fetch issue | barrier | wait for the rows\n",
           SB_LAB_WG, (long long)chunks);
    for (int w = 0; w < SB_WG_MMA_WAVES + SB_WG_LOAD_WAVES; w++)
        printf("  wave %2d %s  %7.0f %7.0f %7.0f %7.0f   sum %7.0f   clock %4.0f MHz\n", w, w < SB_WG_MMA_WAVES ? "mfma" : "load", (double)hc[w][1] / chunks, (double)hc[w][2] / chunks,
               (double)hc[w][3] / chunks, (double)hc[w][4] / chunks, (double)hc[w][SB_LAB_PHASES] / chunks, hc[w][SB_LAB_PHASES + 1] ? hc[w][SB_LAB_PHASES] / (hc[w][SB_LAB_PHASES + 1] / 100.0) : 0.0);
#endif
    LAB_CHECK(hipFree(A));
    LAB_CHECK(hipFree(B));
    LAB_CHECK(hipFree(part));
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 200;
    const int64_t K = argc > 2 ? atoll(argv[2]) : 492000;   // the update's rows; the AGG layer has three times as many
    run<3, 1>(K, reps);
    run<1, 3>(K, reps);
    run<1, 1>(3 * K, reps);
    run<2, 1>(K, reps);
    run<1, 2>(K, reps);
    return 0;
}
