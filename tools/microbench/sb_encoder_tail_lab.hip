// sb_encoder_tail_lab.hip -- lab of the rollout encoder tail (csrc/sb_encoder_tail.hpp): times the fused launch beside the two
// k_sb_gemm_n128 launches it replaces, on the same operands, alternating, and compares the results bit for bit.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I distributed_multi_agent_reinforcement_learning_amd/csrc -I include \
//         tools/microbench/sb_encoder_tail_lab.hip -o tools/microbench/sb_encoder_tail_lab
//   ./tools/microbench/sb_encoder_tail_lab [semantic rows ...]        (default 65536: cfg2's 2 x 4096 environments x 8 pursuers)
// Results: profiles/r18_encoder_tail_lab.txt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mappo_ops.h"
#include "sb_gemm.hpp"
#include "sb_encoder_tail.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

static float rnd(uint64_t &s) {   // uniform in (-1, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((int64_t)(s >> 11) - (1ll << 52)) * (1.0f / (float)(1ll << 52));
}

int main(int argc, char **argv) {
    std::vector<int64_t> sizes;
    for (int a = 1; a < argc; a++) sizes.push_back(atoll(argv[a]));
    if (sizes.empty()) sizes.push_back(65536);
    for (int64_t Rs : sizes) {
        const int ldw = 388;
        std::vector<float> h_m3((size_t)Rs * 384), h_wa(128 * 128), h_ba(128), h_ws((size_t)128 * ldw), h_c((size_t)Rs * 128);
        uint64_t s = 12345 + Rs;
        for (auto &v : h_m3) v = 1.7f * rnd(s);
        for (auto &v : h_wa) v = 0.17f * rnd(s);
        for (auto &v : h_ba) v = 0.55f + rnd(s);
        for (auto &v : h_ws) v = 0.17f * rnd(s);
        for (auto &v : h_c) v = rnd(s);
        float *m3, *wa, *ba, *ws, *c0, *emb, *y2, *y1;
        CK(hipMalloc(&m3, h_m3.size() * 4)); CK(hipMalloc(&wa, h_wa.size() * 4)); CK(hipMalloc(&ba, h_ba.size() * 4)); CK(hipMalloc(&ws, h_ws.size() * 4));
        CK(hipMalloc(&c0, h_c.size() * 4)); CK(hipMalloc(&emb, h_m3.size() * 4)); CK(hipMalloc(&y2, h_c.size() * 4)); CK(hipMalloc(&y1, h_c.size() * 4));
        CK(hipMemcpy(m3, h_m3.data(), h_m3.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(wa, h_wa.data(), h_wa.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(ba, h_ba.data(), h_ba.size() * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(ws, h_ws.data(), h_ws.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(c0, h_c.data(), h_c.size() * 4, hipMemcpyHostToDevice));
        hipStream_t st = nullptr;
        const float *wse = ws + 4;   // the column block [:, 4:] of the (128, 388) semantic weight
        auto two = [&](float *y) {
            int rc = launch_sb_gemm_best<4, 1>(3 * Rs, m3, 128, wa, 128, ba, nullptr, 0, emb, 128, 1, st);
            if (!rc) rc = launch_sb_gemm_best<12, 1>(Rs, emb, 384, wse, ldw, nullptr, y, 128, y, 128, 0, st);
            if (rc) { fprintf(stderr, "two launches: error %d\n", rc); exit(1); }
        };
        auto one = [&](float *y) {
            const int rc = launch_sb_encoder_tail(Rs, m3, 384, wa, ba, wse, ldw, y, 128, y, 128, st);
            if (rc) { fprintf(stderr, "one launch: error %d\n", rc); exit(1); }
        };
        // results (in place onto the same addend)
        CK(hipMemcpy(y2, c0, h_c.size() * 4, hipMemcpyDeviceToDevice)); CK(hipMemcpy(y1, c0, h_c.size() * 4, hipMemcpyDeviceToDevice));
        two(y2); one(y1);
        CK(hipDeviceSynchronize());
        std::vector<uint32_t> r2(h_c.size()), r1(h_c.size());
        CK(hipMemcpy(r2.data(), y2, h_c.size() * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(r1.data(), y1, h_c.size() * 4, hipMemcpyDeviceToHost));
        size_t diff = 0;
        for (size_t k = 0; k < r1.size(); k++) diff += r1[k] != r2[k];
        printf("rows %lld: %zu of %zu outputs differ in bits\n", (long long)Rs, diff, r1.size());
        // times: 12 rounds of 50 launches each, the two forms alternating
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        std::vector<float> t2, t1;
        for (int k = 0; k < 5; k++) { two(y2); one(y1); }
        for (int round = 0; round < 12; round++) {
            for (int which = 0; which < 2; which++) {
                CK(hipEventRecord(e0, st));
                for (int k = 0; k < 50; k++) { if (which) one(y1); else two(y2); }
                CK(hipEventRecord(e1, st));
                CK(hipEventSynchronize(e1));
                float ms = 0.f;
                CK(hipEventElapsedTime(&ms, e0, e1));
                (which ? t1 : t2).push_back(ms * 1000.f / 50.f);
            }
        }
        std::sort(t2.begin(), t2.end()); std::sort(t1.begin(), t1.end());
        printf("rows %lld: two launches %.1f us (min %.1f, max %.1f)   one launch %.1f us (min %.1f, max %.1f)\n", (long long)Rs, t2[6], t2.front(), t2.back(),
               t1[6], t1.front(), t1.back());
        fflush(stdout);
        CK(hipFree(m3)); CK(hipFree(wa)); CK(hipFree(ba)); CK(hipFree(ws)); CK(hipFree(c0)); CK(hipFree(emb)); CK(hipFree(y2)); CK(hipFree(y1));
        if (diff) return 2;
    }
    return 0;
}
