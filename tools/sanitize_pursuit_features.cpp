// Stand-alone sanitizer driver of the host side of env_3d's line-of-sight policy features (csrc/pursuit_features.hpp and
// e3d_pursuit_features_host of csrc/e3d_env.hip).  It needs no GPU and no Python: build it together with the
// library's source and run it,
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -pthread -Iinclude -I<package>/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -fsanitize=address,undefined \
//         <package>/csrc/e3d_env.hip tools/sanitize_pursuit_features.cpp -o sanitize_pursuit_features && ./sanitize_pursuit_features
// Every array is a heap block of exactly the size the ABI names, so a read or write past a record, an adjacency row or an output row
// is a report.  P = 1, 9, 33 (the pursuer counts of the kernel's 8-, 16- and 64-lane groups), all three evader models, random states
// with inactive pursuers and an inactive evader, and the relay chains.  Exit status 0: clean.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "e3d_env.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, (0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

static int fail(const char *what, int P, int mode) {
    fprintf(stderr, "FAILED: %s (P %d, mode %d)\n", what, P, mode);
    return 1;
}

static int run_random(int P) {
    const int N = 5;
    e3d_config c = {P, 200, 0.7, 1.0, 3.0, 6.0, 0.5, 0.785, 0.4, 0.5};
    std::vector<double> p((size_t)N * 7 * P), e((size_t)N * 7), tg((size_t)N * 3);
    std::vector<int32_t> ts(N);
    std::vector<float> pp((size_t)N * P * P), pe((size_t)N * P), fa((size_t)N * P * E3D_FEAT2), fc(fa.size());
    for (int n = 0; n < N; n++) {
        for (int i = 0; i < P; i++) {
            const bool on = uniform() < 0.75;
            for (int k = 0; k < 3; k++) p[((size_t)n * 7 + k) * P + i] = on ? 20 * uniform() : 1000.0;
            p[((size_t)n * 7 + 3) * P + i] = on ? 6.28 * uniform() - 3.14 : 0;
            p[((size_t)n * 7 + 4) * P + i] = on ? 3 * uniform() - 1.5 : 0;
            p[((size_t)n * 7 + 5) * P + i] = on ? 0.7 * uniform() : 0;
            p[((size_t)n * 7 + 6) * P + i] = on;
            pe[(size_t)n * P + i] = uniform() < 0.5;
            for (int j = 0; j < P; j++) pp[((size_t)n * P + i) * P + j] = uniform() < 0.5;
        }
        const bool e_on = n != 2;
        for (int k = 0; k < 3; k++) { e[(size_t)n * 7 + k] = e_on ? 20 * uniform() : 1000.0; tg[(size_t)n * 3 + k] = 20 * uniform(); }
        e[(size_t)n * 7 + 3] = e_on ? 6.28 * uniform() - 3.14 : 0; e[(size_t)n * 7 + 4] = e_on ? 3 * uniform() - 1.5 : 0;
        e[(size_t)n * 7 + 5] = e_on ? uniform() : 0; e[(size_t)n * 7 + 6] = e_on;
        ts[n] = (int32_t)(200 * uniform());
    }
    for (int mode = 0; mode < 3; mode++) {
        for (size_t k = 0; k < fa.size(); k++) fa[k] = fc[k] = 7.f;
        if (e3d_pursuit_features_host(&c, N, p.data(), e.data(), tg.data(), ts.data(), pp.data(), pe.data(), mode, fa.data(), fc.data())) return fail("rc", P, mode);
        for (int n = 0; n < N; n++)
            for (int i = 0; i < P; i++) {
                const float *a = &fa[((size_t)n * P + i) * E3D_FEAT2], *q = &fc[((size_t)n * P + i) * E3D_FEAT2];
                const bool on = p[((size_t)n * 7 + 6) * P + i] != 0, e_on = e[(size_t)n * 7 + 6] != 0;
                for (int k = 0; k < E3D_FEAT2; k++) {
                    if (!(a[k] == a[k]) || !(q[k] == q[k]) || a[k] == 7.f || q[k] == 7.f) return fail("nan or an unwritten column", P, mode);
                    if (!on && (a[k] != 0.f || q[k] != 0.f)) return fail("inactive row not zero", P, mode);
                }
                if (on && q[16] != (e_on ? 1.f : 0.f)) return fail("critic k", P, mode);
                if (on && a[16] != 0.f && a[16] != 1.f) return fail("actor k", P, mode);
                if (on && mode == 2 && a[16] != q[16]) return fail("global k", P, mode);
                if (on && mode == 0 && a[16] != (e_on && pe[(size_t)n * P + i] == 1.f ? 1.f : 0.f)) return fail("sensed k", P, mode);
            }
    }
    if (e3d_pursuit_features_host(&c, N, p.data(), e.data(), tg.data(), ts.data(), pp.data(), pe.data(), 3, fa.data(), fc.data()) != E3D_ERR_BAD_CONFIG)
        return fail("bad mode accepted", P, 3);
    return 0;
}

// P pursuers in a line that hear their two neighbours only; the last one alone senses; `dead` (or -1) is inactive
static int run_chain(int P, int dead) {
    e3d_config c = {P, 200, 0.7, 1.0, 3.0, 6.0, 0.5, 0.785, 0.4, 0.5};
    std::vector<double> p((size_t)7 * P, 0.0), e(7, 0.0), tg(3, 10.0);
    std::vector<int32_t> ts(1, 7);
    std::vector<float> pp((size_t)P * P, 0.f), pe(P, 0.f), fa((size_t)P * E3D_FEAT2), fc(fa.size());
    for (int i = 0; i < P; i++) {
        const bool on = i != dead;
        p[i] = on ? 5.0 * i : 1000.0; p[(size_t)6 * P + i] = on;
        for (int j = 0; j < P; j++) pp[(size_t)i * P + j] = on && j != dead && abs(i - j) <= 1;
    }
    pe[P - 1] = 1.f;
    e[0] = 5.0 * (P - 1) + 1; e[5] = 0.5; e[6] = 1;
    if (e3d_pursuit_features_host(&c, 1, p.data(), e.data(), tg.data(), ts.data(), pp.data(), pe.data(), E3D_EVADER_OBS_TEAM, fa.data(), fc.data()))
        return fail("rc", P, 1);
    for (int i = 0; i < P; i++) {
        const float want = (dead < 0 || i > dead) ? 1.f : 0.f;
        if (fa[(size_t)i * E3D_FEAT2 + 16] != want) return fail("chain relay", P, dead);
    }
    return 0;
}

int main() {
    int bad = 0;
    for (int P : {1, 9, 33}) bad |= run_random(P);
    for (int P : {9, 33}) bad |= run_chain(P, -1) | run_chain(P, P / 2);
    bad |= run_chain(1, -1);
    if (!bad) printf("sanitize_pursuit_features: clean\n");
    return bad;
}
