// Stand-alone sanitizer driver of the host side of env_3d's centralised critic input (csrc/central_critic.hpp and
// e3d_central_features_host of csrc/e3d_env.hip).  It needs no GPU and no Python: build it together with the
// library's source and run it,
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -pthread -Iinclude -I<package>/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -fsanitize=address,undefined \
//         <package>/csrc/e3d_env.hip tools/sanitize_central_critic.cpp -o sanitize_central_critic && ./sanitize_central_critic
// Every array is a heap block of exactly the size the ABI names, so a read or write past a record, an adjacency row or an output row
// (the critic's rows are E3D_CENTRAL_FEAT(P) wide) is a report.  P = 1, 2, 8, 9, 16, all three evader models, random states with
// inactive pursuers and an inactive evader; every column written, empty slots zero, filled slots a unit heading; P = 17 refused with
// nothing written.  Exit status 0: clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

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

static int run_random(int P, bool refused) {
    const int N = 5, CF = E3D_CENTRAL_FEAT(P);
    e3d_config c = {P, 200, 0.7, 1.0, 3.0, 6.0, 0.5, 0.785, 0.4, 0.5};
    std::vector<double> p((size_t)N * 7 * P), e((size_t)N * 7), tg((size_t)N * 3);
    std::vector<int32_t> ts(N);
    std::vector<float> pp((size_t)N * P * P), pe((size_t)N * P), fa((size_t)N * P * E3D_FEAT2), fc((size_t)N * P * CF);
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
        e[(size_t)n * 7 + 5] = e_on ? uniform() : 0; e[(size_t)n * 7 + 6] = e_on;
        ts[n] = (int32_t)(200 * uniform());
    }
    for (int mode = 0; mode < 3; mode++) {
        for (float &v : fa) v = 7.f;
        for (float &v : fc) v = 7.f;
        const int rc = e3d_central_features_host(&c, N, p.data(), e.data(), tg.data(), ts.data(), pp.data(), pe.data(), mode, fa.data(), fc.data());
        if (refused) {
            if (rc != E3D_ERR_BAD_CONFIG) return fail("P above E3D_CENTRAL_MAX_P accepted", P, mode);
            for (float v : fc) if (v != 7.f) return fail("a refused call wrote", P, mode);
            continue;
        }
        if (rc) return fail("rc", P, mode);
        for (int n = 0; n < N; n++) {
            int team = 0;
            for (int i = 0; i < P; i++) team += p[((size_t)n * 7 + 6) * P + i] != 0;
            for (int i = 0; i < P; i++) {
                const float *a = &fa[((size_t)n * P + i) * E3D_FEAT2], *q = &fc[((size_t)n * P + i) * CF];
                const bool on = p[((size_t)n * 7 + 6) * P + i] != 0;
                for (int k = 0; k < E3D_FEAT2; k++)
                    if (!(a[k] == a[k]) || a[k] == 7.f || (!on && a[k] != 0.f)) return fail("actor row", P, mode);
                for (int k = 0; k < CF; k++)
                    if (!(q[k] == q[k]) || q[k] == 7.f || (!on && q[k] != 0.f)) return fail("nan, an unwritten column or an inactive row not zero", P, mode);
                for (int s = 0; s < P - 1; s++) {
                    const float *b = q + E3D_FEAT2 + E3D_CENTRAL_MATE * s;
                    const double u = sqrt((double)b[4] * b[4] + (double)b[5] * b[5] + (double)b[6] * b[6]);
                    if (on && s < team - 1) {
                        if (fabs(u - 1.0) > 1e-6 || !(b[3] > 0.f)) return fail("filled slot", P, mode);
                        if (s > 0 && b[3] < b[3 - E3D_CENTRAL_MATE]) return fail("slots not in the order of distance", P, mode);
                    } else {
                        for (int k = 0; k < E3D_CENTRAL_MATE; k++) if (b[k] != 0.f) return fail("empty slot not zero", P, mode);
                    }
                }
            }
        }
    }
    return 0;
}

int main() {
    int bad = 0;
    for (int P : {1, 2, 8, 9, 16}) bad |= run_random(P, false);
    bad |= run_random(17, true);
    if (!bad) printf("sanitize_central_critic: clean\n");
    return bad;
}
