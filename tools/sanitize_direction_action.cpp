// Stand-alone sanitizer driver of the host side of env_3d's direction-vector action head (csrc/direction_action.hpp and
// gauss_direction_map_host / e3d_direction_label_host of csrc/e3d_env.hip).  It needs no GPU and no Python: build
// it together with the library's source and run it,
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -pthread -Iinclude -I<package>/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -fsanitize=address,undefined \
//         <package>/csrc/e3d_env.hip tools/sanitize_direction_action.cpp -o sanitize_direction_action && ./sanitize_direction_action
// Every array is a heap block of exactly the size the ABI names (R x 4 floats, R x 3 doubles), so a read or write past a row is a
// report.  The edge table of the map, exact; R = 1, 7, 300 random rows through both entries and the round trip label -> map within
// 2e-7; the null and size checks.  Exit status 0: clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "e3d_env.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, (0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

static int fail(const char *what, int R) {
    fprintf(stderr, "FAILED: %s (R %d)\n", what, R);
    return 1;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static int run_edges() {
    const float u[5][4] = {{-1.f, 0.f, 0.f, 0.25f}, {-1.f, -0.f, 0.f, 0.25f}, {0.f, 0.f, 0.f, 2.f}, {0.f, 0.f, 1.f, -3.f}, {0.f, 1.f, 0.f, 0.25f}};
    const double want[5][3] = {{1, 0, 0.25}, {-1, 0, 0.25}, {0, 0, 1}, {0, 1, -1}, {0.5, 0, 0.25}};
    std::vector<float> in((const float *)u, (const float *)u + 20);
    std::vector<double> out(15, 7.0);
    if (gauss_direction_map_host(5, in.data(), out.data())) return fail("edge rc", 5);
    for (int r = 0; r < 5; r++)
        for (int a = 0; a < 3; a++)
            if (!same_bits(out[(size_t)r * 3 + a], want[r][a])) return fail("edge table", r);
    return 0;
}

static int run_random(int R) {
    std::vector<double> g((size_t)R * 3), env((size_t)R * 3, 7.0);
    std::vector<float> lab((size_t)R * 4, 7.f);
    for (int r = 0; r < R; r++) {
        g[(size_t)r * 3] = 1.998 * uniform() - 0.999;
        g[(size_t)r * 3 + 1] = 1.998 * uniform() - 0.999;
        g[(size_t)r * 3 + 2] = r % 3 ? 2 * uniform() - 1 : -1.0;
    }
    if (e3d_direction_label_host(R, g.data(), lab.data())) return fail("label rc", R);
    if (gauss_direction_map_host(R, lab.data(), env.data())) return fail("map rc", R);
    for (int r = 0; r < R; r++) {
        const float *l = &lab[(size_t)r * 4];
        const double n = sqrt((double)l[0] * l[0] + (double)l[1] * l[1] + (double)l[2] * l[2]);
        if (!(fabs(n - 1.0) <= 2e-7)) return fail("label is not a unit vector", R);
        if (l[3] != (float)g[(size_t)r * 3 + 2]) return fail("label speed", R);
        for (int a = 0; a < 2; a++)
            if (!(fabs(env[(size_t)r * 3 + a] - g[(size_t)r * 3 + a]) <= 2e-7)) return fail("round trip", R);
        if (env[(size_t)r * 3 + 2] != (double)l[3]) return fail("round trip speed", R);
    }
    // wide latent vectors: every output lies in [-1, 1]
    std::vector<float> u((size_t)R * 4);
    for (size_t k = 0; k < u.size(); k++) u[k] = (float)(6 * uniform() - 3);
    for (size_t k = 0; k < env.size(); k++) env[k] = 7.0;
    if (gauss_direction_map_host(R, u.data(), env.data())) return fail("map rc", R);
    for (size_t k = 0; k < env.size(); k++)
        if (!(env[k] >= -1.0 && env[k] <= 1.0)) return fail("map out of range or unwritten", R);
    return 0;
}

static int run_checks() {
    std::vector<float> u(4, 0.f), lab(4, 7.f);
    std::vector<double> g(3, 0.0), env(3, 7.0);
    int bad = 0;
    bad |= gauss_direction_map_host(1, nullptr, env.data()) != E3D_ERR_NULL || gauss_direction_map_host(1, u.data(), nullptr) != E3D_ERR_NULL;
    bad |= e3d_direction_label_host(1, nullptr, lab.data()) != E3D_ERR_NULL || e3d_direction_label_host(1, g.data(), nullptr) != E3D_ERR_NULL;
    bad |= gauss_direction_map_host(-1, u.data(), env.data()) != E3D_ERR_BAD_CONFIG || e3d_direction_label_host(-1, g.data(), lab.data()) != E3D_ERR_BAD_CONFIG;
    bad |= gauss_direction_map_host(0, u.data(), env.data()) != 0 || e3d_direction_label_host(0, g.data(), lab.data()) != 0;
    bad |= env[0] != 7.0 || lab[0] != 7.f;
    return bad ? fail("argument checks", 0) : 0;
}

int main() {
    int bad = run_edges() | run_checks();
    for (int R : {1, 7, 300}) bad |= run_random(R);
    if (!bad) printf("sanitize_direction_action: clean\n");
    return bad;
}
