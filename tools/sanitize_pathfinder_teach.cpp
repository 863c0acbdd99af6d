// Stand-alone sanitizer driver of the host side of the pathfinder's teacher launch (pe_pursuer_pathfinder_teach_host of csrc/pe_env.hip
// over csrc/pe_pathfinder.hpp).  It needs no GPU and no Python: build it together with the library's source and
// run it,
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -pthread -Iinclude -I<package>/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -fsanitize=address,undefined \
//         <package>/csrc/pe_env.hip <package>/csrc/pe_reset.cpp tools/sanitize_pathfinder_teach.cpp -o sanitize_pathfinder_teach \
//     && ./sanitize_pathfinder_teach
// Every array is a heap block of exactly the size the ABI names, so a read or write past a grid, a record, a cached field, a key or a
// label row is a report.  W x H = 5 x 7 and 40 x 40, P = 2, 9, 16; the sequence empty cache -> hit -> moved evader against the plain
// host twin every time; a_star through a stride greater than P with the gaps left alone; follow over half of the environments; every
// refused argument without a write.  Exit status 0: clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pe_env.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, (0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

static int fail(const char *what, int W, int H, int P) {
    fprintf(stderr, "FAILED: %s (%d x %d, P %d)\n", what, W, H, P);
    return 1;
}

static pe_config config(int W, int H, int P) {
    pe_config c;
    memset(&c, 0, sizeof c);
    c.W = W; c.H = H; c.P = P;
    c.def_tau = 0.2; c.def_dt = 0.1; c.def_collision_radius = 0.5;
    for (int k = 0; k < 8; k++) { c.action_u[k][0] = 2.0 * cos(k * M_PI / 4); c.action_u[k][1] = 2.0 * sin(k * M_PI / 4); }
    return c;
}

static int run(int W, int H, int P) {
    const int N = 6, WH = W * H, STRIDE = P + 5;
    const pe_config c = config(W, H, P);
    std::vector<uint8_t> grid((size_t)N * WH), follow(N);
    std::vector<double> def((size_t)N * 4 * P), eva((size_t)N * 4);
    for (auto &g : grid) g = uniform() < 0.15;
    for (int n = 0; n < N; n++) {
        follow[n] = n < N / 2;
        for (int i = 0; i < P; i++) {
            def[((size_t)n * 4 + 0) * P + i] = uniform() * (W - 1);
            def[((size_t)n * 4 + 1) * P + i] = uniform() * (H - 1);
            def[((size_t)n * 4 + 2) * P + i] = 4 * uniform() - 2;
            def[((size_t)n * 4 + 3) * P + i] = 4 * uniform() - 2;
        }
        eva[(size_t)n * 4 + 0] = 1 + floor(uniform() * (W - 2));     // on a cell centre off the border: the moves below are exact
        eva[(size_t)n * 4 + 1] = 1 + floor(uniform() * (H - 2));
        eva[(size_t)n * 4 + 2] = 2 * uniform() - 1;
        eva[(size_t)n * 4 + 3] = 2 * uniform() - 1;
    }
    std::vector<int32_t> field((size_t)N * WH, -11), key((size_t)N * 2, -1), hits(N, 0), action((size_t)N * P), actions((size_t)N * P),
        plain((size_t)N * P), dfield((size_t)N * WH), pfield((size_t)N * WH), kstar((size_t)N * P), pkstar((size_t)N * P);
    std::vector<uint16_t> blocked((size_t)N * P), pblocked((size_t)N * P);
    std::vector<float> a_star((size_t)(N - 1) * STRIDE + P);        // the last environment's row ends the block
    const pe_pathfinder_cache ca = {field.data(), key.data(), hits.data()};
    const pe_pathfinder_label lb = {follow.data(), action.data(), a_star.data(), STRIDE};
    const pe_pathfinder_diag dg = {dfield.data(), kstar.data(), blocked.data()}, pdg = {pfield.data(), pkstar.data(), pblocked.data()};
    // empty cache -> hit -> moved evader (a neighbouring cell in the even environments, inside the cell in the odd ones)
    for (int step = 0; step < 3; step++) {
        if (step == 2)
            for (int n = 0; n < N; n++) eva[(size_t)n * 4] += (n & 1) ? 0.25 : 1.0;
        for (auto &a : action) a = 7;
        for (auto &a : a_star) a = -2.0f;
        if (pe_pursuer_pathfinder_host(&c, N, grid.data(), def.data(), eva.data(), nullptr, plain.data(), &pdg)) return fail("plain twin", W, H, P);
        if (pe_pursuer_pathfinder_teach_host(&c, N, grid.data(), def.data(), eva.data(), nullptr, &ca, &lb, actions.data(), &dg))
            return fail("teach twin", W, H, P);
        if (actions != plain || dfield != pfield || kstar != pkstar || blocked != pblocked) return fail("teach != plain", W, H, P);
        if (field != pfield) return fail("cached field", W, H, P);
        for (int n = 0; n < N; n++) {
            const int want = step == 0 ? 0 : (step == 1 ? 1 : ((n & 1) ? 2 : 1));
            if (hits[n] != want) return fail("hit count", W, H, P);
            if (key[2 * n] != (int)eva[(size_t)n * 4] * H + (int)eva[(size_t)n * 4 + 1] || key[2 * n + 1] != 10) return fail("key", W, H, P);
            for (int i = 0; i < P; i++) {
                if (a_star[(size_t)n * STRIDE + i] != (float)plain[(size_t)n * P + i]) return fail("a_star", W, H, P);
                if (action[(size_t)n * P + i] != (follow[n] ? plain[(size_t)n * P + i] : 7)) return fail("follow", W, H, P);
            }
            for (int i = P; i < STRIDE && n + 1 < N; i++)
                if (a_star[(size_t)n * STRIDE + i] != -2.0f) return fail("a_star gap", W, H, P);
        }
    }
    // no cache, no labels, no actions: only diag is written
    if (pe_pursuer_pathfinder_teach_host(&c, N, grid.data(), def.data(), eva.data(), nullptr, nullptr, nullptr, nullptr, &dg)) return fail("all NULL", W, H, P);
    if (dfield != pfield) return fail("all NULL field", W, H, P);
    // every refused argument, without a write
    const auto f0 = field, k0 = key, h0 = hits, ac0 = action, as0 = actions;
    const auto s0 = a_star;
    pe_pathfinder_params bad = {0.5, 1.0, 1001, 0};
    pe_config big = c;
    big.W = 91; big.H = 91;
    const pe_pathfinder_label short_stride = {follow.data(), action.data(), a_star.data(), P - 1}, no_action = {follow.data(), nullptr, a_star.data(), STRIDE};
    const pe_pathfinder_cache no_field = {nullptr, key.data(), hits.data()}, no_key = {field.data(), nullptr, hits.data()};
    int rc[6];
    rc[0] = pe_pursuer_pathfinder_teach_host(&c, N, grid.data(), def.data(), eva.data(), &bad, &ca, &lb, actions.data(), nullptr);
    rc[1] = pe_pursuer_pathfinder_teach_host(&big, N, grid.data(), def.data(), eva.data(), nullptr, &ca, &lb, actions.data(), nullptr);
    rc[2] = pe_pursuer_pathfinder_teach_host(&c, N, grid.data(), def.data(), eva.data(), nullptr, &ca, &short_stride, actions.data(), nullptr);
    rc[3] = pe_pursuer_pathfinder_teach_host(&c, N, grid.data(), def.data(), eva.data(), nullptr, &ca, &no_action, actions.data(), nullptr);
    rc[4] = pe_pursuer_pathfinder_teach_host(&c, N, grid.data(), def.data(), eva.data(), nullptr, &no_field, &lb, actions.data(), nullptr);
    rc[5] = pe_pursuer_pathfinder_teach_host(&c, N, grid.data(), def.data(), eva.data(), nullptr, &no_key, &lb, actions.data(), nullptr);
    const int want[6] = {PE_ERR_BAD_CONFIG, PE_ERR_BAD_CONFIG, PE_ERR_BAD_CONFIG, PE_ERR_NULL, PE_ERR_NULL, PE_ERR_NULL};
    for (int k = 0; k < 6; k++)
        if (rc[k] != want[k]) return fail("refusal code", W, H, k);
    if (field != f0 || key != k0 || hits != h0 || action != ac0 || actions != as0 || a_star != s0) return fail("a refused call wrote", W, H, P);
    return 0;
}

int main() {
    const int sizes[2][2] = {{5, 7}, {40, 40}}, teams[3] = {2, 9, 16};
    for (auto &s : sizes)
        for (int P : teams)
            if (run(s[0], s[1], P)) return 1;
    printf("sanitize_pathfinder_teach: clean\n");
    return 0;
}
