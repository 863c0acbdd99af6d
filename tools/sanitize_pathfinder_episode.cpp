// Stand-alone sanitizer driver of the host side of the episode labeller (pe_pathfinder_label_episode_host and pe_env_record_state_host
// of csrc/pe_env.hip over csrc/pe_pathfinder.hpp).  It needs no GPU and no Python: build it together with the
// library's source and run it,
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -pthread -Iinclude -I<package>/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -fsanitize=address,undefined \
//         <package>/csrc/pe_env.hip <package>/csrc/pe_reset.cpp tools/sanitize_pathfinder_episode.cpp -o sanitize_pathfinder_episode \
//     && ./sanitize_pathfinder_episode
// Every array is a heap block of exactly the size the ABI names: the trace and a_star are strided views whose last record ends the
// block, so a read or write past a grid, a record, a label row or builds is a report.  W x H = 5 x 7 and 40 x 40, P = 2, 9, 16, T = 1
// and 6; the states go into the trace through pe_env_record_state_host tick by tick, the labels are compared with the per-tick host twin on
// every tick, builds with the count of cell changes, the gaps of every stride stay as filled, and every refused argument returns
// without a write.  Exit status 0: clean.
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

static int run(int W, int H, int P, int T) {
    const int N = 4, WH = W * H;
    // strides above one record; the last record of the last environment ends each block
    const int64_t d_tick = 4 * P + 3, d_env = d_tick * T + 5, e_tick = 7, e_env = e_tick * T + 2, a_tick = P + 1, a_env = a_tick * T + 4;
    const pe_config c = config(W, H, P);
    std::vector<uint8_t> grid((size_t)N * WH);
    for (auto &g : grid) g = uniform() < 0.15;
    std::vector<double> tdef((size_t)((N - 1) * d_env + (T - 1) * d_tick + 4 * P), 1e9), teva((size_t)((N - 1) * e_env + (T - 1) * e_tick + 4), 1e9);
    std::vector<float> a_star((size_t)((N - 1) * a_env + (T - 1) * a_tick + P), -2.0f);
    std::vector<int32_t> builds(N, -1), want_builds(N, 0), plain((size_t)N * P), dfield((size_t)N * WH, -5), pfield((size_t)N * WH), kstar((size_t)N * P),
        pkstar((size_t)N * P), last_cell(N, -1);
    std::vector<uint16_t> blocked((size_t)N * P), pblocked((size_t)N * P);
    std::vector<float> want((size_t)N * T * P);
    std::vector<double> def((size_t)N * 4 * P), eva((size_t)N * 4), ex(N), ey(N);
    const pe_pathfinder_diag dg = {dfield.data(), kstar.data(), blocked.data()}, pdg = {pfield.data(), pkstar.data(), pblocked.data()};
    for (int n = 0; n < N; n++) { ex[n] = 1 + floor(uniform() * (W - 2)); ey[n] = 1 + floor(uniform() * (H - 2)); }
    for (int t = 0; t < T; t++) {
        for (int n = 0; n < N; n++) {
            for (int i = 0; i < P; i++) {
                def[((size_t)n * 4 + 0) * P + i] = uniform() * (W - 1);
                def[((size_t)n * 4 + 1) * P + i] = uniform() * (H - 1);
                def[((size_t)n * 4 + 2) * P + i] = 4 * uniform() - 2;
                def[((size_t)n * 4 + 3) * P + i] = 4 * uniform() - 2;
            }
            // the evader: inside its cell (t = 1, 2), the neighbouring cell (3), back (4), outside the map (5)
            double x = ex[n], y = ey[n];
            if (t == 1 || t == 2) x += 0.25 * t - 0.375;
            if (t == 3) x += (x + 1 <= W - 1) ? 1.0 : -1.0;
            if (t == 5) { x = -0.75; y = H + 1.5; }
            eva[(size_t)n * 4 + 0] = x; eva[(size_t)n * 4 + 1] = y;
            eva[(size_t)n * 4 + 2] = 2 * uniform() - 1; eva[(size_t)n * 4 + 3] = 2 * uniform() - 1;
            const int cx = x < 0 ? 0 : (int)nearbyint(x), cy = y > H - 1 ? H - 1 : (int)nearbyint(y), cell = cx * H + cy;
            want_builds[n] += cell != last_cell[n];
            last_cell[n] = cell;
        }
        if (pe_env_record_state_host(&c, N, def.data(), eva.data(), tdef.data() + t * d_tick, d_env, teva.data() + t * e_tick, e_env))
            return fail("record_state", W, H, P);
        if (pe_pursuer_pathfinder_host(&c, N, grid.data(), def.data(), eva.data(), nullptr, plain.data(), &pdg)) return fail("plain twin", W, H, P);
        for (int n = 0; n < N; n++)
            for (int i = 0; i < P; i++) want[((size_t)n * T + t) * P + i] = (float)plain[(size_t)n * P + i];
    }
    const pe_pathfinder_trace tr = {tdef.data(), d_env, d_tick, teva.data(), e_env, e_tick, T, 0};
    if (pe_pathfinder_label_episode_host(&c, N, grid.data(), nullptr, &tr, a_star.data(), a_env, a_tick, builds.data(), &dg)) return fail("episode twin", W, H, P);
    if (builds != want_builds) return fail("builds", W, H, P);
    if (dfield != pfield || kstar != pkstar || blocked != pblocked) return fail("last tick's diag", W, H, P);
    for (size_t j = 0; j < a_star.size(); j++) {
        const int64_t n = j / a_env, r = j % a_env, t = r / a_tick, i = r % a_tick;
        const bool label = t < T && i < P;
        if (a_star[j] != (label ? want[((size_t)n * T + t) * P + i] : -2.0f)) return fail(label ? "a_star" : "a_star gap", W, H, P);
    }
    for (size_t j = 0; j < tdef.size(); j++) {
        const int64_t r = j % d_env, t = r / d_tick, i = r % d_tick;
        if (!(t < T && i < 4 * P) && tdef[j] != 1e9) return fail("trace def gap", W, H, P);
    }
    for (size_t j = 0; j < teva.size(); j++) {
        const int64_t r = j % e_env, t = r / e_tick, i = r % e_tick;
        if (!(t < T && i < 4) && teva[j] != 1e9) return fail("trace eva gap", W, H, P);
    }
    // builds and diag NULL: the same labels
    const auto labels = a_star;
    if (pe_pathfinder_label_episode_host(&c, N, grid.data(), nullptr, &tr, a_star.data(), a_env, a_tick, nullptr, nullptr) || a_star != labels)
        return fail("builds / diag NULL", W, H, P);
    // every refused argument, without a write
    const auto b0 = builds, f0 = dfield;
    const auto d0 = tdef, e0 = teva;
    pe_pathfinder_params bad = {0.5, 1.0, 1001, 0};
    pe_config big = c;
    big.W = 91; big.H = 91;
    pe_pathfinder_trace t0 = tr, no_def = tr, no_eva = tr, s1 = tr, s2 = tr, s3 = tr, s4 = tr;
    t0.T = 0; no_def.def = nullptr; no_eva.eva = nullptr;
    s1.def_env_stride = 4 * P - 1; s2.def_tick_stride = 4 * P - 1; s3.eva_env_stride = 3; s4.eva_tick_stride = 3;
    struct { const pe_config *cfg; const pe_pathfinder_params *prm; const pe_pathfinder_trace *tr; float *a; int64_t ae, at; const uint8_t *g; int want; } calls[] = {
        {&c, &bad, &tr, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_BAD_CONFIG}, {&big, nullptr, &tr, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_BAD_CONFIG},
        {&c, nullptr, &t0, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_BAD_CONFIG}, {&c, nullptr, nullptr, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_NULL},
        {&c, nullptr, &no_def, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_NULL}, {&c, nullptr, &no_eva, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_NULL},
        {&c, nullptr, &tr, nullptr, a_env, a_tick, grid.data(), PE_ERR_NULL}, {&c, nullptr, &tr, a_star.data(), a_env, a_tick, nullptr, PE_ERR_NULL},
        {&c, nullptr, &tr, a_star.data(), P - 1, a_tick, grid.data(), PE_ERR_BAD_CONFIG}, {&c, nullptr, &tr, a_star.data(), a_env, P - 1, grid.data(), PE_ERR_BAD_CONFIG},
        {&c, nullptr, &s1, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_BAD_CONFIG}, {&c, nullptr, &s2, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_BAD_CONFIG},
        {&c, nullptr, &s3, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_BAD_CONFIG}, {&c, nullptr, &s4, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_BAD_CONFIG},
        {nullptr, nullptr, &tr, a_star.data(), a_env, a_tick, grid.data(), PE_ERR_NULL}};
    int k = 0;
    for (auto &q : calls) {
        if (pe_pathfinder_label_episode_host(q.cfg, N, q.g, q.prm, q.tr, q.a, q.ae, q.at, builds.data(), &dg) != q.want) return fail("refusal code", W, H, k);
        k++;
    }
    if (pe_env_record_state_host(&c, N, def.data(), eva.data(), nullptr, d_env, teva.data(), e_env) != PE_ERR_NULL ||
        pe_env_record_state_host(&c, N, def.data(), eva.data(), tdef.data(), d_env, nullptr, e_env) != PE_ERR_NULL ||
        pe_env_record_state_host(&c, N, nullptr, eva.data(), tdef.data(), d_env, teva.data(), e_env) != PE_ERR_NULL ||
        pe_env_record_state_host(&c, N, def.data(), eva.data(), tdef.data(), 4 * P - 1, teva.data(), e_env) != PE_ERR_BAD_CONFIG ||
        pe_env_record_state_host(&c, N, def.data(), eva.data(), tdef.data(), d_env, teva.data(), 3) != PE_ERR_BAD_CONFIG)
        return fail("record_state refusal code", W, H, P);
    if (builds != b0 || dfield != f0 || a_star != labels || tdef != d0 || teva != e0) return fail("a refused call wrote", W, H, P);
    return 0;
}

int main() {
    const int sizes[2][2] = {{5, 7}, {40, 40}}, teams[3] = {2, 9, 16}, ticks[2] = {1, 6};
    for (auto &s : sizes)
        for (int P : teams)
            for (int T : ticks)
                if (run(s[0], s[1], P, T)) return 1;
    printf("sanitize_pathfinder_episode: clean\n");
    return 0;
}
