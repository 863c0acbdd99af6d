// Stand-alone sanitizer driver of the host side of the env_3d actor's team attention (csrc/team_attention.hpp: team_comm_mask_host,
// team_attention_fwd_host, team_attention_bwd_host).  It needs no GPU and no Python: this file includes the
// header as csrc/mappo_ops.hip does, so one translation unit is the whole program,
//   hipcc --offload-arch=gfx950 -x hip -O1 -g -std=c++17 -Iinclude -I<package>/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -fsanitize=address,undefined \
//         tools/sanitize_team_attention.cpp -o sanitize_team_attention && ./sanitize_team_attention
// Every array is a heap block of exactly the size the ABI names, so a read or write past a row, a word or an lse plane is a report.
// P = 1, 8, 9, 64, H = 1, 2, 4, 8, G = 3, random words with garbage bits at or above P and a self-only group: finite outputs, every
// element written, the self-only group returns v, d_v = d_out and d_q = d_k = 0; P = 0, 65, H = 3, G = -1 and null pointers refused
// with nothing written.  Exit status 0: clean.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mappo_ops.h"
#include "team_attention.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t bits64() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static float uniform() { return (float)((double)(bits64() >> 11) / 9007199254740992.0 * 2.0 - 1.0); }

static int fail(const char *what, int P, int H) {
    fprintf(stderr, "FAILED: %s (P %d, H %d)\n", what, P, H);
    return 1;
}

static const float MARK = 7.f;

static int run(int P, int H) {
    const int G = 3;
    const size_t R = (size_t)G * P;
    std::vector<float> adj((size_t)G * P * P), live(R), qkv(R * 384), out(R * 128, MARK), lse((size_t)G * H * P, MARK), d_out(R * 128), d_qkv(R * 384, MARK);
    std::vector<int64_t> words(R, -1);
    for (float &v : adj) v = uniform() < 0.3f;
    for (float &v : live) v = uniform() < 0.6f;
    for (float &v : qkv) v = uniform();
    for (float &v : d_out) v = uniform();
    if (team_comm_mask_host(G, P, adj.data(), (int64_t)P * P, live.data(), P, words.data(), P)) return fail("mask rc", P, H);
    for (int g = 0; g < G; g++)
        for (int i = 0; i < P; i++) {
            const uint64_t w = (uint64_t)words[(size_t)g * P + i];
            if (!((w >> i) & 1) || (P < 64 && (w >> P))) return fail("mask word", P, H);
            for (int j = 0; j < P; j++)
                if (((w >> j) & 1) != (((uint64_t)words[(size_t)g * P + j] >> i) & 1)) return fail("mask not symmetric", P, H);
        }
    for (int g = 0; g < G; g++)
        for (int i = 0; i < P; i++) {
            if (g == 1) words[(size_t)g * P + i] = (int64_t)(1ull << i);                       // a self-only group
            else if (P < 64) words[(size_t)g * P + i] |= (int64_t)(bits64() << P);             // garbage at or above P
        }
    if (team_attention_fwd_host(G, P, H, qkv.data(), words.data(), out.data(), lse.data())) return fail("fwd rc", P, H);
    if (team_attention_fwd_host(G, P, H, qkv.data(), words.data(), out.data(), nullptr)) return fail("fwd rc without lse", P, H);
    if (team_attention_bwd_host(G, P, H, qkv.data(), words.data(), lse.data(), d_out.data(), d_qkv.data())) return fail("bwd rc", P, H);
    for (float v : out) if (!isfinite(v) || v == MARK) return fail("out", P, H);
    for (float v : lse) if (!isfinite(v) || v == MARK) return fail("lse", P, H);
    for (float v : d_qkv) if (!isfinite(v) || v == MARK) return fail("d_qkv", P, H);
    for (int i = 0; i < P; i++)
        for (int k = 0; k < 128; k++) {
            const size_t r = (size_t)P + i;
            if (out[r * 128 + k] != qkv[r * 384 + 256 + k]) return fail("self-only out != v", P, H);
            if (d_qkv[r * 384 + 256 + k] != d_out[r * 128 + k]) return fail("self-only d_v != d_out", P, H);
            if (d_qkv[r * 384 + k] != 0.f || d_qkv[r * 384 + 128 + k] != 0.f) return fail("self-only d_q, d_k != 0", P, H);
        }
    return 0;
}

static int refused() {
    std::vector<float> qkv(384, 1.f), out(128, MARK), lse(8, MARK), d_out(128, 1.f), d_qkv(384, MARK), adj(1, 1.f), live(1, 1.f);
    std::vector<int64_t> words(1, 1);
    int bad = 0;
    const int PH[][2] = {{0, 4}, {65, 4}, {8, 3}, {8, 0}, {8, 16}};
    for (auto &ph : PH) {
        bad |= team_attention_fwd_host(1, ph[0], ph[1], qkv.data(), words.data(), out.data(), lse.data()) != MO_ERR_BAD_ARG;
        bad |= team_attention_bwd_host(1, ph[0], ph[1], qkv.data(), words.data(), lse.data(), d_out.data(), d_qkv.data()) != MO_ERR_BAD_ARG;
    }
    bad |= team_attention_fwd_host(-1, 1, 1, qkv.data(), words.data(), out.data(), lse.data()) != MO_ERR_BAD_ARG;
    bad |= team_attention_fwd_host(1, 1, 1, nullptr, words.data(), out.data(), lse.data()) != MO_ERR_BAD_ARG;
    bad |= team_attention_fwd_host(1, 1, 1, qkv.data(), nullptr, out.data(), lse.data()) != MO_ERR_BAD_ARG;
    bad |= team_attention_fwd_host(1, 1, 1, qkv.data(), words.data(), nullptr, lse.data()) != MO_ERR_BAD_ARG;
    bad |= team_attention_bwd_host(1, 1, 1, qkv.data(), words.data(), nullptr, d_out.data(), d_qkv.data()) != MO_ERR_BAD_ARG;
    bad |= team_attention_bwd_host(1, 1, 1, qkv.data(), words.data(), lse.data(), d_out.data(), nullptr) != MO_ERR_BAD_ARG;
    bad |= team_comm_mask_host(1, 65, adj.data(), 65 * 65, live.data(), 65, words.data(), 65) != MO_ERR_BAD_ARG;
    bad |= team_comm_mask_host(1, 1, adj.data(), 0, live.data(), 1, words.data(), 1) != MO_ERR_BAD_ARG;
    bad |= team_comm_mask_host(1, 1, nullptr, 1, live.data(), 1, words.data(), 1) != MO_ERR_BAD_ARG;
    bad |= team_attention_fwd_host(0, 1, 1, qkv.data(), words.data(), out.data(), lse.data()) != 0;     // G = 0 succeeds, nothing written
    bad |= team_attention_bwd_host(0, 1, 1, qkv.data(), words.data(), lse.data(), d_out.data(), d_qkv.data()) != 0;
    for (float v : out) bad |= v != MARK;
    for (float v : lse) bad |= v != MARK;
    for (float v : d_qkv) bad |= v != MARK;
    bad |= words[0] != 1;
    return bad ? fail("a refused call was accepted or wrote", 0, 0) : 0;
}

int main() {
    int bad = 0;
    for (int P : {1, 8, 9, 64})
        for (int H : {1, 2, 4, 8}) bad |= run(P, H);
    bad |= refused();
    if (!bad) printf("sanitize_team_attention: clean\n");
    return bad;
}
