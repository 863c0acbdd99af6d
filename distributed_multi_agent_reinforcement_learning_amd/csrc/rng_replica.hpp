// rng_replica.hpp -- bit-exact host replicas of the generator streams the reference environments draw from:
// CPython's random.Random (MT19937 + init_by_array seeding + _randbelow_with_getrandbits) and numpy's legacy
// RandomState (MT19937 + init_genrand seeding, random_sample, polar Box-Muller legacy_gauss with its cached value).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace rngrep {

struct MT19937 {
    uint32_t mt[624];
    int idx;
    void init_genrand(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = 624;
    }
    void init_by_array(const uint32_t *key, int len) {
        init_genrand(19650218u);
        int i = 1, j = 0;
        int k = 624 > len ? 624 : len;
        for (; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
            i++; j++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
            if (j >= len) j = 0;
        }
        for (k = 623; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            i++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000u;
        idx = 624;
    }
    uint32_t next() {
        if (idx >= 624) {
            for (int k = 0; k < 624; k++) {
                uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }
};

// CPython random.Random seeded with a non-negative int (Lib/random.py seed -> _randommodule.c init_by_array)
struct PyRandom {
    MT19937 g;
    void seed(uint64_t a) {
        uint32_t key[2] = {(uint32_t)a, (uint32_t)(a >> 32)};
        g.init_by_array(key, key[1] ? 2 : 1);
    }
    uint32_t getrandbits(int k) { return g.next() >> (32 - k); }  // 1 <= k <= 32
    uint32_t randbelow(uint32_t n) {                              // _randbelow_with_getrandbits
        int k = 0;
        for (uint32_t v = n; v; v >>= 1) k++;
        uint32_t r = getrandbits(k);
        while (r >= n) r = getrandbits(k);
        return r;
    }
    int randint(int a, int b) { return a + (int)randbelow((uint32_t)(b - a + 1)); }
};

// numpy.random.RandomState (legacy) seeded with a 32-bit int: rand(), normal()
struct NpRandom {
    MT19937 g;
    bool has_gauss = false;
    double gauss = 0.0;
    void seed(uint32_t s) { g.init_genrand(s); has_gauss = false; gauss = 0.0; }
    double random_sample() {
        uint32_t a = g.next() >> 5, b = g.next() >> 6;
        return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    }
    double legacy_gauss() {
        if (has_gauss) { has_gauss = false; double t = gauss; gauss = 0.0; return t; }
        double f, x1, x2, r2;
        do {
            x1 = 2.0 * random_sample() - 1.0;
            x2 = 2.0 * random_sample() - 1.0;
            r2 = x1 * x1 + x2 * x2;
        } while (r2 >= 1.0 || r2 == 0.0);
        f = sqrt(-2.0 * log(r2) / r2);
        gauss = f * x1;
        has_gauss = true;
        return f * x2;
    }
    double normal(double loc, double scale) { return loc + scale * legacy_gauss(); }
};

// Resume blobs: one NpRandom as a fixed little-endian record independent of struct padding -- the MT19937 key (624 x u32),
// its position (i32), has_gauss (i32, 0 or 1) and the cached gauss (f64).
constexpr size_t NP_RANDOM_STATE_BYTES = 624 * 4 + 4 + 4 + 8;

inline void np_random_pack(const NpRandom &r, unsigned char *out) {
    const int32_t idx = r.g.idx, hg = r.has_gauss ? 1 : 0;
    memcpy(out, r.g.mt, 624 * 4);
    memcpy(out + 624 * 4, &idx, 4);
    memcpy(out + 624 * 4 + 4, &hg, 4);
    memcpy(out + 624 * 4 + 8, &r.gauss, 8);
}

// false (r untouched) when the record cannot come from np_random_pack: position outside [0, 624] or has_gauss not 0 / 1
inline bool np_random_unpack(NpRandom &r, const unsigned char *in) {
    int32_t idx, hg;
    memcpy(&idx, in + 624 * 4, 4);
    memcpy(&hg, in + 624 * 4 + 4, 4);
    if (idx < 0 || idx > 624 || (hg != 0 && hg != 1)) return false;
    memcpy(r.g.mt, in, 624 * 4);
    r.g.idx = idx;
    r.has_gauss = hg != 0;
    memcpy(&r.gauss, in + 624 * 4 + 8, 8);
    return true;
}

// Header of a resetter's state blob (n2n_resetter_get_state, e3d_resetter_get_state): a format tag and the shape it was taken
// from; the NpRandom records of environments 0 .. N-1 follow.
struct ResetterStateHeader {
    uint32_t tag;
    int32_t N, P, E;
};

inline int64_t resetter_state_bytes(int N) { return (int64_t)sizeof(ResetterStateHeader) + (int64_t)N * (int64_t)NP_RANDOM_STATE_BYTES; }

inline void resetter_state_get(const ResetterStateHeader &h, const NpRandom *rng, void *out) {
    unsigned char *o = (unsigned char *)out;
    memcpy(o, &h, sizeof(h));
    for (int n = 0; n < h.N; n++) np_random_pack(rng[n], o + sizeof(h) + (size_t)n * NP_RANDOM_STATE_BYTES);
}

// all or nothing: false (rng untouched) when the blob's header is not `want` or one of its records is malformed
inline bool resetter_state_set(const ResetterStateHeader &want, NpRandom *rng, const void *in) {
    const unsigned char *b = (const unsigned char *)in;
    ResetterStateHeader h;
    memcpy(&h, b, sizeof(h));
    if (h.tag != want.tag || h.N != want.N || h.P != want.P || h.E != want.E) return false;
    NpRandom probe;
    for (int n = 0; n < h.N; n++)
        if (!np_random_unpack(probe, b + sizeof(h) + (size_t)n * NP_RANDOM_STATE_BYTES)) return false;
    for (int n = 0; n < h.N; n++) np_random_unpack(rng[n], b + sizeof(h) + (size_t)n * NP_RANDOM_STATE_BYTES);
    return true;
}

}  // namespace rngrep
