// team_attention.hpp -- algo.e3d_comm: attention of the env_3d trainer: one round of masked multi-head attention between the embeddings
// of the pursuers of one environment at one tick (C ABI: include/mappo_ops.h team_comm_mask / team_attention_fwd / team_attention_bwd;
// DESIGN.md section 7m; specification: tests/team_attention_ref.py).  Included once, from csrc/mappo_ops.hip.
//
// A group is P consecutive rows of qkv (G P, 384) = q | k | v, 128 columns each; head h is columns [h D, (h + 1) D), D = 128 / H.
// Lane layout (both kernels): a workgroup of 256 lanes is 8 row slots of 32 lanes; lane c of a slot owns columns [4 c, 4 c + 4) of its
// row, so a head is 32 / H neighbouring lanes and a dot product over a head is 4 fused multiply-adds and an xor butterfly over those
// lanes (every lane of the head ends with the same bits).  A workgroup takes a tile of TILE / P whole groups (TILE rows of LDS), so a
// group never spans workgroups, and every sum over team-mates runs over j (or i) = 0 .. P - 1 in that order inside one lane: the
// result of a group depends on nothing but its own rows and words.  No atomics.
// Forward: k and v of the tile go to LDS once (16-byte loads), a slot holds its query row in registers and runs the online softmax
// (soft_step) over the keys.  Backward: q, k, v and d_out of the tile go to LDS once; pass A has a slot per query (delta, dQ), pass B a
// slot per key (dK, dV); both recompute the probabilities as exp(s - lse).
// Every fused multiply-add is written as fmaf and contraction is off in every function: s - m, s - lse and dp - delta are differences of
// the rounded values, the same bits in the forward and in both backward passes (a lone key gives exp(0) = 1 and dp - delta = 0 exactly).
#pragma once
#include <math.h>
#include <stdint.h>

namespace tatt {

constexpr int E = 128, ROW = 3 * E, C4 = E / 4, MAX_P = 64, SLOTS = 8;
constexpr int fwd_tile(int PT) { return PT <= 32 ? 32 : 64; }   // rows of k | v in LDS: 32 or 64 KB
constexpr int bwd_tile(int PT) { return PT <= 16 ? 16 : PT; }   // rows of q | k | v | d_out in LDS: 32, 64 or 128 KB

__host__ __device__ inline bool heads_ok(int H) { return H == 1 || H == 2 || H == 4 || H == 8; }

// the hearing set M_i of pursuer i as a word: bit j iff j == i, or both are live and each is in the other's communication range
__host__ __device__ inline uint64_t comm_word(int P, int i, const float *adj /* [P][P] */, const float *live /* [P] */) {
    uint64_t w = 0;
    if (live[i] != 0.f)
        for (int j = 0; j < P; j++)
            if (live[j] != 0.f && adj[i * P + j] != 0.f && adj[j * P + i] != 0.f) w |= 1ull << j;
    return w | (1ull << i);
}

// what a kernel reads of a stored word: bits at or above P dropped, bit i taken as set (a query always hears itself)
__host__ __device__ inline uint64_t query_word(uint64_t w, int P, int i) { return (P >= 64 ? w : w & ((1ull << P) - 1)) | (1ull << i); }

// a lane's part of a dot product: its four columns, in this order
__host__ __device__ inline float dot4(const float4 a, const float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }

// one key of the online softmax of a (query, head): the running maximum m (-inf before the first key), the sum l of exp(s - m) and
// the lane's four columns of sum exp(s - m) v.  A single key leaves l = 1 and acc = v exactly.
__host__ __device__ inline void soft_step(float s, const float4 v, float &m, float &l, float4 &acc) {
#pragma clang fp contract(off)
    const float mn = fmaxf(m, s);
    const float c = expf(m - mn), p = expf(s - mn);
    l = fmaf(l, c, p);
    acc.x = fmaf(acc.x, c, p * v.x);
    acc.y = fmaf(acc.y, c, p * v.y);
    acc.z = fmaf(acc.z, c, p * v.z);
    acc.w = fmaf(acc.w, c, p * v.w);
    m = mn;
}

__host__ __device__ inline void axpy4(float4 &y, float a, const float4 x) {
    y.x = fmaf(a, x.x, y.x);
    y.y = fmaf(a, x.y, y.y);
    y.z = fmaf(a, x.z, y.z);
    y.w = fmaf(a, x.w, y.w);
}

__host__ __device__ inline float head_scale(int H) { return 1.0f / sqrtf((float)(E / H)); }

// the butterfly over the 32 / H lanes of a head
template <int H>
__device__ inline float head_sum(float s) {
#pragma unroll
    for (int off = 1; off < 32 / H; off <<= 1) s += __shfl_xor(s, off);
    return s;
}

__global__ __launch_bounds__(256) void k_team_comm_mask(int64_t n, int P, const float *__restrict__ adj, int64_t adj_stride, const float *__restrict__ live,
                                                        int64_t live_stride, int64_t *__restrict__ words, int64_t words_stride) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t g = r / P;
    const int i = (int)(r - g * P);
    words[g * words_stride + i] = (int64_t)comm_word(P, i, adj + g * adj_stride, live + g * live_stride);
}

template <int PT, int H>
__global__ __launch_bounds__(256) void k_team_attention_fwd(int64_t G, int P, const float *__restrict__ qkv, const int64_t *__restrict__ words,
                                                            float *__restrict__ out, float *__restrict__ lse) {
#pragma clang fp contract(off)
    constexpr int TILE = fwd_tile(PT), HL = 32 / H, UF = PT <= 16 ? PT : 8 /* keys of one unrolled trip */;
    __shared__ float4 kv[TILE * 2 * C4];   // [row][k: 32 lanes | v: 32 lanes]
    const int gpt = TILE / P;              // whole groups of a tile
    const int64_t g0 = (int64_t)blockIdx.x * gpt;
    const int ng = (int)(G - g0 < gpt ? G - g0 : gpt);
    const int nrows = ng * P;
    const float4 *src = (const float4 *)(qkv + g0 * P * ROW);
    for (int idx = threadIdx.x; idx < nrows * 2 * C4; idx += 256) kv[idx] = src[(idx >> 6) * (ROW / 4) + C4 + (idx & 63)];
    __syncthreads();
    const int slot = threadIdx.x >> 5, c = threadIdx.x & 31;
    const float scale = head_scale(H);
    for (int base = 0; base < nrows; base += SLOTS) {   // (a slot past the last row repeats it and stores nothing: no lane leaves the butterflies)
        const bool valid = base + slot < nrows;
        const int lr = valid ? base + slot : nrows - 1;
        const int gl = lr / P, i = lr - gl * P;
        const float4 q = src[lr * (ROW / 4) + c];
        const uint64_t w = query_word((uint64_t)words[(g0 + gl) * P + i], P, i);
        const float4 *kr = kv + gl * P * 2 * C4;
        float m = -INFINITY, l = 0.f;
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < P; j0 += UF) {   // (UF keys a trip, the ones at or above P on row P - 1 with their bit clear)
#pragma unroll
            for (int u = 0; u < UF; u++) {
                const int j = j0 + u, jj = j < P ? j : P - 1;
                const float s = head_sum<H>(dot4(q, kr[jj * 2 * C4 + c])) * scale;
                if ((w >> j) & 1) soft_step(s, kr[jj * 2 * C4 + C4 + c], m, l, acc);
            }
        }
        if (!valid) continue;
        const float inv = 1.0f / l;
        ((float4 *)(out + (g0 * P + lr) * E))[c] = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
        if (lse && (c & (HL - 1)) == 0) lse[((g0 + gl) * H + c / HL) * P + i] = m + logf(l);
    }
}

template <int PT, int H>
__global__ __launch_bounds__(256) void k_team_attention_bwd(int64_t G, int P, const float *__restrict__ qkv, const int64_t *__restrict__ words,
                                                            const float *__restrict__ lse, const float *__restrict__ d_out, float *__restrict__ d_qkv) {
#pragma clang fp contract(off)
    constexpr int TILE = bwd_tile(PT), HL = 32 / H, UF = PT <= 16 ? PT : 8 /* keys of one unrolled trip */, RS = 4 * C4;   // an LDS row: q | k | v | d_out, 32 lanes each
    __shared__ float4 rows[TILE * RS];
    __shared__ float lse_s[TILE * H], delta_s[TILE * H];             // [group of the tile][head][pursuer], as lse itself
    __shared__ uint64_t word_s[TILE];
    const int gpt = TILE / P;
    const int64_t g0 = (int64_t)blockIdx.x * gpt;
    const int ng = (int)(G - g0 < gpt ? G - g0 : gpt);
    const int nrows = ng * P;
    const float4 *src = (const float4 *)(qkv + g0 * P * ROW), *dsrc = (const float4 *)(d_out + g0 * P * E);
    for (int idx = threadIdx.x; idx < nrows * RS; idx += 256) {
        const int r = idx >> 7, k = idx & 127;
        rows[idx] = k < 3 * C4 ? src[r * (ROW / 4) + k] : dsrc[r * C4 + k - 3 * C4];
    }
    for (int idx = threadIdx.x; idx < nrows * H; idx += 256) lse_s[idx] = lse[g0 * H * P + idx];
    for (int idx = threadIdx.x; idx < nrows; idx += 256) word_s[idx] = query_word((uint64_t)words[g0 * P + idx], P, idx % P);
    __syncthreads();
    const int slot = threadIdx.x >> 5, c = threadIdx.x & 31, h = c / HL;
    const float scale = head_scale(H);
    float4 *dst = (float4 *)(d_qkv + g0 * P * ROW);
    // pass A, a slot per query i: delta_i = dO_i . sum_j a_ij v_j per head, then dQ_i = sum_j a_ij (dO_i . v_j - delta_i) k_j / sqrt(D)
    for (int base = 0; base < nrows; base += SLOTS) {
        const bool valid = base + slot < nrows;
        const int lr = valid ? base + slot : nrows - 1;
        const int gl = lr / P, i = lr - gl * P;
        const float4 q = rows[lr * RS + c], go = rows[lr * RS + 3 * C4 + c];
        const uint64_t w = word_s[lr];
        const float ls = lse_s[(gl * H + h) * P + i];
        const float4 *gr = rows + gl * P * RS;
        float4 o = {0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < P; j0 += UF) {
#pragma unroll
            for (int u = 0; u < UF; u++) {
                const int j = j0 + u, jj = j < P ? j : P - 1;
                const float s = head_sum<H>(dot4(q, gr[jj * RS + C4 + c])) * scale;
                if ((w >> j) & 1) axpy4(o, expf(s - ls), gr[jj * RS + 2 * C4 + c]);
            }
        }
        const float delta = head_sum<H>(dot4(go, o));
        float4 dq = {0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < P; j0 += UF) {
#pragma unroll
            for (int u = 0; u < UF; u++) {
                const int j = j0 + u, jj = j < P ? j : P - 1;
                const float4 kj = gr[jj * RS + C4 + c];
                const float s = head_sum<H>(dot4(q, kj)) * scale;
                const float dp = head_sum<H>(dot4(go, gr[jj * RS + 2 * C4 + c]));
                if ((w >> j) & 1) axpy4(dq, expf(s - ls) * (dp - delta) * scale, kj);
            }
        }
        if (!valid) continue;
        dst[lr * (ROW / 4) + c] = dq;
        if ((c & (HL - 1)) == 0) delta_s[(gl * H + h) * P + i] = delta;
    }
    __syncthreads();
    // pass B, a slot per key j: dK_j = sum_i dS_ij q_i / sqrt(D), dV_j = sum_i a_ij dO_i over the queries i that hear j
    for (int base = 0; base < nrows; base += SLOTS) {
        const bool valid = base + slot < nrows;
        const int lr = valid ? base + slot : nrows - 1;
        const int gl = lr / P, j = lr - gl * P;
        const float4 kj = rows[lr * RS + C4 + c], vj = rows[lr * RS + 2 * C4 + c];
        const float4 *gr = rows + gl * P * RS;
        float4 dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
        for (int i0 = 0; i0 < P; i0 += UF) {
#pragma unroll
            for (int u = 0; u < UF; u++) {
                const int i = i0 + u, ii = i < P ? i : P - 1;
                const float4 qi = gr[ii * RS + c], gi = gr[ii * RS + 3 * C4 + c];
                const float s = head_sum<H>(dot4(qi, kj)) * scale;
                const float dp = head_sum<H>(dot4(gi, vj));
                if (i < P && ((word_s[gl * P + ii] >> j) & 1)) {
                    const float a = expf(s - lse_s[(gl * H + h) * P + ii]);
                    axpy4(dk, a * (dp - delta_s[(gl * H + h) * P + ii]) * scale, qi);
                    axpy4(dv, a, gi);
                }
            }
        }
        if (!valid) continue;
        dst[lr * (ROW / 4) + C4 + c] = dk;
        dst[lr * (ROW / 4) + 2 * C4 + c] = dv;
    }
}

// ---- the same row functions on the host: a lane's dot4 per 4 columns and the butterfly's pairwise tree over the lanes of a head ----
inline float head_sum_host(float *p, int n) {   // p[0] as lane 0 of the butterfly ends: ((p0 + p1) + (p2 + p3)) + ...
    for (int off = 1; off < n; off <<= 1)
        for (int a = 0; a < n; a += 2 * off) p[a] = p[a] + p[a + off];
    return p[0];
}

inline float4 ld4(const float *p) { return make_float4(p[0], p[1], p[2], p[3]); }

inline float head_dot_host(const float *a, const float *b, int HL) {
#pragma clang fp contract(off)
    float part[C4];
    for (int c = 0; c < HL; c++) part[c] = dot4(ld4(a + 4 * c), ld4(b + 4 * c));
    return head_sum_host(part, HL);
}

inline void fwd_group_host(int P, int H, const float *qkv, const int64_t *words, float *out, float *lse) {
#pragma clang fp contract(off)
    const int HL = 32 / H, D = E / H;
    const float scale = head_scale(H);
    for (int i = 0; i < P; i++) {
        const uint64_t w = query_word((uint64_t)words[i], P, i);
        for (int h = 0; h < H; h++) {
            float m[C4], l[C4];
            float4 acc[C4];
            for (int c = 0; c < HL; c++) { m[c] = -INFINITY; l[c] = 0.f; acc[c] = make_float4(0.f, 0.f, 0.f, 0.f); }
            for (int j = 0; j < P; j++) {
                if (!((w >> j) & 1)) continue;
                const float s = head_dot_host(qkv + i * ROW + h * D, qkv + j * ROW + E + h * D, HL) * scale;
                for (int c = 0; c < HL; c++) soft_step(s, ld4(qkv + j * ROW + 2 * E + h * D + 4 * c), m[c], l[c], acc[c]);
            }
            for (int c = 0; c < HL; c++) {
                const float inv = 1.0f / l[c];
                float *o = out + i * E + h * D + 4 * c;
                o[0] = acc[c].x * inv; o[1] = acc[c].y * inv; o[2] = acc[c].z * inv; o[3] = acc[c].w * inv;
            }
            if (lse) lse[h * P + i] = m[0] + logf(l[0]);
        }
    }
}

inline void bwd_group_host(int P, int H, const float *qkv, const int64_t *words, const float *lse, const float *d_out, float *d_qkv) {
#pragma clang fp contract(off)
    const int HL = 32 / H, D = E / H;
    const float scale = head_scale(H);
    float delta[MAX_P * 8];
    for (int i = 0; i < P; i++) {
        const uint64_t w = query_word((uint64_t)words[i], P, i);
        for (int h = 0; h < H; h++) {
            const float *q = qkv + i * ROW + h * D, *go = d_out + i * E + h * D;
            const float ls = lse[h * P + i];
            float4 o[C4], dq[C4];
            float part[C4];
            for (int c = 0; c < HL; c++) o[c] = dq[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = 0; j < P; j++) {
                if (!((w >> j) & 1)) continue;
                const float s = head_dot_host(q, qkv + j * ROW + E + h * D, HL) * scale;
                for (int c = 0; c < HL; c++) axpy4(o[c], expf(s - ls), ld4(qkv + j * ROW + 2 * E + h * D + 4 * c));
            }
            for (int c = 0; c < HL; c++) part[c] = dot4(ld4(go + 4 * c), o[c]);
            const float dl = delta[h * P + i] = head_sum_host(part, HL);
            for (int j = 0; j < P; j++) {
                if (!((w >> j) & 1)) continue;
                const float *kj = qkv + j * ROW + E + h * D;
                const float s = head_dot_host(q, kj, HL) * scale, dp = head_dot_host(go, qkv + j * ROW + 2 * E + h * D, HL);
                for (int c = 0; c < HL; c++) axpy4(dq[c], expf(s - ls) * (dp - dl) * scale, ld4(kj + 4 * c));
            }
            for (int c = 0; c < HL; c++) {
                float *d = d_qkv + i * ROW + h * D + 4 * c;
                d[0] = dq[c].x; d[1] = dq[c].y; d[2] = dq[c].z; d[3] = dq[c].w;
            }
        }
    }
    for (int j = 0; j < P; j++)
        for (int h = 0; h < H; h++) {
            const float *kj = qkv + j * ROW + E + h * D, *vj = qkv + j * ROW + 2 * E + h * D;
            float4 dk[C4], dv[C4];
            for (int c = 0; c < HL; c++) dk[c] = dv[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int i = 0; i < P; i++) {
                if (!((query_word((uint64_t)words[i], P, i) >> j) & 1)) continue;
                const float *qi = qkv + i * ROW + h * D, *gi = d_out + i * E + h * D;
                const float s = head_dot_host(qi, kj, HL) * scale, dp = head_dot_host(gi, vj, HL);
                const float a = expf(s - lse[h * P + i]);
                for (int c = 0; c < HL; c++) {
                    axpy4(dk[c], a * (dp - delta[h * P + i]) * scale, ld4(qi + 4 * c));
                    axpy4(dv[c], a, ld4(gi + 4 * c));
                }
            }
            for (int c = 0; c < HL; c++) {
                float *d = d_qkv + j * ROW + E + h * D + 4 * c, *e = d + E;
                d[0] = dk[c].x; d[1] = dk[c].y; d[2] = dk[c].z; d[3] = dk[c].w;
                e[0] = dv[c].x; e[1] = dv[c].y; e[2] = dv[c].z; e[3] = dv[c].w;
            }
        }
}

static inline bool shape_ok(int64_t G, int P, int H) { return G >= 0 && P >= 1 && P <= MAX_P && heads_ok(H) && G * P < (int64_t)1 << 31; }

template <int PT, int H>
static int launch_fwd(int64_t G, int P, const float *qkv, const int64_t *words, float *out, float *lse, hipStream_t st) {
    const int gpt = fwd_tile(PT) / P;
    hipLaunchKernelGGL((k_team_attention_fwd<PT, H>), dim3((unsigned)((G + gpt - 1) / gpt)), dim3(256), 0, st, G, P, qkv, words, out, lse);
    return (int)hipGetLastError();
}

template <int PT, int H>
static int launch_bwd(int64_t G, int P, const float *qkv, const int64_t *words, const float *lse, const float *d_out, float *d_qkv, hipStream_t st) {
    const int gpt = bwd_tile(PT) / P;
    hipLaunchKernelGGL((k_team_attention_bwd<PT, H>), dim3((unsigned)((G + gpt - 1) / gpt)), dim3(256), 0, st, G, P, qkv, words, lse, d_out, d_qkv);
    return (int)hipGetLastError();
}

}  // namespace tatt

#define TATT_H(F, PT, ...)                                 \
    switch (H) {                                           \
        case 1: return tatt::F<PT, 1>(__VA_ARGS__);        \
        case 2: return tatt::F<PT, 2>(__VA_ARGS__);        \
        case 4: return tatt::F<PT, 4>(__VA_ARGS__);        \
        default: return tatt::F<PT, 8>(__VA_ARGS__);       \
    }
#define TATT_DISPATCH(F, ...)                              \
    if (P <= 8) { TATT_H(F, 8, __VA_ARGS__) }              \
    if (P <= 16) { TATT_H(F, 16, __VA_ARGS__) }            \
    if (P <= 32) { TATT_H(F, 32, __VA_ARGS__) }            \
    TATT_H(F, 64, __VA_ARGS__)

extern "C" {

int team_comm_mask(int64_t G, int32_t P, const float *pp_adj, int64_t adj_stride, const float *live, int64_t live_stride, int64_t *words,
                   int64_t words_stride, void *stream) {
    if (!tatt::shape_ok(G, P, 1) || !pp_adj || !live || !words || adj_stride < (int64_t)P * P || live_stride < P || words_stride < P) return MO_ERR_BAD_ARG;
    if (G == 0) return 0;
    const int64_t n = G * P;
    hipLaunchKernelGGL(tatt::k_team_comm_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, P, pp_adj, adj_stride, live,
                       live_stride, words, words_stride);
    return (int)hipGetLastError();
}

int team_attention_fwd(int64_t G, int32_t P, int32_t H, const float *qkv, const int64_t *words, float *out, float *lse, void *stream) {
    if (!tatt::shape_ok(G, P, H) || !qkv || !words || !out || (((uintptr_t)qkv | (uintptr_t)out) & 15)) return MO_ERR_BAD_ARG;
    if (G == 0) return 0;
    TATT_DISPATCH(launch_fwd, G, P, qkv, words, out, lse, (hipStream_t)stream)
}

int team_attention_bwd(int64_t G, int32_t P, int32_t H, const float *qkv, const int64_t *words, const float *lse, const float *d_out, float *d_qkv,
                       void *stream) {
    if (!tatt::shape_ok(G, P, H) || !qkv || !words || !lse || !d_out || !d_qkv) return MO_ERR_BAD_ARG;
    if (((uintptr_t)qkv | (uintptr_t)d_out | (uintptr_t)d_qkv) & 15) return MO_ERR_BAD_ARG;
    if (G == 0) return 0;
    TATT_DISPATCH(launch_bwd, G, P, qkv, words, lse, d_out, d_qkv, (hipStream_t)stream)
}

int team_comm_mask_host(int64_t G, int32_t P, const float *pp_adj, int64_t adj_stride, const float *live, int64_t live_stride, int64_t *words,
                        int64_t words_stride) {
    if (!tatt::shape_ok(G, P, 1) || !pp_adj || !live || !words || adj_stride < (int64_t)P * P || live_stride < P || words_stride < P) return MO_ERR_BAD_ARG;
    for (int64_t g = 0; g < G; g++)
        for (int i = 0; i < P; i++) words[g * words_stride + i] = (int64_t)tatt::comm_word(P, i, pp_adj + g * adj_stride, live + g * live_stride);
    return 0;
}

int team_attention_fwd_host(int64_t G, int32_t P, int32_t H, const float *qkv, const int64_t *words, float *out, float *lse) {
    if (!tatt::shape_ok(G, P, H) || !qkv || !words || !out) return MO_ERR_BAD_ARG;
    for (int64_t g = 0; g < G; g++)
        tatt::fwd_group_host(P, H, qkv + g * P * tatt::ROW, words + g * P, out + g * P * tatt::E, lse ? lse + g * H * P : nullptr);
    return 0;
}

int team_attention_bwd_host(int64_t G, int32_t P, int32_t H, const float *qkv, const int64_t *words, const float *lse, const float *d_out,
                            float *d_qkv) {
    if (!tatt::shape_ok(G, P, H) || !qkv || !words || !lse || !d_out || !d_qkv) return MO_ERR_BAD_ARG;
    for (int64_t g = 0; g < G; g++)
        tatt::bwd_group_host(P, H, qkv + g * P * tatt::ROW, words + g * P, lse + g * H * P, d_out + g * P * tatt::E, d_qkv + g * P * tatt::ROW);
    return 0;
}

}  // extern "C"
