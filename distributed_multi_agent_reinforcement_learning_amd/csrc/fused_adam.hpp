// fused_adam.hpp -- algo.minibatch_steps of the env_3d / env_n2n trainers: the gradient clip and the Adam step of one mini-batch in two
// launches over flat fp32 arrays (C ABI: include/mappo_ops.h fused_adam_norm / fused_adam_step; numpy
// restatement: tests/fused_adam_ref.py).  Included once, from csrc/mappo_ops.hip.
//
// state: six f64 on the device, (step, b1t, b2t, norm, coef, skipped) = the number of steps taken, the running products beta1^step and
// beta2^step (1 at the start; products, not pow, so numpy reproduces them), the gradient norm and the clip coefficient of the last
// call, and the number of calls whose norm was not finite.  Launch 1 writes norm and coef and advances step, b1t, b2t; launch 2 reads
// them.  A non-finite norm advances nothing but `skipped` and sets coef to fadam::SKIP, under which launch 2 stores nothing.
// All f64 arithmetic is written with contraction off: the stated expressions rounded operation by operation, as numpy evaluates them.
#pragma once
#include <math.h>

namespace fadam {

constexpr int NSTATE = 6;
constexpr int BLOCKS = 256;        // workgroups of either launch at most: one full grid pass is BLOCKS x 256 lanes x 4 elements
constexpr double SKIP = -1.0;      // coef of a skipped step (a real coefficient is in (0, 1])

// the end of launch 1 from the sum of squares: clip_grad_norm_'s coefficient (max_norm <= 0: no clip, exactly 1) and the step counters
__host__ __device__ inline void advance(double *st, double sumsq, double max_norm, double beta1, double beta2) {
#pragma clang fp contract(off)
    const double norm = sqrt(sumsq);
    st[3] = norm;
    if (!(norm <= 1.79769313486231570815e308)) {   // inf or NaN
        st[4] = SKIP;
        st[5] += 1.0;
        return;
    }
    double coef = 1.0;
    if (max_norm > 0.0) {
        coef = max_norm / (norm + 1e-6);
        if (coef > 1.0) coef = 1.0;
    }
    st[4] = coef;
    st[0] += 1.0;
    st[1] *= beta1;
    st[2] *= beta2;
}

// the per-call constants of launch 2: 1 - b1t and sqrt(1 - b2t)
struct Bias {
    double c1, s2;
};

__host__ __device__ inline Bias bias(double b1t, double b2t) {
#pragma clang fp contract(off)
    Bias b;
    b.c1 = 1.0 - b1t;
    b.s2 = sqrt(1.0 - b2t);
    return b;
}

// one element of launch 2, in f64 from the fp32 inputs
__host__ __device__ inline void row(float &p, float g, float &m, float &v, double coef, Bias b, double lr, double beta1, double beta2, double eps) {
#pragma clang fp contract(off)
    const double gc = (double)g * coef;
    const double m64 = beta1 * (double)m + (1.0 - beta1) * gc;
    const double v64 = beta2 * (double)v + ((1.0 - beta2) * gc) * gc;
    const double den = sqrt(v64) / b.s2 + eps;
    const double p64 = (double)p - lr * ((m64 / b.c1) / den);
    m = (float)m64;
    v = (float)v64;
    p = (float)p64;
}

// Launch 1.  Every thread adds (double)g^2 over its lanes of the grid-stride loop (16-byte lanes; the n % 4 tail elements go to the
// first threads of workgroup 0), the workgroup adds its 256 threads in a fixed order (wave butterflies, then the four waves) and
// stores one f64 partial.  The last workgroup to take a ticket adds the partials in index order and finishes the state.  The partials
// cross workgroups inside the launch: they are stored and loaded as agent-scope atomics (past the per-CU cache) between a release
// before the ticket and an acquire after it.
__global__ __launch_bounds__(256) void k_fused_adam_norm(int64_t n4, int64_t n, const float *__restrict__ g, double *state, double *partials,
                                                         unsigned int *ticket, double max_norm, double beta1, double beta2) {
    __shared__ double red[4];
    __shared__ double part[BLOCKS];
    __shared__ bool last;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 x = ((const float4 *)g)[i];
        s += (double)x.x * (double)x.x;
        s += (double)x.y * (double)x.y;
        s += (double)x.z * (double)x.z;
        s += (double)x.w * (double)x.w;
    }
    const int64_t it = 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && it < n) s += (double)g[it] * (double)g[it];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(partials + blockIdx.x, (red[0] + red[1]) + (red[2] + red[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
        if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    if (!last) return;
    if (threadIdx.x < gridDim.x) part[threadIdx.x] = __hip_atomic_load(partials + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (unsigned b = 0; b < gridDim.x; b++) sum += part[b];
        advance(state, sum, max_norm, beta1, beta2);
        *ticket = 0u;
    }
}

// Launch 2: row() on every element, n4 16-byte lanes in a grid-stride loop, then the n - 4 n4 tail elements (workgroup 0).
__global__ __launch_bounds__(256) void k_fused_adam_step(int64_t n4, int64_t n, float *__restrict__ p, const float *__restrict__ g,
                                                         float *__restrict__ m, float *__restrict__ v, const double *__restrict__ state, double lr,
                                                         double beta1, double beta2, double eps) {
    const double coef = state[4];
    if (coef == SKIP) return;
    const Bias b = bias(state[1], state[2]);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 pp = ((float4 *)p)[i], mm = ((float4 *)m)[i], vv = ((float4 *)v)[i];
        const float4 gg = ((const float4 *)g)[i];
        row(pp.x, gg.x, mm.x, vv.x, coef, b, lr, beta1, beta2, eps);
        row(pp.y, gg.y, mm.y, vv.y, coef, b, lr, beta1, beta2, eps);
        row(pp.z, gg.z, mm.z, vv.z, coef, b, lr, beta1, beta2, eps);
        row(pp.w, gg.w, mm.w, vv.w, coef, b, lr, beta1, beta2, eps);
        ((float4 *)p)[i] = pp;
        ((float4 *)m)[i] = mm;
        ((float4 *)v)[i] = vv;
    }
    const int64_t i = 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && i < n) row(p[i], g[i], m[i], v[i], coef, b, lr, beta1, beta2, eps);
}

static inline bool betas_ok(double beta1, double beta2) { return beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0; }

}  // namespace fadam

extern "C" {

int64_t fused_adam_workspace(void) { return (int64_t)(fadam::BLOCKS + 2) * sizeof(double); }

int fused_adam_grid(int64_t n) {
    const int64_t blocks = (n / 4 + 255) / 256;
    return (int)(blocks < 1 ? 1 : (blocks < fadam::BLOCKS ? blocks : fadam::BLOCKS));
}

int fused_adam_norm(int64_t n, const float *g, double *state, void *workspace, double max_norm, double beta1, double beta2, void *stream) {
    if (n < 1 || !g || !state || !workspace || !fadam::betas_ok(beta1, beta2) || max_norm != max_norm) return MO_ERR_BAD_ARG;
    if (((uintptr_t)g & 15) || ((uintptr_t)workspace & 15)) return MO_ERR_BAD_ARG;
    double *partials = (double *)workspace;
    unsigned int *ticket = (unsigned int *)(partials + fadam::BLOCKS);   // zero before the first call; the kernel leaves it zero
    hipLaunchKernelGGL(fadam::k_fused_adam_norm, dim3(fused_adam_grid(n)), dim3(256), 0, (hipStream_t)stream, n / 4, n, g, state, partials, ticket,
                       max_norm, beta1, beta2);
    return (int)hipGetLastError();
}

int fused_adam_step(int64_t n, float *p, const float *g, float *m, float *v, const double *state, double lr, double beta1, double beta2,
                    double eps, void *stream) {
    if (n < 1 || !p || !g || !m || !v || !state || !fadam::betas_ok(beta1, beta2) || !(eps >= 0.0) || lr != lr) return MO_ERR_BAD_ARG;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return MO_ERR_BAD_ARG;
    hipLaunchKernelGGL(fadam::k_fused_adam_step, dim3(fused_adam_grid(n)), dim3(256), 0, (hipStream_t)stream, n / 4, n, p, g, m, v, state, lr, beta1,
                       beta2, eps);
    return (int)hipGetLastError();
}

// fadam::advance on the host (no device): state [6] from a sum of squares, as the last workgroup of launch 1 leaves it
int fused_adam_advance_host(double *state, double sumsq, double max_norm, double beta1, double beta2) {
    if (!state || !fadam::betas_ok(beta1, beta2) || max_norm != max_norm) return MO_ERR_BAD_ARG;
    fadam::advance(state, sumsq, max_norm, beta1, beta2);
    return 0;
}

// fadam::row on the host, in place on p, m, v [n], under state's coef, b1t, b2t: nothing is stored when the step was skipped.  The CPU
// checks compare it with the numpy restatement bit for bit.
int fused_adam_rows_host(int64_t n, float *p, const float *g, float *m, float *v, const double *state, double lr, double beta1, double beta2,
                         double eps) {
    if (n < 0 || !p || !g || !m || !v || !state || !fadam::betas_ok(beta1, beta2) || !(eps >= 0.0) || lr != lr) return MO_ERR_BAD_ARG;
    if (state[4] == fadam::SKIP) return 0;
    const fadam::Bias b = fadam::bias(state[1], state[2]);
    for (int64_t i = 0; i < n; i++) fadam::row(p[i], g[i], m[i], v[i], state[4], b, lr, beta1, beta2, eps);
    return 0;
}

}  // extern "C"
