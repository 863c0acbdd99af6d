/*
 * pe_env_diag.h -- TEST-ONLY entry points of libpe_env.so (not part of the drop-in boundary of pe_env.h).
 * They expose, for the parity tests, the exact-arithmetic building blocks the tick kernel relies on.
 */
#ifndef PE_ENV_DIAG_H
#define PE_ENV_DIAG_H
#include <stdint.h>

#include "pe_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device f64 primitives against the host (tests/test_env_gpu.py): out[5][n] = norm2(a,b) = sqrt(fma(b,b,a*a)), a / b,
 * round-half-even(a), a / c0 and b / c1 through the kernel's three-flop division by a host-known constant. */
int pe_diag_norm2(int32_t n, const double *a, const double *b, double *out, double c0, double c1, void *stream);
/* Host only (no GPU): the comparison threshold the tick kernel uses in place of sqrt(x) <= r (strict: sqrt(x) < r) ... */
double pe_diag_sq_threshold(double r, int32_t strict);
/* ... and the reciprocal it divides by a constant with (0 = the plain IEEE division is used). */
double pe_diag_div_reciprocal(double b);

/* Host only (no GPU): what the launcher chooses for a configuration and a launch form -- every run-time selected code path of the
 * tick kernel.  The launcher itself launches from this record (csrc/pe_env.hip plan_launch), the kernel's own two choices
 * (one_load, grid staging) are the same inline predicates, so the record cannot drift from what runs.
 * form: OR of PE_FORM_*; the entry points are observe = OBS, step = STEP, step_observe = STEP|OBS, evader_step = EVA (|REPLAN),
 * tick = STEP|OBS|EVA (|REPLAN). */
enum { PE_FORM_STEP = 1, PE_FORM_OBS = 2, PE_FORM_EVA = 4, PE_FORM_REPLAN = 8 };
enum { PE_GRID_WIDE = 0, PE_GRID_COPY16 = 16, PE_GRID_COPY4 = 4, PE_GRID_COPY1 = 1 };
typedef struct pe_launch_plan {
    int32_t wpb;            /* wavefronts (= environments) per workgroup: 4 or 1 */
    int32_t lds_per_env;    /* bytes of LDS per environment (16-byte aligned) */
    int32_t lds_bytes;      /* dynamic LDS of the launch = wpb * lds_per_env */
    int32_t needs_attr;     /* lds_bytes > 48 KB: hipFuncAttributeMaxDynamicSharedMemorySize is raised first */
    int32_t fast8;          /* P <= 8: the 8 x 8 lane tiles of dev_step / dev_observe */
    int32_t rw_shift;       /* log2 of the raser row length in words, -1 = not a power of two (lane / RW) */
    uint32_t o4_magic;      /* multiply-shift constant of idx / (O / 4), 0 = plain division */
    int32_t one_load;       /* P * RW <= 64: the LiDAR rows are gathered with one load per lane (else a loop) */
    int32_t grid_copy;      /* PE_GRID_*: registers up front (wide) or copy_in's 16 / 4 / 1-byte form */
    int32_t tape_loop;      /* tape_len > 32: the tape's tail is staged by a second, looped copy */
    double inv_def_tau, inv_eva_tau, inv_six;  /* div_const reciprocals, 0 = IEEE division */
} pe_launch_plan;
int pe_diag_launch_plan(const pe_config *cfg, int32_t form, pe_launch_plan *out);

/* pe_pursuer_pathfinder with one more output: sweeps [N] int32 (DEVICE), the sweeps the distance field of each environment took,
 * the last one (which changed nothing) included.  Measurement only. */
int pe_diag_pathfinder_sweeps(const pe_config *cfg, const pe_state *st, const pe_pathfinder_params *prm, int32_t *actions, int32_t *sweeps,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif
