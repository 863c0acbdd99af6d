/*
 * n2n_env.h -- C ABI of the MI355X (gfx950) batched env_n2n environment (continuous 2-D pursuit).
 *
 * Replaces, for N independent environments, the methods of the reference class
 * environment/env_n2n/particle_env.py:105 `ParticleEnv` cited per entry point.  The evader's heading command -- in the
 * reference the result of eva.e_f (scipy SLSQP, eva.py:36-53) -- is an input of the tick; n2n_evader_slsqp computes it.
 * Conventions as in pe_env.h: device pointers owned by the caller, caller's hipStream_t as void*, 0 == success.
 * Several environments share one 64-lane wavefront (lane = (environment, agent slot); 4 environments per wave at P = 16).
 */
#ifndef N2N_ENV_H
#define N2N_ENV_H
#include <stdint.h>
#include "policy_record.h"

#ifdef __cplusplus
extern "C" {
#endif

#define N2N_MAX_P 64
#define N2N_MAX_E 8
#define N2N_ERR_BAD_CONFIG 30001
#define N2N_ERR_NULL 30002
#define N2N_ERR_BAD_STATE 30003      /* n2n_resetter_set_state: the blob's header does not match this resetter */
#define N2N_ERR_RESET_FAILED 30004   /* gen_init_p_pos / gen_init_e_pos (:239-281) found no placement within N2N_RESET_MAX_DRAWS draws */
#define N2N_RESETTER_STATE_TAG 0x3152324eu   /* "N2R1": format of n2n_resetter_get_state */
/* The reference's placement loops reject a candidate closer than 2 to an earlier point and never give up; in the 16 x 16 box of the
 * pursuers that stops converging between 40 and 48 of them.  Each loop here (pursuers, evaders) draws at most this many candidates, then
 * keeps the last one and n2n_resetter_reset returns N2N_ERR_RESET_FAILED; the value and the meaning are those of E3D_RESET_MAX_DRAWS and
 * PE_RESET_MAX_DRAWS.  A reset that succeeds consumes the generator exactly as the reference does. */
#define N2N_RESET_MAX_DRAWS 100000

typedef struct n2n_config {      /* particle_env.py:108-121,147 */
    int32_t P, E, episode_limit, pad0;
    double p_vmax, e_vmax, p_sen_range, p_comm_range, kill_radius, ang_lmt, step_size;
} n2n_config;

typedef struct n2n_state {
    int32_t N, pad0;
    double *p;           /* [N][5][P]  x[P], y[P], phi[P], v[P], active[P]  (SoA over agents inside the record) */
    double *e;           /* [N][5][E]                                                                          */
    double *target;      /* [N][2]                                                                             */
    int32_t *time_step;  /* [N]                                                                                */
} n2n_state;

typedef struct n2n_obs_out {     /* fp32, NULL skips; *_stride = elements between environments */
    float *p_state; int64_t p_state_stride;   /* [N][P][3]  get_team_state(True, rules=False)  (:367-384)          */
    float *e_state; int64_t e_state_stride;   /* [N][E][3]                                                         */
    float *pp_adj;  int64_t pp_adj_stride;    /* [N][P][P]  get_adj_mat(p, p, p_comm_range)  (:386-397)            */
    float *pe_adj;  int64_t pe_adj_stride;    /* [N][P][E]  get_adj_mat(p, e, p_sen_range)                         */
} n2n_obs_out;

int n2n_config_check(const n2n_config *cfg);
/* ParticleEnv.reset hand-over: host p [N][P][5], e [N][E][5] (x, y, phi, v, active), target [N][2] -> device records */
int n2n_env_load(const n2n_config *cfg, const n2n_state *st, const double *p, const double *e, const double *target, void *stream);
int n2n_env_observe(const n2n_config *cfg, const n2n_state *st, const n2n_obs_out *out, void *stream);
/* One fused tick: Evader.step with the commanded heading e_cmd [N][E] in [-1, 1] (:74-99, driven by evader_step :179-198)
 * -> ParticleEnv.step(actions [N][P]) (:164-177: Pursuer.step :34-67, reward :316-334, update_agent_active :336-365,
 * get_done :283-304) -> observations of the new state.  reward [N][P] fp32, active [N][P] u8, done [N] u8. */
int n2n_env_tick(const n2n_config *cfg, const n2n_state *st, const int32_t *actions, const double *e_cmd, float *reward,
                 uint8_t *active, uint8_t *done, const n2n_obs_out *out, void *stream);

/* The reference's evader: for every active evader, eva.e_f (eva.py:36-80) -- scipy's SLSQP (ftol 1e-6, <= 100 iterations,
 * 2-point finite-difference gradient) minimising obj_func (:60-80) over the heading in [-pi, pi] from 0 -- written as the
 * normalised command e_cmd [N][E] that n2n_env_tick consumes; 0 for inactive evaders (never passed to e_f in evader_step
 * :179-198).  Only active pursuers within e_sen_range (3, particle_env.py:114) count; their speeds are read from the FULL
 * pursuer list at the index of the in-range list (p_v0[ne], eva.py:67).  One lane per (environment, evader), no host
 * synchronisation.  The _nit form also writes the major iterations taken per evader, nit [N][E] (NULL skips). */
int n2n_evader_slsqp(const n2n_config *cfg, const n2n_state *st, double *e_cmd, void *stream);
int n2n_evader_slsqp_nit(const n2n_config *cfg, const n2n_state *st, double *e_cmd, int32_t *nit, void *stream);
/* The same computation on the host, on host records laid out as the device ones (p [N][5][P], e [N][5][E], target [N][2]). */
int n2n_evader_slsqp_host(const n2n_config *cfg, int32_t N, const double *p, const double *e, const double *target, double *e_cmd,
                          int32_t *nit);

/* ---- MAPPO on env_n2n (n2n_agent.py) ----
 * Same lane layout as the tick (lane = (environment, agent slot)).  fp32 outputs with *_rs = elements between environments, so
 * they may land in dense static storage or in step t of (N, T, ...) buffers; a NULL output is skipped.  A row is LIVE when its
 * pursuer is active at the start of the step and its environment was not done before it. */
typedef struct n2n_policy_io {
    const float *pp_in; int64_t pp_in_rs;   /* [N][P][P] the tick's pp_adj (n2n_obs_out), required with pp_adj          */
    const float *pe_in; int64_t pe_in_rs;   /* [N][P][E] the tick's pe_adj, required with pe_adj                        */
    float *p4;    int64_t p4_rs;            /* [N][P][4] (x, y, v cos phi, v sin phi); cos / sin in f64, then rounded;
                                               a row that is not live is zero                                          */
    float *e4;    int64_t e4_rs;            /* [N][E][4] the same for the evaders; an inactive evader's row is zero     */
    float *e_ref; int64_t e_ref_rs;         /* [N][4] the lowest-index active evader's row, zeros when none is active    */
    float *live;  int64_t live_rs;          /* [N][P] 1 / 0                                                             */
    float *pp_adj; int64_t pp_adj_rs;       /* [N][P][P] pp_in where pursuers i and j are both live, else 0             */
    float *pe_adj; int64_t pe_adj_rs;       /* [N][P][E] pe_in where pursuer i is live and evader k active, else 0     */
} n2n_policy_io;

typedef struct n2n_policy_acc {  /* per-environment episode accumulators [N], zeroed by the caller before the first step */
    uint8_t *done_before;        /* the environment reported done in an earlier step                                  */
    uint8_t *ended;              /* it ended for a reason other than the time limit (evader at target, no pursuer or no
                                    evader left), in this or an earlier step                                          */
    uint8_t *captured;           /* every evader was captured before done                                             */
    float *ret;                  /* sum over steps of sum_p reward * live (fp32, agents summed in order per step)      */
    float *length;               /* steps taken before done                                                            */
} n2n_policy_acc;

typedef struct n2n_record_io {
    const float *live;  int64_t live_rs;    /* [N][P] this step's live mask (n2n_policy_inputs), required               */
    const float *value; int64_t value_rs;   /* [N][P] the critic's value of this step, required with v                  */
    float *r;      int64_t r_rs;            /* [N][P] reward * live, or what the options of policy_record.h make of it  */
    float *active; int64_t active_rs;       /* [N][P] live                                                              */
    float *v;      int64_t v_rs;            /* [N][P] value * live                                                      */
    float *v_next; int64_t v_next_rs;       /* [N][P] set to 0 where the pursuer is inactive after the step or its
                                               environment has ended (time limit excepted); other entries untouched     */
} n2n_record_io;

/* Before the policy step: the DHGN's inputs from the records p, e, the tick's adjacencies and done_before [N] (NULL: none done). */
int n2n_policy_inputs(const n2n_config *cfg, const n2n_state *st, const uint8_t *done_before, const n2n_policy_io *io, void *stream);
/* After n2n_env_tick: buffer row t and the accumulators from the tick's reward [N][P] and done [N] and the records after it.  opts: NULL,
 * or the reward options of policy_record.h (RewardScaling, distance shaping, team reward sharing), in the same launch.  One launch, the
 * tick's lane layout.  Before any launch: a NULL argument (io->live, io->v without io->value and the five accumulators included) is
 * N2N_ERR_NULL, then n2n_config_check, then with opts->team an alpha outside [0, 1] is N2N_ERR_BAD_CONFIG; N < 1 returns 0. */
int n2n_policy_record(const n2n_config *cfg, const n2n_state *st, const float *reward, const uint8_t *done, const n2n_record_io *io,
                      const n2n_policy_acc *acc, const policy_record_opts *opts, void *stream);
/* phi [N][P] f64 = the shaping potential of the current records (after a reset), what opts->phi carries from tick to tick:
 * Phi(n, p) = -coef * min_k |pos_p - pos_k| over the ACTIVE evaders k (x, y; sqrt(dx dx + dy dy)), 0 when the pursuer is inactive or no
 * evader is active. */
int n2n_shaping_begin(const n2n_config *cfg, const n2n_state *st, double *phi, double coef, void *stream);

/* ---- scripted pursuers: a deterministic lead-pursuit law as a yardstick policy (csrc/guidance.hpp) ----
 * lead: the longest look-ahead in the environment's time units; a team-mate closer than sep_range pushes with weight sep_gain.
 * Each must be finite and >= 0 (N2N_ERR_BAD_CONFIG otherwise). */
typedef struct n2n_guidance_params { double lead, sep_range, sep_gain; } n2n_guidance_params;
/* actions [N][P] int32 in 0..8, what n2n_env_tick takes (and head_sample writes), from the current records.  Active pursuer i against
 * the nearest active evader (lowest index on ties):
 *   r = e_pos - p_i, d = sqrt(rx rx + ry ry); e_vel = v_e (cos phi_e, sin phi_e); t = min(d / p_vmax, lead);
 *   g = aim / |aim| with aim = r + t e_vel (0 when |aim| is 0); every active team-mate j != i with 0 < d_ij < sep_range adds
 *   sep_gain (p_i - p_j) / d_ij (sep_range - d_ij) / sep_range, in index order; k = rint(atan2(g_y, g_x) / (pi / 4)) reduced to 1..8
 *   (0 and -8 map to 8; the tick turns k pi / 4 > pi into its negative angle).
 * g exactly 0, the pursuer inactive, or no evader active: action 0 (stop, keep the heading).
 * One launch in the tick's lane layout, evaders and team-mates through shuffles, f64, no host synchronisation; the records are only
 * read. */
int n2n_pursuer_guidance(const n2n_config *cfg, const n2n_state *st, const n2n_guidance_params *params, int32_t *actions, void *stream);

/* Host side of ParticleEnv.reset (:200-281) with a bit-exact replica of numpy's legacy RandomState per environment
 * (np.random.seed(seeds[n])).  Fills host arrays p [N][P][5], e [N][E][5], target [N][2].  N2N_ERR_RESET_FAILED when a placement loop
 * of any environment gave up (N2N_RESET_MAX_DRAWS); the arrays are filled all the same, with points that may be closer than 2. */
void *n2n_resetter_create(const n2n_config *cfg, int32_t N, const uint32_t *seeds);
void n2n_resetter_destroy(void *resetter);
int n2n_resetter_reset(void *resetter, double *p, double *e, double *target, int32_t n_threads);
/* Resume support: the generator of every environment as one blob of n2n_resetter_state_bytes bytes -- a 16-byte header
 * (u32 tag N2N_RESETTER_STATE_TAG, i32 N, P, E), then per environment the MT19937 key (624 x u32), its position (i32),
 * has_gauss (i32) and the cached gauss (f64).  set_state restores a blob of get_state; a blob whose header does not match this
 * resetter (or with a malformed record) is rejected with N2N_ERR_BAD_STATE and leaves the resetter as it was. */
int64_t n2n_resetter_state_bytes(void *resetter);
int n2n_resetter_get_state(void *resetter, void *out);
int n2n_resetter_set_state(void *resetter, const void *in);

#ifdef __cplusplus
}
#endif
#endif
