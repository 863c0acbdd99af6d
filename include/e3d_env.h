/*
 * e3d_env.h -- C ABI of the MI355X (gfx950) batched env_3d environment (continuous 3-D pursuit; SURVEY 8f row 4, BASELINE
 * config 5).
 *
 * Replaces, for N independent environments, the methods of the reference class
 * environment/env_3d/particle_env.py:76 `ParticleEnv` cited per entry point.  Pursuer actions are CONTINUOUS
 * (a in [-1, 1]^3: heading, pitch, speed; Point.step :25-55).  The evader's command -- in the reference the result of eva.e_f
 * (scipy SLSQP, eva.py:87-148) -- is an input of the tick; e3d_evader_slsqp computes it.  Conventions as in pe_env.h: device
 * pointers owned by the caller, caller's hipStream_t as void*, 0 == success.
 * Several environments share one 64-lane wavefront (lane = (environment, pursuer), 8 environments per wave for P <= 8).
 */
#ifndef E3D_ENV_H
#define E3D_ENV_H
#include <stdint.h>
#include "policy_record.h"

#ifdef __cplusplus
extern "C" {
#endif

#define E3D_MAX_P 64
#define E3D_ERR_BAD_CONFIG 40001
#define E3D_ERR_NULL 40002
#define E3D_ERR_RESET_FAILED 40003   /* gen_init_p_pos (:151-164) found no placement within E3D_RESET_MAX_DRAWS draws */
#define E3D_ERR_BAD_STATE 40004      /* e3d_resetter_set_state: the blob's header does not match this resetter */
#define E3D_RESETTER_STATE_TAG 0x31523345u   /* "E3R1": format of e3d_resetter_get_state */
#define E3D_RESET_MAX_DRAWS 100000

typedef struct e3d_config {      /* particle_env.py:78-121 */
    int32_t P, max_step;
    double p_vmax, e_vmax, p_sen_range, p_comm_range, kill_radius, ang_lmt, v_lmt, step_size;
} e3d_config;

typedef struct e3d_state {
    int32_t N, pad0;
    double *p;           /* [N][7][P]  x[P], y[P], z[P], phi[P], gamma[P], v[P], active[P] (SoA over agents inside the record) */
    double *e;           /* [N][7]     the evader (e_num == 1, initialize :134-135)                                        */
    double *target;      /* [N][3]                                                                                         */
    int32_t *time_step;  /* [N]                                                                                            */
} e3d_state;

typedef struct e3d_obs_out {     /* fp32, NULL skips; *_stride = elements between environments */
    float *p_state; int64_t p_state_stride;   /* [N][P][6]  get_team_state(True, rules=False)  (:247-265)                  */
    float *e_state; int64_t e_state_stride;   /* [N][1][6]                                                                 */
    float *pp_adj;  int64_t pp_adj_stride;    /* [N][P][P]  get_adj_mat(p, p, p_comm_range)  (:328-340)                    */
    float *pe_adj;  int64_t pe_adj_stride;    /* [N][P][1]  get_adj_mat(p, e, p_sen_range)                                 */
} e3d_obs_out;

int e3d_config_check(const e3d_config *cfg);
/* ParticleEnv.reset hand-over: host p [N][P][7], e [N][7] (x, y, z, phi, gamma, v, active), target [N][3] -> device records */
int e3d_env_load(const e3d_config *cfg, const e3d_state *st, const double *p, const double *e, const double *target, void *stream);
int e3d_env_observe(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, void *stream);
/* One fused tick: Point.step of the evader with the command e_cmd [N][3] in [-1, 1] (evader_step :354-378; skipped, as there,
 * when the evader is inactive or no pursuer is left) -> ParticleEnv.step(actions [N][P][3], f64) (:205-219: Point.step,
 * reward :267-284, update_agent_active :286-326, get_done :221-241) -> observations of the new state.
 * reward [N][P] fp32, active [N][P] u8, done [N] u8. */
int e3d_env_tick(const e3d_config *cfg, const e3d_state *st, const double *actions, const double *e_cmd, float *reward,
                 uint8_t *active, uint8_t *done, const e3d_obs_out *out, void *stream);

/* Policy features of the env_3d trainer, both (N, P, 16) fp32 tensors (dense) in one launch; reads the records and out->pp_adj /
 * out->pe_adj of the current state (e3d_env_observe / e3d_env_tick fill them).  Pursuer i, state s_i = (x, y, z, phi, gamma, v), evader e:
 *   cols 0-5   s_i                                  (both)
 *   cols 6-11  (e - s_i) pe_adj[i]  |  (e - s_i) active_e
 *   col  12    pe_adj[i]            |  active_e
 *   cols 13-15 mean of pos_j - pos_i over j != i with pp_adj[i][j] = 1  |  over every active j != i  (0 if there is none)
 * (actor | critic); rows of inactive pursuers are zero. */
int e3d_policy_features(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, float *actor_feat, float *critic_feat, void *stream);

/* ---- algo.use_obs_norm: running mean / std normalisation of the policy features (csrc/obs_norm.hpp) ----
 * norm_state [2][33] f64 on the device: row 0 the actor's features, row 1 the critic's, each n, mean[16], M2[16] (all 0 at the start).
 * e3d_policy_features_norm writes, for the fp32 feature x that e3d_policy_features would write,
 *   n == 0:  x                      (so the outputs are e3d_policy_features' bits until the first update)
 *   else:    (float)min(max(((double)x - mean) / (sqrt(M2 / n) + 1e-8), -clip), clip)      (clip finite and > 0)
 * rows of inactive pursuers stay exactly zero.  slots != NULL: the same launch adds, per network and column, c = the number of
 * counted rows, S1 = sum d and S2 = sum d d, d = (double)x - mean, over the rows of active pursuers with live[n * live_rs + p] != 0
 * (the live mask of e3d_record_io) to the slot of each workgroup: slots [e3d_obs_norm_slots(N P)][2][33] f64 (c, S1[16], S2[16]),
 * zeroed by the caller before the first launch; a slot is owned by one workgroup, f64, fixed order, no atomics.  norm_state is
 * only read.  slots == NULL: nothing is accumulated and live is not read. */
int e3d_policy_features_norm(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, float *actor_feat, float *critic_feat,
                             const double *norm_state, double clip, const float *live, int64_t live_rs, double *slots, void *stream);
int64_t e3d_obs_norm_slots(int64_t rows);   /* slots of a launch over `rows` = N P feature rows */
/* sums [2][33] = the nslots slots added in index order (what a data-parallel job all-reduces); the slots are left as they are */
int e3d_obs_norm_reduce(const double *slots, int64_t nslots, double *sums, void *stream);
/* Merges the totals C = sums[.][0], A = S1, Q = S2 into norm_state, per network and column: C == 0 changes nothing; otherwise
 * n' = n + C, delta = A / C, mean' = mean + A / n', M2' = M2 + (Q - A delta) + delta delta (n C / n').  Then zeroes the nslots
 * slots (slots == NULL: none). */
int e3d_obs_norm_update(double *norm_state, const double *sums, double *slots, int64_t nslots, void *stream);

/* ---- MAPPO bookkeeping of one lockstep tick (e3d_agent.py), the structs of n2n_env.h for env_3d ----
 * fp32 rows with *_rs = elements between environments (dense storage or step t of an (N, T, P) buffer); a NULL output is skipped.
 * A row is LIVE when its pursuer was active at the start of the step and its environment was not done before it. */
typedef struct e3d_policy_acc {  /* per-environment episode accumulators [N], zeroed by the caller before the first step */
    uint8_t *done_before;        /* the environment reported done in an earlier step                                          */
    uint8_t *ended;              /* it ended for a reason other than the time limit (evader dead, no pursuer active, evader
                                    within the kill radius of the target), in this or an earlier step                         */
    uint8_t *captured;           /* the evader was captured before done                                                        */
    float *ret;                  /* sum over steps of sum_p reward * live (fp32, agents summed in order per step); raw reward  */
    float *length;               /* steps taken before done                                                                    */
} e3d_policy_acc;

typedef struct e3d_record_io {
    const float *live;  int64_t live_rs;    /* [N][P] this step's live mask, required (first step: the active flags after reset) */
    const float *value; int64_t value_rs;   /* [N][P] the critic's value of this step, required with v                           */
    float *r;      int64_t r_rs;            /* [N][P] reward * live, or what the options of policy_record.h make of it           */
    float *active; int64_t active_rs;       /* [N][P] live                                                                       */
    float *v;      int64_t v_rs;            /* [N][P] value * live                                                               */
    float *v_next; int64_t v_next_rs;       /* [N][P] set to 0 where the pursuer is inactive after the step or its environment
                                               has ended (time limit excepted); other entries untouched                         */
    float *live_next; int64_t live_next_rs; /* [N][P] the next step's live mask: active after the step and the environment not
                                               done after it; may be the storage of `live` (every lane reads its entry first)    */
} e3d_record_io;

/* After e3d_env_tick: buffer row t, the next live mask and the accumulators from the tick's reward [N][P] and done [N] and the records
 * after it.  opts: NULL, or the reward options of policy_record.h (RewardScaling, distance shaping, team reward sharing), in the same
 * launch.  One launch, the tick's lane layout.  Before any launch: a NULL argument (io->live, io->v without io->value and the five
 * accumulators included) is E3D_ERR_NULL, then e3d_config_check, then with opts->team an alpha outside [0, 1] is E3D_ERR_BAD_CONFIG;
 * N < 1 returns 0. */
int e3d_policy_record(const e3d_config *cfg, const e3d_state *st, const float *reward, const uint8_t *done, const e3d_record_io *io,
                      const e3d_policy_acc *acc, const policy_record_opts *opts, void *stream);
/* phi [N][P] f64 = the shaping potential of the current records (after a reset), what opts->phi carries from tick to tick:
 * Phi(n, p) = -coef * |pos_p - pos_e| (x, y, z; sqrt(dx dx + dy dy + dz dz) summed left to right), 0 when the pursuer or the evader is
 * inactive. */
int e3d_shaping_begin(const e3d_config *cfg, const e3d_state *st, double *phi, double coef, void *stream);

/* ---- scripted pursuers: a deterministic lead-pursuit law as a yardstick policy (csrc/guidance.hpp) ----
 * lead: the longest look-ahead in the environment's time units; a team-mate closer than sep_range pushes with weight sep_gain.
 * Each must be finite and >= 0 (E3D_ERR_BAD_CONFIG otherwise). */
typedef struct e3d_guidance_params { double lead, sep_range, sep_gain; } e3d_guidance_params;
/* actions [N][P][3] f64 in [-1, 1], what e3d_env_tick takes, from the current records.  Active pursuer i, active evader:
 *   r = e_pos - p_i, d = sqrt(rx rx + ry ry + rz rz); e_vel = v_e (cos gamma_e cos phi_e, cos gamma_e sin phi_e, sin gamma_e);
 *   t = min(d / p_vmax, lead); g = aim / |aim| with aim = r + t e_vel (0 when |aim| is 0); every active team-mate j != i with
 *   0 < d_ij < sep_range adds sep_gain (p_i - p_j) / d_ij (sep_range - d_ij) / sep_range, in index order;
 *   a0 = atan2(g_y, g_x) / pi, a1 = atan2(g_z, sqrt(g_x g_x + g_y g_y)) / (pi / 2), a2 = 1.
 * g exactly 0, or the pursuer or the evader inactive: hold, a0 = phi_i / pi, a1 = gamma_i / (pi / 2), a2 = -1.
 * One launch in the tick's lane layout, team-mates through shuffles, f64, no host synchronisation; the records are only read. */
int e3d_pursuer_guidance(const e3d_config *cfg, const e3d_state *st, const e3d_guidance_params *params, double *actions, void *stream);

/* ---- algo.e3d_features: pursuit -- line-of-sight policy features with a model of who knows where the evader is (csrc/pursuit_features.hpp,
 * DESIGN.md section 7g; specification: tests/e3d_features_ref.py) ----
 * Both (N, P, E3D_FEAT2) fp32 tensors (dense, 16-byte aligned) in one launch, from the records, st->target, st->time_step and out->pp_adj /
 * out->pe_adj of the current state.  Pursuer i: position p_i, u_i = (cos gamma_i cos phi_i, cos gamma_i sin phi_i, sin gamma_i), speed v_i;
 * r = e_pos - p_i, d = sqrt(rx rx + ry ry + rz rz), rh = r / d (0 when d is 0); e_vel = v_e (cos gamma_e cos phi_e, cos gamma_e sin phi_e,
 * sin gamma_e); W = E3D_WORLD.  The columns, the same for both networks:
 *   0-2   p_i / (W / 2) - 1          3-5   u_i                     6  v_i / p_vmax
 *   7-9   k rh                       10    k d / W                 11-13  k e_vel / e_vmax
 *   14    k (-rh . (e_vel - v_i u_i)) / (e_vmax + p_vmax)  (the closing speed)       15  k (u_i . rh)      16  k
 *   17-19 k (target - e_pos) / W
 *   20-24 the nearest visible team-mate j: (p_j - p_i) / d_ij (0 when d_ij is 0), d_ij / W, kill_radius / max(d_ij, kill_radius)
 *   25-29 the second nearest, the same five (a missing team-mate leaves its block 0)
 *   30    |V_i| / max(P - 1, 1)      31    time_step / max_step
 * k, who knows the evader: the critic's is active_e; the actor's follows evader_obs --
 *   SENSED  pe_adj[i] active_e (the rule of e3d_policy_features);
 *   TEAM    active_e when some pursuer of i's connected component senses the evader (pe_adj[j] == 1), i included: the components of the
 *           graph over the active pursuers with an edge i - j when pp_adj[i][j] == 1 or pp_adj[j][i] == 1 -- a sighting is relayed along
 *           communication links, over as many hops as the component has;
 *   GLOBAL  active_e (what the scripted pursuers read).
 * V_i, the visible team-mates: the actor's are the active j != i with pp_adj[i][j] == 1, the critic's every active j != i; nearest by
 * dx dx + dy dy + dz dz, the lowest index on ties.  Rows of inactive pursuers are zero; with the evader inactive columns 7-19 are zero.
 * f64 arithmetic in the order written, rounded to fp32 at the store.  One launch in the tick's lane layout, team-mates through shuffles, no
 * atomics, no host synchronisation; only the two outputs are written.  An evader_obs that is none of the three: E3D_ERR_BAD_CONFIG. */
#define E3D_FEAT2 32
#define E3D_WORLD 20.0   /* the side of the reset cube (particle_env.py:138-142) */
enum { E3D_EVADER_OBS_SENSED = 0, E3D_EVADER_OBS_TEAM = 1, E3D_EVADER_OBS_GLOBAL = 2 };
int e3d_pursuit_features(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, int32_t evader_obs, float *actor_feat,
                         float *critic_feat, void *stream);
/* The same computation on the host, on host records laid out as the device ones (p [N][7][P], e [N][7], target [N][3], time_step [N]) and
 * dense adjacencies pp_adj [N][P][P], pe_adj [N][P]; no alignment is required of the outputs. */
int e3d_pursuit_features_host(const e3d_config *cfg, int32_t N, const double *p, const double *e, const double *target, const int32_t *time_step,
                              const float *pp_adj, const float *pe_adj, int32_t evader_obs, float *actor_feat, float *critic_feat);

/* ---- algo.e3d_critic: central -- the critic's row with every team-mate in it (csrc/central_critic.hpp, DESIGN.md section 7k;
 * specification: tests/central_critic_ref.py) ----
 * e3d_pursuit_features with a wider critic tensor, in one launch: actor_feat (N, P, E3D_FEAT2) is byte for byte what
 * e3d_pursuit_features writes under the same evader_obs; critic_feat is (N, P, E3D_CENTRAL_FEAT(P)) fp32, dense, 16-byte aligned.
 * The critic's row of an active pursuer i:
 *   0-31             the critic row of e3d_pursuit_features
 *   32 + 8 s ...     slot s = 0 .. P - 2: the s-th team-mate j of V_i, the active j != i in the order of dx dx + dy dy + dz dz (strict <:
 *                    the lowest index first on an exact tie) --
 *                    0-2 (p_j - p_i) / d_ij (0 when d_ij is 0)   3 d_ij / W   4-6 u_j   7 v_j / p_vmax
 * Slots s >= |V_i| are zero, and so is the row of an inactive pursuer.  A slot's 0-3 are the values of the nearest-two blocks (columns
 * 20-23, 25-28 for s = 0, 1), its 4-7 are columns 3-6 of team-mate j's own row.  f64 arithmetic in the order written, rounded to fp32
 * at the store.  The tick's lane layout, team-mates through shuffles, no LDS, no atomics, no host synchronisation; only the two outputs
 * are written.  P > E3D_CENTRAL_MAX_P, an evader_obs that is none of the three, or a misaligned output: E3D_ERR_BAD_CONFIG, before any
 * launch; N = 0 touches nothing. */
#define E3D_CENTRAL_MATE 8
#define E3D_CENTRAL_MAX_P 16
#define E3D_CENTRAL_FEAT(P) (E3D_FEAT2 + E3D_CENTRAL_MATE * ((P) - 1))
int e3d_central_features(const e3d_config *cfg, const e3d_state *st, const e3d_obs_out *out, int32_t evader_obs, float *actor_feat,
                         float *critic_feat, void *stream);
/* The same computation on the host, on the inputs of e3d_pursuit_features_host; no alignment is required of the outputs. */
int e3d_central_features_host(const e3d_config *cfg, int32_t N, const double *p, const double *e, const double *target, const int32_t *time_step,
                              const float *pp_adj, const float *pe_adj, int32_t evader_obs, float *actor_feat, float *critic_feat);

/* ---- algo.gauss_squash: direction -- the map of the direction-vector action head on the host (csrc/direction_action.hpp, DESIGN.md
 * section 7h; specification: tests/direction_ref.py).  The device side is gauss_head_sample_ex / e3d_bc_select of mappo_ops.h ----
 * gauss_direction_map_host: u [R][4] fp32, the policy's latent action (u_x, u_y, u_z, s) -> env_action [R][3] f64,
 *   a0 = atan2(u_y, u_x) / pi, a1 = atan2(u_z, hypot(u_x, u_y)) / (pi / 2), a2 = s, each clamped to [-1, 1].
 * e3d_direction_label_host: g [R][3] f64, guidance actions -> a_star [R][4] fp32, the label (cos gam cos phi, cos gam sin phi, sin gam, g2)
 *   with phi = g0 pi, gam = g1 pi / 2.
 * A null pointer: E3D_ERR_NULL; R < 0: E3D_ERR_BAD_CONFIG; R = 0 touches nothing. */
int gauss_direction_map_host(int32_t R, const float *u, double *env_action);
int e3d_direction_label_host(int32_t R, const double *g, float *a_star);

/* The reference's evader: eva.e_f (eva.py:87-148) -- scipy's SLSQP (ftol 1e-6, <= 100 iterations, 2-point finite-difference
 * gradient) minimising obj_func (:212-240) over (heading, pitch, speed), started at the evader's state, bounded by the
 * environment's ang_lmt / v_lmt (:130-135) -- written as the command e_cmd [N][3] that e3d_env_tick consumes; zeros when the
 * evader is inactive or no pursuer is active (the tick does not move it then).  Only active pursuers within e_sen_range
 * (3, particle_env.py:86) count; the objective's own kinematics use the literals ang_lmt pi/4, v_lmt 0.4, step 0.5 (:214-227).
 * One lane per environment, no host synchronisation.  The _nit form also writes the major iterations taken, nit [N]. */
int e3d_evader_slsqp(const e3d_config *cfg, const e3d_state *st, double *e_cmd, void *stream);
int e3d_evader_slsqp_nit(const e3d_config *cfg, const e3d_state *st, double *e_cmd, int32_t *nit, void *stream);
/* The same computation on the host, on host records laid out as the device ones (p [N][7][P], e [N][7], target [N][3]). */
int e3d_evader_slsqp_host(const e3d_config *cfg, int32_t N, const double *p, const double *e, const double *target, double *e_cmd,
                          int32_t *nit);

/* Host side of ParticleEnv.reset (:137-203) with a bit-exact replica of numpy's legacy RandomState per environment
 * (np.random.seed(seeds[n])).  Fills host arrays p [N][P][7], e [N][7], target [N][3]. */
void *e3d_resetter_create(const e3d_config *cfg, int32_t N, const uint32_t *seeds);
void e3d_resetter_destroy(void *resetter);
int e3d_resetter_reset(void *resetter, double *p, double *e, double *target, int32_t n_threads);
/* Resume support: the generator of every environment as one blob of e3d_resetter_state_bytes bytes -- a 16-byte header
 * (u32 tag E3D_RESETTER_STATE_TAG, i32 N, P, E = 1), then per environment the MT19937 key (624 x u32), its position (i32),
 * has_gauss (i32) and the cached gauss (f64).  set_state restores a blob of get_state; a blob whose header does not match this
 * resetter (or with a malformed record) is rejected with E3D_ERR_BAD_STATE and leaves the resetter as it was. */
int64_t e3d_resetter_state_bytes(void *resetter);
int e3d_resetter_get_state(void *resetter, void *out);
int e3d_resetter_set_state(void *resetter, const void *in);

#ifdef __cplusplus
}
#endif
#endif
