/*
 * policy_record.h -- the reward options of the MAPPO bookkeeping launch, one record for e3d_policy_record (e3d_env.h) and
 * n2n_policy_record (n2n_env.h).
 *
 * The launch after a tick writes row t of the buffer and advances the episode accumulators.  Three options, any subset of them in that
 * same launch, change what the reward row io->r receives; a NULL record means all three are off (io->r = reward * live).  Per
 * environment that was not done before the step, with x = reward[P] (every pursuer's, an inactive one's 0 included), the options act in
 * the order team -> shaping -> scaling -> buffer row:
 *
 * team != 0 -- team reward sharing (algo.team_reward: alpha; csrc/team_reward.hpp).  With s = sum_k x_k live_k
 *   (f64, index order), m_p = (1 - alpha) x_p + (alpha s) live_p takes the place of the raw reward in everything that follows:
 *   io->r = (float)m * live, the shaping step receives m, the scaling step receives m or the shaped m.  alpha must be a number in [0, 1]:
 *   *_ERR_BAD_CONFIG otherwise, before any launch.  alpha = 0 still runs the team code; with team == 0 alpha is not read.
 *
 * phi != NULL -- potential-based distance shaping (algo.reward_shaping: distance; csrc/reward_shaping.hpp).  phi [N][P] f64 carries the
 *   potential of the state a tick starts from, Phi(n, p) = -coef * (the distance of pursuer p to its evader), 0 when there is none; the
 *   distance is each library's own and stands with its *_shaping_begin, which writes Phi of the current records (after a reset).
 *   Phi' = Phi of the records after the tick, Phi_next = 0 where v_next is zeroed (pursuer inactive after the step, or the episode
 *   ended, the time limit excepted), else Phi'; x = reward + (gamma Phi_next - phi) live; phi = Phi'; io->r = (float)x * live, or what
 *   the scaling step makes of x.
 *
 * rs != NULL -- the reference's RewardScaling (DHGN/normalization.py:38-52, csrc/reward_scale.hpp).  rs [N][1 + 3P] f64: n, mean[P],
 *   S[P], R[P] per environment; the caller zeroes it once (and R at every episode start: RewardScaling.reset).  R = gamma R + x; n += 1;
 *   n == 1: mean = std = R, else mean' = mean + (R - mean) / n, S += (R - mean)(R - mean'), std = sqrt(S / n);
 *   io->r = (float)(x / (std + 1e-8)) * live.
 *
 * Environments done before the step leave phi and rs untouched (r = reward * live, zero).  acc->ret keeps the raw reward under every
 * option, and everything but io->r, phi and rs is what the launch writes without options.  gamma is the one discount of shaping and
 * scaling (algo.gamma).  An option's pointer is its switch, so "scaling without a state" and "shaping without a potential" cannot be
 * asked for and have no error code.
 */
#ifndef POLICY_RECORD_H
#define POLICY_RECORD_H
#include <stdint.h>

typedef struct {
    double *rs;      /* NULL: no RewardScaling; else the state [N][1 + 3P] f64 */
    double *phi;     /* NULL: no distance shaping; else the potential [N][P] f64 */
    double gamma;    /* the one discount of scaling and shaping (read only when rs or phi) */
    double coef;     /* shaping coefficient (read only when phi) */
    double alpha;    /* team sharing coefficient in [0, 1] (read and checked only when team) */
    int32_t team;    /* 0: no sharing; else the TEAM instantiations, alpha = 0 included */
    int32_t pad0;
} policy_record_opts;   /* 48 bytes */

#endif
