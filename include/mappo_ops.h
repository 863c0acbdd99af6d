/*
 * mappo_ops.h -- C ABI of the MI355X (gfx950) fused ops of the MAPPO update/rollout path.
 *
 * These replace torch op sequences of the reference (DHGN/mappo_parallel.py); there is no native boundary in the
 * reference, the seam is the Python methods cited per entry point.  All pointers are DEVICE pointers owned by the
 * caller, kernels are enqueued on the caller's hipStream_t (passed as void*), return value 0 == success
 * (otherwise a hipError_t / MO_ERR_* code).  fp32 throughout (the 1e-4 parity tolerance rules out bf16).
 */
#ifndef MAPPO_OPS_H
#define MAPPO_OPS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MO_ERR_BAD_ARG 20001

/* adjacency source of dhgn_msg_agg_* */
enum { MO_ADJ_TENSOR = 0,   /* actor: the observed adjacency                                            */
       MO_ADJ_ONES = 1,     /* critic: torch.ones_like(adj) over all K neighbours (AttributeDataset, :64-65) */
       MO_ADJ_VALID = 2,    /* critic in a batched rollout: ones over the first kvalid[row] real neighbours  */
       MO_ADJ_BITS = 3 };   /* actor, 0/1 adjacency bit-packed: adj is uint32 [R][P][MO_ADJ_ROW_WORDS(K)], bit j of row i =
                               adj[i][j] (the env's o_adj_bits, include/pe_env.h); identical results to MO_ADJ_TENSOR  */
#define MO_ADJ_ROW_WORDS(K) (((((K) + 31) >> 5) + 3) & ~3)

/*
 * Vertex-level message + mean aggregation of one DHGN relation, never materialising the (R,P,K,E) message:
 *   out[r,i,:] = sum_j abar[r,i,j] * ReLU( W[:, :4] (p[r,i] - q[r',j]) + W[:, 4:8] (p[r,i] - e[r]) + b )
 *   abar = adj / max(sum_j |adj|, 1e-12)            (F.normalize(adj, p=1, dim=-1))
 * i.e. DHGN.coordinate + DHGN.message + the matmul of DHGN.mean_operator (DHGN/mappo_parallel.py:235-239,
 * 323-334, 346-347) for relation 0 (q = p, din = 8, e given), 1 (q = e, K = 1) and 2 (q = obstacles).
 *   R rows, P agents, K neighbours, E features (multiple of 64, <= 256), din in {4, 8};
 *   K = 0 is an empty relation (env_n2n: no obstacles): q and adj may be NULL, out gets zeros, the backward exact zero dW, db;
 *   p [R][P][4] (rows p_row_stride elements apart, likewise e and adj: rows may be slices buffer[:, t] of (N,T,..)
 *   replay-buffer tensors); q [R/q_div][K][4] (q_div p-rows share one q-row: obstacles are static over an episode);
 *   e [R][4] or NULL (din == 4); adj [R][P][K] float (MO_ADJ_TENSOR) or packed words (MO_ADJ_BITS); kvalid [R/q_div] (MO_ADJ_VALID);
 *   W [E][din]; b [E]; out [R][P][E] with out_stride elements between consecutive [E] vectors (out_stride = 3E
 *   writes relation r of an [R][P][3][E] tensor when out points at slot r).
 */
int dhgn_msg_agg_fwd(int32_t R, int32_t P, int32_t K, int32_t E, int32_t din, const float *p, int64_t p_row_stride,
                     const float *q, int64_t q_row_stride, int32_t q_div, const float *e, int64_t e_row_stride, const void *adj,
                     int64_t adj_row_stride, int32_t adj_mode, const int32_t *kvalid, const float *W, const float *b,
                     float *out, int64_t out_stride /* elements between consecutive (row, agent) vectors, >= E */, void *stream);

/*
 * The three relations of DHGN.encoder for the same R rows in ONE launch (DHGN/mappo_parallel.py:256-281): relation r writes
 * slot r of out [R][P][3][E] (out_stride = elements between consecutive (row, agent) vectors, >= 3 E).  Same arithmetic as
 * three dhgn_msg_agg_fwd calls (bit-identical); exists because the rollout's per-tick calls are launch-latency bound.
 */
typedef struct mo_msg_rel {
    int32_t K, din, q_div, adj_mode;
    const float *q; int64_t q_rs;       /* [R/q_div][K][4] */
    const float *e; int64_t e_rs;       /* [R][4] or NULL (din == 4) */
    const void *adj; int64_t adj_rs;    /* MO_ADJ_TENSOR: float [R][P][K]; MO_ADJ_BITS: packed words; else NULL */
    const int32_t *kvalid;              /* MO_ADJ_VALID: [R/q_div] */
    const float *W, *b;                 /* [E][din], [E] */
} mo_msg_rel;
int dhgn_msg_agg3_fwd(const mo_msg_rel *rel /* [3] */, int32_t R, int32_t P, int32_t E, const float *p, int64_t p_row_stride, float *out,
                      int64_t out_stride, void *stream);
/*
 * Actor AND critic of one rollout tick in one launch.  Both networks hold the same DHGN instance (mappo_parallel.py:582-616,
 * critic built on the actor's shared_net), so the messages ReLU(W [p_i - q_j, ..] + b) are the same numbers; only the mean's
 * weights differ: rel[r] carries the ACTOR's adjacency (MO_ADJ_TENSOR or MO_ADJ_BITS; rel[r].kvalid unused), the critic's is
 * all ones (AttributeDataset :64-65) -- for the obstacle relation over the first o_kvalid[row / q_div] neighbours when
 * o_kvalid != NULL (batched rollout), else over all K.  out_actor / out_critic [R][P][3][E], bit-identical to
 * dhgn_msg_agg3_fwd called once per network.
 */
int dhgn_msg_agg3_pair_fwd(const mo_msg_rel *rel /* [3] */, int32_t R, int32_t P, int32_t E, const float *p, int64_t p_row_stride,
                           const int32_t *o_kvalid, float *out_actor, float *out_critic, int64_t out_stride, void *stream);

/* The update's form of the paired launch: the actor's three relations and the critic's relations 0 and 1 (ones adjacency); slot 2
 * of out_critic is NOT written -- in training the critic's obstacle relation averages over all K padded slots and is
 * left to dhgn_msg_agg_ones_sorted_fwd. */
int dhgn_msg_agg3_pair01_fwd(const mo_msg_rel *rel /* [3] */, int32_t R, int32_t P, int32_t E, const float *p, int64_t p_row_stride,
                             float *out_actor, float *out_critic, int64_t out_stride, void *stream);
/* Backward of ONE relation for actor and critic together (shared weights W, b: DHGN/mappo_parallel.py:582-616): the actor's
 * gradient under the float adjacency adj [R][P][K] and the critic's under ones over all K neighbours, summed into dW / db in one
 * pass over the messages (g_ij = [z_ij > 0] (abar_ij gout_actor_i + gout_critic_i / K)).  Arguments as dhgn_msg_agg_bwd. */
int dhgn_msg_agg_bwd_pair(int32_t R, int32_t P, int32_t K, int32_t E, int32_t din, const float *p, int64_t p_row_stride, const float *q,
                          int64_t q_row_stride, int32_t q_div, const float *e, int64_t e_row_stride, const float *adj, int64_t adj_row_stride,
                          const float *W, const float *b, const float *gout_actor, const float *gout_critic, int64_t gout_stride, float *dW,
                          float *db, void *workspace, void *stream);
/* The pair forms above (forward: one wave per row, R > 2048; backward: dhgn_msg_agg_bwd_pair and the packed obstacle rows of
 * dhgn_msg_agg_bwd) have instantiations for a FULL team of 8 with the model's relation shapes (defender K = 8 / din 8, evader K = 1 /
 * din 4, packed obstacle rows with 16 < K and 8 MO_ADJ_ROW_WORDS(K) <= 128), in which those shapes are compile-time constants: the same
 * arithmetic in the same order, bit-identical results.  on = 0 sends every shape to the generic forms (the A/B switch
 * ops.MSG_FULL_TEAM); returns the previous setting.  Not thread-safe against concurrent launches. */
int dhgn_msg_full_team(int on);
/* The same launch, which also writes the position part of DHGN's semantic layer for these rows, pos[r][i][:] = bp + Wp p[r][i]
 * (Wp [E][4]: the first four input columns of semantic_layer.weight, wp_row_stride elements between its rows; mappo_parallel.py:
 * 284-303) -- the addend the embedding part of that layer accumulates into; the same numbers for both networks, written to
 * pos_actor and (if not NULL) pos_critic, [R][P] vectors of E floats, pos_stride (>= E) elements apart (E: dense; 2 E: the right
 * half of a [R P][2 E] operand that a later layer reads as one concatenated input). */
int dhgn_msg_agg3_pair_pos_fwd(const mo_msg_rel *rel /* [3] */, int32_t R, int32_t P, int32_t E, const float *p, int64_t p_row_stride,
                               const int32_t *o_kvalid, float *out_actor, float *out_critic, int64_t out_stride, const float *Wp,
                               int64_t wp_row_stride, const float *bp, float *pos_actor, float *pos_critic, int64_t pos_stride, void *stream);

/*
 * Backward of the above w.r.t. W and b (the inputs are data, they carry no gradient): recomputes the
 * pre-activation, masks with ReLU', reduces over all (r,i,j) without atomics (per-workgroup partials in
 * `workspace`, then one deterministic second pass).  gout [R][P][E]; dW [E][din]; db [E] are OVERWRITTEN.
 * workspace: at least dhgn_msg_agg_bwd_workspace(E, din) bytes.
 */
int64_t dhgn_msg_agg_bwd_workspace(int32_t E, int32_t din);
int dhgn_msg_agg_bwd(int32_t R, int32_t P, int32_t K, int32_t E, int32_t din, const float *p, int64_t p_row_stride,
                     const float *q, int64_t q_row_stride, int32_t q_div, const float *e, int64_t e_row_stride, const void *adj,
                     int64_t adj_row_stride, int32_t adj_mode, const int32_t *kvalid, const float *W, const float *b,
                     const float *gout, int64_t gout_stride, float *dW, float *db, void *workspace, void *stream);

/*
 * The same aggregate for adjacency == ones over a neighbour set shared by q_div consecutive rows (the critic's obstacle relation
 * in training: torch.ones_like(adj) over the padded obstacle slots, AttributeDataset :64-65, q = the episode's obstacles) in
 * O(log K) per (row, agent, feature) instead of O(K): per (q-row, feature) the K pre-activation offsets d_j = W q_j are sorted
 * once, sum_j relu(c - d_j) = m c - prefix_d[m] with m = #{d_j < c} found by a two-level rank search (csrc/mappo_ops.hip
 * k_msg_ones_sorted_*).  din == 4, K <= 255, E a multiple of 16, R a multiple of q_div (dhgn_msg_agg_ones_sorted_ok).
 * fwd: save_m (R P E bytes) and qtab ((R / q_div) E 4 (K + 1) floats) -- both may be NULL without a backward pass -- are what bwd
 * consumes; their layouts are private to the kernel pair ([q-row][block of 16 features][pair][16] and [q-row][block][4][K+1][16]);
 * bwd: dW [E][4], db [E] OVERWRITTEN; partials: scratch of the size dhgn_msg_agg_ones_sorted_workspace reports.
 * Sums are reassociated (prefix sums): results agree with dhgn_msg_agg_fwd/bwd(MO_ADJ_ONES) to fp32 rounding, not bit for bit.
 */
int dhgn_msg_agg_ones_sorted_ok(int32_t R, int32_t P, int32_t K, int32_t E, int32_t din, int32_t q_div);
int64_t dhgn_msg_agg_ones_sorted_workspace(int32_t R, int32_t P, int32_t K, int32_t E, int32_t q_div, int64_t *m_bytes, int64_t *qtab_bytes,
                                           int64_t *partial_bytes);
int dhgn_msg_agg_ones_sorted_fwd(int32_t R, int32_t P, int32_t K, int32_t E, const float *p, int64_t p_row_stride, const float *q,
                                 int64_t q_row_stride, int32_t q_div, const float *W, const float *b, float *out, int64_t out_stride,
                                 uint8_t *save_m, float *qtab, void *stream);
int dhgn_msg_agg_ones_sorted_bwd(int32_t R, int32_t P, int32_t K, int32_t E, const float *p, int64_t p_row_stride, int32_t q_div,
                                 const float *gout, int64_t gout_stride, const uint8_t *save_m, const float *qtab, float *dW, float *db,
                                 void *partials, void *stream);

/*
 * GAE reverse scan + value target + advantage normalisation (DHGN/mappo_parallel.py:643-658):
 *   delta = (r + gamma v[:,1:] - v[:,:-1]) * active ; gae_t = delta_t + gamma lamda gae_{t+1}
 *   v_target = adv + v[:,:-1] ; if use_adv_norm: adv = (adv - mean) / (std_unbiased + 1e-5) * active
 * r, active, adv, v_target [N][T][P]; v [N][T+1][P].  Statistics over all N*T*P elements, accumulated in f64 through per-workgroup
 * partials added in index order (no atomics: the same input gives the same bits every run).
 * stats (device, gae_advnorm_workspace() bytes; the first 4 doubles: sum, sum of squared deviations, mean, std) is scratch + output.
 */
int64_t gae_advnorm_workspace(void);
int gae_advnorm(int32_t N, int32_t T, int32_t P, const float *r, const float *v, const float *active, float gamma,
                float lamda, int32_t use_adv_norm, float *adv, float *v_target, double *stats, void *stream);

/*
 * Value normalisation of the env_3d / env_n2n trainers (algo.use_value_norm; csrc/value_norm.hpp, tests/value_norm_ref.py).
 * vn_state: 3 f64 on the device, (m, q, d), all 0 at the start.  d == 0: mean 0, std 1; else mean = m / d and
 * std = sqrt(max(q / d - mean^2, 1e-2)).  The state never visits the host.
 *
 * gae_advnorm_vn: gae_advnorm on the denormalised values v std + mean, where v[:, t] of t < T is masked by active[:, t] and
 *   v[:, T] by vmask [N][P] (a masked value is exactly 0, not the mean).  With d == 0 adv and v_target are gae_advnorm's bits.
 *   sums (3 f64, device) <- S1 = sum y, S2 = sum y^2, c = the count over the live rows (active != 0) of the fp32 v_target, f64
 *   through per-workgroup partials added in index order (no atomics).  stats: gae_advnorm_vn_workspace() bytes, as gae_advnorm's.
 * value_norm_update: m = beta m + (1 - beta) (S1 / c), q likewise with S2, d = beta d + (1 - beta); nothing when c == 0.
 *   sums may have been summed over ranks.  0 < beta < 1.
 * value_norm_targets: out[i] = (v_target[i] - mean) / std where active[i] != 0, else 0; n elements, pointers 16-byte aligned.
 */
int64_t gae_advnorm_vn_workspace(void);
int gae_advnorm_vn(int32_t N, int32_t T, int32_t P, const float *r, const float *v, const float *active, const float *vmask,
                   const double *vn_state, float gamma, float lamda, int32_t use_adv_norm, float *adv, float *v_target, double *stats,
                   double *sums, void *stream);
int value_norm_update(double *vn_state, const double *sums, double beta, void *stream);
int value_norm_targets(int64_t n, const float *v_target, const float *active, const double *vn_state, float *out, void *stream);

/*
 * The gradient clip and the Adam step of one mini-batch (algo.minibatch_steps of the env_3d / env_n2n trainers; csrc/fused_adam.hpp,
 * tests/fused_adam_ref.py): two launches over flat fp32 arrays of n elements, all pointers 16-byte aligned.
 * state: 6 f64 on the device, (step, b1t, b2t, norm, coef, skipped); at the start (0, 1, 1, 0, 1, 0).  workspace:
 *   fused_adam_workspace() bytes, zero before the first call (per-workgroup partials and the ticket, which the kernel leaves zero).
 * fused_adam_norm: norm = sqrt(sum (double)g[i]^2), f64 per-workgroup partials (fused_adam_grid(n) workgroups, each over a fixed
 *   slice in a fixed order) that the last workgroup to arrive adds in index order: no float atomics, the same bits every run.
 *   coef = min(1, max_norm / (norm + 1e-6)), exactly 1 when max_norm <= 0.  A finite norm: step += 1, b1t *= beta1, b2t *= beta2;
 *   else skipped += 1 and coef = -1, under which fused_adam_step stores nothing.
 * fused_adam_step: per element, in f64 from the fp32 inputs, no contraction, in this order:
 *   gc = g coef; m64 = beta1 m + (1 - beta1) gc; v64 = beta2 v + ((1 - beta2) gc) gc; den = sqrt(v64) / sqrt(1 - b2t) + eps;
 *   p64 = p - lr ((m64 / (1 - b1t)) / den); p, m, v <- (float) of p64, m64, v64.
 * fused_adam_advance_host / fused_adam_rows_host: the end of launch 1 from a sum of squares and the element step of launch 2 on the
 *   host (no device), the same inline functions; rows_host updates p, m, v [n] in place under state's coef, b1t, b2t.
 */
int64_t fused_adam_workspace(void);
int fused_adam_grid(int64_t n);
int fused_adam_norm(int64_t n, const float *g, double *state, void *workspace, double max_norm, double beta1, double beta2, void *stream);
int fused_adam_step(int64_t n, float *p, const float *g, float *m, float *v, const double *state, double lr, double beta1, double beta2,
                    double eps, void *stream);
int fused_adam_advance_host(double *state, double sumsq, double max_norm, double beta1, double beta2);
int fused_adam_rows_host(int64_t n, float *p, const float *g, float *m, float *v, const double *state, double lr, double beta1, double beta2,
                         double eps);

/*
 * Categorical(probs).sample() + log_prob for a batch of rows (DHGN/mappo_parallel.py:446-448) with a counter-based
 * generator (Philox4x32-10; stream = (seed, offset + row)): probs [R][A] -> action [R] int32, logp [R].
 * greedy != 0 gives probs.argmax(-1) instead (choose_action(deterministic=True), :442-444; first maximum wins).
 * A category of probability 0 is never sampled from a row whose total is positive ("Sampling").
 */
int categorical_sample(int32_t R, int32_t A, const float *probs, uint64_t seed, uint64_t offset, int32_t greedy,
                       int32_t *action, float *logp, void *stream);
/* Same with the stream offset kept in device memory (*counter, advanced by R after sampling), so the call can be
 * captured in a hipGraph and replayed with fresh random numbers. */
int categorical_sample_counter(int32_t R, int32_t A, const float *probs, uint64_t seed, uint64_t *counter, int32_t greedy,
                               int32_t *action, float *logp, void *stream);

/*
 * The pre-forward hook of torch.nn.utils.spectral_norm on a small head (the reference's value head, DHGN/mappo_parallel.py:485)
 * as one launch: n_power_iterations times  v = normalize(W^T u), u = normalize(W v)  IN PLACE (as the hook does, also under
 * no_grad), then sigma = u . (W v) and w_eff = W / sigma.  W, w_eff [A][H], u [A], v [H]; A <= 16, H <= 1024;
 * normalize(x) = x / max(||x||_2, eps).  n_power_iterations = 0 is the hook's eval-mode form (u, v untouched).
 */
int spectral_norm_weight(int32_t A, int32_t H, const float *W, float *u, float *v, float eps, int32_t n_power_iterations, float *w_eff,
                         void *stream);

/*
 * Output heads of one rollout tick (choose_action / get_value, DHGN/mappo_parallel.py:422-448), H = 128 features, A <= 16 outputs:
 *   head_linear: y [R][A] = feat [R][H] W^T + b  (the value head: A = 1, y = the rollout's value storage).
 *   head_sample: softmax(feat W^T + b) -> Categorical sample (Philox stream (seed, *counter + row), as categorical_sample_counter)
 *                and its log-probability, or the argmax when greedy != 0: action [R] int32, logp [R]; *counter advances by R.
 *                ticket: one zero-initialised uint32 in device memory owned by the caller (the kernel leaves it zero).
 * One launch each instead of GEMM + bias (+ softmax + sample + counter update); no autograd (rollout only).
 */
int head_linear(int32_t R, int32_t A, int32_t H, const float *feat, const float *W, const float *b, float *y, void *stream);
int head_sample(int32_t R, int32_t A, int32_t H, const float *feat, const float *W, const float *b, uint64_t seed, uint64_t *counter,
                uint32_t *ticket, int32_t greedy, int32_t *action, float *logp, void *stream);

/*
 * torch.nn.GRU cell between the two MFMA GEMMs (reference DHGN/mappo_parallel.py:397,424,434; gate order r, z, n):
 *   r = s(gi_r + gh_r + b_hr) ; z = s(gi_z + gh_z + b_hz) ; hn = gh_n + b_hn ; n = tanh(gi_n + r hn) ; h' = (1-z) n + z h
 * gi = x W_ih^T + b_ih [B][3H], gh = h W_hh^T [B][3H] (bias b_hh [3H] added here), h_prev / h_out [B][H];
 * save (training) [4][B][H] receives r, z, n, hn.  The backward kernel turns dL/dh' (dout + dcarry, either may be
 * NULL... dcarry may be NULL) into dgi, dgh [B][3H] and the direct path dh_direct = dh' * z [B][H].
 */
int gru_gates_fwd(int32_t B, int32_t H, const float *gi, const float *gh, const float *b_hh, const float *h_prev, float *h_out,
                  float *save, void *stream);
int gru_gates_bwd(int32_t B, int32_t H, const float *dout, const float *dcarry, const float *save, const float *h_prev, float *dgi,
                  float *dgh, float *dh_direct, void *stream);

/*
 * Whole-sequence GRU layer in one persistent launch (H = 128 only): gi [T B][3H] is the input projection
 * x W_ih^T + b_ih (one MFMA GEMM), the recurrence over T runs inside the kernel with W_hh held in registers as
 * v_mfma_f32_16x16x4_f32 operands and the h tile (16 batch rows per workgroup) in LDS.  out [T][B][H] time-major.
 * save (or NULL: no backward): gru_seq_save_elems(T, B) floats, the gates (r, z, n, hn) of every step in the kernel pair's own
 * lane order -- opaque, only gru_seq_bwd reads it.  The backward kernel consumes dout [T][B][H] (dL/d out) and produces
 * dgi [T B][3H] = (dr, dz, dn), dh0 [B][H] and, for the recurrent weight gradient dW_hh = [dr dz dnr]^T h_prev, EITHER
 * dgh [T][B][3H] = (dr, dz, dnr) time-major OR only dnr [T][B][H] (exactly one of the two pointers is non-NULL).  The second
 * form stores dr, dz once: valid when dgi itself is time-major (gi_agents == 0), the caller then takes the first 2H columns of
 * dgh from dgi.
 * gi_agents: row order of gi and dgi.  0: time-major, row t B + b.  P > 0: the order of the encoder's output rows
 * (episode n, step t, agent p) with sequence b = n P + p, row ((b / P) T + t) P + b % P (B a multiple of P) -- the input
 * projection and its gradients then run on the embedding as it lies in memory, without the permuted copies around the GRU
 * (_sequence_features, DHGN/mappo_parallel.py:426-437).
 * All pointers 16-byte aligned.
 */
int64_t gru_seq_save_elems(int32_t T, int32_t B);
/* Several independent layers in ONE launch (the actor's and the critic's layer of the same depth, for every mini-batch of a group:
 * same T and gi_agents; own weights, inputs and B): at a data-parallel rank's share of the batch one layer is a few dozen workgroups
 * that run T sequential steps, and a launch takes as long as at full size; together the layers fill the chip in the same time.
 * Records of HOST memory holding DEVICE pointers, meaning as in gru_seq_fwd / gru_seq_bwd. */
#define MO_GRU_MAX_NETS 24
#define MO_GRU_CELL_MAX_NETS 4
/* B (per record): this layer's number of sequences, <= the launch's B argument (0: the launch's B) -- the layers of one launch may be
 * ragged (the last mini-batch of an epoch is smaller); gi / out / save / dgi / ... of a record are sized by ITS B. */
typedef struct mo_gru_seq_net { const float *gi, *w_hh, *b_hh, *h0; float *out, *save; int32_t B, pad0; } mo_gru_seq_net;
typedef struct mo_gru_seq_bwd_net {
    const float *dout, *save, *out, *h0, *w_hh;
    float *dgi, *dgh, *dnr, *dh0, *db_ih, *db_hh;
    void *workspace;   /* >= gru_seq_bwd_workspace(B) bytes when db_ih / db_hh are requested; one per record */
    int32_t B, pad0;
} mo_gru_seq_bwd_net;
int gru_seq_fwd_multi(int32_t n_nets, const mo_gru_seq_net *nets, int32_t T, int32_t B, int32_t H, int32_t gi_agents, void *stream);
int gru_seq_bwd_multi(int32_t n_nets, const mo_gru_seq_bwd_net *nets, int32_t T, int32_t B, int32_t H, int32_t gi_agents, void *stream);
/* The same recurrences in fp32 arithmetic on the bf16 matrix pipe (exact three-way operand splits, csrc/sb_gru_seq.hpp): same records,
 * same (interchangeable) save layout, results equal to the fp32-MFMA kernels' to fp32 rounding.  `runtime.matmul: split_bf16`. */
int gru_seq_split_fwd_multi(int32_t n_nets, const mo_gru_seq_net *nets, int32_t T, int32_t B, int32_t H, int32_t gi_agents, void *stream);
int gru_seq_split_bwd_multi(int32_t n_nets, const mo_gru_seq_bwd_net *nets, int32_t T, int32_t B, int32_t H, int32_t gi_agents, void *stream);
int gru_seq_fwd(int32_t T, int32_t B, int32_t H, const float *gi, const float *w_hh, const float *b_hh, const float *h0, float *out,
                float *save, int32_t gi_agents, void *stream);
int64_t gru_seq_bwd_workspace(int32_t B);
/* db_ih / db_hh [3H] (optional, both or none): column sums of dgi / dgh, reduced from per-workgroup partials in
 * `workspace` (>= gru_seq_bwd_workspace(B) bytes) by a deterministic second pass. */
int gru_seq_bwd(int32_t T, int32_t B, int32_t H, const float *dout, const float *save, const float *out, const float *h0,
                const float *w_hh, float *dgi, float *dgh, float *dnr, float *dh0, float *db_ih, float *db_hh, int32_t gi_agents,
                void *workspace, void *stream);

/*
 * One torch.nn.GRU layer step for a large batch without autograd (the rollout's choose_action / get_value,
 * DHGN/mappo_parallel.py:422-425 with seq_len 1): h_out = GRUCell(x, h_prev), both projections and the gate math in
 * one persistent launch (weights in registers as fp32 MFMA operands).  I = H = 128; x, h_prev, h_out [B][H] dense;
 * w_ih, w_hh [3H][H] (torch gate order r, z, n); h_out must not alias x or h_prev.
 */
int gru_cell_fwd(int32_t B, int32_t H, const float *x, const float *h_prev, const float *w_ih, const float *w_hh, const float *b_ih,
                 const float *b_hh, float *h_out, void *stream);
/* Several independent cells of one shape (actor and critic) in ONE launch; records of HOST memory holding DEVICE pointers, meaning as
 * in gru_cell_fwd (n_nets <= MO_GRU_CELL_MAX_NETS).  The persistent workgroups (one per CU) are divided between the cells. */
typedef struct mo_gru_cell_net { const float *x, *h_prev, *w_ih, *w_hh, *b_ih, *b_hh; float *h_out; } mo_gru_cell_net;
int gru_cell_fwd_multi(int32_t n_nets, const mo_gru_cell_net *nets, int32_t B, int32_t H, void *stream);
/* The same cells in fp32 ARITHMETIC ON THE bf16 MATRIX PIPE: every fp32 operand is split exactly into three bf16 pieces
 * (x = x1 + x2 + x3) and a product is the six piece products with i + j <= 4 on v_mfma_f32_16x16x32_bf16 with fp32 accumulation --
 * the dropped terms are below one fp32 rounding of the product; inputs, outputs and the state stay fp32 and the error against f64
 * equals the fp32-MFMA kernel's (csrc/mappo_ops.hip k_gru_cell_sb).  Same records and results to fp32 rounding as
 * gru_cell_fwd_multi, EXCEPT that h_out must not alias h_prev or x (two workgroups share a row tile). */
int gru_cell_split_fwd_multi(int32_t n_nets, const mo_gru_cell_net *nets, int32_t B, int32_t H, void *stream);
/* Y[R][128] = act(X[R][K] W[128][K]^T + bias [+ C]) in the same split arithmetic (fp32 in, fp32 out, fp32 accumulation; K in {128, 256,
 * 384}): the rollout's Linear layers (torch.nn.Linear of DHGN/mappo_parallel.py:148-233).  bias, C may be NULL; C may be Y (accumulate in
 * place); relu != 0 applies max(., 0) last.  ldx, ldw, ldc, ldy: row strides in floats (multiples of 4: X, C, Y may be column blocks of
 * wider matrices); all pointers 16-byte aligned. */
int sb_gemm_n128(int64_t R, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias, int32_t relu, const float *C,
                 int64_t ldc, float *Y, int64_t ldy, void *stream);
/* The same for N outputs: (N, K) in {(128, 128), (128, 256), (128, 384), (256, 128), (384, 128)} -- (384, 128) is a GRU input projection
 * x W_ih^T + b_ih, (256, 128) the input gradient of an FCRA layer. */
int sb_gemm(int64_t R, int32_t N, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias, int32_t relu, const float *C,
            int64_t ldc, float *Y, int64_t ldy, void *stream);
/* The rollout encoder's tail as ONE launch (DHGN.forward_pair; DHGN/mappo_parallel.py:148-203):
 *   Y[s] = sum over r = 0, 1, 2 of Ws[:, 128 r .. 128 r + 127] relu(w_agg m3[s][r] + b_agg) + C[s]      for the Rs semantic rows s,
 * bit-identical to sb_gemm(3 Rs, 128, 128, m3, 128, w_agg, 128, b_agg, 1, NULL, 0, emb, 128) followed by
 * sb_gemm(Rs, 128, 384, emb, 384, Ws, ldw, NULL, 0, C, ldc, Y, ldy) without the (Rs, 384) embedding in memory.  m3 [Rs][3][128] (row stride
 * ldx >= 384: a row's three relation vectors are contiguous); w_agg [128][128] and b_agg [128] dense; Ws [128][384] (row stride ldw: a
 * column block of the semantic layer's weight); C, Y [Rs][128] (row strides ldc, ldy; C may be Y, m3 must not overlap Y).  Strides in
 * floats, multiples of 4; all pointers 16-byte aligned. */
int sb_encoder_tail(int64_t Rs, const float *m3, int64_t ldx, const float *w_agg, const float *b_agg, const float *Ws, int64_t ldw, const float *C,
                    int64_t ldc, float *Y, int64_t ldy, void *stream);
/* sb_gemm (N = 128, K in {128, 256}) that also writes the sign bits of its result: y_sign_bits[row * ld_bytes + j], bit k = (Y[row][8 j + k] > 0),
 * N / 8 bytes per row (rows ld_bytes apart: Y may be a column block of a wider matrix and the bytes a column block of its bit matrix).
 * Behind the ReLU epilogue these are relu'(Y): sb_gemm_masked_bits reads them in the backward of the layer that consumes Y. */
int sb_gemm_signs(int64_t R, int32_t N, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias, int32_t relu, const float *C,
                  int64_t ldc, float *Y, int64_t ldy, uint8_t *y_sign_bits, int64_t ld_bytes, void *stream);
/* The input gradient of a Linear layer whose INPUT is the output of a ReLU layer, with that ReLU's backward and the bias gradient of
 * the layer in front of it in the same pass (autograd's threshold_backward + sum(0) of DHGN/mappo_parallel.py:148-233's relu(Linear)
 * chains):  Y = (X W^T) * (M > 0) on the first mask_cols columns (a multiple of 128; the others are plain X W^T),  colsum[N] = column
 * sums of Y.  M [R][N] (row stride ldm) is the saved ReLU output; (N, K) in {(256, 128), (384, 128), (128, 384)}.  The column sums are
 * reduced from per-workgroup partials in `workspace` (>= sb_gemm_masked_workspace(N) bytes) in a fixed order: same bits every run. */
int64_t sb_gemm_masked_workspace(int32_t N);
int sb_gemm_masked(int64_t R, int32_t N, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const float *M, int64_t ldm,
                   int32_t mask_cols, float *Y, int64_t ldy, float *colsum, void *workspace, void *stream);
/* The same with the mask as sign bits (sb_gemm_signs' layout, N / 8 bytes per row, row stride ld_bytes): 1 bit per element read instead of 4 bytes. */
int sb_gemm_masked_bits(int64_t R, int32_t N, int32_t K, const float *X, int64_t ldx, const float *W, int64_t ldw, const uint8_t *sign_bits,
                        int64_t ld_bytes, int32_t mask_cols, float *Y, int64_t ldy, float *colsum, void *workspace, void *stream);
/* The update encoder's tail (DHGN._after_messages) as one launch each way.
 * sb_encoder_tail_train: sb_encoder_tail that also writes what the backward reads -- emb [Rs][384] (row stride lde floats, a multiple of 4:
 * relu(w_agg m3[s][r] + b_agg) at columns 128 r ..) and its sign bits emb_sign_bits [Rs][48] (row stride ld_bytes; sb_gemm_signs' layout per
 * relation row: byte 16 r + j, bit k = emb[s][128 r + 8 j + k] > 0).  Bit-identical to sb_gemm_signs(3 Rs, 128, 128, ..) + sb_gemm(Rs, 128, 384, ..).
 * sb_encoder_tail_bwd: for the gradient g [Rs][128] (row stride ldg) of Y,
 *   ga[s][r] = (g[s] Ws[:, 128 r .. 128 r + 127]) * (emb[s][r] > 0)  -> ga [Rs][384] (row stride ldga),   colsum[384] = column sums of ga,
 *   d_m3[s][r] = ga[s][r] w_agg                                      -> d_m3 [Rs][384] (row stride ldd),
 * bit-identical to sb_gemm_masked_bits(Rs, 384, 128, g, ldg, Ws^T, ..) followed by sb_gemm(3 Rs, 128, 128, ga, 128, w_agg^T, ..), the column
 * sums included (per-workgroup partials in `workspace`, >= sb_encoder_tail_bwd_workspace() bytes, reduced in a fixed order).  Ws and w_agg
 * are the weights as stored (no transposed copies).  Strides in floats, multiples of 4; all float pointers 16-byte aligned. */
int sb_encoder_tail_train(int64_t Rs, const float *m3, int64_t ldx, const float *w_agg, const float *b_agg, const float *Ws, int64_t ldw, const float *C,
                          int64_t ldc, float *Y, int64_t ldy, float *emb, int64_t lde, uint8_t *emb_sign_bits, int64_t ld_bytes, void *stream);
int64_t sb_encoder_tail_bwd_workspace(void);
int sb_encoder_tail_bwd(int64_t Rs, const float *g, int64_t ldg, const float *Ws, int64_t ldw, const float *w_agg, const uint8_t *emb_sign_bits,
                        int64_t ld_bytes, float *ga, int64_t ldga, float *d_m3, int64_t ldd, float *colsum, void *workspace, void *stream);

/*
 * PPO clipped-surrogate policy loss and clipped value loss of one mini-batch with their gradients
 * (DHGN/mappo_parallel.py:692-706):
 *   ratio = exp(logp_now - logp_old); actor = -min(ratio adv, clamp(ratio, 1-eps, 1+eps) adv) - entropy_coef entropy
 *   critic = use_value_clip ? max((clamp(v_now - v_old, -eps, eps) + v_old - v_target)^2, (v_now - v_target)^2) : (v_now - v_target)^2
 *   losses[0] = sum(actor * active) / active_sum ; losses[1] = sum(critic * active) / active_sum
 * grad_* = d(losses[0] + losses[1]) / d(logp_now | entropy | values_now), autograd's tie rules for min / max / clamp.
 * n elements (= episodes x T x P) per tensor, dense fp32; active_sum: device scalar sum(active); workspace >=
 * ppo_loss_workspace() bytes.  Deterministic (f64 partial sums added in a fixed order).
 */
int64_t ppo_loss_workspace(void);
int ppo_loss_fwd_bwd(int64_t n, const float *logp_now, const float *entropy, const float *logp_old, const float *adv, const float *active,
                     const float *values_now, const float *values_old, const float *v_target, const float *active_sum, float epsilon,
                     float entropy_coef, int32_t use_value_clip, float *losses, float *grad_logp, float *grad_entropy, float *grad_values,
                     void *workspace, void *stream);
/* The same losses from the policy's probabilities prob[.., A] (A <= 16): torch.distributions.Categorical(prob).log_prob(action) and
 * .entropy() (DHGN/mappo_parallel.py:451-456: renormalisation, the clamp of probs_to_logits, the gather) are evaluated inside the pass
 * and the gradient with respect to prob comes out instead of grad_logp / grad_entropy.  The n = d0 d1 d2 rows are indexed (i0, i1, i2);
 * prob and grad_prob are read / written at i0 p_s0 + i1 p_s1 + i2 p_s2 (+ k, k < A), values_now at i0 v_s0 + i1 v_s1 + i2 v_s2 (strides in
 * floats: the heads' outputs are time-major views); action (float-valued indices) and the other operands are dense in row order. */
int ppo_loss_prob_fwd_bwd(int64_t n, int32_t A, const float *prob, float *grad_prob, int64_t d1, int64_t d2, int64_t p_s0, int64_t p_s1, int64_t p_s2,
                          const float *action, const float *logp_old, const float *adv, const float *active, const float *values_now, int64_t v_s0,
                          int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target, const float *active_sum, float epsilon,
                          float entropy_coef, int32_t use_value_clip, float *losses, float *grad_values, void *workspace, void *stream);

/*
 * Diagonal-Gaussian policy of the env_3d trainer (csrc/gauss_policy.hpp), A <= 16 action dimensions on H = 128 features.
 * gauss_head_sample: mu = feat [R][H] W^T + b, a = mu + exp(log_std) z with z ~ N(0, 1) from the Philox stream of head_sample (row r:
 *   counter *counter + r, key seed; noise block j = dims 4 j .. 4 j + 3 uses counter word c2 = j; u = ((o >> 8) + 1/2) 2^-24 per output
 *   word, Box-Muller on (o0, o1) and (o2, o3)); a = mu when greedy != 0 (z = 0).  action [R][A] fp32 (unclipped), env_action [R][A]
 *   f64 = clamp(a, -1, 1), logp [R] = sum_d (-z_d^2 / 2 - log_std_d - ln sqrt(2 pi)).  *counter advances by R; ticket as head_sample.
 * ppo_loss_gauss_fwd_bwd: the losses of ppo_loss_prob_fwd_bwd with logp_now = Normal(mu, exp(log_std)).log_prob(action).sum(-1) and
 *   entropy = Normal.entropy().sum(-1); mu / grad_mu [.., A] at i0 m_s0 + i1 m_s1 + i2 m_s2, values_now as in ppo_loss_prob_fwd_bwd;
 *   action [n][A] dense.  Also writes grad_log_std [A] = d losses[0] / d log_std (f64 per-block partials, fixed order);
 *   workspace >= ppo_loss_gauss_workspace() bytes.
 */
int gauss_head_sample(int32_t R, int32_t A, int32_t H, const float *feat, const float *W, const float *b, const float *log_std, uint64_t seed,
                      uint64_t *counter, uint32_t *ticket, int32_t greedy, float *action, double *env_action, float *logp, void *stream);
int64_t ppo_loss_gauss_workspace(void);
int ppo_loss_gauss_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1, int64_t m_s2,
                           const float *log_std, const float *action, const float *logp_old, const float *adv, const float *active,
                           const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                           const float *active_sum, float epsilon, float entropy_coef, int32_t use_value_clip, float *losses, float *grad_values,
                           float *grad_log_std, void *workspace, void *stream);

/*
 * The same policy with a state-dependent log-std and / or tanh squashing.
 * gauss_head_sample_ex: ls_raw = feat W_ls^T + b_ls (state mode: W_ls [A][H] and b_ls [A] non-NULL, log_std NULL, A <= 8) or the
 *   log_std [A] vector (param mode: W_ls = b_ls = NULL, A <= 16); ls = clamp(ls_raw, log_std_min, log_std_max) (min < max, +-inf allowed);
 *   u = mu + exp(ls) z with the noise, counter and ticket of gauss_head_sample.  action [R][A] = u (both squash modes), env_action f64 =
 *   clamp(u, -1, 1) (squash 0) or tanh(u) (squash 1), logp = sum_d (-z_d^2 / 2 - ls_d - ln sqrt(2 pi)) - squash * sum_d c(u_d) with
 *   c(u) = log(1 - tanh(u)^2) = 2 (ln 2 - u - softplus(-2 u)).  Param mode, squash 0 and bounds -inf / +inf give gauss_head_sample's bits.
 * ppo_loss_gauss_ex_fwd_bwd: ppo_loss_gauss_fwd_bwd with logp_now = Normal(mu, exp(ls)).log_prob(action).sum(-1) - squash * sum c(action)
 *   (c carries no gradient), entropy = sum_d (1/2 + ln sqrt(2 pi) + ls_d), ls = clamp(ls_raw, log_std_min, log_std_max).  ls_raw [.., A]
 *   at i0 l_s0 + i1 l_s1 + i2 l_s2: per row (state mode; grad_log_std written per row at the same offsets) or, with l_s0 = l_s1 = l_s2 =
 *   0, one [A] vector (param mode; grad_log_std [A] summed through the f64 per-block partials).  The ls_raw gradient is 0 where ls_raw
 *   lies outside [log_std_min, log_std_max].  workspace >= ppo_loss_gauss_ex_workspace() bytes.
 * squash 2, the direction-vector head (algo.gauss_squash: direction; csrc/direction_action.hpp): A must be 4,
 *   u = (u_x, u_y, u_z, s); action [R][4] = u, env_action [R][3] f64 = (atan2(u_y, u_x) / pi, atan2(u_z, hypot(u_x, u_y)) / (pi / 2), s),
 *   each clamped to [-1, 1]; logp is the plain Normal log-density of u over its four dimensions (the map belongs to the environment: no
 *   Jacobian term).  All four Philox words of the row's one call are used.  ppo_loss_gauss_ex_fwd_bwd takes squash 2 as squash 0.
 */
int gauss_head_sample_ex(int32_t R, int32_t A, int32_t H, const float *feat, const float *W, const float *b, const float *W_ls, const float *b_ls,
                         const float *log_std, float log_std_min, float log_std_max, int32_t squash, uint64_t seed, uint64_t *counter,
                         uint32_t *ticket, int32_t greedy, float *action, double *env_action, float *logp, void *stream);
int64_t ppo_loss_gauss_ex_workspace(void);
int ppo_loss_gauss_ex_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1, int64_t m_s2,
                              const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2, float log_std_min,
                              float log_std_max, int32_t squash, const float *action, const float *logp_old, const float *adv, const float *active,
                              const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                              const float *active_sum, float epsilon, float entropy_coef, int32_t use_value_clip, float *losses, float *grad_values,
                              void *workspace, void *stream);

/*
 * Update diagnostics (algo.update_diagnostics / algo.target_kl; csrc/ppo_diag.hpp).  The four *_diag calls are
 * the plain calls -- same arguments, same losses and gradients byte for byte, the same two launches -- plus `double *diag`: eight f64
 * sums over the call's live rows (active != 0, each counted once), ADDED to diag[0..7] on the device (zero it once per update):
 *   0 the count; 1 expm1(lr) - lr in f64 (k3 estimator of KL(old || new), lr = fp32 logp_now - logp_old); 2 [ratio < 1 - eps or
 *   ratio > 1 + eps] (ratio = expf(lr), the loss's own fp32 comparisons); 3 entropy; 4 v_target; 5 v_target^2; 6 (v_target - v_now)^2;
 *   7 ratio.  logp_now and entropy are the fp32 values the row hands to the loss (formed inside the pass by the prob / gauss calls).
 * Deterministic: f64 per-block partials behind the loss partials, added in a fixed order by eight more workgroups of the finish
 * launch; no atomics.  workspace >= ppo_loss_diag_workspace() bytes (ppo_loss / ppo_loss_prob) or ppo_loss_gauss_diag_workspace()
 * bytes (ppo_loss_gauss / ppo_loss_gauss_ex).  ppo_loss_gauss_ex_fwd_bwd_diag in state mode takes A <= 8, the state-mode head's limit.
 * ppo_ratio: lr[i] = logp_now[i] - logp_old[i] and ratio[i] = expf(lr[i]) as the loss forms them (fp32), for checks and probes.
 * ppo_diag_rows_host: the row step on the host (no device): terms [n][8], the eight terms of row i, 0 for an inactive row.
 */
int64_t ppo_loss_diag_workspace(void);
int64_t ppo_loss_gauss_diag_workspace(void);
int ppo_loss_fwd_bwd_diag(int64_t n, const float *logp_now, const float *entropy, const float *logp_old, const float *adv, const float *active,
                          const float *values_now, const float *values_old, const float *v_target, const float *active_sum, float epsilon,
                          float entropy_coef, int32_t use_value_clip, float *losses, float *grad_logp, float *grad_entropy, float *grad_values,
                          void *workspace, void *stream, double *diag);
int ppo_loss_prob_fwd_bwd_diag(int64_t n, int32_t A, const float *prob, float *grad_prob, int64_t d1, int64_t d2, int64_t p_s0, int64_t p_s1,
                               int64_t p_s2, const float *action, const float *logp_old, const float *adv, const float *active,
                               const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                               const float *active_sum, float epsilon, float entropy_coef, int32_t use_value_clip, float *losses,
                               float *grad_values, void *workspace, void *stream, double *diag);
int ppo_loss_gauss_fwd_bwd_diag(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                                int64_t m_s2, const float *log_std, const float *action, const float *logp_old, const float *adv,
                                const float *active, const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old,
                                const float *v_target, const float *active_sum, float epsilon, float entropy_coef, int32_t use_value_clip,
                                float *losses, float *grad_values, float *grad_log_std, void *workspace, void *stream, double *diag);
int ppo_loss_gauss_ex_fwd_bwd_diag(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                                   int64_t m_s2, const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2,
                                   float log_std_min, float log_std_max, int32_t squash, const float *action, const float *logp_old,
                                   const float *adv, const float *active, const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2,
                                   const float *values_old, const float *v_target, const float *active_sum, float epsilon, float entropy_coef,
                                   int32_t use_value_clip, float *losses, float *grad_values, void *workspace, void *stream, double *diag);
int ppo_ratio(int64_t n, const float *logp_now, const float *logp_old, float *lr, float *ratio, void *stream);
int ppo_diag_rows_host(int64_t n, const float *lr, const float *ratio, const float *ent, const float *v_now, const float *v_tgt,
                       const float *active, float eps, double *terms);

/*
 * Imitation warm start of the env_3d / env_n2n trainers (algo.bc_iterations; csrc/imitation.hpp; specification: tests/imitation_ref.py).
 * bc_loss_gauss_fwd_bwd: the Gaussian negative log-likelihood of the teacher's action `target` [n][A] under mu and
 * ls = clamp(ls_raw, log_std_min, log_std_max), with the views and the ls_raw modes of ppo_loss_gauss_ex_fwd_bwd:
 *   d = target - mu (wrap0 != 0: dimension 0 taken modulo 2 into [-1, 1)), la = sum_a 0.5 d^2 exp(-2 ls) + (fit_std ? ls : 0),
 *   losses[0] = sum_i active la / sum active; grad_mu = -(active / sum active) d exp(-2 ls); grad_log_std (per row in state mode, [A] in
 *   param mode) = (active / sum active)(1 - d^2 exp(-2 ls)) on the closed range of the bounds with fit_std, exactly 0 otherwise.
 * bc_loss_cat_fwd_bwd: the cross-entropy -log clamp(p[label], eps32, 1 - eps32) of the renormalised row, exactly as
 * ppo_loss_prob_fwd_bwd forms its log-probability, with its gradient through the clamp and the normalisation; label [n] as floats.
 * Both: losses[1], grad_values are the critic part of the PPO calls with the same bits; sums (NULL: skipped) [2] f64, to which the call
 * ADDS sum_i active sum_a d^2 (gauss) or the number of live rows whose argmax (lowest index on ties) is the label (cat), and sum active.
 * workspace >= bc_loss_workspace() bytes.  Deterministic (f64 per-block partials added in a fixed order, no atomics).
 * bc_loss_gauss_ex_fwd_bwd: bc_loss_gauss_fwd_bwd with `metric`: 0 the call above, bit for bit (it forwards here); 1 (A >= 3, the
 *   direction-vector head) sums[0] receives sum_i active angle_i instead, angle_i = atan2f(|mu x t|, mu . t) in fp32 radians between
 *   mu[:3] and target[:3] of row i, pi / 2 where |mu[:3]|^2 is 0; wrap0 is then ignored.  Losses and gradients do not depend on metric.
 * e3d_bc_select / n2n_bc_select: one launch per rollout tick.  guide: the scripted pursuers' actions ([N][P][3] f64 / [N][P] int32);
 * the label of every row goes to a_star + n * row_stride (floats) + the row's offset -- (float)g, or with squash == 1
 * (float)atanh(clamp(g, -bound, bound)) evaluated in f64, or (float)k -- and the guide's action replaces the network's
 * (env_action / a_n) in the environments with follow[n] != 0.  Nothing else is written.  e3d_bc_select with squash == 2: the label has
 * four floats per pursuer (row_stride >= 4 P), (cos gam cos phi, cos gam sin phi, sin gam, g2) with phi = g0 pi, gam = g1 pi / 2 in f64
 * rounded to fp32; bound is ignored.
 */
int64_t bc_loss_workspace(void);
int bc_loss_gauss_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1, int64_t m_s2,
                          const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2, float log_std_min, float log_std_max,
                          int32_t fit_std, int32_t wrap0, const float *target, const float *active, const float *values_now, int64_t v_s0,
                          int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target, const float *active_sum, float epsilon,
                          int32_t use_value_clip, float *losses, float *grad_values, double *sums, void *workspace, void *stream);
int bc_loss_gauss_ex_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                             int64_t m_s2, const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2, float log_std_min,
                             float log_std_max, int32_t fit_std, int32_t wrap0, int32_t metric, const float *target, const float *active,
                             const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                             const float *active_sum, float epsilon, int32_t use_value_clip, float *losses, float *grad_values, double *sums,
                             void *workspace, void *stream);
int bc_loss_cat_fwd_bwd(int64_t n, int32_t A, const float *prob, float *grad_prob, int64_t d1, int64_t d2, int64_t p_s0, int64_t p_s1, int64_t p_s2,
                        const float *label, const float *active, const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2,
                        const float *values_old, const float *v_target, const float *active_sum, float epsilon, int32_t use_value_clip,
                        float *losses, float *grad_values, double *sums, void *workspace, void *stream);
int e3d_bc_select(int32_t N, int32_t P, const double *guide, const uint8_t *follow, int32_t squash, double bound, double *env_action, float *a_star,
                  int64_t row_stride, void *stream);
int n2n_bc_select(int32_t N, int32_t P, const int32_t *guide, const uint8_t *follow, int32_t *a_n, float *a_star, int64_t row_stride, void *stream);

/*
 * Teacher-regularised PPO of the env_3d / env_n2n trainers (algo.bc_coef; csrc/kickstart.hpp; specification: tests/kickstart_ref.py).
 * ppo_bc_loss_gauss_fwd_bwd: the row of ppo_loss_gauss_ex_fwd_bwd (squash, the bounds, the ls_raw modes and views as there) and the row
 * of bc_loss_gauss_ex_fwd_bwd (target, fit_std, wrap0, metric as there) on mu, ls and 1 / sigma^2 loaded once:
 *   losses[0] = sum_i active la_ppo / sum active + coef sum_i active la_bc / sum active, losses[1] and grad_values: the critic part of
 *   ppo_loss_gauss_ex_fwd_bwd with the same bits; grad_mu = grad_mu_ppo + coef grad_mu_bc, grad_log_std = grad_ls_ppo + coef grad_ls_bc
 *   (per row in state mode, [A] in param mode; the imitation part exactly 0 without fit_std, the whole 0 outside the closed bounds).
 * ppo_bc_loss_cat_fwd_bwd: the row of ppo_loss_prob_fwd_bwd and the row of bc_loss_cat_fwd_bwd on one normalised row of prob;
 *   grad_prob is the sum of the two gradients through the shared normalisation; the critic part has ppo_loss_prob_fwd_bwd's bits.
 * Both: coef finite and >= 0; sums (NULL: skipped) [3] f64, to which the call ADDS the imitation call's metric sum (sum_i active sum_a
 * d*^2, or with metric 1 sum_i active angle_i; the label hits), sum active, and sum_i active la_bc (the unweighted imitation loss);
 * diag (NULL: skipped; gauss with a per-row ls_raw: A 3 or 4 only, the widths a policy of this feature has) [8] f64, to which the call
 * ADDS the PPO row's update diagnostics exactly as the _diag PPO calls do; losses and
 * gradients do not depend on sums or diag.  workspace >= ppo_bc_loss_workspace() bytes.  Two launches; deterministic (f64 per-block
 * partials added in a fixed order, no atomics).  A bad argument returns MO_ERR_BAD_ARG before anything is launched.
 */
int64_t ppo_bc_loss_workspace(void);
int ppo_bc_loss_gauss_fwd_bwd(int64_t n, int32_t A, const float *mu, float *grad_mu, int64_t d1, int64_t d2, int64_t m_s0, int64_t m_s1,
                              int64_t m_s2, const float *ls_raw, float *grad_log_std, int64_t l_s0, int64_t l_s1, int64_t l_s2, float log_std_min,
                              float log_std_max, int32_t squash, int32_t fit_std, int32_t wrap0, int32_t metric, const float *action,
                              const float *target, const float *logp_old, const float *adv, const float *active, const float *values_now,
                              int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target, const float *active_sum,
                              float epsilon, float entropy_coef, float coef, int32_t use_value_clip, float *losses, float *grad_values, double *sums,
                              double *diag, void *workspace, void *stream);
int ppo_bc_loss_cat_fwd_bwd(int64_t n, int32_t A, const float *prob, float *grad_prob, int64_t d1, int64_t d2, int64_t p_s0, int64_t p_s1,
                            int64_t p_s2, const float *action, const float *label, const float *logp_old, const float *adv, const float *active,
                            const float *values_now, int64_t v_s0, int64_t v_s1, int64_t v_s2, const float *values_old, const float *v_target,
                            const float *active_sum, float epsilon, float entropy_coef, float coef, int32_t use_value_clip, float *losses,
                            float *grad_values, double *sums, double *diag, void *workspace, void *stream);

/*
 * Team attention of the env_3d actor (algo.e3d_comm: attention; csrc/team_attention.hpp; specification: tests/team_attention_ref.py;
 * DESIGN.md section 7m): one round of masked multi-head attention inside every group of P consecutive rows (the pursuers of one
 * environment at one tick), 1 <= P <= 64, H in {1, 2, 4, 8} heads of D = 128 / H columns, fp32.
 * team_comm_mask: words[g * words_stride + i] = the hearing set M_i of pursuer i of group g as a 64-bit word, bit j set iff j == i, or
 *   live[g][i], live[g][j], pp_adj[g][i][j] and pp_adj[g][j][i] are all non-zero.  pp_adj [G][P][P] and live [G][P] are dense inside a
 *   group; the strides are in elements between groups (words may be a time slice of an (N, T, P) buffer).  One launch.
 * team_attention_fwd: qkv [G P][384] = q | k | v (dense rows, 16-byte aligned), head h in columns [h D, (h + 1) D) of each third:
 *   s_ij = q_i^h . k_j^h / sqrt(D),  a_i. = softmax over j in M_i of s_ij (the maximum subtracted),  out [G P][128]: o_i^h = sum_j a_ij v_j^h,
 *   lse [G][H][P] (NULL: not written) = log sum_{j in M_i} exp(s_ij).  Of words [G][P] the bits at or above P are ignored and bit i is
 *   taken as set.  A query that hears only itself returns v_i exactly.
 * team_attention_bwd: with a_ij = exp(s_ij - lse_i) recomputed (no [G][H][P][P] tensor exists anywhere), d_qkv [G P][384] = dQ | dK | dV:
 *   dV_j = sum_i a_ij dO_i,  dS_ij = a_ij (dO_i . v_j - sum_l a_il dO_i . v_l),  dQ_i = sum_j dS_ij k_j / sqrt(D),  dK_j = sum_i dS_ij q_i / sqrt(D).
 * A group never spans workgroups and every sum over i or j is taken by one lane in index order: no atomics, the same bits from run to
 * run, and group g's result does not depend on G or on the other groups of the launch.  G = 0 succeeds and writes nothing; P, H, G out
 * of range, a NULL or misaligned pointer or a stride below the dense one return MO_ERR_BAD_ARG before any launch or write.
 * The _host entries run the same row functions on the host with no device (CPU tests, a sanitizer driver).
 */
int team_comm_mask(int64_t G, int32_t P, const float *pp_adj, int64_t adj_stride, const float *live, int64_t live_stride, int64_t *words,
                   int64_t words_stride, void *stream);
int team_attention_fwd(int64_t G, int32_t P, int32_t H, const float *qkv, const int64_t *words, float *out, float *lse, void *stream);
int team_attention_bwd(int64_t G, int32_t P, int32_t H, const float *qkv, const int64_t *words, const float *lse, const float *d_out, float *d_qkv,
                       void *stream);
int team_comm_mask_host(int64_t G, int32_t P, const float *pp_adj, int64_t adj_stride, const float *live, int64_t live_stride, int64_t *words,
                        int64_t words_stride);
int team_attention_fwd_host(int64_t G, int32_t P, int32_t H, const float *qkv, const int64_t *words, float *out, float *lse);
int team_attention_bwd_host(int64_t G, int32_t P, int32_t H, const float *qkv, const int64_t *words, const float *lse, const float *d_out,
                            float *d_qkv);

/*
 * Records one rollout tick into the replay buffer (MAPPO.run_episode's minibuffer.store_transition,
 * DHGN/mappo_parallel.py:783-805, for N environments at once): for every item, row n of the dense [N][row_bytes] source
 * goes to dst + n * dst_row_stride (slot [n, t] of an (N, T, ...) buffer tensor); i32_to_f32 converts int32 actions to
 * the buffer's float32.  If raw != NULL, episode_return[n] += sum_p raw[n][p] (the evaluator's episode reward).
 * The item array is read on the host at call time.
 */
#define MO_RECORD_MAX_ITEMS 16
typedef struct {
    const void *src;
    void *dst;
    int64_t dst_row_stride; /* bytes between consecutive environments in dst */
    int32_t row_bytes;      /* multiple of 4 */
    int32_t i32_to_f32;
} mo_record_item;
int rollout_record(int32_t N, int32_t n_items, const mo_record_item *items, const float *raw, float *episode_return, int32_t P, void *stream);

/*
 * Weight gradient of a Linear / GRU projection, C = A^T B reduced over all K rows of a minibatch:
 *   C [M][N] (dense) = (accumulate ? C : 0) + sum_k A[k][:]^T B[k][:] ;  A [K][M] (lda), B [K][N] (ldb), row-major fp32.
 * Replaces the `grad_output.t() @ input` GEMMs autograd runs for torch.nn.Linear / torch.nn.GRU weights in
 * MAPPO.train (DHGN/mappo_parallel.py:660-708, loss.backward()).  Split-K over one workgroup per CU, fp32 MFMA,
 * partial tiles in `workspace` (>= wgrad_tn_workspace(M, N) bytes) added in a fixed order: results are deterministic.
 * M, N multiples of 128 (<= 1024), lda/ldb multiples of 4, A/B 16-byte aligned; anything else -> MO_ERR_BAD_ARG
 * (the caller keeps such shapes on the BLAS library).
 */
int64_t wgrad_tn_workspace(int32_t M, int32_t N);
int wgrad_tn(int64_t K, int32_t M, int32_t N, const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int32_t accumulate,
             void *workspace, void *stream);
/* The same product in fp32 arithmetic on the bf16 matrix pipe (exact three-way operand splits, see gru_cell_split_fwd_multi): (M, N) in
 * {128, 256, 384}^2 with M + N <= 512 and M N < 65536; workspace >= wgrad_split_workspace(M, N) bytes; deterministic. */
int64_t wgrad_split_workspace(int32_t M, int32_t N);
int wgrad_split_tn(int64_t K, int32_t M, int32_t N, const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int32_t accumulate,
                   void *workspace, void *stream);
/* The same with A given as two column blocks [A1 (K x M1) | A2 (K x M2)], M = M1 + M2 (each with its own row stride): one pass over B for
 * a product whose left operand lives in two tensors -- the GRU's dW_hh = [dr dz | dnr]^T h_prev (dr, dz: the first 2H columns of dgi). */
int wgrad_split_tn2(int64_t K, int32_t M1, int32_t M2, int32_t N, const float *A1, int64_t lda1, const float *A2, int64_t lda2, const float *B, int64_t ldb,
                    float *C, int32_t accumulate, void *workspace, void *stream);
/*
 * Neighbour mean of DHGN.fcra (DHGN/mappo_parallel.py:204-233: `torch.matmul(F.normalize(adj, p=1, dim=-1), hist)`), R rows of P
 * agents and E features:  out[r][i][:] = act( sum_j abar[r][i][j] z[r][j][:] + bias ),  act = ReLU when relu != 0.
 *   actor (out_actor != NULL): abar = adj / max(sum_j |adj|, 1e-12), adj [R][P][P] (adj_row_stride elements between rows);
 *   critic (out_critic != NULL): abar = 1 / P (the normalised ones_like(adj) of AttributeDataset :64-65).
 * z_* are read in place from a (N, T', P, E) history buffer: row r = (n, t) = (r / T, r % T) starts at n * episode_stride +
 * t * step_stride (T = 1 and episode_stride = P E: a dense [R][P][E] tensor); bias [E] or NULL; out_*: [R][P] vectors of E floats,
 * out_stride (>= E) elements apart (E: dense; 2 E: the left half of the [agg | h] operand of the FCRA layer, :227-231).
 * Either output may be NULL; both together serve the rollout's paired actor / critic tick.
 */
int fcra_neighbour_mean(int32_t R, int32_t P, int32_t E, int32_t T, const float *z_actor, int64_t za_episode_stride, int64_t za_step_stride,
                        const float *z_critic, int64_t zc_episode_stride, int64_t zc_step_stride, const float *adj, int64_t adj_row_stride,
                        const float *bias, int32_t relu, float *out_actor, float *out_critic, int64_t out_stride, void *stream);
/* Several such aggregations of one shape in ONE launch (the FCRA hops of a rollout tick: every hop reads a stored history slot, none
 * reads another hop's result): same R, P, E, T, strides, adjacency, relu and out_stride; own inputs, bias and outputs per job. */
#define MO_NBR_MAX_JOBS 4
typedef struct mo_nbr_job { const float *z_actor, *z_critic, *bias; float *out_actor, *out_critic; } mo_nbr_job;
int fcra_neighbour_mean_multi(int32_t n_jobs, const mo_nbr_job *jobs, int32_t R, int32_t P, int32_t E, int32_t T, int64_t za_episode_stride,
                              int64_t za_step_stride, int64_t zc_episode_stride, int64_t zc_step_stride, const float *adj, int64_t adj_row_stride,
                              int32_t relu, int64_t out_stride, void *stream);

/*
 * ReLU backward and the bias gradient of the Linear in front of it in one pass (autograd: aten::threshold_backward, then
 * grad.sum(0) re-reading it; MAPPO.train's loss.backward(), DHGN/mappo_parallel.py:660-708):
 *   gin [R][F] = gout * [y > 0] (y = the saved ReLU output);  colsum [F] = sum_r gin[r][:].
 * Rows are F contiguous floats, g_row_stride / y_row_stride (>= F, multiples of 4) elements apart for gout / y (a column block of
 * a wider matrix), dense for gin; F a multiple of 4 with F/4 dividing 256; 16-byte aligned pointers.  Deterministic
 * (per-workgroup partials in `workspace` >= relu_bwd_colsum_workspace(F) bytes, reduced in a fixed order in f64).
 */
int64_t relu_bwd_colsum_workspace(int32_t F);
int relu_bwd_colsum(int64_t R, int32_t F, const float *gout, int64_t g_row_stride, const float *y, int64_t y_row_stride, float *gin, float *colsum,
                    void *workspace, void *stream);

/*
 * Weight gradient of a Linear layer with at most 16 inputs or outputs (the K = 4 position part of DHGN's semantic layer, the action
 * and value heads; autograd's `grad_output.t() @ input`, DHGN/mappo_parallel.py:660-708) as one streaming pass:
 *   C [NS][F] = sum_r S[r][:]^T X[r][:]   (transposed != 0: C [F][NS]);  S [R][NS] (lds), X [R][F] (ldx), F a multiple of 64.
 * colsum_x [F] = sum_r X[r][:], colsum_s [NS] = sum_r S[r][:] (NULL skips): the bias gradient, whichever operand is grad_output.
 * Deterministic (per-workgroup partials in `workspace` >= wgrad_skinny_workspace(NS, F) bytes, reduced in a fixed order in f64).
 */
int64_t wgrad_skinny_workspace(int32_t NS, int32_t F);
int wgrad_skinny(int64_t R, int32_t NS, int32_t F, const float *S, int64_t lds, const float *X, int64_t ldx, int32_t transposed, float *C,
                 float *colsum_x, float *colsum_s, void *workspace, void *stream);

const char *mappo_ops_error_string(int code);

#ifdef __cplusplus
}
#endif
#endif
