"""MAPPO on env_n2n (continuous 2-D pursuit, several evaders, no obstacles): BASELINE config 4 on the environment it names.

The reference has no env_n2n learner.  This module drives the pursuit model itself -- `build_actor_critic`: the DHGN encoder
shared by `SharedActor` (2-layer GRU, 9-way Categorical head) and `SharedCritic` (spectrally normalised value head), so the state_dict
keys are the reference's -- with the PPO update, GAE and data-parallel protocol of `MAPPO` / `Trainer`.  DESIGN.md section 7b.
* inputs: ParticleEnv.policy_inputs (csrc/n2n_env.hip n2n_policy_inputs, one launch per tick): pursuers and evaders as
  (x, y, v cos phi, v sin phi), the live mask, the masked adjacencies and e_ref, the evader of the defender relation's p_i - e term;
* relations: defender (P x P), evader (P x E, E >= 1) and an EMPTY obstacle relation (K = 0: its slot is zero, its dW and db are 0);
* bookkeeping: ParticleEnv.policy_record (n2n_policy_record, one launch per tick): masked reward / value / active rows of the buffer and
  the per-environment return, length, capture and end flags.
"""
import json
import os
import time

import torch

from . import guidance as gd
from . import ops
from . import value_norm as vnorm
from .minibatch_steps import MAX_GRAD_NORM, minibatch_steps_options
from .reward_shaping import reward_shaping_options
from .update_diag import LOG_KEYS, UpdateDiag, first_epoch_over, update_diag_options
from .model import build_actor_critic, sequence_forward_pair
from .n2n_env import ParticleEnv
from .trainer import (BUCKET_ALIGN, FusedAdam, GradBucket, ParamBucket, ParticleRunState, allreduce_sum_, broadcast_weights_,
                      enable_tuned_gemms, init_distributed, resume_path, save_resume_atomic)

MAX_P = 16   # the message kernels' agents per row (csrc/mappo_ops.hip MAX_P)


class _N2nRollout:
    """static device storage of one lockstep rollout of N environments: the policy inputs, the history ring (slot t % M holds tick t's
    actor [0] and critic [1] embedding; M = depth + 1, each network reads its own last `depth` embeddings), the GRU states (ping-pong
    between two buffers), the episode accumulators and the position of the action-sampling stream"""

    def __init__(self, agent, env):
        dev, L, H, Em, d = agent.device, agent.num_layers, agent.rnn_hidden_dim, agent.embedding_dim, agent.depth
        N, P, E = env.num_envs, env.p_num, env.e_num
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.N, self.P, self.E, self.d, self.M = N, P, E, d, d + 1
        self.p4, self.e4, self.e_ref, self.live = z(N, P, 4), z(N, E, 4), z(N, 4), z(N, P)
        self.pp, self.pe = z(N, P, P), z(N, P, E)
        self.o, self.o_adj = z(N, 0, 4), z(N, P, 0)          # env_n2n has no obstacles: the third relation is empty
        self.ring = z(self.M, 2, N, P, Em)
        self.hbuf_a, self.hbuf_c = z(2, L, N * P, H), z(2, L, N * P, H)
        self.a_n = torch.zeros((N, P), dtype=torch.int32, device=dev)
        self.logp, self.v = z(N, P), z(N, P)
        self.counter = torch.full((1,), int(agent.sample_rank) << 40, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.t = 0

    def reset(self):
        for x in (self.ring, self.hbuf_a, self.hbuf_c):
            x.zero_()
        self.t = 0

    def hops(self, t):
        """hop k = the embedding of tick t - 1 - k (zero before the episode's first tick), per network"""
        return [self.ring[(t - 1 - k) % self.M][0] for k in range(self.d)], [self.ring[(t - 1 - k) % self.M][1] for k in range(self.d)]


class N2nMAPPO:
    """rollout (run_episode / explore_env) and PPO update (train) of the DHGN actor / critic on env_n2n"""

    def __init__(self, cfg, batch_size, mini_batch_size, device="cuda"):
        a = cfg.algo
        if bool(a.get("use_reward_norm", False)):
            raise ValueError("algo.use_reward_norm: true is not supported on env_n2n (runtime.env: n2n); set it to false")
        self.use_reward_scaling = bool(a.get("use_reward_scaling", False))   # the reference's RewardScaling in policy_record
        self.use_value_norm, self.value_norm_beta = vnorm.value_norm_options(cfg)   # ValueNorm on the value targets
        self.reward_shaping, self.shaping_coef = reward_shaping_options(cfg)   # distance shaping in policy_record
        self.update_diagnostics, self.target_kl = update_diag_options(cfg)   # what the update did, from the loss launches
        self.minibatch_steps = minibatch_steps_options(cfg)   # one clip + Adam step per mini-batch, fused
        self.guidance = gd.guidance_options(cfg)   # the scripted pursuers of run_episode(policy="guidance")
        if bool(a.get("use_obs_norm", False)):
            raise ValueError("algo.use_obs_norm: true is built for runtime.env e3d only; the env_n2n inputs are node states whose "
                             "differences the message kernels form and whose zero rows stand for absent nodes (set use_obs_norm to false)")
        if int(cfg.env.num_defender) > MAX_P:
            raise ValueError(f"env.num_defender={cfg.env.num_defender}: the DHGN message kernels take at most {MAX_P} pursuers per row")
        if int(cfg.env.state_dim) != 4 or int(cfg.env.action_dim) != 9 or int(a.num_relation) != 3:
            raise ValueError("env_n2n runs the pursuit model: env.state_dim 4, env.action_dim 9, algo.num_relation 3")
        self.batch_size, self.mini_batch_size = int(batch_size), int(mini_batch_size)
        self.max_train_steps, self.lr, self.gamma, self.lamda = a.max_train_steps, a.lr, a.gamma, a.lamda
        self.epsilon, self.entropy_coef = a.epsilon, a.entropy_coef
        self.use_grad_clip, self.use_lr_decay = a.use_grad_clip, a.use_lr_decay
        self.use_adv_norm, self.use_value_clip = a.use_adv_norm, a.use_value_clip
        self.num_layers, self.embedding_dim, self.rnn_hidden_dim = int(a.num_layers), int(a.embedding_dim), int(a.rnn_hidden_dim)
        self.depth = int(a.depth)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("N2nMAPPO runs on the GPU only (HIP kernels, no CPU fallback)")
        if str(a.get("encoder", "dhgn")).lower() != "dhgn":
            raise ValueError("env_n2n trains the DHGN encoder only (algo.encoder: dhgn)")
        self.actor, self.critic = build_actor_critic(cfg, self.device)
        if not (self.actor.use_rnn and self.critic.use_rnn):
            raise ValueError("env_n2n trains the GRU actor / critic only (algo.use_rnn: true)")
        enc = self.actor.shared_net
        # the parameter order of MAPPO.ac_parameters (the reference's, :631)
        self.ac_parameters = (list(enc.parameters()) + list(self.actor.GRU.parameters()) + list(self.critic.GRU.parameters())
                              + list(self.critic.Mean.parameters()) + list(self.actor.Mean.parameters()))
        self.param_bucket = None
        if self.minibatch_steps:   # the parameters and their gradients as two flat tensors of one layout, stepped by two launches
            self.param_bucket = ParamBucket(self.ac_parameters)
            self.ac_optimizer = FusedAdam(self.param_bucket, lr=self.lr, eps=1e-5)
        else:
            self.ac_optimizer = torch.optim.Adam(self.ac_parameters, lr=self.lr, eps=1e-5)
        self.value_norm = vnorm.ValueNorm(self.value_norm_beta, self.device) if self.use_value_norm else None
        self.diag = UpdateDiag(self.device) if self.update_diagnostics else None
        self.last_update_diag = None   # algo.update_diagnostics: the dict of the last train() call
        rt = cfg.get("runtime", {})
        self.sample_seed = int(rt.get("seed", 0))
        self.sample_rank = int(rt.get("sample_rank", 0))   # Philox counter of rank r starts at r << 40 (as MAPPO)
        self.total_step = 0
        self.grad_bucket = GradBucket(self.ac_parameters, BUCKET_ALIGN) if self.minibatch_steps else None   # (off: the trainer's)
        self.last_optimizer_steps = self.last_skipped_steps = 0   # algo.minibatch_steps: of the last train() call
        self.buffer = None
        self._states = {}

    # ---- rollout -------------------------------------------------------------------------------------------------------------
    def _state(self, env):
        st = self._states.get(id(env))
        if st is None or st.N != env.num_envs:
            st = self._states[id(env)] = _N2nRollout(self, env)
        return st

    def _policy_step(self, st, greedy=False):
        """DHGN for both networks in one pass (forward_pair, into the ring) -> both GRU cells (one launch per layer) -> value ->
        Categorical head and sample (ops.head_sample, int32 actions)"""
        N, P, Em = st.N, st.P, self.embedding_dim
        hops_a, hops_c = st.hops(st.t)
        slot = st.ring[st.t % st.M]
        emb = self.actor.shared_net.forward_pair(st.p4, st.e4, st.o, st.pp, st.pe, st.o_adj, hops_a, hops_c, None, 1, slot, e_ref=st.e_ref)
        cur, nxt = st.t & 1, (st.t + 1) & 1
        fa, fc = ops.gru_step_multi([emb[0].reshape(-1, Em), emb[1].reshape(-1, Em)], [st.hbuf_a[cur], st.hbuf_c[cur]],
                                    [self.actor.GRU, self.critic.GRU], hiddens_out=[st.hbuf_a[nxt], st.hbuf_c[nxt]])
        self.critic.head(fc.reshape(N, P, -1), out=st.v)
        w_a = self.actor.head_weight()
        ops.head_sample(fa.contiguous(), w_a, self.actor.Mean.bias, self.sample_seed, st.counter, st.ticket, (st.a_n, st.logp), greedy=greedy)
        st.t += 1

    def _bootstrap_value(self, st):
        """the critic's value of the state after the last step: its DHGN pass (history = its own last embeddings), GRU cell and head"""
        N, P = st.N, st.P
        _, hops_c = st.hops(st.t)
        enc = self.critic.shared_net
        emb = enc(st.p4, st.e4, st.o, st.pp, st.pe, st.o_adj, hops_c, True, None, 1, None, e_ref=st.e_ref)
        (fc,) = ops.gru_step_multi([emb.reshape(N * P, -1)], [st.hbuf_c[st.t & 1]], [self.critic.GRU], hiddens_out=[st.hbuf_c[(st.t + 1) & 1]])
        return self.critic.head(fc.reshape(N, P, -1)).reshape(N, P)

    def new_buffer(self, N, T, P, E):
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)
        d, Em = self.depth, self.embedding_dim
        buf = dict(p_state=z(N, T, P, 4), e_state=z(N, T, E, 4), e_ref=z(N, T, 4), p_adj=z(N, T, P, P), e_adj=z(N, T, P, E),
                   actor_historical_embedding=z(N, T + d, P, Em), critic_historical_embedding=z(N, T + d, P, Em),
                   a_n=z(N, T, P), a_logprob_n=z(N, T, P), r=z(N, T, P), active=z(N, T, P), v_n=z(N, T + 1, P))
        if self.value_norm is not None:
            buf["v_mask"] = z(N, P)   # the bootstrap mask of v_n[:, T] (algo.use_value_norm only)
        return buf

    @torch.no_grad()
    def run_episode(self, env, buf=None, greedy=False, policy="network"):
        """N episodes in lockstep for T = env.episode_limit ticks.  Per tick: policy_inputs, the policy step, the SLSQP evader, the tick,
        policy_record, and (with a buffer) one rollout_record launch.  Row (n, t, p) is live iff pursuer p was active at the start of step t
        and environment n was not done before it; r, v_n and `active` of other rows are zero, so is v_n[n, t + 1, p] when pursuer p or
        episode n ended in step t for a reason other than the time limit; v_n[:, T] is the critic's bootstrap value under that rule.
        With algo.use_reward_scaling and a buffer, r is the scaled reward (env.reward_scale advances); acc["ret"] stays the raw return.
        With algo.reward_shaping: distance and a buffer, r (what is scaled, when both are on) carries the shaping term
        gamma Phi' - Phi (env.shaping_phi, written by shaping_begin after the reset).
        policy="guidance" (buf must be None): the tick takes the scripted pursuers' actions (guidance_episode below) instead of the
        network's; no network, sampler or sampling counter is touched, the accumulators are the same.
        Returns the per-environment accumulators (done_before, ended, captured, ret, length)."""
        gd.check_policy(policy, buf)
        if policy == "guidance":
            return guidance_episode(env)
        N, P, T, d = env.num_envs, env.p_num, env.episode_limit, self.depth
        env.reset()
        st = self._state(env)
        st.reset()
        acc = env.new_accumulators()
        scale_gamma = self.gamma if (self.use_reward_scaling and buf is not None) else None   # evaluation never scales
        shaping_gamma = self.gamma if (self.reward_shaping == "distance" and buf is not None) else None   # ... and never shapes
        if shaping_gamma is not None:
            env.shaping_begin()
        for t in range(T):
            env.policy_inputs(st.p4, st.e4, st.e_ref, st.live, st.pp, st.pe, acc["done_before"])
            self._policy_step(st, greedy)
            env.evader_step()
            env.step(st.a_n)
            if buf is None:
                env.policy_record(acc, st.live)
                continue
            env.policy_record(acc, st.live, st.v, buf["r"][:, t], buf["active"][:, t], buf["v_n"][:, t], buf["v_n"][:, t + 1],
                              scale_gamma=scale_gamma, shaping_gamma=shaping_gamma)
            items = [(st.p4, buf["p_state"][:, t]), (st.e4, buf["e_state"][:, t]), (st.e_ref, buf["e_ref"][:, t]), (st.pp, buf["p_adj"][:, t]),
                     (st.pe, buf["e_adj"][:, t]), (st.a_n, buf["a_n"][:, t]), (st.logp, buf["a_logprob_n"][:, t])]
            if d:   # the update reads the stored embeddings as FCRA history only
                slot = st.ring[(st.t - 1) % st.M]
                items += [(slot[0], buf["actor_historical_embedding"][:, t + d]), (slot[1], buf["critic_historical_embedding"][:, t + d])]
            ops.rollout_record(items)
        if buf is not None:
            # the state after the last step without the done mask: the time limit sets done for every environment in the last tick, and
            # the truncated episodes are the ones whose bootstrap value counts (vmask removes those that ended for another reason)
            env.policy_inputs(st.p4, st.e4, st.e_ref, st.live, st.pp, st.pe, None)
            vmask = env.active_t.float() * (acc["ended"] == 0).float()[:, None]
            buf["v_n"][:, T].copy_(self._bootstrap_value(st) * vmask)
            if self.value_norm is not None:   # the denormalisation of v_n[:, T] needs the mask itself: 0 std + mean is not 0
                buf["v_mask"].copy_(vmask)
        return acc

    def explore_env(self, env):
        """one episode per environment into the buffer -> (mean return, buffer, env-steps, stats)"""
        N, P, E, T = env.num_envs, env.p_num, env.e_num, env.episode_limit
        if self.buffer is None or self.buffer["r"].shape != (N, T, P) or self.buffer["e_state"].shape[2] != E:
            self.buffer = self.new_buffer(N, T, P, E)
        acc = self.run_episode(env, self.buffer)
        mean_r, cap, mlen = torch.stack((acc["ret"].mean(), acc["captured"].float().mean(), acc["length"].mean())).tolist()
        return mean_r, self.buffer, N * T, dict(capture_rate=cap, episode_length=mlen)

    # ---- update ------------------------------------------------------------------------------------------------------------------
    def minibatch_inputs(self, buf, n0, n1):
        """episodes [n0, n1) of the buffer as one sequence batch: (obs dict, actor history slices, critic history slices)"""
        T, P, E, d = buf["r"].shape[1], buf["r"].shape[2], buf["e_state"].shape[2], self.depth
        R = (n1 - n0) * T
        dev = buf["r"].device
        obs = dict(p_state=buf["p_state"][n0:n1].reshape(R, P, 4), e_state=buf["e_state"][n0:n1].reshape(R, E, 4),
                   e_ref=buf["e_ref"][n0:n1].reshape(R, 4), o_state=torch.zeros((R, 0, 4), device=dev), q_div=1,
                   p_adj=buf["p_adj"][n0:n1].reshape(R, P, P), e_adj=buf["e_adj"][n0:n1].reshape(R, P, E),
                   o_adj=torch.zeros((R, P, 0), device=dev))
        hist_a = [buf["actor_historical_embedding"][n0:n1, d - 1 - k: d - 1 - k + T] for k in range(d)]
        hist_c = [buf["critic_historical_embedding"][n0:n1, d - 1 - k: d - 1 - k + T] for k in range(d)]
        return obs, hist_a, hist_c

    def sequence_forward(self, buf, n0, n1):
        """-> prob (B, T, P, 9), values (B, T, P) of episodes [n0, n1) (model.sequence_forward_pair)"""
        obs, hist_a, hist_c = self.minibatch_inputs(buf, n0, n1)
        prob, values = sequence_forward_pair(self.actor, self.critic, obs, hist_a, hist_c, n1 - n0, buf["r"].shape[1])
        return prob, values[..., 0]

    def train(self, buf, total_steps):
        """GAE + advantage normalisation over all rows (ops.gae_advnorm), then sequential mini-batches of whole episodes, the
        gradient clipped to 5.0 after each (as MAPPO.train).  With algo.minibatch_steps every mini-batch instead starts from a zeroed
        bucket and ends with the gradient SUM over ranks and one fused clip + Adam step (FusedAdam.step), and
        last_optimizer_steps / last_skipped_steps count them.  Returns (critic loss, actor loss) averaged over the mini-batches."""
        N = buf["r"].shape[0]
        with torch.no_grad():
            if self.value_norm is not None:   # GAE on denormalised values, the state's step, the targets under the new statistics
                adv, v_target = self.value_norm.gae_targets(buf, self.gamma, self.lamda, self.use_adv_norm)
            else:
                adv, v_target = ops.gae_advnorm(buf["r"], buf["v_n"], buf["active"], self.gamma, self.lamda, self.use_adv_norm)
        if self.grad_bucket is not None:
            self.grad_bucket.zero()
        else:
            self.ac_optimizer.zero_grad()
        opt = self.ac_optimizer if self.minibatch_steps else None   # FusedAdam: zero, backward, reduce and step per mini-batch
        obj_c = obj_a = 0.0
        k = 0
        diag = self.diag   # algo.update_diagnostics: every loss call adds its eight sums (None: the plain calls)
        if diag is not None:
            diag.begin()
        for n0 in range(0, N, self.mini_batch_size):
            n1 = min(n0 + self.mini_batch_size, N)
            if opt is not None and n0:
                self.grad_bucket.zero()
            prob, values = self.sequence_forward(buf, n0, n1)
            la, lc = ops.ppo_loss_prob(prob, buf["a_n"][n0:n1], values, buf["a_logprob_n"][n0:n1], adv[n0:n1], buf["active"][n0:n1],
                                       buf["v_n"][n0:n1, :-1] if self.use_value_clip else None, v_target[n0:n1], self.epsilon,
                                       self.entropy_coef, self.use_value_clip, **({} if diag is None else {"diag": diag.sums}))
            (la + lc).backward()
            if opt is not None:   # the clip acts on the gradient summed over ranks: the same coefficient and weights everywhere
                allreduce_sum_(self.grad_bucket.flat)
                opt.step(self.grad_bucket.flat, MAX_GRAD_NORM if self.use_grad_clip else 0.0)
                if diag is not None and self.use_grad_clip:
                    diag.note_grad_norm(opt.grad_norm)
            elif self.use_grad_clip:
                norm = torch.nn.utils.clip_grad_norm_(self.ac_parameters, 5.0)
                if diag is not None:
                    diag.note_grad_norm(norm)
            obj_c = obj_c + lc.detach().double()
            obj_a = obj_a + la.detach().double()
            k += 1
        if self.use_lr_decay:
            self.lr_decay(total_steps)
        extra = () if opt is None else (opt.skipped,)   # the count of skipped steps rides in the read the call has anyway
        if diag is not None:   # one read for the two losses, the eight sums (all-reduced over ranks) and the gradient norm
            (obj_c, obj_a, *extra), self.last_update_diag = diag.read(obj_c, obj_a, *extra)
        elif opt is not None:
            obj_c, obj_a, *extra = torch.stack((obj_c, obj_a, *extra)).tolist()
        if opt is not None:
            self.last_optimizer_steps, self.last_skipped_steps = k, int(extra[0] - opt.skipped_seen)
            opt.skipped_seen = extra[0]
        return float(obj_c) / k, float(obj_a) / k

    def lr_decay(self, total_steps):
        lr_now = self.lr * (1 - total_steps / self.max_train_steps)
        for p in self.ac_optimizer.param_groups:
            p["lr"] = lr_now
        self.total_step = total_steps

    def save_model(self, cwd, best=False):
        """cwd/n2n_actor.pth and n2n_critic.pth (best: n2n_actor_best.pth, n2n_critic_best.pth), the two state_dicts; with
        algo.use_value_norm the sibling n2n_value_norm.pth (n2n_value_norm_best.pth): beta and the state"""
        os.makedirs(cwd, exist_ok=True)
        sfx = "_best" if best else ""
        torch.save(self.actor.state_dict(), os.path.join(cwd, f"n2n_actor{sfx}.pth"))
        torch.save(self.critic.state_dict(), os.path.join(cwd, f"n2n_critic{sfx}.pth"))
        vn_path = os.path.join(cwd, f"n2n_value_norm{sfx}.pth")
        if self.value_norm is not None:
            torch.save(self.value_norm.entry(), vn_path)
        elif os.path.exists(vn_path):   # a file of an earlier option-on run in the same directory does not belong to these weights
            os.remove(vn_path)

    def load_model(self, cwd, best=False):
        """the weights save_model(cwd, best) wrote; ValueError when they belong to the other algo.use_value_norm"""
        sfx = "_best" if best else ""
        vn_path = os.path.join(cwd, f"n2n_value_norm{sfx}.pth")
        entry = torch.load(vn_path, map_location="cpu") if os.path.exists(vn_path) else None
        vnorm.check_entry(self, entry, os.path.join(cwd, f"n2n_critic{sfx}.pth"), check_beta=False)
        self.actor.load_state_dict(torch.load(os.path.join(cwd, f"n2n_actor{sfx}.pth"), map_location=self.device))
        self.critic.load_state_dict(torch.load(os.path.join(cwd, f"n2n_critic{sfx}.pth"), map_location=self.device))
        if self.value_norm is not None:
            self.value_norm.load_entry(entry)


@torch.no_grad()
def guidance_episode(env):
    """N episodes in lockstep for T = env.episode_limit ticks with the scripted lead-pursuit pursuers (ParticleEnv.guidance_actions, one
    launch per tick) where run_episode has its policy step: the live mask (policy_inputs), the evaders' command, the tick and
    policy_record are run_episode's, so the raw return, the captured flag and the length mean what they mean there.  Needs no agent.
    Returns the per-environment accumulators (done_before, ended, captured, ret, length)."""
    env.reset()
    live = torch.zeros((env.num_envs, env.p_num), dtype=torch.float32, device=env.device)
    acc = env.new_accumulators()
    for _ in range(env.episode_limit):
        env.policy_inputs(None, None, None, live, None, None, acc["done_before"])
        actions = env.guidance_actions()
        env.evader_step()
        env.step(actions)
        env.policy_record(acc, live)
    return acc


def make_env(cfg, num_envs, rank=0, device="cuda", seed_offset=0, training=True):
    """ParticleEnv of one rank: environment n of rank r is reset from seed + max(1000, num_envs) r + n (as Pursuit_Env).  A training
    environment owns the RewardScaling state when algo.use_reward_scaling is on and the shaping state when algo.reward_shaping is
    distance; evaluation environments (training=False) never do."""
    base = int(cfg.runtime.get("seed", 0)) + seed_offset + max(1000, num_envs) * rank
    env = ParticleEnv(num_envs=num_envs, seeds=[base + n for n in range(num_envs)], device=device, episode_limit=int(cfg.env.max_steps),
                      evader=str(cfg.runtime.get("n2n_evader", "slsqp")))
    env.initialize(int(cfg.env.num_defender), int(cfg.env.num_evader))
    if training and bool(cfg.algo.get("use_reward_scaling", False)):
        env.enable_reward_scaling()
    mode, coef = reward_shaping_options(cfg)
    if training and mode == "distance":
        env.enable_reward_shaping(coef)
    env.set_guidance(*gd.guidance_options(cfg))
    return env


class N2nTrainer(ParticleRunState):
    """One rank of the data-parallel env_n2n job: rollout, then epochs x (update, gradient all-reduce, Adam step); with
    algo.minibatch_steps the update itself reduces and steps after every mini-batch and the epoch loop does neither."""

    def __init__(self, cfg, num_envs=None, num_eval_envs=64, eval_every=0, tuned_gemms=True):
        self.rank, self.local_rank, self.world = init_distributed()
        self.tuned_gemms = enable_tuned_gemms() if tuned_gemms else False
        self.cfg = cfg
        self.device = torch.device("cuda", self.local_rank % max(1, torch.cuda.device_count()))
        torch.cuda.set_device(self.device)
        self.num_envs = int(num_envs if num_envs is not None else cfg.runtime.num_envs)
        self.env = make_env(cfg, self.num_envs, self.rank, self.device)
        torch.manual_seed(int(cfg.runtime.get("seed", 0)))
        self.agent = N2nMAPPO(cfg, self.num_envs, max(1, round(self.num_envs / 10)), self.device)
        self.agent.sample_rank = self.rank
        self.bucket = self.agent.grad_bucket or GradBucket(self.agent.ac_parameters)   # (algo.minibatch_steps: the agent's own)
        self.agent.grad_bucket = self.bucket
        if self.agent.value_norm is not None:
            self.agent.value_norm.allreduce = allreduce_sum_   # (S1, S2, c) over ranks; without a process group a no-op
        if self.agent.diag is not None:
            self.agent.diag.allreduce = allreduce_sum_         # the eight diagnostic sums over ranks, likewise
        self.last_epoch_diags = []
        broadcast_weights_([self.agent.actor, self.agent.critic])
        self.num_eval_envs, self.eval_every = int(num_eval_envs), int(eval_every)
        self.eval_env = None
        self.eval_baseline, self.baseline_record = gd.eval_baseline_options(cfg), None   # runtime.eval_baseline
        self.eval_return_std = None
        self.recorder, self.best_eval_return = [], -float("inf")
        self.total_steps = 0
        self.iteration = 0

    def iterate(self):
        """-> (env-steps of this iteration over all ranks, log record)"""
        cfg, agent = self.cfg, self.agent
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        mean_r, buf, steps, stats = agent.explore_env(self.env)
        ev[1].record()
        self.total_steps += steps * self.world
        self.last_epoch_diags, epochs_run = [], 0
        per_minibatch, opt_steps, skipped = agent.minibatch_steps, 0, 0
        for _ in range(int(cfg.algo.epochs)):
            with torch.enable_grad():
                obj_c, obj_a = agent.train(buf, self.total_steps)
            over = False
            if agent.diag is not None:
                self.last_epoch_diags.append(agent.last_update_diag)
                # algo.target_kl: the policy has moved past the target on this buffer -- the remaining epochs are skipped; the sums are
                # all-reduced, so every rank stops here.  Stepping once per epoch, this epoch's gradient is discarded as well (the next
                # train() zeroes the bucket); with algo.minibatch_steps its steps were already taken and stand
                over = first_epoch_over([agent.last_update_diag["approx_kl"]], agent.target_kl) is not None
                if over and not per_minibatch:
                    break
            if per_minibatch:   # algo.minibatch_steps: train() reduced and stepped after every mini-batch; an epoch over the KL target
                opt_steps += agent.last_optimizer_steps   # is the last one and its steps stand (there is nothing left to discard)
                skipped += agent.last_skipped_steps
            else:
                allreduce_sum_(self.bucket.flat)
                agent.ac_optimizer.step()
            epochs_run += 1
            if over:
                break
        ev[2].record()
        self.iteration += 1
        self.last_events = ev
        log = dict(iteration=self.iteration, total_steps=self.total_steps, mean_return=mean_r, capture_rate=stats["capture_rate"],
                   episode_length=stats["episode_length"], critic_loss=obj_c, actor_loss=obj_a)
        if agent.diag is not None:   # of the last train() call, like the two losses
            log.update({k: agent.last_update_diag[k] for k in LOG_KEYS}, epochs_run=epochs_run)
        if per_minibatch:
            log.update(optimizer_steps=opt_steps, skipped_steps=skipped)
        if self.eval_every and self.iteration % self.eval_every == 0 and self.rank == 0:
            log.update(self.evaluate())
        return steps * self.world, log

    def evaluate(self):
        """synchronous greedy episode (argmax) on num_eval_envs environments of their own seeds; the std of the return over them goes to
        self.eval_return_std (a recorder column, not a log key)"""
        ev = self.make_eval_env()
        acc = self.agent.run_episode(ev, None, greedy=True)
        ret = acc["ret"]
        sd = ret.std() if ret.numel() > 1 else ret.new_zeros(())
        r, c, l, self.eval_return_std = torch.stack((ret.mean(), acc["captured"].float().mean(), acc["length"].mean(), sd)).tolist()
        rec = dict(eval_return=r, eval_capture_rate=c, eval_episode_length=l)
        if self.eval_baseline is not None:
            rec.update(self.baseline())
        return rec

    def baseline(self):
        """runtime.eval_baseline: guidance -- the scripted pursuers' return, capture rate and episode length on num_eval_envs
        environments of the evaluation seeds (seed + 10^6 + n), as baseline_* fields.  The law is deterministic and the environments
        are its own (their first episode; the evaluation environments and their generators are not touched), so it runs once and
        every later evaluation record carries the same figures."""
        if self.baseline_record is None:
            env = make_env(self.cfg, self.num_eval_envs, 0, self.device, seed_offset=10 ** 6, training=False)
            acc = self.agent.run_episode(env, None, policy="guidance")
            self.baseline_record = gd.baseline_record(acc["ret"], acc["captured"], acc["length"])
        return dict(self.baseline_record)

    def make_eval_env(self):
        """the evaluation environments (created once): num_eval_envs of their own seeds, seed + 10^6 + n"""
        if self.eval_env is None:
            self.eval_env = make_env(self.cfg, self.num_eval_envs, 0, self.device, seed_offset=10 ** 6, training=False)
        return self.eval_env

    def last_breakdown_ms(self):
        torch.cuda.synchronize()
        ev = self.last_events
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def train_n2n(cfg, max_iterations=None, num_eval_envs=64, eval_every=1, save_resume=None, resume=None):
    """the env_n2n training loop (main --config cfg4_n2n): until max_train_steps env-steps or max_iterations; rank 0 prints one JSON log
    line per iteration, records every evaluation (recorder.npy, learning curve, the _best weights: ParticleRunState.record_evaluation)
    and saves the final weights under algo.save_cwd.  resume / save_resume: directories of the per-rank resume bundles read before the
    first iteration / written after every one."""
    tr = N2nTrainer(cfg, num_eval_envs=num_eval_envs, eval_every=eval_every)
    if resume is not None:
        tr.load_resume(resume_path(resume, tr.rank))
    while tr.total_steps < cfg.algo.max_train_steps:
        t0 = time.time()
        steps, log = tr.iterate()
        if tr.rank == 0:
            rollout_ms, update_ms = tr.last_breakdown_ms()
            log.update(rollout_ms=round(rollout_ms, 2), update_ms=round(update_ms, 2), seconds=round(time.time() - t0, 3))
            print(json.dumps(log), flush=True)
            if "eval_return" in log:
                tr.record_evaluation(log, cfg.algo.save_cwd)
        if save_resume is not None:
            save_resume_atomic(tr, save_resume)
        if max_iterations is not None and tr.iteration >= max_iterations:
            break
    if tr.rank == 0:
        tr.agent.save_model(cfg.algo.save_cwd)
    return tr
