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
import os

import torch

from . import guidance as gd
from . import ops
from . import value_norm as vnorm
from .model import build_actor_critic, sequence_forward_pair
from .n2n_env import ParticleEnv
from .particle_agent import ParticleMAPPO, ParticleTrainer, finish_env, train_particle

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


class N2nMAPPO(ParticleMAPPO):
    """rollout (run_episode) and PPO loss (_minibatch_loss) of the DHGN actor / critic on env_n2n; the update loop is ParticleMAPPO.train"""

    ENV = "env_n2n (runtime.env: n2n)"

    def _options(self, cfg):
        a = cfg.algo
        if bool(a.get("use_obs_norm", False)):
            raise ValueError("algo.use_obs_norm: true is built for runtime.env e3d only; the env_n2n inputs are node states whose "
                             "differences the message kernels form and whose zero rows stand for absent nodes (set use_obs_norm to false)")
        if str(a.get("e3d_comm", "none")) != "none":
            raise ValueError(f"algo.e3d_comm: {a.get('e3d_comm')} is built for runtime.env e3d only; the DHGN encoder of env_n2n already passes "
                             "messages along pp_adj (leave the key out)")
        if int(cfg.env.num_defender) > MAX_P:
            raise ValueError(f"env.num_defender={cfg.env.num_defender}: the DHGN message kernels take at most {MAX_P} pursuers per row")
        if int(cfg.env.state_dim) != 4 or int(cfg.env.action_dim) != 9 or int(a.num_relation) != 3:
            raise ValueError("env_n2n runs the pursuit model: env.state_dim 4, env.action_dim 9, algo.num_relation 3")
        self.depth = int(a.depth)

    def _build(self, cfg):
        if str(cfg.algo.get("encoder", "dhgn")).lower() != "dhgn":
            raise ValueError("env_n2n trains the DHGN encoder only (algo.encoder: dhgn)")
        self.actor, self.critic = build_actor_critic(cfg, self.device)
        if not (self.actor.use_rnn and self.critic.use_rnn):
            raise ValueError("env_n2n trains the GRU actor / critic only (algo.use_rnn: true)")
        enc = self.actor.shared_net
        # the parameter order of MAPPO.ac_parameters (the reference's, :631)
        self.ac_parameters = (list(enc.parameters()) + list(self.actor.GRU.parameters()) + list(self.critic.GRU.parameters())
                              + list(self.critic.Mean.parameters()) + list(self.actor.Mean.parameters()))

    # ---- rollout -------------------------------------------------------------------------------------------------------------
    def _rollout(self, env):
        return _N2nRollout(self, env)

    def _buffer_dims(self, env):
        return env.num_envs, env.episode_limit, env.p_num, env.e_num

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
        if self.teacher:
            buf["a_star"] = z(N, T, P)   # the scripted pursuers' action of every row (algo.bc_iterations / bc_coef only)
        return buf

    @torch.no_grad()
    def run_episode(self, env, buf=None, greedy=False, policy="network", follow=None):
        """N episodes in lockstep for T = env.episode_limit ticks.  Per tick: policy_inputs, the policy step, the SLSQP evader, the tick,
        policy_record, and (with a buffer) one rollout_record launch.  Row (n, t, p) is live iff pursuer p was active at the start of step t
        and environment n was not done before it; r, v_n and `active` of other rows are zero, so is v_n[n, t + 1, p] when pursuer p or
        episode n ended in step t for a reason other than the time limit; v_n[:, T] is the critic's bootstrap value under that rule.
        With algo.use_reward_scaling and a buffer, r is the scaled reward (env.reward_scale advances); acc["ret"] stays the raw return.
        With algo.reward_shaping: distance and a buffer, r (what is scaled, when both are on) carries the shaping term
        gamma Phi' - Phi (env.shaping_phi, written by shaping_begin after the reset).  With algo.team_reward: alpha > 0 and a buffer,
        the reward that enters all of this is (1 - alpha) x + alpha (the team's sum of the step).
        policy="guidance" (buf must be None): the tick takes the scripted pursuers' actions (guidance_episode below) instead of the
        network's; no network, sampler or sampling counter is touched, the accumulators are the same.
        follow (explore_expert; needs a buffer): a (N,) uint8 mask -- every tick labels buf["a_star"][:, t] with the scripted pursuers'
        actions and executes them in the environments whose mask is set (_expert_tick); buf["a_n"] then holds the executed action.
        Returns the per-environment accumulators (done_before, ended, captured, ret, length)."""
        gd.check_policy(policy, buf)
        if policy == "guidance":
            return guidance_episode(env)
        d = self.depth
        env.reset()
        st = self._state(env)
        st.reset()
        acc = env.new_accumulators()
        scale_gamma, shaping_gamma = self._shaping_gammas(env, buf)
        team_coef = self._team_coef(buf)
        for t in range(env.episode_limit):
            env.policy_inputs(st.p4, st.e4, st.e_ref, st.live, st.pp, st.pe, acc["done_before"])
            self._policy_step(st, greedy)
            if follow is not None:
                self._expert_tick(env, st.a_n, buf, t, follow)
            env.evader_step()
            env.step(st.a_n)
            if buf is None:
                env.policy_record(acc, st.live)
                continue
            env.policy_record(acc, st.live, st.v, buf["r"][:, t], buf["active"][:, t], buf["v_n"][:, t], buf["v_n"][:, t + 1],
                              scale_gamma=scale_gamma, shaping_gamma=shaping_gamma, team_coef=team_coef)
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
            self._record_bootstrap(env, st, buf, acc)
        return acc

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

    def _minibatch_loss(self, buf, n0, n1, adv, v_target, dk):
        prob, values = self.sequence_forward(buf, n0, n1)
        return ops.ppo_loss_prob(prob, *self._loss_tail(buf, n0, n1, values, adv, v_target), **dk)

    BC_METRIC = "bc_accuracy"

    def bc_metric(self, hits, rows):
        """the share of live rows whose most probable action is the label, from the launches' two sums"""
        return hits / rows if rows else float("nan")

    def _imitation_loss(self, buf, n0, n1, v_target, sums):
        prob, values = self.sequence_forward(buf, n0, n1)
        return ops.bc_loss_cat(prob, buf["a_star"][n0:n1], *self._imitation_tail(buf, n0, n1, values, v_target), sums=sums)

    def _kick_loss(self, buf, n0, n1, adv, v_target, coef, sums, dk):
        prob, values = self.sequence_forward(buf, n0, n1)
        a_n, *tail = self._loss_tail(buf, n0, n1, values, adv, v_target)
        return ops.ppo_bc_loss_cat(prob, a_n, buf["a_star"][n0:n1], *tail[:-1], coef, tail[-1], sums=sums, **dk)

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
    """ParticleEnv of one rank: environment n of rank r is reset from seed + max(1000, num_envs) r + n (as Pursuit_Env), with the
    options of a training or an evaluation environment (particle_agent.finish_env)"""
    base = int(cfg.runtime.get("seed", 0)) + seed_offset + max(1000, num_envs) * rank
    env = ParticleEnv(num_envs=num_envs, seeds=[base + n for n in range(num_envs)], device=device, episode_limit=int(cfg.env.max_steps),
                      evader=str(cfg.runtime.get("n2n_evader", "slsqp")))
    env.initialize(int(cfg.env.num_defender), int(cfg.env.num_evader))
    return finish_env(env, cfg, training)


class N2nTrainer(ParticleTrainer):
    """ParticleTrainer of N2nMAPPO on env_n2n; its log lines carry the device-event times of the rollout and the update"""
    agent_cls, make_env, log_breakdown = N2nMAPPO, staticmethod(make_env), True


def train_n2n(cfg, **kw):
    """the env_n2n training loop (main --config cfg4_n2n): particle_agent.train_particle on N2nTrainer"""
    return train_particle(N2nTrainer, cfg, **kw)
