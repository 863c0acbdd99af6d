"""MAPPO with a diagonal-Gaussian policy on env_3d (continuous 3-D pursuit, BASELINE config 5).

The reference has no learner for env_3d (DHGN/mappo_parallel.py:7 imports torch.distributions.Normal and never uses it).
This module is the package's own: the PPO update, GAE and data-parallel protocol of `MAPPO` / `Trainer`, with
* features: csrc/e3d_env.hip k_e3d_features (16 per pursuer, actor and critic),
* encoder: Linear(16 -> 128) + ReLU, Linear(128 -> 128) + ReLU per network, then the 2-layer GRU trunk of `SharedActor`,
* actor head: Mean = Linear(128 -> A) and a state-independent log_std (A), a = mu + exp(log_std) z, z ~ N(0, 1), unclipped in the
  buffer and clamped to [-1, 1] for the environment (ops.gauss_head_sample, one launch per tick),
* critic head: the spectrally normalised value head of `SharedCritic`,
* loss: ops.ppo_loss_gauss (Normal.log_prob / entropy inside the PPO launch, gradients for mu, log_std and the values).
Two options, both off by default: `algo.gauss_std: state` replaces the log_std vector by a head
LogStd = Linear(128 -> A) on the GRU features, `algo.gauss_squash: tanh` sends tanh(u) to the environment instead of clamp(u, -1, 1)
and subtracts log(1 - tanh(u)^2) from the log-probability; ls is clamped to [algo.log_std_min, algo.log_std_max].  With either on,
the rollout takes ops.gauss_head_sample_ex and the update ops.ppo_loss_gauss_ex; with both off, the calls above.
`algo.gauss_squash: direction` (needs env.action_dim 3): the policy is a Gaussian over a 4-vector u = (u_x, u_y,
u_z, s) -- `latent_dim` 4 sizes the heads, the rollout's `action`, and the buffer's `a_n` / `a_star` -- and the environment receives the
heading and the pitch of (u_x, u_y, u_z) and s (csrc/direction_action.hpp); the log-probability is the plain Normal one of u, the
imitation label is the teacher's unit vector, and the logged imitation metric is `bc_angle_deg` instead of `bc_action_mse`.
`algo.e3d_features: pursuit` (off by default) replaces the 16 features by the 32 line-of-sight features of
ParticleEnv.pursuit_features, and `algo.e3d_evader_obs: sensed | team | global` says when the actor knows where the evader is.
`algo.e3d_critic: central` (off by default; needs the pursuit features): the critic alone reads
ParticleEnv.central_features' row, the 32 columns plus 8 per team-mate (`critic_feat_dim`); the actor, the sampler and the environment
are the ones of `local`, so execution stays decentralised.
`algo.use_obs_norm` (off by default; obs_norm.py): both encoders read the features normalised by a running mean / std that is frozen
during a rollout and merged once after it; the first rollout is the option-off one bit for bit.
`algo.e3d_comm: attention` (off by default; algo.e3d_comm_heads: 1 | 2 | 4 | 8, default 4): between the actor's
encoder and its GRU, one round of multi-head attention between the embeddings of the pursuers that can talk to each other at that tick
(TeamComm: emb_i + out(attention(qkv(emb))_i) over the hearing set M_i = {i} + the live j with pp_adj[i][j] and pp_adj[j][i]; one
ops.comm_mask launch per tick writes the sets as 64-bit words into the buffer's `comm` field, ops.team_attention is the same kernel in
the rollout and in the update).  comm.out starts at zero, so the first rollout is the option-off one bit for bit; the critic is untouched.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils import spectral_norm

from . import guidance as gd
from . import obs_norm as onorm
from . import ops
from . import value_norm as vnorm
from .e3d_env import CENTRAL_MAX_P, EVADER_OBS, PURSUIT_FEAT, ParticleEnv, central_feat
from .model import HeadLinear, _make_linear, _ortho_linear, _Trunk
from .particle_agent import ParticleMAPPO, ParticleTrainer, finish_env, train_particle

FEAT = 16   # e3d_policy_features columns (include/e3d_env.h); algo.e3d_features: pursuit has PURSUIT_FEAT
E3D_FEATURES = ("basic", "pursuit")
E3D_CRITIC = ("local", "central")
E3D_COMM = ("none", "attention")


class E3dEncoder(nn.Module):
    """Linear(in_dim -> E) + ReLU, Linear(E -> E) + ReLU on the policy features (rows, in_dim = 16, 32 or the central critic's) -> (rows, E)"""

    def __init__(self, in_dim, embedding_dim):
        super().__init__()
        self.fc1 = nn.Linear(in_dim, embedding_dim)
        self.fc2 = nn.Linear(embedding_dim, embedding_dim)

    def forward(self, x):
        h = F.relu(ops.linear_skinny(x, self.fc1.weight, self.fc1.bias))
        return ops.linear(h, self.fc2.weight, self.fc2.bias, relu=True)


GAUSS_STD, GAUSS_SQUASH = ("param", "state"), ("clip", "tanh", "direction")
GAUSS_SD_MAX_A = 8   # state mode: a lane of the rollout head holds 2 A x 8 weights (csrc/gauss_policy.hpp k_gauss_head_ex)


class GaussianActor(_Trunk):
    """gauss_std "param": log_std is a parameter vector; "state": LogStd = Linear(128 -> A) on the GRU features, created after Mean
    (it draws from the generator like any layer) and then set to weight 0, bias log_std_init, so that sigma starts as param mode's"""

    def __init__(self, in_dim, embedding_dim, action_dim, num_layers, rnn_hidden_dim, log_std_init=0.0, is_sn=False, gauss_std="param"):
        super().__init__()
        self.shared_net = E3dEncoder(in_dim, embedding_dim)
        self.num_layers, self.rnn_input_dim, self.rnn_hidden_dim = num_layers, embedding_dim, rnn_hidden_dim
        self.GRU = nn.GRU(embedding_dim, rnn_hidden_dim, num_layers)
        self.Mean = _make_linear(rnn_hidden_dim, action_dim, is_sn, HeadLinear)
        if gauss_std == "state":
            self.LogStd = HeadLinear(rnn_hidden_dim, action_dim)
            with torch.no_grad():
                self.LogStd.weight.zero_()
                self.LogStd.bias.fill_(float(log_std_init))
        else:
            self.log_std = nn.Parameter(torch.full((action_dim,), float(log_std_init)))


class TeamComm(nn.Module):
    """algo.e3d_comm: attention -- emb (G P, E) rows in groups of P pursuers and their (G, P) hearing-set words -> emb + out(o), o the
    masked multi-head attention of qkv(emb) inside every group (ops.team_attention); out starts at zero, so the layer starts as the identity"""

    def __init__(self, embedding_dim, heads):
        super().__init__()
        self.heads = int(heads)
        self.qkv = nn.Linear(embedding_dim, 3 * embedding_dim)
        self.out = nn.Linear(embedding_dim, embedding_dim)
        with torch.no_grad():
            self.out.weight.zero_()
            self.out.bias.zero_()

    def forward(self, emb, words):
        # (the kernels read dense words: the rollout's, a time slice of the buffer, are copied -- N P words; the update's are dense)
        o = ops.team_attention(ops.linear(emb, self.qkv.weight, self.qkv.bias), words.contiguous(), self.heads)
        return emb + ops.linear(o, self.out.weight, self.out.bias)


class E3dCritic(_Trunk):
    def __init__(self, in_dim, embedding_dim, num_layers, rnn_hidden_dim, is_sn=False):
        super().__init__()
        self.shared_net = E3dEncoder(in_dim, embedding_dim)
        self.num_layers, self.rnn_input_dim, self.rnn_hidden_dim = num_layers, embedding_dim, rnn_hidden_dim
        self.GRU = nn.GRU(embedding_dim, rnn_hidden_dim, num_layers)
        head = _ortho_linear(rnn_hidden_dim, 1, HeadLinear)
        self.Mean = spectral_norm(head) if is_sn else head


class _E3dRollout:
    """static device storage of one lockstep rollout of N environments (the GRU states ping-pong between two buffers: the
    split-bf16 cell cannot update in place) and the position of its action-sampling stream"""

    def __init__(self, agent, N, P):
        dev, L, H, A, U = agent.device, agent.num_layers, agent.rnn_hidden_dim, agent.action_dim, agent.latent_dim
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
        self.N, self.P = N, P
        self.fa, self.fc = z(N, P, agent.feat_dim), z(N, P, agent.critic_feat_dim)
        self.hbuf_a, self.hbuf_c = z(2, L, N * P, H), z(2, L, N * P, H)
        self.action, self.env_action, self.logp, self.v = z(N, P, U), z(N, P, A, dt=torch.float64), z(N, P), z(N, P)
        self.counter = torch.full((1,), int(agent.sample_rank) << 40, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.live = z(N, P)   # this step's live mask (e3d_policy_record keeps it current)
        if agent.e3d_comm == "attention":
            self.comm = z(N, P, dt=torch.int64)   # this step's hearing sets (ops.comm_mask), where no buffer row takes them
        self.t = 0


def gauss_policy_options(cfg):
    """-> (gauss_std, gauss_squash, log_std_min, log_std_max) of cfg.algo, validated (ValueError naming the key)"""
    a = cfg.algo
    std, squash = str(a.get("gauss_std", "param")), str(a.get("gauss_squash", "clip"))
    if std not in GAUSS_STD:
        raise ValueError(f"algo.gauss_std: {std!r} is not one of {GAUSS_STD}")
    if squash not in GAUSS_SQUASH:
        raise ValueError(f"algo.gauss_squash: {squash!r} is not one of {GAUSS_SQUASH}")
    lo, hi = float(a.get("log_std_min", -5.0)), float(a.get("log_std_max", 2.0))
    if not lo < hi:
        raise ValueError(f"algo.log_std_min ({lo}) must be below algo.log_std_max ({hi})")
    if squash == "direction" and int(cfg.env.action_dim) != ops.DIRECTION_ENV:
        raise ValueError(f"algo.gauss_squash: direction needs env.action_dim {ops.DIRECTION_ENV} (heading, pitch, speed: the commands the "
                         f"direction vector maps to), got {int(cfg.env.action_dim)}")
    if std == "state" and latent_dim(squash, int(cfg.env.action_dim)) > GAUSS_SD_MAX_A:
        raise ValueError(f"algo.gauss_std: state supports env.action_dim <= {GAUSS_SD_MAX_A} (got {int(cfg.env.action_dim)})")
    return std, squash, lo, hi


def latent_dim(gauss_squash, action_dim):
    """the width of the policy's Gaussian: the four dimensions (u_x, u_y, u_z, s) in direction mode, else the environment's actions"""
    return ops.DIRECTION_LATENT if gauss_squash == "direction" else action_dim


def e3d_feature_options(cfg):
    """-> (e3d_features, e3d_evader_obs) of cfg.algo, validated (ValueError naming the key).  e3d_evader_obs belongs to pursuit: with
    basic only its default passes.  The default `sensed` keeps the reference's observation model; it is a choice, not a measurement."""
    a = cfg.algo
    feats, obs = str(a.get("e3d_features", "basic")), str(a.get("e3d_evader_obs", "sensed"))
    if feats not in E3D_FEATURES:
        raise ValueError(f"algo.e3d_features: {feats!r} is not one of {E3D_FEATURES}")
    if obs not in EVADER_OBS:
        raise ValueError(f"algo.e3d_evader_obs: {obs!r} is not one of {EVADER_OBS}")
    if feats == "basic" and obs != "sensed":
        raise ValueError(f"algo.e3d_evader_obs: {obs} needs algo.e3d_features: pursuit (the basic features know the sensed evader only)")
    if feats == "pursuit" and bool(a.get("use_obs_norm", False)):
        raise ValueError("algo.use_obs_norm: true is not supported with algo.e3d_features: pursuit (the normaliser's state and kernels are "
                         "16 columns wide; the pursuit features are built to be of unit scale)")
    return feats, obs


def e3d_critic_options(cfg):
    """-> e3d_critic of cfg.algo, validated (ValueError naming the key): "local", the critic reads the feature set's own critic row, or
    "central" (DESIGN.md section 7k), ParticleEnv.central_features' row with every team-mate in it -- which extends the pursuit features
    and is unrolled over at most CENTRAL_MAX_P pursuers"""
    critic = str(cfg.algo.get("e3d_critic", "local"))
    if critic not in E3D_CRITIC:
        raise ValueError(f"algo.e3d_critic: {critic!r} is not one of {E3D_CRITIC}")
    if critic == "central":
        if str(cfg.algo.get("e3d_features", "basic")) != "pursuit":
            raise ValueError("algo.e3d_critic: central needs algo.e3d_features: pursuit (its row is the pursuit critic row plus the team-mates)")
        if int(cfg.env.num_defender) > CENTRAL_MAX_P:
            raise ValueError(f"algo.e3d_critic: central supports env.num_defender <= {CENTRAL_MAX_P} (got {int(cfg.env.num_defender)})")
    return critic


def e3d_comm_options(cfg):
    """-> (e3d_comm, e3d_comm_heads) of cfg.algo, validated (ValueError naming the key): "none", or "attention" (DESIGN.md section 7m), one
    round of team attention between the actor's encoder and its GRU -- whose kernels are compiled for 128-wide embeddings and keep a
    pursuer's hearing set in one 64-bit word"""
    a = cfg.algo
    comm = str(a.get("e3d_comm", "none"))
    if comm not in E3D_COMM:
        raise ValueError(f"algo.e3d_comm: {comm!r} is not one of {E3D_COMM}")
    try:
        heads = int(a.get("e3d_comm_heads", 4))
    except (TypeError, ValueError):
        heads = None
    if heads not in ops.COMM_HEADS or isinstance(a.get("e3d_comm_heads", 4), bool):
        raise ValueError(f"algo.e3d_comm_heads: {a.get('e3d_comm_heads')!r} is not one of {ops.COMM_HEADS}")
    if comm == "attention":
        if int(a.embedding_dim) != ops.COMM_E:
            raise ValueError(f"algo.e3d_comm: attention needs algo.embedding_dim {ops.COMM_E} (the width its kernels are compiled for), "
                             f"got {int(a.embedding_dim)}")
        if int(cfg.env.num_defender) > ops.COMM_MAX_P:
            raise ValueError(f"algo.e3d_comm: attention supports env.num_defender <= {ops.COMM_MAX_P} (one mask word per pursuer), "
                             f"got {int(cfg.env.num_defender)}")
    return comm, heads


class E3dMAPPO(ParticleMAPPO):
    """rollout (run_episode) and PPO loss (_minibatch_loss) of the Gaussian policy on env_3d; the update loop is ParticleMAPPO.train"""

    ENV = "env_3d (runtime.env: e3d)"

    def _options(self, cfg):
        self.e3d_features, self.e3d_evader_obs = e3d_feature_options(cfg)   # line-of-sight features
        self.feat_dim = PURSUIT_FEAT if self.e3d_features == "pursuit" else FEAT
        self.e3d_critic = e3d_critic_options(cfg)   # the critic's input with every team-mate
        # the width of the critic's rows; feat_dim stays the actor's
        self.critic_feat_dim = central_feat(int(cfg.env.num_defender)) if self.e3d_critic == "central" else self.feat_dim
        self.e3d_comm, self.e3d_comm_heads = e3d_comm_options(cfg)   # team attention in the actor
        self.use_obs_norm, self.obs_norm_clip = onorm.obs_norm_options(cfg)   # running mean / std on the policy features
        self.gauss_std, self.gauss_squash, self.log_std_min, self.log_std_max = gauss_policy_options(cfg)
        self.policy_ex = (self.gauss_std, self.gauss_squash) != ("param", "clip")   # the _ex kernels only when an option is on
        self.action_dim = int(cfg.env.action_dim)
        self.latent_dim = latent_dim(self.gauss_squash, self.action_dim)   # what the heads emit and the buffer stores
        if self.gauss_squash == "direction":
            self.BC_METRIC = "bc_angle_deg"
        if self.kick.on and self.action_dim != 3:
            raise ValueError(f"algo.bc_coef > 0 needs env.action_dim 3 (heading, pitch, speed: what the scripted pursuers command), "
                             f"got {self.action_dim}")
        if self.imitation.on and self.action_dim != 3:
            raise ValueError(f"algo.bc_iterations > 0 needs env.action_dim 3 (heading, pitch, speed: what the scripted pursuers command), "
                             f"got {self.action_dim}")
        # the heading residual is taken modulo 2 in clip mode only: a periodic quantity through tanh has no wrap-around residual, and a
        # direction vector has no periodic dimension at all
        self.bc_wrap0 = self.imitation.heading_wrap and self.gauss_squash == "clip"

    def _build(self, cfg):
        a, sn = cfg.algo, bool(cfg.algo.use_spectral_norm)
        self.actor = GaussianActor(self.feat_dim, self.embedding_dim, self.latent_dim, self.num_layers, self.rnn_hidden_dim,
                                   float(a.get("log_std_init", 0.0)), sn, self.gauss_std).to(self.device)
        self.critic = E3dCritic(self.critic_feat_dim, self.embedding_dim, self.num_layers, self.rnn_hidden_dim, sn).to(self.device)
        self.ac_parameters = list(self.actor.parameters()) + list(self.critic.parameters())
        if self.e3d_comm == "attention":   # constructed last, after the critic: every other parameter keeps the generator draws of `none`
            self.actor.comm = TeamComm(self.embedding_dim, self.e3d_comm_heads).to(self.device)
            self.ac_parameters += list(self.actor.comm.parameters())
        self.obs_norm = onorm.ObsNorm(self.obs_norm_clip, self.device) if self.use_obs_norm else None

    # ---- rollout -------------------------------------------------------------------------------------------------------------
    def _rollout(self, env):
        return _E3dRollout(self, env.num_envs, env.p_num)

    def _buffer_dims(self, env):
        return env.num_envs, env.max_step, env.p_num

    def _policy_step(self, st, greedy=False, words=None):
        """features -> both encoders (with algo.e3d_comm: attention the actor's embeddings then hear their team under `words`, this tick's
        (N, P) hearing sets) -> both GRU cells (one launch per layer) -> value -> Gaussian head and sample"""
        N, P, E = st.N, st.P, self.embedding_dim
        emb_a = self.actor.shared_net(st.fa.view(N * P, self.feat_dim))
        if self.e3d_comm == "attention":
            emb_a = self.actor.comm(emb_a.reshape(N * P, E), words)
        emb_c = self.critic.shared_net(st.fc.view(N * P, self.critic_feat_dim))
        cur, nxt = st.t & 1, (st.t + 1) & 1
        fa, fc = ops.gru_step_multi([emb_a.reshape(-1, E), emb_c.reshape(-1, E)], [st.hbuf_a[cur], st.hbuf_c[cur]], [self.actor.GRU, self.critic.GRU],
                                    hiddens_out=[st.hbuf_a[nxt], st.hbuf_c[nxt]])
        self.critic.head(fc.contiguous(), out=st.v)
        m = self.actor.Mean
        if self.policy_ex:
            ls = (self.actor.LogStd.weight, self.actor.LogStd.bias) if self.gauss_std == "state" else self.actor.log_std
            ops.gauss_head_sample_ex(fa.contiguous(), m.weight, m.bias, ls, self.sample_seed, st.counter, st.ticket,
                                     (st.action, st.env_action, st.logp), greedy=greedy, log_std_min=self.log_std_min,
                                     log_std_max=self.log_std_max, squash=self.gauss_squash)
        else:
            ops.gauss_head_sample(fa.contiguous(), m.weight, m.bias, self.actor.log_std, self.sample_seed, st.counter, st.ticket,
                                  (st.action, st.env_action, st.logp), greedy=greedy)
        st.t += 1

    def _features(self, env, st, accumulate=False):
        """the policy features of the current state into st.fa / st.fc; with algo.use_obs_norm normalised under the agent's state, and,
        when `accumulate` (the ticks of a training rollout), the sums of the raw features of the live rows added to the slots;
        with algo.e3d_features: pursuit the 32 line-of-sight features under algo.e3d_evader_obs (never normalised), and with
        algo.e3d_critic: central the wide critic rows from the same launch"""
        if self.e3d_critic == "central":
            return env.central_features(st.fa, st.fc, self.e3d_evader_obs)
        if self.e3d_features == "pursuit":
            return env.pursuit_features(st.fa, st.fc, self.e3d_evader_obs)
        on = self.obs_norm
        if on is None:
            return env.policy_features(st.fa, st.fc)
        if not accumulate:
            return env.policy_features(st.fa, st.fc, on.state, on.clip)
        return env.policy_features(st.fa, st.fc, on.state, on.clip, st.live, on.slots_for(st.N * st.P))

    def _bootstrap_value(self, st):
        """the critic's value of the state after the last step (its encoder, GRU cell and head only)"""
        N, P = st.N, st.P
        emb_c = self.critic.shared_net(st.fc.view(N * P, self.critic_feat_dim))
        (fc,) = ops.gru_step_multi([emb_c.reshape(N * P, -1)], [st.hbuf_c[st.t & 1]], [self.critic.GRU], hiddens_out=[st.hbuf_c[(st.t + 1) & 1]])
        return self.critic.head(fc.contiguous()).reshape(N, P)

    def new_buffer(self, N, T, P):
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)
        buf = dict(feat_a=z(N, T, P, self.feat_dim), feat_c=z(N, T, P, self.critic_feat_dim), a_n=z(N, T, P, self.latent_dim), a_logprob_n=z(N, T, P), r=z(N, T, P),
                   active=z(N, T, P), v_n=z(N, T + 1, P))
        if self.value_norm is not None:
            buf["v_mask"] = z(N, P)   # the bootstrap mask of v_n[:, T] (algo.use_value_norm only)
        if self.e3d_comm == "attention":
            buf["comm"] = torch.zeros((N, T, P), dtype=torch.int64, device=self.device)   # the hearing sets of every row, one word each
        if self.teacher:
            buf["a_star"] = z(N, T, P, self.latent_dim)   # the scripted pursuers' action of every row, in the policy's pre-squash space (algo.bc_iterations / bc_coef only)
        return buf

    @torch.no_grad()
    def run_episode(self, env, buf=None, greedy=False, policy="network", follow=None):
        """N episodes in lockstep for T = env.max_step ticks.  Row (n, t, p) is live iff environment n was not done before step t and
        pursuer p was active at its start; rewards, values and the `active` mask of other rows are zero, so is v_n[n, t + 1, p] when
        pursuer p or episode n ended in step t for any reason but the time limit; v_n[:, T] is the critic's bootstrap value.  The masks
        and the per-environment accumulators are one launch per tick (ParticleEnv.policy_record); with algo.use_reward_scaling and a
        buffer, r is the scaled reward (env.reward_scale advances) while the return stays the raw one; with algo.reward_shaping:
        distance and a buffer, r (what is scaled, when both are on) carries the shaping term gamma Phi' - Phi (env.shaping_phi); with
        algo.team_reward: alpha > 0 and a buffer, the reward that enters all of this is (1 - alpha) x + alpha (the team's sum of the step).
        With algo.use_obs_norm the features (and feat_a / feat_c) are normalised under obs_norm.state, which no tick changes; with a
        buffer every tick adds the sums of its live rows to obs_norm.slots (explore_env merges them).
        policy="guidance" (buf must be None): the tick takes the scripted pursuers' actions (guidance_episode below) instead of the
        network's; no network, sampler or sampling counter is touched, the accumulators and the returned triple are the same.
        follow (explore_expert; needs a buffer): a (N,) uint8 mask -- every tick labels buf["a_star"][:, t] with the scripted pursuers'
        actions and executes them in the environments whose mask is set (_expert_tick).
        Returns per-environment (return, captured, length) device tensors."""
        gd.check_policy(policy, buf)
        if policy == "guidance":
            return guidance_episode(env)
        env.reset()
        st = self._state(env)
        st.hbuf_a.zero_()
        st.hbuf_c.zero_()
        st.t = 0
        st.live.copy_(env.active_t)   # no environment is done; policy_record writes the next step's mask
        acc = env.new_accumulators()
        scale_gamma, shaping_gamma = self._shaping_gammas(env, buf)
        team_coef = self._team_coef(buf)
        for t in range(env.max_step):
            self._features(env, st, accumulate=buf is not None)   # evaluation never accumulates
            words = None
            if self.e3d_comm == "attention":   # who hears whom at this tick, straight into the buffer's row
                words = ops.comm_mask(env.obs["pp_adj"], st.live, st.comm if buf is None else buf["comm"][:, t])
            self._policy_step(st, greedy, words)
            if follow is not None:
                self._expert_tick(env, st.env_action, buf, t, follow)
            env.evader_step()
            env.step(st.env_action)
            if buf is None:
                env.policy_record(acc, st.live, live_next=st.live)
                continue
            buf["feat_a"][:, t].copy_(st.fa)
            buf["feat_c"][:, t].copy_(st.fc)
            buf["a_n"][:, t].copy_(st.action)
            buf["a_logprob_n"][:, t].copy_(st.logp)
            env.policy_record(acc, st.live, st.v, buf["r"][:, t], buf["active"][:, t], buf["v_n"][:, t], buf["v_n"][:, t + 1], st.live,
                              scale_gamma=scale_gamma, shaping_gamma=shaping_gamma, team_coef=team_coef)
        if buf is not None:
            self._features(env, st)   # the state after the last step: normalised, not counted
            self._record_bootstrap(env, st, buf, acc)
        return acc["ret"], acc["captured"] != 0, acc["length"]

    # ---- update ------------------------------------------------------------------------------------------------------------------
    def sequence_forward(self, feat_a, feat_c, batch, steps, return_ls_raw=False, words=None):
        """(batch, T, P, feat_dim / critic_feat_dim) features of whole episodes -> mu (batch, T, P, A) and values (batch, T, P), time-major views; with
        return_ls_raw also ls_raw (state mode: the LogStd head on the same GRU features, (batch, T, P, A); param mode: log_std);
        words (algo.e3d_comm: attention): the (batch, T, P) hearing sets of the rows, whose groups are P consecutive rows"""
        P = feat_a.shape[2]
        R = batch * steps * P
        emb_a, emb_c = self.actor.shared_net(feat_a.reshape(R, self.feat_dim)), self.critic.shared_net(feat_c.reshape(R, self.critic_feat_dim))
        if self.e3d_comm == "attention":
            emb_a = self.actor.comm(emb_a, words.reshape(batch * steps, P))
        h0 = [torch.zeros(m.num_layers, batch * P, m.rnn_hidden_dim, dtype=emb_a.dtype, device=emb_a.device) for m in (self.actor, self.critic)]
        fa, fc = ops.gru_multi([emb_a, emb_c], h0, [self.actor.GRU, self.critic.GRU], agents=P, steps=steps, zero_state=True)
        fa, fc = fa.reshape(steps, batch, P, -1), fc.reshape(steps, batch, P, -1)
        mu = self.actor.Mean(fa).permute(1, 0, 2, 3)
        values = self.critic.Mean(fc).permute(1, 0, 2, 3)[..., 0]
        if not return_ls_raw:
            return mu, values
        ls_raw = self.actor.LogStd(fa).permute(1, 0, 2, 3) if self.gauss_std == "state" else self.actor.log_std
        return mu, values, ls_raw

    def _words(self, buf, n0, n1):
        """the hearing sets of episodes [n0, n1) (algo.e3d_comm: attention; None without it: the buffer has no such field)"""
        return buf["comm"][n0:n1] if self.e3d_comm == "attention" else None

    def _minibatch_loss(self, buf, n0, n1, adv, v_target, dk):
        mu, values, ls_raw = self.sequence_forward(buf["feat_a"][n0:n1], buf["feat_c"][n0:n1], n1 - n0, buf["r"].shape[1], return_ls_raw=True,
                                                     words=self._words(buf, n0, n1))
        tail = self._loss_tail(buf, n0, n1, values, adv, v_target)
        if self.policy_ex:
            return ops.ppo_loss_gauss_ex(mu, ls_raw, *tail, log_std_min=self.log_std_min, log_std_max=self.log_std_max,
                                         squash=self.gauss_squash, **dk)
        return ops.ppo_loss_gauss(mu, ls_raw, *tail, **dk)

    BC_METRIC = "bc_action_mse"

    def bc_metric(self, sq_sum, rows):
        """the mean squared residual per action dimension over the live rows (after the heading wrap), from the launches' two sums;
        in direction mode (BC_METRIC is bc_angle_deg) the first sum is of angles in radians: the mean angle between mu[:3] and the
        teacher's unit vector, in degrees"""
        if not rows:
            return float("nan")
        if self.gauss_squash == "direction":
            return math.degrees(sq_sum / rows)
        return sq_sum / (self.action_dim * rows)

    def _imitation_loss(self, buf, n0, n1, v_target, sums):
        mu, values, ls_raw = self.sequence_forward(buf["feat_a"][n0:n1], buf["feat_c"][n0:n1], n1 - n0, buf["r"].shape[1], return_ls_raw=True,
                                                     words=self._words(buf, n0, n1))
        lo, hi = (self.log_std_min, self.log_std_max) if self.policy_ex else (-float("inf"), float("inf"))
        return ops.bc_loss_gauss(mu, ls_raw, buf["a_star"][n0:n1], *self._imitation_tail(buf, n0, n1, values, v_target), log_std_min=lo,
                                 log_std_max=hi, fit_std=self.imitation.fit_std, wrap0=self.bc_wrap0, sums=sums,
                                 metric="angle" if self.gauss_squash == "direction" else "mse")

    def _kick_loss(self, buf, n0, n1, adv, v_target, coef, sums, dk):
        mu, values, ls_raw = self.sequence_forward(buf["feat_a"][n0:n1], buf["feat_c"][n0:n1], n1 - n0, buf["r"].shape[1], return_ls_raw=True,
                                                     words=self._words(buf, n0, n1))
        lo, hi = (self.log_std_min, self.log_std_max) if self.policy_ex else (-float("inf"), float("inf"))
        a_n, *tail = self._loss_tail(buf, n0, n1, values, adv, v_target)
        return ops.ppo_bc_loss_gauss(mu, ls_raw, a_n, buf["a_star"][n0:n1], *tail[:-1], coef, tail[-1], log_std_min=lo, log_std_max=hi,
                                     squash=self.gauss_squash, fit_std=self.imitation.fit_std, wrap0=self.bc_wrap0,
                                     metric="angle" if self.gauss_squash == "direction" else "mse", sums=sums, **dk)

    def policy_meta(self):
        """the "policy" entry of checkpoints and resume bundles: None in the default mode (param, clip, basic features), whose files
        carry none; e3d_features / e3d_evader_obs only with algo.e3d_features: pursuit, e3d_critic only with algo.e3d_critic: central,
        e3d_comm / e3d_comm_heads only with algo.e3d_comm: attention"""
        meta = {}
        if self.policy_ex:
            meta.update(gauss_std=self.gauss_std, gauss_squash=self.gauss_squash, log_std_min=self.log_std_min, log_std_max=self.log_std_max)
        if self.e3d_features == "pursuit":
            meta.update(e3d_features=self.e3d_features, e3d_evader_obs=self.e3d_evader_obs)
        if self.e3d_critic == "central":
            meta.update(e3d_critic=self.e3d_critic)
        if getattr(self, "e3d_comm", "none") == "attention":
            meta.update(e3d_comm=self.e3d_comm, e3d_comm_heads=self.e3d_comm_heads)
        return meta or None

    def check_policy_meta(self, meta, what):
        """ValueError naming the config key when a file's policy (its "policy" entry; None = the default mode) is not this agent's:
        gauss_std and gauss_squash, and with an option on (where the bounds act) log_std_min / log_std_max as well -- other bounds would
        neither reproduce the saved policy nor continue its run bit for bit; and the feature set and its evader model (a file without the
        entries was written with basic, sensed, local): other inputs fit neither the first layer nor what the weights were trained on;
        and e3d_comm with, where it is on, its head count (a file without the entry was written with none): the actor has the layer or not"""
        meta = meta or {}
        for key, default in (("e3d_features", "basic"), ("e3d_evader_obs", "sensed"), ("e3d_critic", "local"), ("e3d_comm", "none"),
                             ("gauss_std", "param"), ("gauss_squash", "clip")):
            theirs, mine = meta.get(key, default), getattr(self, key, default)
            if theirs != mine:
                raise ValueError(f"{what} was written with algo.{key}: {theirs}, this agent has algo.{key}: {mine}")
        if getattr(self, "e3d_comm", "none") == "attention":   # (heads split the same weights differently: the shapes would load)
            theirs, mine = int(meta["e3d_comm_heads"]), self.e3d_comm_heads
            if theirs != mine:
                raise ValueError(f"{what} was written with algo.e3d_comm_heads: {theirs}, this agent has algo.e3d_comm_heads: {mine}")
        if self.policy_ex:   # (the default mode has no bounds; its files carry no entry)
            for key in ("log_std_min", "log_std_max"):
                theirs, mine = float(meta[key]), getattr(self, key)
                if theirs != mine:
                    raise ValueError(f"{what} was written with algo.{key}: {theirs}, this agent has algo.{key}: {mine}")

    def save_model(self, cwd, best=False):
        """cwd/e3d_state_dicts.pt (best: e3d_state_dicts_best.pt), the actor's and critic's state_dicts (and, with a non-default
        algo.gauss_std / gauss_squash / e3d_features, the "policy" entry of policy_meta; with algo.use_value_norm the "value_norm" entry: beta and the state;
        with algo.use_obs_norm the "obs_norm" entry: the clip and the state)"""
        os.makedirs(cwd, exist_ok=True)
        sd = {"actor": self.actor.state_dict(), "critic": self.critic.state_dict()}
        if self.policy_meta() is not None:
            sd["policy"] = self.policy_meta()
        if self.value_norm is not None:   # algo.use_value_norm: the critic's outputs mean nothing without the statistics
            sd["value_norm"] = self.value_norm.entry()
        if self.obs_norm is not None:     # algo.use_obs_norm: the weights mean nothing without the statistics of their inputs
            sd["obs_norm"] = self.obs_norm.entry()
        torch.save(sd, os.path.join(cwd, f"e3d_state_dicts{'_best' if best else ''}.pt"))

    def load_model(self, cwd, best=False):
        """the weights save_model(cwd, best) wrote; ValueError when they belong to another gauss_std / gauss_squash, algo.use_value_norm or
        algo.use_obs_norm"""
        path = os.path.join(cwd, f"e3d_state_dicts{'_best' if best else ''}.pt")
        sd = torch.load(path, map_location=self.device)
        self.check_policy_meta(sd.get("policy"), path)
        vnorm.check_entry(self, sd.get("value_norm"), path, check_beta=False)
        onorm.check_entry(self, sd.get("obs_norm"), path, check_clip=False)
        self.actor.load_state_dict(sd["actor"])
        self.critic.load_state_dict(sd["critic"])
        if self.value_norm is not None:
            self.value_norm.load_entry(sd["value_norm"])
        if self.obs_norm is not None:
            self.obs_norm.load_entry(sd["obs_norm"])


@torch.no_grad()
def guidance_episode(env):
    """N episodes in lockstep for T = env.max_step ticks with the scripted lead-pursuit pursuers (ParticleEnv.guidance_actions, one
    launch per tick) where run_episode has its policy step: the evader's command, the tick and policy_record are run_episode's, so the
    raw return, the captured flag and the length mean what they mean there.  Needs no agent.
    Returns per-environment (return, captured, length) device tensors."""
    env.reset()
    live = env.active_t.float()   # no environment is done; policy_record writes the next step's mask
    acc = env.new_accumulators()
    for _ in range(env.max_step):
        actions = env.guidance_actions()
        env.evader_step()
        env.step(actions)
        env.policy_record(acc, live, live_next=live)
    return acc["ret"], acc["captured"] != 0, acc["length"]


def make_env(cfg, num_envs, rank=0, device="cuda", seed_offset=0, training=True):
    """ParticleEnv of one rank: environment n of rank r is reset from seed + max(1000, num_envs) r + n (as Pursuit_Env), with the
    options of a training or an evaluation environment (particle_agent.finish_env)"""
    base = int(cfg.runtime.get("seed", 0)) + seed_offset + max(1000, num_envs) * rank
    env = ParticleEnv(num_envs=num_envs, seeds=[base + n for n in range(num_envs)], device=device, max_step=int(cfg.env.max_steps),
                      evader=str(cfg.runtime.get("e3d_evader", "slsqp")))
    env.initialize(int(cfg.env.num_defender))
    return finish_env(env, cfg, training)


class E3dTrainer(ParticleTrainer):
    """ParticleTrainer of E3dMAPPO on env_3d"""
    agent_cls, make_env = E3dMAPPO, staticmethod(make_env)


def train_e3d(cfg, **kw):
    """the env_3d training loop (main --config cfg5): particle_agent.train_particle on E3dTrainer"""
    return train_particle(E3dTrainer, cfg, **kw)
