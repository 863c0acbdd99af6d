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
`algo.use_obs_norm` (off by default; obs_norm.py): both encoders read the features normalised by a running mean / std that is frozen
during a rollout and merged once after it; the first rollout is the option-off one bit for bit.
"""
import json
import os
import time

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils import spectral_norm

from . import guidance as gd
from . import obs_norm as onorm
from . import ops
from . import value_norm as vnorm
from .minibatch_steps import MAX_GRAD_NORM, minibatch_steps_options
from .reward_shaping import reward_shaping_options
from .update_diag import LOG_KEYS, UpdateDiag, first_epoch_over, update_diag_options
from .e3d_env import ParticleEnv
from .model import HeadLinear, _make_linear, _ortho_linear, _Trunk
from .trainer import (BUCKET_ALIGN, FusedAdam, GradBucket, ParamBucket, ParticleRunState, allreduce_sum_, broadcast_weights_,
                      enable_tuned_gemms, init_distributed, resume_path, save_resume_atomic)

FEAT = 16   # e3d_policy_features columns (include/e3d_env.h)


class E3dEncoder(nn.Module):
    """Linear(16 -> E) + ReLU, Linear(E -> E) + ReLU on the policy features (rows, 16) -> (rows, E)"""

    def __init__(self, in_dim, embedding_dim):
        super().__init__()
        self.fc1 = nn.Linear(in_dim, embedding_dim)
        self.fc2 = nn.Linear(embedding_dim, embedding_dim)

    def forward(self, x):
        h = F.relu(ops.linear_skinny(x, self.fc1.weight, self.fc1.bias))
        return ops.linear(h, self.fc2.weight, self.fc2.bias, relu=True)


GAUSS_STD, GAUSS_SQUASH = ("param", "state"), ("clip", "tanh")
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
        dev, L, H, A = agent.device, agent.num_layers, agent.rnn_hidden_dim, agent.action_dim
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
        self.N, self.P = N, P
        self.fa, self.fc = z(N, P, FEAT), z(N, P, FEAT)
        self.hbuf_a, self.hbuf_c = z(2, L, N * P, H), z(2, L, N * P, H)
        self.action, self.env_action, self.logp, self.v = z(N, P, A), z(N, P, A, dt=torch.float64), z(N, P), z(N, P)
        self.counter = torch.full((1,), int(agent.sample_rank) << 40, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.live = z(N, P)   # this step's live mask (e3d_policy_record keeps it current)
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
    if std == "state" and int(cfg.env.action_dim) > GAUSS_SD_MAX_A:
        raise ValueError(f"algo.gauss_std: state supports env.action_dim <= {GAUSS_SD_MAX_A} (got {int(cfg.env.action_dim)})")
    return std, squash, lo, hi


class E3dMAPPO:
    """rollout (run_episode / explore_env) and PPO update (train) of the Gaussian policy on env_3d"""

    def __init__(self, cfg, batch_size, mini_batch_size, device="cuda"):
        a = cfg.algo
        if bool(a.get("use_reward_norm", False)):
            raise ValueError("algo.use_reward_norm: true is not supported on env_3d (runtime.env: e3d); set it to false")
        self.use_reward_scaling = bool(a.get("use_reward_scaling", False))   # the reference's RewardScaling in policy_record
        self.use_value_norm, self.value_norm_beta = vnorm.value_norm_options(cfg)   # ValueNorm on the value targets
        self.reward_shaping, self.shaping_coef = reward_shaping_options(cfg)   # distance shaping in policy_record
        self.use_obs_norm, self.obs_norm_clip = onorm.obs_norm_options(cfg)   # running mean / std on the policy features
        self.gauss_std, self.gauss_squash, self.log_std_min, self.log_std_max = gauss_policy_options(cfg)
        self.update_diagnostics, self.target_kl = update_diag_options(cfg)   # what the update did, from the loss launches
        self.minibatch_steps = minibatch_steps_options(cfg)   # one clip + Adam step per mini-batch, fused
        self.guidance = gd.guidance_options(cfg)   # the scripted pursuers of run_episode(policy="guidance")
        self.policy_ex = (self.gauss_std, self.gauss_squash) != ("param", "clip")   # the _ex kernels only when an option is on
        self.batch_size, self.mini_batch_size = int(batch_size), int(mini_batch_size)
        self.max_train_steps, self.lr, self.gamma, self.lamda = a.max_train_steps, a.lr, a.gamma, a.lamda
        self.epsilon, self.entropy_coef = a.epsilon, a.entropy_coef
        self.use_grad_clip, self.use_lr_decay = a.use_grad_clip, a.use_lr_decay
        self.use_adv_norm, self.use_value_clip = a.use_adv_norm, a.use_value_clip
        self.action_dim, self.num_layers = int(cfg.env.action_dim), int(a.num_layers)
        self.embedding_dim, self.rnn_hidden_dim = int(a.embedding_dim), int(a.rnn_hidden_dim)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("E3dMAPPO runs on the GPU only (HIP kernels, no CPU fallback)")
        sn = bool(a.use_spectral_norm)
        self.actor = GaussianActor(FEAT, self.embedding_dim, self.action_dim, self.num_layers, self.rnn_hidden_dim,
                                   float(a.get("log_std_init", 0.0)), sn, self.gauss_std).to(self.device)
        self.critic = E3dCritic(FEAT, self.embedding_dim, self.num_layers, self.rnn_hidden_dim, sn).to(self.device)
        self.ac_parameters = list(self.actor.parameters()) + list(self.critic.parameters())
        self.param_bucket = None
        if self.minibatch_steps:   # the parameters and their gradients as two flat tensors of one layout, stepped by two launches
            self.param_bucket = ParamBucket(self.ac_parameters)
            self.ac_optimizer = FusedAdam(self.param_bucket, lr=self.lr, eps=1e-5)
        else:
            self.ac_optimizer = torch.optim.Adam(self.ac_parameters, lr=self.lr, eps=1e-5)
        self.value_norm = vnorm.ValueNorm(self.value_norm_beta, self.device) if self.use_value_norm else None
        self.obs_norm = onorm.ObsNorm(self.obs_norm_clip, self.device) if self.use_obs_norm else None
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
            st = self._states[id(env)] = _E3dRollout(self, env.num_envs, env.p_num)
        return st

    def _policy_step(self, st, greedy=False):
        """features -> both encoders -> both GRU cells (one launch per layer) -> value -> Gaussian head and sample"""
        N, P, E = st.N, st.P, self.embedding_dim
        emb_a = self.actor.shared_net(st.fa.view(N * P, FEAT))
        emb_c = self.critic.shared_net(st.fc.view(N * P, FEAT))
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
        when `accumulate` (the ticks of a training rollout), the sums of the raw features of the live rows added to the slots"""
        on = self.obs_norm
        if on is None:
            return env.policy_features(st.fa, st.fc)
        if not accumulate:
            return env.policy_features(st.fa, st.fc, on.state, on.clip)
        return env.policy_features(st.fa, st.fc, on.state, on.clip, st.live, on.slots_for(st.N * st.P))

    def _bootstrap_value(self, st):
        """the critic's value of the state after the last step (its encoder, GRU cell and head only)"""
        N, P = st.N, st.P
        emb_c = self.critic.shared_net(st.fc.view(N * P, FEAT))
        (fc,) = ops.gru_step_multi([emb_c.reshape(N * P, -1)], [st.hbuf_c[st.t & 1]], [self.critic.GRU], hiddens_out=[st.hbuf_c[(st.t + 1) & 1]])
        return self.critic.head(fc.contiguous()).reshape(N, P)

    def new_buffer(self, N, T, P):
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)
        buf = dict(feat_a=z(N, T, P, FEAT), feat_c=z(N, T, P, FEAT), a_n=z(N, T, P, self.action_dim), a_logprob_n=z(N, T, P), r=z(N, T, P),
                   active=z(N, T, P), v_n=z(N, T + 1, P))
        if self.value_norm is not None:
            buf["v_mask"] = z(N, P)   # the bootstrap mask of v_n[:, T] (algo.use_value_norm only)
        return buf

    @torch.no_grad()
    def run_episode(self, env, buf=None, greedy=False, policy="network"):
        """N episodes in lockstep for T = env.max_step ticks.  Row (n, t, p) is live iff environment n was not done before step t and
        pursuer p was active at its start; rewards, values and the `active` mask of other rows are zero, so is v_n[n, t + 1, p] when
        pursuer p or episode n ended in step t for any reason but the time limit; v_n[:, T] is the critic's bootstrap value.  The masks
        and the per-environment accumulators are one launch per tick (ParticleEnv.policy_record); with algo.use_reward_scaling and a
        buffer, r is the scaled reward (env.reward_scale advances) while the return stays the raw one; with algo.reward_shaping:
        distance and a buffer, r (what is scaled, when both are on) carries the shaping term gamma Phi' - Phi (env.shaping_phi).
        With algo.use_obs_norm the features (and feat_a / feat_c) are normalised under obs_norm.state, which no tick changes; with a
        buffer every tick adds the sums of its live rows to obs_norm.slots (explore_env merges them).
        policy="guidance" (buf must be None): the tick takes the scripted pursuers' actions (guidance_episode below) instead of the
        network's; no network, sampler or sampling counter is touched, the accumulators and the returned triple are the same.
        Returns per-environment (return, captured, length) device tensors."""
        gd.check_policy(policy, buf)
        if policy == "guidance":
            return guidance_episode(env)
        N, P, T = env.num_envs, env.p_num, env.max_step
        env.reset()
        st = self._state(env)
        st.hbuf_a.zero_()
        st.hbuf_c.zero_()
        st.t = 0
        st.live.copy_(env.active_t)   # no environment is done; policy_record writes the next step's mask
        acc = env.new_accumulators()
        scale_gamma = self.gamma if (self.use_reward_scaling and buf is not None) else None   # evaluation never scales
        shaping_gamma = self.gamma if (self.reward_shaping == "distance" and buf is not None) else None   # ... and never shapes
        if shaping_gamma is not None:
            env.shaping_begin()
        for t in range(T):
            self._features(env, st, accumulate=buf is not None)   # evaluation never accumulates
            self._policy_step(st, greedy)
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
                              scale_gamma=scale_gamma, shaping_gamma=shaping_gamma)
        if buf is not None:
            self._features(env, st)   # the state after the last step: normalised, not counted
            vmask = env.active_t.float() * (acc["ended"] == 0).float()[:, None]
            buf["v_n"][:, T].copy_(self._bootstrap_value(st) * vmask)
            if self.value_norm is not None:   # the denormalisation of v_n[:, T] needs the mask itself: 0 std + mean is not 0
                buf["v_mask"].copy_(vmask)
        return acc["ret"], acc["captured"] != 0, acc["length"]

    def explore_env(self, env):
        """one episode per environment into a fresh buffer -> (mean return, buffer, env-steps, stats)"""
        N, P, T = env.num_envs, env.p_num, env.max_step
        if self.buffer is None or self.buffer["r"].shape != (N, T, P):
            self.buffer = self.new_buffer(N, T, P)
        ret, captured, length = self.run_episode(env, self.buffer)
        if self.obs_norm is not None:   # one merge per rollout: the statistics the next rollout is normalised under
            self.obs_norm.commit()
        mean_r, cap, mlen = torch.stack((ret.mean(), captured.float().mean(), length.mean())).tolist()
        return mean_r, self.buffer, N * T, dict(capture_rate=cap, episode_length=mlen)

    # ---- update ------------------------------------------------------------------------------------------------------------------
    def sequence_forward(self, feat_a, feat_c, batch, steps, return_ls_raw=False):
        """(batch, T, P, 16) features of whole episodes -> mu (batch, T, P, A) and values (batch, T, P), time-major views; with
        return_ls_raw also ls_raw (state mode: the LogStd head on the same GRU features, (batch, T, P, A); param mode: log_std)"""
        P = feat_a.shape[2]
        R = batch * steps * P
        emb_a, emb_c = self.actor.shared_net(feat_a.reshape(R, FEAT)), self.critic.shared_net(feat_c.reshape(R, FEAT))
        h0 = [torch.zeros(m.num_layers, batch * P, m.rnn_hidden_dim, dtype=emb_a.dtype, device=emb_a.device) for m in (self.actor, self.critic)]
        fa, fc = ops.gru_multi([emb_a, emb_c], h0, [self.actor.GRU, self.critic.GRU], agents=P, steps=steps, zero_state=True)
        fa, fc = fa.reshape(steps, batch, P, -1), fc.reshape(steps, batch, P, -1)
        mu = self.actor.Mean(fa).permute(1, 0, 2, 3)
        values = self.critic.Mean(fc).permute(1, 0, 2, 3)[..., 0]
        if not return_ls_raw:
            return mu, values
        ls_raw = self.actor.LogStd(fa).permute(1, 0, 2, 3) if self.gauss_std == "state" else self.actor.log_std
        return mu, values, ls_raw

    def train(self, buf, total_steps):
        """GAE + advantage normalisation over all rows (ops.gae_advnorm), then sequential mini-batches of whole episodes, the
        gradient clipped to 5.0 after each (as MAPPO.train).  With algo.minibatch_steps every mini-batch instead starts from a zeroed
        bucket and ends with the gradient SUM over ranks and one fused clip + Adam step (FusedAdam.step), and
        last_optimizer_steps / last_skipped_steps count them.  Returns (critic loss, actor loss) averaged over the mini-batches."""
        N, T, P = buf["r"].shape
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
            mu, values, ls_raw = self.sequence_forward(buf["feat_a"][n0:n1], buf["feat_c"][n0:n1], n1 - n0, T, return_ls_raw=True)
            args = (buf["a_n"][n0:n1], values, buf["a_logprob_n"][n0:n1], adv[n0:n1], buf["active"][n0:n1],
                    buf["v_n"][n0:n1, :-1] if self.use_value_clip else None, v_target[n0:n1], self.epsilon, self.entropy_coef,
                    self.use_value_clip)
            dk = {} if diag is None else {"diag": diag.sums}
            if self.policy_ex:
                la, lc = ops.ppo_loss_gauss_ex(mu, ls_raw, *args, log_std_min=self.log_std_min, log_std_max=self.log_std_max,
                                               squash=self.gauss_squash, **dk)
            else:
                la, lc = ops.ppo_loss_gauss(mu, ls_raw, *args, **dk)
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

    def policy_meta(self):
        """the "policy" entry of checkpoints and resume bundles: None in the default mode (param, clip), whose files carry none"""
        if not self.policy_ex:
            return None
        return dict(gauss_std=self.gauss_std, gauss_squash=self.gauss_squash, log_std_min=self.log_std_min, log_std_max=self.log_std_max)

    def check_policy_meta(self, meta, what):
        """ValueError naming the config key when a file's policy (its "policy" entry; None = the default mode) is not this agent's:
        gauss_std and gauss_squash, and with an option on (where the bounds act) log_std_min / log_std_max as well -- other bounds would
        neither reproduce the saved policy nor continue its run bit for bit"""
        meta = meta or {}
        for key, default in (("gauss_std", "param"), ("gauss_squash", "clip")):
            theirs, mine = meta.get(key, default), getattr(self, key)
            if theirs != mine:
                raise ValueError(f"{what} was written with algo.{key}: {theirs}, this agent has algo.{key}: {mine}")
        if self.policy_ex:   # (the default mode has no bounds; its files carry no entry)
            for key in ("log_std_min", "log_std_max"):
                theirs, mine = float(meta[key]), getattr(self, key)
                if theirs != mine:
                    raise ValueError(f"{what} was written with algo.{key}: {theirs}, this agent has algo.{key}: {mine}")

    def save_model(self, cwd, best=False):
        """cwd/e3d_state_dicts.pt (best: e3d_state_dicts_best.pt), the actor's and critic's state_dicts (and, with a non-default
        algo.gauss_std / gauss_squash, the "policy" entry of policy_meta; with algo.use_value_norm the "value_norm" entry: beta and the state;
        with algo.use_obs_norm the "obs_norm" entry: the clip and the state)"""
        os.makedirs(cwd, exist_ok=True)
        sd = {"actor": self.actor.state_dict(), "critic": self.critic.state_dict()}
        if self.policy_ex:
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
    """ParticleEnv of one rank: environment n of rank r is reset from seed + max(1000, num_envs) r + n (as Pursuit_Env).  A training
    environment owns the RewardScaling state when algo.use_reward_scaling is on and the shaping state when algo.reward_shaping is
    distance; evaluation environments (training=False) never do."""
    base = int(cfg.runtime.get("seed", 0)) + seed_offset + max(1000, num_envs) * rank
    env = ParticleEnv(num_envs=num_envs, seeds=[base + n for n in range(num_envs)], device=device, max_step=int(cfg.env.max_steps),
                      evader=str(cfg.runtime.get("e3d_evader", "slsqp")))
    env.initialize(int(cfg.env.num_defender))
    if training and bool(cfg.algo.get("use_reward_scaling", False)):
        env.enable_reward_scaling()
    mode, coef = reward_shaping_options(cfg)
    if training and mode == "distance":
        env.enable_reward_shaping(coef)
    env.set_guidance(*gd.guidance_options(cfg))
    return env


class E3dTrainer(ParticleRunState):
    """One rank of the data-parallel env_3d job: rollout, then epochs x (update, gradient all-reduce, Adam step); with
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
        self.agent = E3dMAPPO(cfg, self.num_envs, max(1, round(self.num_envs / 10)), self.device)
        self.agent.sample_rank = self.rank
        self.bucket = self.agent.grad_bucket or GradBucket(self.agent.ac_parameters)   # (algo.minibatch_steps: the agent's own)
        self.agent.grad_bucket = self.bucket
        if self.agent.value_norm is not None:
            self.agent.value_norm.allreduce = allreduce_sum_   # (S1, S2, c) over ranks; without a process group a no-op
        if self.agent.obs_norm is not None:
            self.agent.obs_norm.allreduce = allreduce_sum_     # the (2, 33) feature sums of a rollout over ranks, likewise
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
        """synchronous greedy episode (a = mu) on num_eval_envs environments of their own seeds and sampling stream; the std of the
        return over them goes to self.eval_return_std (a recorder column, not a log key)"""
        ev = self.make_eval_env()
        ret, captured, length = self.agent.run_episode(ev, None, greedy=True)
        sd = ret.std() if ret.numel() > 1 else ret.new_zeros(())
        r, c, l, self.eval_return_std = torch.stack((ret.mean(), captured.float().mean(), length.mean(), sd)).tolist()
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
            self.baseline_record = gd.baseline_record(*self.agent.run_episode(env, None, policy="guidance"))
        return dict(self.baseline_record)

    def make_eval_env(self):
        """the evaluation environments (created once): num_eval_envs of their own seeds, seed + 10^6 + n"""
        if self.eval_env is None:
            self.eval_env = make_env(self.cfg, self.num_eval_envs, 0, self.device, seed_offset=10 ** 6, training=False)
        return self.eval_env

    def last_breakdown_ms(self):
        ev = self.last_events
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def train_e3d(cfg, max_iterations=None, num_eval_envs=64, eval_every=1, save_resume=None, resume=None):
    """the env_3d training loop (main --config cfg5): until max_train_steps env-steps or max_iterations; rank 0 prints one JSON log
    line per iteration, records every evaluation (recorder.npy, learning curve, the _best weights: ParticleRunState.record_evaluation)
    and saves the final weights under algo.save_cwd.  resume / save_resume: directories of the per-rank resume bundles read before the
    first iteration / written after every one."""
    tr = E3dTrainer(cfg, num_eval_envs=num_eval_envs, eval_every=eval_every)
    if resume is not None:
        tr.load_resume(resume_path(resume, tr.rank))
    while tr.total_steps < cfg.algo.max_train_steps:
        t0 = time.time()
        steps, log = tr.iterate()
        if tr.rank == 0:
            log["seconds"] = round(time.time() - t0, 3)
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
