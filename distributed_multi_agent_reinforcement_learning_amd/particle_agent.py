"""The shared core of the env_3d and env_n2n learners (e3d_agent.py, n2n_agent.py; DESIGN.md sections 7a-7e): `ParticleMAPPO`, the
options, the optimiser set-up and the PPO update loop of `E3dMAPPO` / `N2nMAPPO`; `ParticleTrainer`, one rank of the data-parallel job;
`train_particle`, the training loop of `main`.  An agent module keeps its network, its rollout tick and its loss call; an algorithm
option of the update or the trainer is written here, once."""
import json
import time

import torch

from . import guidance as gd
from . import imitation as im
from . import kickstart as ks
from . import ops
from . import value_norm as vnorm
from .minibatch_steps import MAX_GRAD_NORM, minibatch_steps_options
from .readback import BcSums, KickSums, read_back
from .reward_shaping import reward_shaping_options
from .team_reward import team_reward_options
from .trainer import (BUCKET_ALIGN, FusedAdam, GradBucket, ParamBucket, ParticleRunState, allreduce_sum_, broadcast_weights_,
                      rank_setup, resume_path, save_resume_atomic)
from .update_diag import LOG_KEYS, UpdateDiag, first_epoch_over, update_diag_options


def episode_triple(result):
    """what run_episode / guidance_episode returned -> per-environment (return, captured, length): env_3d's triple as it is, env_n2n's
    accumulators by their keys (`captured` is a uint8 0 / 1 flag there)"""
    if isinstance(result, dict):
        return result["ret"], result["captured"] != 0, result["length"]
    return result


def finish_env(env, cfg, training):
    """the options of an initialised ParticleEnv: a training environment owns the RewardScaling state when algo.use_reward_scaling is on
    and the shaping state when algo.reward_shaping is distance, evaluation environments (training=False) never do; both take the
    scripted pursuers' settings"""
    if training and bool(cfg.algo.get("use_reward_scaling", False)):
        env.enable_reward_scaling()
    mode, coef = reward_shaping_options(cfg)
    if training and mode == "distance":
        env.enable_reward_shaping(coef)
    env.set_guidance(*gd.guidance_options(cfg))
    return env


class ParticleMAPPO(im.OptimizerSchedule):
    """rollout bookkeeping (explore_env) and PPO update (train) of a policy on a particle environment.  A subclass names its
    environment (ENV) and provides _options (its own keys, before the device check), _build (actor, critic, ac_parameters), _rollout
    (the storage of _state), _buffer_dims, new_buffer, run_episode, _bootstrap_value, _minibatch_loss, for algo.bc_iterations
    _imitation_loss, BC_METRIC and bc_metric, and for algo.bc_coef _kick_loss."""

    ENV = None        # "env_3d (runtime.env: e3d)": how the messages name the environment
    obs_norm = None   # algo.use_obs_norm (env_3d only): the agent's ObsNorm

    def __init__(self, cfg, batch_size, mini_batch_size, device="cuda"):
        a = cfg.algo
        if bool(a.get("use_reward_norm", False)):
            raise ValueError(f"algo.use_reward_norm: true is not supported on {self.ENV}; set it to false")
        self.use_reward_scaling = bool(a.get("use_reward_scaling", False))   # the reference's RewardScaling in policy_record
        self.use_value_norm, self.value_norm_beta = vnorm.value_norm_options(cfg)   # ValueNorm on the value targets
        self.reward_shaping, self.shaping_coef = reward_shaping_options(cfg)   # distance shaping in policy_record
        self.team_reward = team_reward_options(cfg)   # team reward sharing in policy_record, 0: off
        self.update_diagnostics, self.target_kl = update_diag_options(cfg)   # what the update did, from the loss launches
        self.minibatch_steps = minibatch_steps_options(cfg)   # one clip + Adam step per mini-batch, fused
        self.guidance = gd.guidance_options(cfg)   # the scripted pursuers of run_episode(policy="guidance")
        self.imitation = im.imitation_options(cfg)   # algo.bc_iterations: the imitation warm start in front of PPO
        self.kick = ks.kickstart_options(cfg)   # algo.bc_coef: the imitation term stays in the PPO loss, decaying
        self.teacher = self.imitation.on or self.kick.on   # the rollout can be labelled: the buffer has the a_star field
        self._options(cfg)
        self.batch_size, self.mini_batch_size = int(batch_size), int(mini_batch_size)
        self.max_train_steps, self.lr, self.gamma, self.lamda = a.max_train_steps, a.lr, a.gamma, a.lamda
        self.epsilon, self.entropy_coef = a.epsilon, a.entropy_coef
        self.use_grad_clip, self.use_lr_decay = a.use_grad_clip, a.use_lr_decay
        self.use_adv_norm, self.use_value_clip = a.use_adv_norm, a.use_value_clip
        self.num_layers, self.embedding_dim, self.rnn_hidden_dim = int(a.num_layers), int(a.embedding_dim), int(a.rnn_hidden_dim)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (HIP kernels, no CPU fallback)")
        self._build(cfg)
        self.param_bucket = None
        if self.minibatch_steps:   # the parameters and their gradients as two flat tensors of one layout, stepped by two launches
            self.param_bucket = ParamBucket(self.ac_parameters)
            self.ac_optimizer = FusedAdam(self.param_bucket, lr=self.lr, eps=1e-5)
        else:
            self.ac_optimizer = torch.optim.Adam(self.ac_parameters, lr=self.lr, eps=1e-5)
        self.value_norm = vnorm.ValueNorm(self.value_norm_beta, self.device) if self.use_value_norm else None
        self.diag = UpdateDiag(self.device) if self.update_diagnostics else None
        self.bc = BcSums(self.device) if self.imitation.on else None
        self.last_bc = None   # algo.bc_iterations: (the extra sum, the live rows) of the last train(imitation=True) call, over ranks
        self.kick_sums = KickSums(self.device) if self.kick.on else None
        self.last_kick = None   # algo.bc_coef: (the metric's sum, the live rows, the sum of the unweighted term) of the last train(kick=) call
        self.last_update_diag = None   # algo.update_diagnostics: the dict of the last train() call
        rt = cfg.get("runtime", {})
        self.sample_seed = int(rt.get("seed", 0))
        self.sample_rank = int(rt.get("sample_rank", 0))   # Philox counter of rank r starts at r << 40 (as MAPPO)
        self.total_step = 0
        self.grad_bucket = GradBucket(self.ac_parameters, BUCKET_ALIGN) if self.minibatch_steps else None   # (off: the trainer's)
        self.last_optimizer_steps = self.last_skipped_steps = 0   # algo.minibatch_steps: of the last train() call
        self.buffer = self._buffer_for = None
        self._states = {}

    def policy_meta(self):
        """the "policy" entry of checkpoints and resume bundles; None: the files carry none"""
        return None

    def check_policy_meta(self, meta, what):
        """ValueError when a file's "policy" entry is not this agent's (an agent without policy options accepts every file)"""

    # ---- rollout -------------------------------------------------------------------------------------------------------------
    def _state(self, env):
        st = self._states.get(id(env))
        if st is None or st.N != env.num_envs:
            st = self._states[id(env)] = self._rollout(env)
        return st

    def _shaping_gammas(self, env, buf):
        """-> (scale_gamma, shaping_gamma) of policy_record for this episode: evaluation (no buffer) never scales and never shapes;
        with shaping the potential of the reset state is taken here"""
        scale_gamma = self.gamma if (self.use_reward_scaling and buf is not None) else None
        shaping_gamma = self.gamma if (self.reward_shaping == "distance" and buf is not None) else None
        if shaping_gamma is not None:
            env.shaping_begin()
        return scale_gamma, shaping_gamma

    def _team_coef(self, buf):
        """-> team_coef of policy_record for this episode: algo.team_reward on a training rollout, None (the unshared entry points)
        when the option is off and in evaluation (no buffer)"""
        return self.team_reward if (self.team_reward != 0.0 and buf is not None) else None

    def _record_bootstrap(self, env, st, buf, acc):
        """v_n[:, T] of a finished rollout: the critic's value of the state after the last step (its inputs are in `st`), zero where
        the pursuer or the episode ended for another reason than the time limit"""
        vmask = env.active_t.float() * (acc["ended"] == 0).float()[:, None]
        buf["v_n"][:, -1].copy_(self._bootstrap_value(st) * vmask)
        if self.value_norm is not None:   # the denormalisation of v_n[:, T] needs the mask itself: 0 std + mean is not 0
            buf["v_mask"].copy_(vmask)

    def explore_env(self, env, follow=None):
        """one episode per environment into the buffer (a fresh one when the sizes changed) -> (mean return, buffer, env-steps, stats);
        follow: explore_expert's mask"""
        dims = self._buffer_dims(env)   # (N, T, P, ...): the arguments of new_buffer
        if self.buffer is None or self._buffer_for != dims:
            self.buffer, self._buffer_for = self.new_buffer(*dims), dims
        kw = {} if follow is None else {"follow": follow}
        ret, captured, length = episode_triple(self.run_episode(env, self.buffer, **kw))
        if self.obs_norm is not None:   # one merge per rollout: the statistics the next rollout is normalised under
            self.obs_norm.commit()
        mean_r, cap, mlen = torch.stack((ret.mean(), captured.float().mean(), length.mean())).tolist()
        return mean_r, self.buffer, dims[0] * dims[1], dict(capture_rate=cap, episode_length=mlen)

    def explore_expert(self, env, beta):
        """explore_env with the teacher in the loop (algo.bc_iterations; algo.bc_coef calls it with beta 0: labels only): every tick also takes env.guidance_actions() and one
        ops.bc_select launch before the environment steps -- the scripted pursuers' actions become the labels buffer["a_star"][:, t] of
        every environment and the executed actions of environments 0 .. round(beta N) - 1; everything else is run_episode's"""
        if not self.teacher:
            raise ValueError(f"explore_expert needs {im.KEY} > 0 (the buffer has no a_star field otherwise)")
        return self.explore_env(env, im.follow_mask(beta, env.num_envs, self.device))

    def _expert_tick(self, env, action, buf, t, follow):
        """the hook of explore_expert inside run_episode's loop, after the policy step and before env.step"""
        ops.bc_select(env.guidance_actions(), follow, action, buf["a_star"][:, t], getattr(self, "gauss_squash", "clip"), self.imitation.target_bound)

    # ---- update ------------------------------------------------------------------------------------------------------------------
    def _loss_tail(self, buf, n0, n1, values, adv, v_target):
        """the arguments every PPO loss launch takes after the policy's own outputs, for episodes [n0, n1)"""
        return (buf["a_n"][n0:n1], values, buf["a_logprob_n"][n0:n1], adv[n0:n1], buf["active"][n0:n1],
                buf["v_n"][n0:n1, :-1] if self.use_value_clip else None, v_target[n0:n1], self.epsilon, self.entropy_coef, self.use_value_clip)

    def _imitation_tail(self, buf, n0, n1, values, v_target):
        """the arguments both imitation loss launches take after the policy's own outputs and the labels, for episodes [n0, n1)"""
        return (values, buf["active"][n0:n1], buf["v_n"][n0:n1, :-1] if self.use_value_clip else None, v_target[n0:n1], self.epsilon,
                self.use_value_clip)

    def train(self, buf, total_steps, imitation=False, kick=None):
        """GAE + advantage normalisation over all rows (ops.gae_advnorm), then sequential mini-batches of whole episodes (forward and
        loss: the subclass's _minibatch_loss), the gradient clipped to MAX_GRAD_NORM after each (as MAPPO.train).  With
        algo.minibatch_steps every mini-batch instead starts from a zeroed bucket and ends with the gradient SUM over ranks and one
        fused clip + Adam step (FusedAdam.step), and last_optimizer_steps / last_skipped_steps count them.
        imitation (algo.bc_iterations): the mini-batch loss is the subclass's _imitation_loss on buf["a_star"]; the update diagnostics,
        the KL target and the learning-rate decay are skipped, everything else is unchanged; the two sums of the imitation metric go
        over ranks and arrive in the call's one host read (last_bc).
        kick (algo.bc_coef): lambda > 0 -- a PPO update in every respect (diagnostics, KL target, learning-rate decay) whose mini-batch
        loss is the subclass's _kick_loss, the PPO loss plus lambda times the imitation loss on buf["a_star"] from one launch; its three
        sums go over ranks and arrive in the same host read (last_kick).
        Returns (critic loss, actor loss) averaged over the mini-batches."""
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
        diag = None if imitation else self.diag   # algo.update_diagnostics: every loss call adds its eight sums (None: the plain calls)
        kick = kick if (kick and not imitation) else None
        if imitation:
            self.bc.sums.zero_()
        if kick is not None:
            self.kick_sums.sums.zero_()
        if diag is not None:
            diag.begin()
        dk = {} if diag is None else {"diag": diag.sums}
        for n0 in range(0, N, self.mini_batch_size):
            n1 = min(n0 + self.mini_batch_size, N)
            if opt is not None and n0:
                self.grad_bucket.zero()
            if imitation:
                la, lc = self._imitation_loss(buf, n0, n1, v_target, self.bc.sums)
            elif kick is not None:
                la, lc = self._kick_loss(buf, n0, n1, adv, v_target, kick, self.kick_sums.sums, dk)
            else:
                la, lc = self._minibatch_loss(buf, n0, n1, adv, v_target, dk)
            (la + lc).backward()
            if opt is not None:   # the clip acts on the gradient summed over ranks: the same coefficient and weights everywhere
                allreduce_sum_(self.grad_bucket.flat)
                opt.step(self.grad_bucket.flat, MAX_GRAD_NORM if self.use_grad_clip else 0.0)
                if diag is not None and self.use_grad_clip:
                    diag.note_grad_norm(opt.grad_norm)
            elif self.use_grad_clip:
                norm = torch.nn.utils.clip_grad_norm_(self.ac_parameters, MAX_GRAD_NORM)
                if diag is not None:
                    diag.note_grad_norm(norm)
            obj_c = obj_c + lc.detach().double()
            obj_a = obj_a + la.detach().double()
            k += 1
        if self.use_lr_decay and not imitation:
            self.lr_decay(total_steps)
        # one read for the two losses, the count of skipped steps and the sums of whichever features ran (each all-reduced over ranks)
        (obj_c, obj_a, *skipped), bc, kicked, sums, norm = read_back(
            (obj_c, obj_a) + (() if opt is None else (opt.skipped,)), self.bc if imitation else None,
            self.kick_sums if kick is not None else None, diag, None if diag is None else (diag.grad_norm,))
        if imitation:
            self.last_bc = tuple(bc)
        if kick is not None:
            self.last_kick = tuple(kicked)
        if diag is not None:
            self.last_update_diag = diag.result(sums, norm[0])
        if opt is not None:
            self.last_optimizer_steps, self.last_skipped_steps = k, int(skipped[0] - opt.skipped_seen)
            opt.skipped_seen = skipped[0]
        return obj_c / k, obj_a / k


class ParticleTrainer(ParticleRunState):
    """One rank of the data-parallel env_3d / env_n2n job: rollout, then epochs x (update, gradient all-reduce, Adam step); with
    algo.minibatch_steps the update itself reduces and steps after every mini-batch and the epoch loop does neither.  A subclass names
    its agent class and its make_env."""

    agent_cls = make_env = None
    log_breakdown = False   # train_particle adds rollout_ms / update_ms to every log line

    def __init__(self, cfg, num_envs=None, num_eval_envs=64, eval_every=0, tuned_gemms=True):
        rank_setup(self, cfg, num_envs, tuned_gemms)
        self.env = self.make_env(cfg, self.num_envs, self.rank, self.device)
        torch.manual_seed(int(cfg.runtime.get("seed", 0)))
        self.agent = self.agent_cls(cfg, self.num_envs, max(1, round(self.num_envs / 10)), self.device)
        self.agent.sample_rank = self.rank
        self.bucket = self.agent.grad_bucket or GradBucket(self.agent.ac_parameters)   # (algo.minibatch_steps: the agent's own)
        self.agent.grad_bucket = self.bucket
        for part in (self.agent.value_norm, self.agent.obs_norm, self.agent.diag, self.agent.bc, self.agent.kick_sums):
            if part is not None:   # (S1, S2, c) / the (2, 33) feature sums of a rollout / the eight diagnostic sums / the two imitation
                part.allreduce = allreduce_sum_   # sums / the three of algo.bc_coef over ranks; without a process group a no-op
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
        # algo.bc_iterations: the leading iterations imitate the scripted pursuers
        imitating, beta = im.phase_step(agent, agent.imitation, self.iteration, self.total_steps)
        lam = 0.0 if imitating else agent.kick.coef_at(self.iteration - agent.imitation.iterations)   # algo.bc_coef: lambda_j of this PPO iteration
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        if imitating:
            mean_r, buf, steps, stats = agent.explore_expert(self.env, beta)
        elif lam > 0.0:   # every tick labelled, no environment follows the teacher: the data stays on-policy
            mean_r, buf, steps, stats = agent.explore_expert(self.env, 0.0)
        else:
            mean_r, buf, steps, stats = agent.explore_env(self.env)
        ev[1].record()
        self.total_steps += steps * self.world
        self.last_epoch_diags, epochs_run = [], 0
        per_minibatch, opt_steps, skipped = agent.minibatch_steps, 0, 0
        for _ in range(int(cfg.algo.epochs)):
            with torch.enable_grad():
                obj_c, obj_a = agent.train(buf, self.total_steps, **({"imitation": True} if imitating else {"kick": lam} if lam > 0.0 else {}))
            over = False
            if agent.diag is not None and not imitating:
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
        if imitating:   # the metric of the last train() call, like the two losses
            log.update(phase="imitation", bc_beta=beta, bc_loss=obj_a, **{agent.BC_METRIC: agent.bc_metric(*agent.last_bc)})
        elif agent.diag is not None:   # of the last train() call, like the two losses
            log.update({k: agent.last_update_diag[k] for k in LOG_KEYS}, epochs_run=epochs_run)
        if lam > 0.0:   # of the last train() call: lambda_j, the unweighted imitation term and its metric
            s, c, b = agent.last_kick
            log.update(bc_coef=lam, bc_aux_loss=b / c if c else float("nan"), **{agent.BC_METRIC: agent.bc_metric(s, c)})
        if per_minibatch:
            log.update(optimizer_steps=opt_steps, skipped_steps=skipped)
        if self.eval_every and self.iteration % self.eval_every == 0 and self.rank == 0:
            log.update(self.evaluate())
        return steps * self.world, log

    def evaluate(self):
        """synchronous greedy episode (a = mu / argmax) on num_eval_envs environments of their own seeds and sampling stream; the std of
        the return over them goes to self.eval_return_std (a recorder column, not a log key)"""
        ret, captured, length = episode_triple(self.agent.run_episode(self.make_eval_env(), None, greedy=True))
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
            env = self.make_env(self.cfg, self.num_eval_envs, 0, self.device, seed_offset=10 ** 6, training=False)
            self.baseline_record = gd.baseline_record(*episode_triple(self.agent.run_episode(env, None, policy="guidance")))
        return dict(self.baseline_record)

    def make_eval_env(self):
        """the evaluation environments (created once): num_eval_envs of their own seeds, seed + 10^6 + n"""
        if self.eval_env is None:
            self.eval_env = self.make_env(self.cfg, self.num_eval_envs, 0, self.device, seed_offset=10 ** 6, training=False)
        return self.eval_env

    def last_breakdown_ms(self):
        torch.cuda.synchronize()
        ev = self.last_events
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def train_particle(trainer_cls, cfg, max_iterations=None, num_eval_envs=64, eval_every=1, save_resume=None, resume=None):
    """the env_3d / env_n2n training loop (main --config cfg5 / cfg4_n2n): until max_train_steps env-steps or max_iterations; rank 0
    prints one JSON log line per iteration, records every evaluation (recorder.npy, learning curve, the _best weights:
    ParticleRunState.record_evaluation) and saves the final weights under algo.save_cwd.  resume / save_resume: directories of the
    per-rank resume bundles read before the first iteration / written after every one."""
    tr = trainer_cls(cfg, num_eval_envs=num_eval_envs, eval_every=eval_every)
    if resume is not None:
        tr.load_resume(resume_path(resume, tr.rank))
    while tr.total_steps < cfg.algo.max_train_steps:
        t0 = time.time()
        steps, log = tr.iterate()
        if tr.rank == 0:
            if tr.log_breakdown:
                rollout_ms, update_ms = tr.last_breakdown_ms()
                log.update(rollout_ms=round(rollout_ms, 2), update_ms=round(update_ms, 2))
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
