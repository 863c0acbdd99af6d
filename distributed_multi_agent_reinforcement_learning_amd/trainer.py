"""Data-parallel MAPPO training loop: one process per GPU, environment shards per rank, one RCCL all-reduce per epoch.

Same protocol as the reference's driver (main.py:41-172): rollouts -> per-learner GAE with its own advantage
normalisation -> gradient SUM over learners -> the same Adam step everywhere -> evaluation / checkpoints.  What was a
parameter-server sum of numpy lists through the Ray object store (main.py:105-129) is one `all_reduce(SUM)` of a
single flat fp32 bucket (~0.6 M elements) over xGMI; weights are never re-broadcast because every rank applies the
identical update.  Rollout data never leaves the GPU that produced it.
"""
import json
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .evaluator import EvaluatorProc, draw_learning_curve
from .mappo import MAPPO
from .imitation import check_entry as check_imitation_entry, phase_step
from .kickstart import check_entry as check_kickstart_entry
from .minibatch_steps import check_entry as check_minibatch_steps_entry
from .pursuit_env import Pursuit_Env
from .pursuit_imitation import check_coef_entry as check_pursuit_kickstart_entry, check_entry as check_pursuit_imitation_entry
from .obs_norm import check_entry as check_obs_norm_entry
from .value_norm import check_entry as check_value_norm_entry


TUNED_GEMM_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop_gfx950.csv")


def enable_tuned_gemms(path=TUNED_GEMM_FILE):
    """Library GEMM solution selection (PyTorch TunableOp over rocBLAS / hipBLASLt) from the committed tuning file
    produced by tools/tune_gemms.py; nothing is tuned at run time.  Returns True when the file was loaded."""
    if os.environ.get("DMARL_TUNED_GEMMS", "1") == "0" or not os.path.exists(path) or not torch.cuda.is_available():
        return False
    try:
        import torch.cuda.tunable as tunable
        tunable.enable(True)
        tunable.tuning_enable(False)
        ok = bool(tunable.read_file(path))
        # TunableOp rewrites its results file at interpreter exit: point it away from the committed table (one per process)
        import tempfile
        tunable.set_filename(os.path.join(tempfile.gettempdir(), f"dmarl_tunableop_{os.getpid()}.csv"), insert_device_ordinal=False)
        return ok
    except Exception:
        return False


def dist_env():
    return int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))


def init_distributed(backend=None):
    """Joins the process group of a multi-rank job (one process per GPU; `nccl` = RCCL over xGMI on a GPU box, `gloo` on CPU).  A
    single-rank job needs no group; an explicitly requested backend (argument or DMARL_DIST_BACKEND) is honoured all the same, so
    the RCCL path -- communicator, broadcast, in-place all-reduce of the device bucket -- can be exercised on one GPU."""
    rank, local_rank, world = dist_env()
    forced = backend or os.environ.get("DMARL_DIST_BACKEND")
    if (world > 1 or forced) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend is None:
            backend = os.environ.get("DMARL_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local_rank, world


def rank_setup(trainer, cfg, num_envs, tuned_gemms):
    """what both trainers start from: the rank in the job, the tuned GEMM table, the configuration, this rank's device and its number
    of environments"""
    trainer.rank, trainer.local_rank, trainer.world = init_distributed()
    trainer.tuned_gemms = enable_tuned_gemms() if tuned_gemms else False
    trainer.cfg = cfg
    trainer.device = torch.device("cuda", trainer.local_rank % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(trainer.device)
    trainer.num_envs = int(num_envs if num_envs is not None else cfg.runtime.num_envs)


def allreduce_sum_(flat):
    """gradient SUM over learners (main.py:121-126), in place; without a process group (single rank) a no-op"""
    if dist.is_initialized():
        if flat.is_cuda and dist.get_backend() == "gloo":  # rehearsal of the N > 1 path on one GPU: stage through the host
            host = flat.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            flat.copy_(host)
        else:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    return flat


def bucket_offsets(params, align=1):
    """-> (the element offset of every parameter in a flat bucket, the bucket's length): the parameters in order, each starting at a
    multiple of `align` elements (the gaps stay zero); align = 1 is the dense layout"""
    offsets, o = [], 0
    for p in params:
        offsets.append(o)
        o += -(-p.numel() // align) * align
    return offsets, o


class GradBucket:
    """The gradients of `params` as views of ONE persistent flat fp32 tensor (ac_parameters order): autograd accumulates straight
    into the bucket, the collective reduces the bucket in place and the optimiser reads the same memory -- no torch.cat before the
    all-reduce and no per-parameter clone after it.  Parameters that receive no gradient (an unused GRU under algo.use_rnn: false)
    contribute zeros, which is what the SUM over learners of `None` entries amounts to (main.py:121-126)."""

    def __init__(self, params, align=1):
        self.params = list(params)
        self.offsets, total = bucket_offsets(self.params, align)   # align > 1: ParamBucket's layout (algo.minibatch_steps)
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.params[0].device)
        self.attach()

    def attach(self):
        for p, o in zip(self.params, self.offsets):
            p.grad = self.flat[o:o + p.numel()].view_as(p)

    def zero(self):
        if any(p.grad is None or p.grad.data_ptr() < self.flat.data_ptr() or p.grad.data_ptr() >= self.flat.data_ptr() + self.flat.numel() * 4
               for p in self.params):
            self.attach()   # someone replaced a gradient tensor (e.g. a zero_grad(set_to_none=True)): re-attach the views
        self.flat.zero_()


BUCKET_ALIGN = 4   # elements: every parameter of a ParamBucket starts on 16 bytes, which the kernels that read weights require


class ParamBucket:
    """algo.minibatch_steps: the parameters themselves as views of ONE persistent flat fp32 tensor (ac_parameters order, every
    parameter on a 16-byte boundary; the gaps are zero and stay zero), so that the fused optimiser steps all of them in one launch.
    The values are copied in and `p.data` is re-pointed; the matching gradient bucket is GradBucket(params, BUCKET_ALIGN)."""

    def __init__(self, params):
        self.params = list(params)
        self.offsets, total = bucket_offsets(self.params, BUCKET_ALIGN)
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.params[0].device)
        self.attach()

    def view(self, k):
        p, o = self.params[k], self.offsets[k]
        return self.flat[o:o + p.numel()].view(p.shape)

    def attached(self):
        return all(p.data_ptr() == self.flat.data_ptr() + 4 * o and p.is_contiguous() for p, o in zip(self.params, self.offsets))

    @torch.no_grad()
    def attach(self):
        """copies the values of every parameter that lives elsewhere into its slot and points the parameter at the slot"""
        for k, (p, o) in enumerate(zip(self.params, self.offsets)):
            if p.data_ptr() != self.flat.data_ptr() + 4 * o or not p.is_contiguous():
                v = self.view(k)
                v.copy_(p.data)
                p.data = v

    def ensure(self):
        if not self.attached():
            self.attach()   # someone re-pointed a parameter (a .to(), a p.data = ...): its values come back in, the views are restored


class FusedAdam:
    """algo.minibatch_steps: torch.optim.Adam(eps=1e-5) with clip_grad_norm_ in front, as two launches on the flat tensors
    (ops.fused_adam; csrc/fused_adam.hpp).  Owns the moments m, v, the device state (step, b1t, b2t, norm, coef, skipped) and the
    workspace; `param_groups` carries the learning rate the way torch's optimisers do, so lr_decay and the resume bundle read and
    write it unchanged.  The kernel writes the weights behind autograd's back: nothing in the package caches a weight by version
    counter (spectral norm recomputes from weight_orig every forward)."""

    KIND = "fused_adam"

    def __init__(self, bucket, lr, betas=(0.9, 0.999), eps=1e-5):
        self.bucket = bucket
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.param_groups = [{"lr": float(lr)}]
        dev = bucket.flat.device
        self.m, self.v = torch.zeros_like(bucket.flat), torch.zeros_like(bucket.flat)
        self.state = ops.fused_adam_state(dev)
        self.workspace = ops.fused_adam_workspace(dev)
        self.skipped_seen = 0.0   # state[5] as last read on the host (the agents' per-call count of skipped steps)

    @property
    def grad_norm(self):
        """the gradient norm of the last step before clipping, a device scalar"""
        return self.state[3]

    @property
    def skipped(self):
        return self.state[5]

    def step(self, grad_flat, max_norm=0.0):
        self.bucket.ensure()
        ops.fused_adam(self.bucket.flat, grad_flat, self.m, self.v, self.state, self.workspace, self.param_groups[0]["lr"], self.betas[0],
                       self.betas[1], self.eps, max_norm)

    def reset_moments(self):
        """m, v and the step count (with the two beta powers) as before the first step; the norm, the coefficient and the count of
        skipped steps stay"""
        self.m.zero_()
        self.v.zero_()
        self.state[0].zero_()
        self.state[1:3].fill_(1.0)

    def state_dict(self):
        return dict(kind=self.KIND, state=self.state.cpu(), m=self.m.cpu(), v=self.v.cpu())

    def load_state_dict(self, sd):
        if not isinstance(sd, dict) or sd.get("kind") != self.KIND or sd["m"].shape != self.m.shape:
            raise ValueError("optimizer state is not a fused_adam state of this parameter layout (algo.minibatch_steps)")
        self.state.copy_(sd["state"])
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.skipped_seen = float(sd["state"][5])


def broadcast_weights_(modules, src=0):
    """initial weight sync from learner 0 (main.py:73-75)"""
    if dist.is_initialized():
        seen = set()
        for m in modules:
            for t in list(m.parameters()) + list(m.buffers()):
                if id(t) not in seen:
                    seen.add(id(t))
                    if t.is_cuda and dist.get_backend() == "gloo":
                        host = t.data.cpu()
                        dist.broadcast(host, src=src)
                        t.data.copy_(host)
                    else:
                        dist.broadcast(t.data, src=src)


def save_checkpoint(actor, critic, cwd, suffix=""):
    """main.py:146-172: eight whole-module files; plus state_dicts (loadable without this package)."""
    os.makedirs(cwd, exist_ok=True)
    torch.save(actor, f"{cwd}/actor{suffix}.pth")
    torch.save(critic, f"{cwd}/critic{suffix}.pth")
    torch.save(actor.shared_net, f"{cwd}/actor_gnn{suffix}.pth")
    torch.save(critic.shared_net, f"{cwd}/critic_gnn{suffix}.pth")
    torch.save(actor.GRU, f"{cwd}/actor_gru{suffix}.pth")
    torch.save(critic.GRU, f"{cwd}/critic_gru{suffix}.pth")
    torch.save(actor.Mean, f"{cwd}/actor_mean{suffix}.pth")
    torch.save(critic.Mean, f"{cwd}/critic_mean{suffix}.pth")
    torch.save({"actor": actor.state_dict(), "critic": critic.state_dict()}, f"{cwd}/state_dicts{suffix}.pt")


def resume_path(directory, rank):
    """the resume bundle of one rank under `main --save-resume DIR` / `--resume DIR`"""
    return os.path.join(directory, f"resume_rank{rank}.pt")


def save_resume_atomic(trainer, directory):
    """trainer.save_resume into DIR/resume_rank{r}.pt through a temporary file and os.replace: a job killed while writing leaves
    the previous bundle, never a torn one"""
    os.makedirs(directory, exist_ok=True)
    path = resume_path(directory, trainer.rank)
    tmp = f"{path}.tmp{os.getpid()}"
    trainer.save_resume(tmp)
    os.replace(tmp, path)


class ParticleRunState:
    """Run protocol of the env_3d / env_n2n trainers (particle_agent.ParticleTrainer): resume bundle, evaluation record and best
    checkpoint.  The trainer provides env, eval_env and make_eval_env(), agent (a ParticleMAPPO: rollout state `agent._state(env)` with
    the sampling counter; save_model / load_model), total_steps, iteration, num_envs, world, rank, device, eval_return_std, recorder and
    best_eval_return.  Every environment episode starts from a reset and every rollout from zero GRU states and history, so the
    reset generators, the sampling counters, the weights and Adam are all the state a run carries from one iteration to the next --
    and, with algo.use_reward_scaling, the training environment's reward_scale (the bundle's "reward_scaling" entry), with
    algo.use_value_norm the agent's value-normaliser state (the "value_norm" entry), with algo.use_obs_norm (env_3d) the agent's
    feature-normaliser state (the "obs_norm" entry; its slots are empty between iterations and are not saved).  With
    algo.minibatch_steps the bundle says so ("minibatch_steps": True) and its "optimizer" is FusedAdam's state.  With algo.bc_iterations
    > 0 the bundle records it ("bc_iterations"): the phase of the next iteration follows from it and the saved iteration count; with
    algo.bc_coef > 0 its "bc_coef" entry is (bc_coef, bc_coef_decay, bc_coef_iterations), from which lambda of every iteration follows."""

    def save_resume(self, path):
        agent, ev = self.agent, self.eval_env
        bundle = dict(actor=agent.actor.state_dict(), critic=agent.critic.state_dict(), optimizer=agent.ac_optimizer.state_dict(),
                      total_steps=self.total_steps, iteration=self.iteration, lr=agent.ac_optimizer.param_groups[0]["lr"],
                      resetter=self.env.get_resetter_state(), n_episode=self.env.n_episode, sample_counter=agent._state(self.env).counter.cpu(),
                      eval_resetter=None if ev is None else ev.get_resetter_state(), eval_n_episode=None if ev is None else ev.n_episode,
                      eval_sample_counter=None if ev is None else agent._state(ev).counter.cpu(),
                      recorder=list(self.recorder), best_eval_return=self.best_eval_return,
                      num_envs=self.num_envs, world=self.world, rank=self.rank)
        meta = agent.policy_meta()
        if meta is not None:   # env_3d with a non-default algo.gauss_std / gauss_squash (E3dMAPPO.policy_meta); default bundles carry none
            bundle["policy"] = meta
        if agent.use_reward_scaling:   # algo.use_reward_scaling: n, mean, S (and R) of every environment; off: no entry
            bundle["reward_scaling"] = self.env.reward_scale.cpu()
        if agent.value_norm is not None:   # algo.use_value_norm: beta and the state (m, q, d); off: no entry
            bundle["value_norm"] = agent.value_norm.entry()
        if agent.obs_norm is not None:     # algo.use_obs_norm: the clip and the state (2, 33); off: no entry
            bundle["obs_norm"] = agent.obs_norm.entry()
        if agent.minibatch_steps:         # algo.minibatch_steps: "optimizer" is FusedAdam's state; off: no entry
            bundle["minibatch_steps"] = True
        if agent.imitation.on:            # algo.bc_iterations: the phase of an iteration follows from it and `iteration`; off: no entry
            bundle["bc_iterations"] = agent.imitation.iterations
        if agent.kick.on:                 # algo.bc_coef: lambda of an iteration follows from the three values; off: no entry
            bundle["bc_coef"] = agent.kick.entry()
        torch.save(bundle, path)

    def load_resume(self, path):
        """restores save_resume(path) into this trainer, fresh or not (the rollout states are created here when missing)"""
        b = torch.load(path, map_location=self.device, weights_only=False)  # our own file (numpy blobs inside)
        if b["num_envs"] != self.num_envs or b["world"] != self.world or b["rank"] != self.rank:
            raise ValueError("resume bundle was written for another num_envs / world size / rank")
        agent = self.agent
        agent.check_policy_meta(b.get("policy"), "resume bundle " + str(path))
        theirs, mine = "reward_scaling" in b, agent.use_reward_scaling
        if theirs != mine:
            raise ValueError(f"resume bundle {path} was written with algo.use_reward_scaling: {str(theirs).lower()}, "
                             f"this agent has algo.use_reward_scaling: {str(mine).lower()}")
        check_value_norm_entry(agent, b.get("value_norm"), f"resume bundle {path}")
        check_obs_norm_entry(agent, b.get("obs_norm"), f"resume bundle {path}")
        check_minibatch_steps_entry(agent, b.get("minibatch_steps"), f"resume bundle {path}")
        check_imitation_entry(agent, b.get("bc_iterations"), f"resume bundle {path}")
        check_kickstart_entry(agent, b.get("bc_coef"), f"resume bundle {path}")
        agent.actor.load_state_dict(b["actor"])
        agent.critic.load_state_dict(b["critic"])
        agent.ac_optimizer.load_state_dict(b["optimizer"])
        if agent.value_norm is not None:
            agent.value_norm.load_entry(b["value_norm"])
        if agent.obs_norm is not None:
            agent.obs_norm.load_entry(b["obs_norm"])   # (zeroes the slots)
        self.total_steps, self.iteration = b["total_steps"], b["iteration"]
        if agent.use_lr_decay:
            agent.lr_decay(self.total_steps)
        else:
            for g in agent.ac_optimizer.param_groups:
                g["lr"] = b["lr"]
        self.env.set_resetter_state(b["resetter"])
        self.env.n_episode = b["n_episode"]
        agent._state(self.env).counter.copy_(b["sample_counter"])
        if mine:
            self.env.reward_scale.copy_(b["reward_scaling"])
        if b["eval_resetter"] is not None:
            ev = self.make_eval_env()
            ev.set_resetter_state(b["eval_resetter"])
            ev.n_episode = b["eval_n_episode"]
            agent._state(ev).counter.copy_(b["eval_sample_counter"])
        self.recorder, self.best_eval_return = list(b["recorder"]), b["best_eval_return"]

    def record_evaluation(self, log, cwd):
        """after an iteration that evaluated (rank 0): one recorder row (total_steps, eval_return, eval_return_std, mean_return,
        critic_loss, actor_loss), saved as cwd/recorder.npy with its learning curve, and the weights under the _best suffix when the
        greedy return did not get worse (main.py:139-156, evaluator.EvaluatorProc.evaluate_and_save)"""
        self.recorder.append((log["total_steps"], log["eval_return"], self.eval_return_std, log["mean_return"], log["critic_loss"],
                              log["actor_loss"]))
        os.makedirs(cwd, exist_ok=True)
        rec = np.array(self.recorder, dtype=np.float64)
        np.save(os.path.join(cwd, "recorder.npy"), rec)
        draw_learning_curve(recorder=rec, cwd=cwd)
        if log["eval_return"] >= self.best_eval_return:
            self.best_eval_return = log["eval_return"]
            self.agent.save_model(cwd, best=True)


class _Done:
    """stand-in for an already finished prefetch thread"""

    def join(self):
        return None


class Trainer:
    """One rank of the data-parallel job."""

    def __init__(self, cfg, num_envs=None, mini_batch_size=None, tuned_gemms=True):
        rank_setup(self, cfg, num_envs, tuned_gemms)
        epi = int(cfg.algo.sample_epi_num)
        batch = self.num_envs * epi
        # main.py:48: mini_batch_size = round(num_workers * sample_epi_num / 10)
        self.mini_batch_size = int(mini_batch_size if mini_batch_size is not None else max(1, round(batch / 10)))
        self.env = Pursuit_Env(cfg, num_envs=self.num_envs, rank=self.rank, device=self.device)
        torch.manual_seed(int(cfg.runtime.get("seed", 0)))
        self.agent = MAPPO(cfg, batch, self.mini_batch_size, "Learner")
        self.agent.sample_rank = self.rank  # disjoint action-sampling streams per rank (mappo.MAPPO.sample_rank)
        self.bucket = GradBucket(self.agent.ac_parameters)   # .grad of every parameter lives in one flat tensor
        self.agent.grad_bucket = self.bucket
        for part in (self.agent.diag, self.agent.bc, self.agent.kick_sums):
            if part is not None:   # algo.update_diagnostics: the eight sums / algo.pathfinder_bc_iterations: the two sums of the imitation
                part.allreduce = allreduce_sum_   # metric / algo.pathfinder_bc_coef: its three sums over ranks; no group, no collective
        self.last_imitation = None   # the log entries of the last iteration when it was an imitation iteration
        self.last_kick = None        # ... when it was a PPO iteration with lambda_j > 0 (algo.pathfinder_bc_coef)
        broadcast_weights_([self.agent.actor, self.agent.critic])
        self.total_steps = 0
        self.iteration = 0
        self.last_log = (0.0, 0.0)

    def iterate(self):
        """rollout + `epochs` updates; returns (env_steps_this_iteration_all_ranks, exp_reward).
        algo.pathfinder_bc_iterations K: iterations 0 .. K - 1 imitate the path-finding pursuers (explore_expert, train(imitation=True)
        at the constant rate pathfinder_bc_lr); iteration K starts PPO from cleared Adam moments.  The phase
        follows from `iteration` alone, so a resumed run continues in it.
        algo.pathfinder_bc_coef: PPO iteration j = iteration - K has lambda_j = coef_at(j); while it is > 0 the rollout is explore_labelled
        (on-policy, every tick labelled) and the update train(kick=lambda_j)."""
        cfg, agent = self.cfg, self.agent
        imitating, beta = phase_step(agent, agent.pathfinder_bc, self.iteration, self.total_steps)
        lam = 0.0 if imitating else agent.pathfinder_kick.coef_at(self.iteration - agent.pathfinder_bc.iterations)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        if imitating:
            exp_r, buffer, steps = agent.explore_expert(self.env, int(cfg.algo.sample_epi_num), beta)
        elif lam > 0.0:
            exp_r, buffer, steps = agent.explore_labelled(self.env, int(cfg.algo.sample_epi_num))
        else:
            exp_r, buffer, steps = agent.explore_env(self.env, int(cfg.algo.sample_epi_num))
        ev[1].record()
        self.env.prefetch_reset()  # the next episode's reset (device: kernels on the side stream; host: a thread) runs while the GPU runs the update
        self.total_steps += steps * self.world
        for _ in range(int(cfg.algo.epochs)):
            with torch.enable_grad():
                obj_c, obj_a, _, _ = agent.train(buffer, self.total_steps, return_grads=False,
                                                 **({"imitation": True} if imitating else {"kick": lam} if lam > 0.0 else {}))
            allreduce_sum_(self.bucket.flat)      # gradient SUM over ranks, in place in the bucket the optimiser reads
            agent.ac_optimizer.step()
            if cfg.algo.use_lr_decay and not imitating:
                agent.lr_decay(self.total_steps)
            self.last_log = (obj_c, obj_a)
        ev[2].record()
        self.last_imitation = None
        if imitating:   # of the last update of the iteration, like last_log; the hit rate is this rank's rollout's
            self.last_imitation = dict(phase="imitation", bc_beta=beta, bc_loss=self.last_log[1], bc_accuracy=agent.bc_accuracy(),
                                       critic_loss=self.last_log[0], pathfinder_hit_rate=agent.last_hit_rate)
        self.last_kick = None
        if lam > 0.0:   # of the last update of the iteration: lambda_j, the unweighted imitation term and its metric; this rank's build rate
            hits, live, nll = agent.last_kick
            self.last_kick = dict(bc_coef=lam, bc_aux_loss=nll / live if live else float("nan"),
                                  bc_accuracy=hits / live if live else float("nan"), pathfinder_build_rate=agent.last_build_rate)
        self.iteration += 1
        self.last_events = ev  # (rollout incl. host reset, update) timings: read after a synchronize
        return steps * self.world, exp_r

    # ---- resume bundle (the reference only saves weights: no optimiser state, step counter or RNG state) ----
    def save_resume(self, path):
        env, agent = self.env, self.agent
        init = env._take_prefetched()  # the next episode may already be drawn: it belongs to the snapshot
        # ... or already reset on the device (prefetch_reset): the bundle then carries the generator streams and tape positions as they
        # stood BEFORE that reset, so the resumed run's first reset re-creates the same episode
        pre = getattr(env, "_pre_reset", None) if getattr(env, "_dev_prefetch", None) is not None else None
        st = getattr(agent, "_rstate", None)
        bundle = dict(actor=agent.actor.state_dict(), critic=agent.critic.state_dict(), optimizer=agent.ac_optimizer.state_dict(),
                      total_steps=self.total_steps, iteration=self.iteration, reward_norm=env.sim.rn.cpu(),
                      tape_pos=(env.sim.meta[:, 2] if pre is None else pre["tape_pos"]).cpu(), sample_counter=None if st is None else st.counter.cpu(),
                      resetter=env.resetter.get_state() if pre is None else env.resetter.get_state(pre["resetter"]), next_init=init,
                      num_envs=self.num_envs, world=self.world, rank=self.rank)
        if agent.pathfinder_bc.on:   # algo.pathfinder_bc_iterations: the phase of an iteration follows from it and `iteration`; off: no entry
            bundle["pathfinder_bc_iterations"] = agent.pathfinder_bc.iterations
        if agent.pathfinder_kick.on:   # algo.pathfinder_bc_coef: lambda of an iteration follows from the three values; off: no entry
            bundle["pathfinder_bc_coef"] = agent.pathfinder_kick.entry()
        torch.save(bundle, path)
        if init is not None:
            env._prefetch = (_Done(), {"init": init})

    def load_resume(self, path):
        b = torch.load(path, map_location=self.device, weights_only=False)  # our own file (numpy blobs inside)
        if b["num_envs"] != self.num_envs or b["world"] != self.world:
            raise ValueError("resume bundle was written for another num_envs / world size")
        env, agent = self.env, self.agent
        check_pursuit_imitation_entry(agent, b.get("pathfinder_bc_iterations"), f"resume bundle {path}")
        check_pursuit_kickstart_entry(agent, b.get("pathfinder_bc_coef"), f"resume bundle {path}")
        if getattr(env, "_dev_prefetch", None) is not None:    # a device reset issued ahead belongs to the run being replaced: let it finish, drop it
            torch.cuda.current_stream().wait_stream(env.sim._side)
            env._dev_prefetch = env._pre_reset = None
        agent.actor.load_state_dict(b["actor"]); agent.critic.load_state_dict(b["critic"])
        agent.ac_optimizer.load_state_dict(b["optimizer"])
        self.total_steps, self.iteration = b["total_steps"], b["iteration"]
        agent.lr_decay(self.total_steps)
        env.sim.rn.copy_(b["reward_norm"])
        env.sim.meta[:, 2] = b["tape_pos"].to(self.device)
        env.resetter.set_state(b["resetter"])
        if b["sample_counter"] is not None:
            agent._rollout_state(env).counter.copy_(b["sample_counter"])
        env._prefetch = (_Done(), {"init": b["next_init"]}) if b["next_init"] is not None else None

    def last_breakdown_ms(self):
        ev = self.last_events
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def _device_weights(module):
    """snapshot of a module's state_dict on its device (no host round trip); the evaluator loads it on its own stream"""
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def train_agent_multiprocessing(cfg, max_iterations=None, num_eval_envs=16, eval_every=1, async_eval=None, save_resume=None, resume=None):
    """main.py:41-172 on the Trainer: runs until the evaluator says stop (total_step > max_train_steps).

    Evaluation is asynchronous like the reference's (main.py:135-158: `evaluator.run.remote(...)`, polled with `ray.wait(...,
    timeout=0.1)` while training goes on): the evaluator is a background actor of ray_shim -- its own host thread and HIP stream on
    rank 0's GPU -- that works on a device-side snapshot of the weights; the training loop only collects a finished evaluation and
    starts the next one with the current weights, it never waits for one.  No rank sits in a collective for the length of an
    evaluation: the per-iteration flag broadcast carries whatever verdict rank 0 holds at that moment.
    `runtime.async_eval: false` (or async_eval=False) evaluates inline on rank 0 (deterministic recorder rows per iteration).
    save_resume: a directory each rank writes its resume bundle to after every iteration; resume: the directory each rank loads its
    bundle from before the first one (main --save-resume / --resume)."""
    from . import pursuit_baseline, pursuit_imitation, ray_shim
    baseline_kind = pursuit_baseline.eval_baseline_options(cfg)   # validated before anything is built
    teacher = pursuit_imitation.pursuit_imitation_options(cfg).on      # likewise: algo.pathfinder_bc_*, runtime.pathfinder_*
    if pursuit_imitation.pursuit_kickstart_options(cfg).on or teacher:   # (algo.pathfinder_bc_coef*, runtime.pathfinder_labeller)
        pursuit_baseline.pathfinder_options(cfg)
    tr = Trainer(cfg)
    tr.baseline = None
    if baseline_kind is not None and tr.rank == 0:
        # the yardstick: one scripted episode on an evaluation environment of its own, once, before the first iteration
        tr.baseline = pursuit_baseline.eval_baseline(cfg, baseline_kind, num_eval_envs)
        print(json.dumps(tr.baseline), flush=True)
    if resume is not None:
        tr.load_resume(resume_path(resume, tr.rank))
    if async_eval is None:
        async_eval = bool(cfg.runtime.get("async_eval", True))
    evaluator = None
    if tr.rank == 0:
        evaluator = ray_shim.remote(EvaluatorProc).options(background=bool(async_eval)).remote(cfg, num_eval_envs)
    cwd = cfg.algo.save_cwd
    if_train = True
    eval_run_ref = None

    def collect(obj):
        """main.py:139-156: the evaluator's verdict, and the checkpoint when the greedy return did not get worse"""
        ok, ref_list = obj[0], obj[1]
        if len(ref_list) > 0:
            actor, critic, recorder = (ray_shim.get(r) for r in ref_list)
            os.makedirs(cwd, exist_ok=True)
            np.save(cwd + "/recorder.npy", recorder)
            draw_learning_curve(recorder=np.array(recorder), cwd=cwd)
            save_checkpoint(actor, critic, cwd)
        return ok

    while if_train:
        t0 = time.time()
        steps, exp_r = tr.iterate()
        if tr.rank == 0:
            print(f"iteration {tr.iteration}: {steps} env-steps in {time.time() - t0:.2f}s")
            if tr.last_imitation is not None:   # algo.pathfinder_bc_iterations: one line per imitation iteration
                print(json.dumps(dict(iteration=tr.iteration, **tr.last_imitation)), flush=True)
            elif tr.last_kick is not None:    # algo.pathfinder_bc_coef: one line per PPO iteration with lambda_j > 0
                more = {} if tr.agent.diag is None else dict(critic_loss=tr.last_log[0], actor_loss=tr.last_log[1], **tr.agent.last_update_diag)
                print(json.dumps(dict(iteration=tr.iteration, **tr.last_kick, **more)), flush=True)
            elif tr.agent.diag is not None:   # algo.update_diagnostics: the last update of the iteration, like last_log
                print(json.dumps(dict(iteration=tr.iteration, critic_loss=tr.last_log[0], actor_loss=tr.last_log[1], **tr.agent.last_update_diag)),
                      flush=True)
            if tr.iteration % eval_every == 0:
                if eval_run_ref is not None:
                    done, _ = ray_shim.wait([eval_run_ref], num_returns=1, timeout=0 if async_eval else None)
                    if done:
                        if_train = collect(ray_shim.get(done[0]))
                        eval_run_ref = None
                if eval_run_ref is None and if_train:
                    eval_run_ref = evaluator.run.remote(_device_weights(tr.agent.actor), _device_weights(tr.agent.critic), tr.total_steps, exp_r,
                                                        tr.last_log)
                    if not async_eval:   # inline: this iteration's verdict and checkpoint, not the previous evaluation's
                        if_train = collect(ray_shim.get(eval_run_ref))
                        eval_run_ref = None
        if tr.world > 1:
            flag = torch.tensor([1 if if_train else 0], device=tr.device if dist.get_backend() != "gloo" else "cpu")
            dist.broadcast(flag, src=0)
            if_train = bool(flag.item())
        if save_resume is not None:
            save_resume_atomic(tr, save_resume)
        if max_iterations is not None and tr.iteration >= max_iterations:
            break
    if tr.rank == 0:
        if eval_run_ref is not None:   # the evaluation still in flight belongs to the run's record
            collect(ray_shim.get(eval_run_ref))
        save_checkpoint(tr.agent.actor, tr.agent.critic, cwd, "_final")
        np.save(cwd + "/recorder.npy", ray_shim.get(evaluator.get_recorder.remote()))
        evaluator._shutdown()
    return tr
