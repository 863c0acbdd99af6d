"""algo.bc_iterations of the env_3d / env_n2n trainers: an imitation warm start from the scripted lead-pursuit pursuers in front of PPO
(kernels: csrc/imitation.hpp; numpy restatement and specification: tests/imitation_ref.py).

The first bc_iterations trainer iterations are imitation iterations.  Their rollout is the network's (ParticleMAPPO.explore_expert: the
features, GRU states, values, rewards and running statistics of run_episode) with two more launches per tick: the scripted pursuers'
actions (ParticleEnv.guidance_actions) and ops.bc_select, which writes them into the buffer's `a_star` field as labels -- for every
environment -- and over the network's actions in the first round(beta_k N) environments, beta_k = bc_beta bc_beta_decay^k.  bc_beta_decay
1 is plain behaviour cloning, below 1 the learner drives more of its own states every iteration and is still labelled on them
(DAgger).  Their update is train(imitation=True): the supervised loss ops.bc_loss_gauss / ops.bc_loss_cat on the same sequence forward,
at the constant learning rate bc_lr, while the critic keeps its PPO loss on the returns.  With bc_iterations 0 (the default) nothing here
runs and no log line, buffer, checkpoint or resume bundle has a new entry."""
import torch

from .options import count, flag, real

KEY = "algo.bc_iterations"
DEFAULT_BETA, DEFAULT_BETA_DECAY, DEFAULT_TARGET_BOUND = 1.0, 1.0, 0.999   # decay and bound: choices, not measurements
LOG_KEYS = ("phase", "bc_beta", "bc_loss")   # of an imitation iteration, plus bc_action_mse (env_3d; bc_angle_deg with gauss_squash: direction) or bc_accuracy (env_n2n)


class ImitationOptions:
    """the validated schedule of an imitation phase (`schedule`); `on` is iterations > 0.  imitation_options adds fit_std, heading_wrap
    and target_bound, pursuit_imitation_options adds cache"""

    def __init__(self, iterations, beta, beta_decay, lr):
        self.iterations, self.beta, self.beta_decay, self.lr = iterations, beta, beta_decay, lr
        self.on = iterations > 0

    def beta_at(self, k):
        """the share of a rank's environments that follow the teacher in imitation iteration k (0-based)"""
        return self.beta * self.beta_decay ** k


def schedule(a, prefix):
    """-> ImitationOptions of algo.<prefix>iterations, <prefix>beta, <prefix>beta_decay and <prefix>lr (prefix "bc_" or "pathfinder_bc_"),
    validated (ValueError naming the key)"""
    key = "algo." + prefix
    it = count(a, key + "iterations")
    beta = real(a, key + "beta", DEFAULT_BETA)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"{key}beta: {beta} is not in [0, 1]")
    decay = real(a, key + "beta_decay", DEFAULT_BETA_DECAY)
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"{key}beta_decay: {decay} is not in (0, 1]")
    lr = real(a, key + "lr", a.lr)
    if not lr > 0.0:
        raise ValueError(f"{key}lr: {lr} is not > 0")
    return ImitationOptions(it, beta, decay, lr)


def imitation_options(cfg):
    """-> ImitationOptions of cfg.algo's bc_* keys, validated (ValueError naming the key)"""
    a = cfg.algo
    o = schedule(a, "bc_")
    o.target_bound = real(a, "algo.bc_target_bound", DEFAULT_TARGET_BOUND)
    if not 0.0 < o.target_bound < 1.0:
        raise ValueError(f"algo.bc_target_bound: {o.target_bound} is not in (0, 1)")
    o.fit_std, o.heading_wrap = flag(a, "algo.bc_fit_std", False), flag(a, "algo.bc_heading_wrap", True)
    return o


def refuse_pursuit(cfg):
    """the pursuit configurations (cfg1-cfg3, `MAPPO`) have no scripted pursuers to imitate"""
    if imitation_options(cfg).on:
        raise ValueError(f"{KEY} is built for runtime.env e3d and n2n only (cfg5, cfg4_n2n): the pursuit configurations have no scripted "
                         "pursuers (set bc_iterations to 0)")


def follow_count(beta, num_envs):
    """round(beta N): the environments 0 .. count - 1 of a rank follow the teacher"""
    return int(round(beta * num_envs))


def follow_mask(beta, num_envs, device):
    """the (N,) uint8 mask of explore_expert: 1 in the environments that execute the teacher's action"""
    follow = torch.zeros(num_envs, dtype=torch.uint8, device=device)
    follow[:follow_count(beta, num_envs)] = 1
    return follow


def check_iterations_entry(key, mine, entry, what):
    """ValueError naming the config key when a resume bundle's entry of an imitation phase's length (None: written with the feature off)
    is not this agent's setting: the phase of every iteration follows from it, and another value would not continue the run"""
    theirs, mine = int(entry or 0), int(mine)
    if theirs != mine:
        raise ValueError(f"{what} was written with {key}: {theirs}, this agent has {key}: {mine}")


def check_entry(agent, entry, what):
    """the "bc_iterations" entry of a resume bundle against this agent's setting"""
    check_iterations_entry(KEY, agent.imitation.iterations, entry, what)


def phase_step(agent, options, iteration, total_steps):
    """-> (whether trainer iteration `iteration` imitates, its beta_k or None).  The leading options.iterations iterations do, at the
    constant learning rate options.lr; the first PPO iteration starts from fresh moments, on the schedule.  The phase follows from
    `iteration` alone, so a resumed run continues in it"""
    if iteration < options.iterations:
        agent.set_lr(options.lr)
        return True, options.beta_at(iteration)
    if options.on and iteration == options.iterations:
        agent.reset_optimizer(total_steps)
    return False, None


class OptimizerSchedule:
    """the learning rate of an agent's ac_optimizer (torch.optim.Adam or trainer.FusedAdam): the linear decay, the constant rate of an
    imitation phase and the step from that phase to PPO.  The agent provides ac_optimizer, lr, max_train_steps and use_lr_decay."""

    def set_lr(self, lr):
        for p in self.ac_optimizer.param_groups:
            p["lr"] = lr

    def reset_optimizer(self, total_steps):
        """the step from the imitation phase to PPO: Adam's moments and step count back to zero (the moments of a supervised loss say
        nothing about the PPO gradient) and the learning rate back on the schedule"""
        opt = self.ac_optimizer
        if hasattr(opt, "reset_moments"):   # FusedAdam
            opt.reset_moments()
        else:
            for st in opt.state.values():
                for key in ("step", "exp_avg", "exp_avg_sq"):
                    st[key].zero_()
        if self.use_lr_decay:
            self.lr_decay(total_steps)
        else:
            self.set_lr(self.lr)

    def lr_decay(self, total_steps):
        self.set_lr(self.lr * (1 - total_steps / self.max_train_steps))
        self.total_step = total_steps
