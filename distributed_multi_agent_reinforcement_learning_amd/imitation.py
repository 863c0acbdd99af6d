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
import math

KEY = "algo.bc_iterations"
DEFAULT_BETA, DEFAULT_BETA_DECAY, DEFAULT_TARGET_BOUND = 1.0, 1.0, 0.999   # decay and bound: choices, not measurements
LOG_KEYS = ("phase", "bc_beta", "bc_loss")   # of an imitation iteration, plus bc_action_mse (env_3d; bc_angle_deg with gauss_squash: direction) or bc_accuracy (env_n2n)


class ImitationOptions:
    """the validated algo.bc_* keys; `on` is bc_iterations > 0"""

    def __init__(self, iterations, beta, beta_decay, lr, fit_std, heading_wrap, target_bound):
        self.iterations, self.beta, self.beta_decay, self.lr = iterations, beta, beta_decay, lr
        self.fit_std, self.heading_wrap, self.target_bound = fit_std, heading_wrap, target_bound
        self.on = iterations > 0

    def beta_at(self, k):
        """the share of a rank's environments that follow the teacher in imitation iteration k (0-based)"""
        return self.beta * self.beta_decay ** k


def _real(a, name, default):
    raw = a.get(name, default)
    if isinstance(raw, bool) or not isinstance(raw, (int, float)) or not math.isfinite(raw):
        raise ValueError(f"algo.{name}: {raw!r} is not a finite number")
    return float(raw)


def _flag(a, name, default):
    raw = a.get(name, default)
    if not isinstance(raw, bool):
        raise ValueError(f"algo.{name}: {raw!r} is not true or false")
    return raw


def imitation_options(cfg):
    """-> ImitationOptions of cfg.algo, validated (ValueError naming the key)"""
    a = cfg.algo
    it = a.get("bc_iterations", 0)
    if isinstance(it, bool) or not isinstance(it, int) or it < 0:
        raise ValueError(f"{KEY}: {it!r} is not an integer >= 0")
    beta = _real(a, "bc_beta", DEFAULT_BETA)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"algo.bc_beta: {beta} is not in [0, 1]")
    decay = _real(a, "bc_beta_decay", DEFAULT_BETA_DECAY)
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"algo.bc_beta_decay: {decay} is not in (0, 1]")
    lr = _real(a, "bc_lr", a.lr)
    if not lr > 0.0:
        raise ValueError(f"algo.bc_lr: {lr} is not > 0")
    bound = _real(a, "bc_target_bound", DEFAULT_TARGET_BOUND)
    if not 0.0 < bound < 1.0:
        raise ValueError(f"algo.bc_target_bound: {bound} is not in (0, 1)")
    return ImitationOptions(int(it), beta, decay, lr, _flag(a, "bc_fit_std", False), _flag(a, "bc_heading_wrap", True), bound)


def refuse_pursuit(cfg):
    """the pursuit configurations (cfg1-cfg3, `MAPPO`) have no scripted pursuers to imitate"""
    if imitation_options(cfg).on:
        raise ValueError(f"{KEY} is built for runtime.env e3d and n2n only (cfg5, cfg4_n2n): the pursuit configurations have no scripted "
                         "pursuers (set bc_iterations to 0)")


def follow_count(beta, num_envs):
    """round(beta N): the environments 0 .. count - 1 of a rank follow the teacher"""
    return int(round(beta * num_envs))


def check_entry(agent, entry, what):
    """ValueError naming the config key when a resume bundle's "bc_iterations" entry (None: written with the feature off) is not this
    agent's setting: the phase of every iteration follows from it, and another value would not continue the run"""
    theirs, mine = int(entry or 0), int(agent.imitation.iterations)
    if theirs != mine:
        raise ValueError(f"{what} was written with {KEY}: {theirs}, this agent has {KEY}: {mine}")
