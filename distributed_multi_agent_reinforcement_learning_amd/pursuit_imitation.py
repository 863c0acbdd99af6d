"""algo.pathfinder_bc_iterations of the Pursuit_Env trainer (cfg1-cfg4): an imitation warm start from the path-finding pursuers in front
of PPO (the teacher: section 7n, include/pe_env.h pe_pursuer_pathfinder_teach).

The first pathfinder_bc_iterations trainer iterations are imitation iterations.  Their rollout is the network's (MAPPO.explore_expert: the
features, GRU states, values, sampling stream and reward-norm state of run_episode) with one more launch per tick, the teacher's, which
writes its actions into the buffer's `a_star` field as labels -- for every environment -- and over the network's actions in the first
round(beta_k N) environments, beta_k = pathfinder_bc_beta pathfinder_bc_beta_decay^k.  Their update is train(imitation=True): ops.bc_loss_cat
on the same sequence forward, at the constant learning rate pathfinder_bc_lr, while the critic keeps its PPO loss on the returns.  The keys
are the flagship's own: algo.bc_iterations and algo.bc_coef stay refused on these configurations (imitation.refuse_pursuit,
kickstart.refuse_pursuit).  With pathfinder_bc_iterations 0 (the default) nothing here runs and no log line, buffer, checkpoint or resume
bundle has a new entry."""
import math

from .imitation import follow_count  # noqa: F401  (the share of followed environments is 7f's rule)

KEY = "algo.pathfinder_bc_iterations"
CACHE_KEY = "runtime.pathfinder_cache"
DEFAULT_BETA, DEFAULT_BETA_DECAY = 1.0, 1.0
DEFAULT_CACHE = True   # measured: DESIGN.md section 7o
LOG_KEYS = ("phase", "bc_beta", "bc_loss", "bc_accuracy", "pathfinder_hit_rate")   # of an imitation iteration, beside iteration and critic_loss


class PursuitImitationOptions:
    """the validated algo.pathfinder_bc_* keys and runtime.pathfinder_cache; `on` is pathfinder_bc_iterations > 0"""

    def __init__(self, iterations, beta, beta_decay, lr, cache):
        self.iterations, self.beta, self.beta_decay, self.lr, self.cache = iterations, beta, beta_decay, lr, cache
        self.on = iterations > 0

    def beta_at(self, k):
        """the share of a rank's environments that follow the teacher in imitation iteration k (0-based)"""
        return self.beta * self.beta_decay ** k


def _real(a, name, default):
    raw = a.get(name, default)
    if isinstance(raw, bool) or not isinstance(raw, (int, float)) or not math.isfinite(raw):
        raise ValueError(f"algo.{name}: {raw!r} is not a finite number")
    return float(raw)


def pursuit_imitation_options(cfg):
    """-> PursuitImitationOptions of cfg, validated (ValueError naming the key)"""
    a = cfg.algo
    it = a.get("pathfinder_bc_iterations", 0)
    if isinstance(it, bool) or not isinstance(it, int) or it < 0:
        raise ValueError(f"{KEY}: {it!r} is not an integer >= 0")
    beta = _real(a, "pathfinder_bc_beta", DEFAULT_BETA)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"algo.pathfinder_bc_beta: {beta} is not in [0, 1]")
    decay = _real(a, "pathfinder_bc_beta_decay", DEFAULT_BETA_DECAY)
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"algo.pathfinder_bc_beta_decay: {decay} is not in (0, 1]")
    lr = _real(a, "pathfinder_bc_lr", a.lr)
    if not lr > 0.0:
        raise ValueError(f"algo.pathfinder_bc_lr: {lr} is not > 0")
    cache = cfg.get("runtime", {}).get("pathfinder_cache", DEFAULT_CACHE)
    if not isinstance(cache, bool):
        raise ValueError(f"{CACHE_KEY}: {cache!r} is not true or false")
    return PursuitImitationOptions(int(it), beta, decay, lr, cache)


def check_entry(agent, entry, what):
    """ValueError naming the config key when a resume bundle's "pathfinder_bc_iterations" entry (None: written with the feature off) is not
    this agent's setting: the phase of every iteration follows from it, and another value would not continue the run"""
    theirs, mine = int(entry or 0), int(agent.pathfinder_bc.iterations)
    if theirs != mine:
        raise ValueError(f"{what} was written with {KEY}: {theirs}, this agent has {KEY}: {mine}")
