"""algo.pathfinder_bc_iterations of the Pursuit_Env trainer (cfg1-cfg4): an imitation warm start from the path-finding pursuers in front
of PPO (the teacher: section 7n, include/pe_env.h pe_pursuer_pathfinder_teach).

The first pathfinder_bc_iterations trainer iterations are imitation iterations.  Their rollout is the network's (MAPPO.explore_expert: the
features, GRU states, values, sampling stream and reward-norm state of run_episode) with one more launch per tick, the teacher's, which
writes its actions into the buffer's `a_star` field as labels -- for every environment -- and over the network's actions in the first
round(beta_k N) environments, beta_k = pathfinder_bc_beta pathfinder_bc_beta_decay^k.  Their update is train(imitation=True): ops.bc_loss_cat
on the same sequence forward, at the constant learning rate pathfinder_bc_lr, while the critic keeps its PPO loss on the returns.  The keys
are the flagship's own: algo.bc_iterations and algo.bc_coef stay refused on these configurations (imitation.refuse_pursuit,
kickstart.refuse_pursuit).  With pathfinder_bc_iterations 0 (the default) nothing here runs and no log line, buffer, checkpoint or resume
bundle has a new entry.  The schedule, its validation and the resume-entry check are section 7f's (imitation.py), under these key names."""
from .imitation import check_iterations_entry, follow_count, schedule  # noqa: F401  (the share of followed environments is 7f's rule)
from .options import flag

KEY = "algo.pathfinder_bc_iterations"
CACHE_KEY = "runtime.pathfinder_cache"
DEFAULT_CACHE = True   # measured: DESIGN.md section 7o
LOG_KEYS = ("phase", "bc_beta", "bc_loss", "bc_accuracy", "pathfinder_hit_rate")   # of an imitation iteration, beside iteration and critic_loss


def pursuit_imitation_options(cfg):
    """-> ImitationOptions of cfg.algo's pathfinder_bc_* keys, with `cache` (runtime.pathfinder_cache), validated (ValueError naming the key)"""
    o = schedule(cfg.algo, "pathfinder_bc_")
    o.cache = flag(cfg.get("runtime", {}), CACHE_KEY, DEFAULT_CACHE)
    return o


def check_entry(agent, entry, what):
    """the "pathfinder_bc_iterations" entry of a resume bundle against this agent's setting"""
    check_iterations_entry(KEY, agent.pathfinder_bc.iterations, entry, what)
