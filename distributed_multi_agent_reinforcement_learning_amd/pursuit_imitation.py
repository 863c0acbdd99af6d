"""algo.pathfinder_bc_iterations of the Pursuit_Env trainer (cfg1-cfg4): an imitation warm start from the path-finding pursuers in front
of PPO (the teacher: section 7n, include/pe_env.h pe_pursuer_pathfinder_teach).

The first pathfinder_bc_iterations trainer iterations are imitation iterations.  Their rollout is the network's (MAPPO.explore_expert: the
features, GRU states, values, sampling stream and reward-norm state of run_episode) with one more launch per tick, the teacher's, which
writes its actions into the buffer's `a_star` field as labels -- for every environment -- and over the network's actions in the first
round(beta_k N) environments, beta_k = pathfinder_bc_beta pathfinder_bc_beta_decay^k.  Their update is train(imitation=True): ops.bc_loss_cat
on the same sequence forward, at the constant learning rate pathfinder_bc_lr, while the critic keeps its PPO loss on the returns.  The keys
are the flagship's own: algo.bc_iterations and algo.bc_coef stay refused on these configurations (imitation.refuse_pursuit,
kickstart.refuse_pursuit).  With pathfinder_bc_iterations 0 (the default) nothing here runs and no log line, buffer, checkpoint or resume
bundle has a new entry.  The schedule, its validation and the resume-entry check are section 7f's (imitation.py), under these key names.

algo.pathfinder_bc_coef: teacher-regularised PPO on the flagship.  PPO iteration j (0-based; trainer iteration
pathfinder_bc_iterations + j) has lambda_j = pathfinder_bc_coef pathfinder_bc_coef_decay^j, and 0 from j = pathfinder_bc_coef_iterations on
when that key is > 0 (kickstart.KickstartOptions under these key names).  While lambda_j > 0 the rollout is MAPPO.explore_labelled -- the
network's own, on-policy, no environment follows the teacher -- and the update is train(kick=lambda_j), whose mini-batch loss is
ops.ppo_bc_loss_cat.  runtime.pathfinder_labeller chooses how that rollout gets its labels: `episode` records the state every step reads
and labels the whole episode afterwards in one launch (pe_pathfinder_label_episode), `tick` runs the teacher's launch inside every tick
as the imitation phase does.  Both give the same bits.  The feature works without an imitation phase; with pathfinder_bc_coef 0 (the
default) nothing of it runs and no log line, buffer, checkpoint or resume bundle has a new entry."""
from .imitation import check_iterations_entry, follow_count, schedule  # noqa: F401  (the share of followed environments is 7f's rule)
from .kickstart import check_options_entry, kickstart_options
from .options import flag

KEY = "algo.pathfinder_bc_iterations"
CACHE_KEY = "runtime.pathfinder_cache"
DEFAULT_CACHE = True   # measured: DESIGN.md section 7o
COEF_KEY = "algo.pathfinder_bc_coef"
LABELLER_KEY = "runtime.pathfinder_labeller"
LABELLERS = ("episode", "tick")
DEFAULT_LABELLER = "episode"   # measured: DESIGN.md section 7p
KICK_LOG_KEYS = ("bc_coef", "bc_aux_loss", "bc_accuracy", "pathfinder_build_rate")   # of a PPO iteration with lambda_j > 0, beside iteration
LOG_KEYS = ("phase", "bc_beta", "bc_loss", "bc_accuracy", "pathfinder_hit_rate")   # of an imitation iteration, beside iteration and critic_loss


def pursuit_imitation_options(cfg):
    """-> ImitationOptions of cfg.algo's pathfinder_bc_* keys, with `cache` (runtime.pathfinder_cache), validated (ValueError naming the key)"""
    o = schedule(cfg.algo, "pathfinder_bc_")
    o.cache = flag(cfg.get("runtime", {}), CACHE_KEY, DEFAULT_CACHE)
    return o


def check_entry(agent, entry, what):
    """the "pathfinder_bc_iterations" entry of a resume bundle against this agent's setting"""
    check_iterations_entry(KEY, agent.pathfinder_bc.iterations, entry, what)


def labeller_option(cfg):
    """-> runtime.pathfinder_labeller, validated (ValueError naming the key)"""
    raw = cfg.get("runtime", {}).get(LABELLER_KEY.partition(".")[2], DEFAULT_LABELLER)
    if not isinstance(raw, str) or raw not in LABELLERS:
        raise ValueError(f"{LABELLER_KEY}: {raw!r} is not one of {', '.join(LABELLERS)}")
    return raw


def pursuit_kickstart_options(cfg):
    """-> KickstartOptions of cfg.algo's pathfinder_bc_coef* keys, with `labeller` (runtime.pathfinder_labeller), validated (ValueError
    naming the key)"""
    o = kickstart_options(cfg, "pathfinder_bc_")
    o.labeller = labeller_option(cfg)
    return o


def check_coef_entry(agent, entry, what):
    """the "pathfinder_bc_coef" entry of a resume bundle against this agent's setting"""
    check_options_entry(agent.pathfinder_kick, entry, what)
