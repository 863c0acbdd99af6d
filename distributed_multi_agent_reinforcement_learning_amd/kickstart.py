"""algo.bc_coef of the env_3d / env_n2n trainers: teacher-regularised PPO -- the imitation term of algo.bc_iterations stays in the PPO
loss with a coefficient that decays over the PPO iterations (kickstarting / DAPG-style regularisation; kernels:
csrc/kickstart.hpp; numpy specification: tests/kickstart_ref.py).

PPO iteration j (0-based; trainer iteration bc_iterations + j) has lambda_j = bc_coef bc_coef_decay^j, and 0 from j = bc_coef_iterations
on when that key is > 0.  While lambda_j > 0 the rollout is ParticleMAPPO.explore_expert(env, 0.0): every tick is labelled by the scripted
pursuers (buffer["a_star"]) and no environment follows them, so the data stays on-policy; the update is train(kick=lambda_j), whose
mini-batch loss is ops.ppo_bc_loss_gauss / ops.ppo_bc_loss_cat: the PPO row and the imitation row of every sample in one launch.  The
term is the imitation phase's own loss (algo.bc_fit_std, bc_heading_wrap and bc_target_bound act on it as they do there), so the two
phases optimise the same quantity.  The feature does not need an imitation phase: bc_coef > 0 with bc_iterations 0 is kickstarting from
scratch.  With bc_coef 0 (the default) nothing here runs and no log line, buffer, checkpoint or resume bundle has a new entry."""
from .options import count, real

KEY = "algo.bc_coef"
DEFAULT_DECAY, DEFAULT_ITERATIONS = 1.0, 0   # choices, not measurements
LOG_KEYS = ("bc_coef", "bc_aux_loss")       # of a PPO iteration with lambda_j > 0, plus the agent's BC_METRIC key
KICK_SUMS = 3   # csrc/kickstart.hpp: the imitation metric's sum, the live-row count, the sum of the unweighted imitation loss


class KickstartOptions:
    """the validated algo.<prefix>coef* keys (`kickstart_options`); `on` is coef > 0, `key` the name of the coefficient's key"""

    def __init__(self, coef, decay, iterations, key=KEY):
        self.coef, self.decay, self.iterations, self.key = coef, decay, iterations, key
        self.on = coef > 0.0

    def coef_at(self, j):
        """lambda_j of PPO iteration j (0-based), in Python floats; 0 before the PPO phase and from the cut-off on"""
        if not self.on or j < 0 or (self.iterations > 0 and j >= self.iterations):
            return 0.0
        return self.coef * self.decay ** j

    def entry(self):
        """the "bc_coef" entry of a resume bundle"""
        return (self.coef, self.decay, self.iterations)


def kickstart_options(cfg, prefix="bc_"):
    """-> KickstartOptions of cfg.algo's <prefix>coef, <prefix>coef_decay and <prefix>coef_iterations (prefix "bc_", or "pathfinder_bc_" on
    the flagship: pursuit_kickstart.py), validated (ValueError naming the key)"""
    a = cfg.algo
    key = "algo." + prefix + "coef"
    coef = real(a, key, 0.0)
    if not coef >= 0.0:
        raise ValueError(f"{key}: {coef} is not >= 0")
    decay = real(a, key + "_decay", DEFAULT_DECAY)
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"{key}_decay: {decay} is not in (0, 1]")
    return KickstartOptions(coef, decay, count(a, key + "_iterations", DEFAULT_ITERATIONS), key)


def refuse_pursuit(cfg):
    """the pursuit configurations (cfg1-cfg3, `MAPPO`) have no scripted pursuers to be regularised towards"""
    if kickstart_options(cfg).on:
        raise ValueError(f"{KEY} is built for runtime.env e3d and n2n only (cfg5, cfg4_n2n): the pursuit configurations have no scripted "
                         "pursuers (set bc_coef to 0)")


def check_options_entry(options, entry, what):
    """ValueError naming the coefficient's config key when a resume bundle's entry of it (None: written with the feature off) is not
    `options`: lambda of every iteration follows from the three values, and others would not continue the run"""
    theirs = None if entry is None else tuple(entry)
    mine = options.entry() if options.on else None
    if theirs != mine:
        name = options.key.partition(".")[2]
        show = lambda e: "0 (off)" if e is None else f"{e[0]} ({name}_decay {e[1]}, {name}_iterations {e[2]})"
        raise ValueError(f"{what} was written with {options.key}: {show(theirs)}, this agent has {options.key}: {show(mine)}")


def check_entry(agent, entry, what):
    """the "bc_coef" entry of a resume bundle against this agent's setting"""
    check_options_entry(agent.kick, entry, what)
