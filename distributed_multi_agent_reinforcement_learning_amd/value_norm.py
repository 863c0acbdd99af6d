"""algo.use_value_norm of the env_3d / env_n2n trainers: the critic learns value targets normalised by running statistics (the
PopArt-style "ValueNorm" of the public MAPPO implementation; DESIGN.md sections 7a, 7b; kernels: csrc/value_norm.hpp; numpy
restatement: tests/value_norm_ref.py).

The critic emits normalised values and the rollout stores them as they are.  Once per update (E3dMAPPO.train / N2nMAPPO.train):
GAE on the values denormalised under the statistics in force (ops.gae_advnorm_vn, masked: a value the rollout zeroed stays 0), the
sums of the new targets over ranks, one moving-average step of the state (ops.value_norm_update) and the targets normalised under
the NEW statistics (ops.value_norm_targets), which the unchanged PPO loss regresses on.  The state lives on the device and never
visits the host while training."""
from . import ops

KEY, BETA_KEY = "algo.use_value_norm", "algo.value_norm_beta"
DEFAULT_BETA = 0.99999


def value_norm_options(cfg):
    """-> (use_value_norm, value_norm_beta) of cfg.algo, validated (ValueError naming the key)"""
    a = cfg.algo
    use, beta = bool(a.get("use_value_norm", False)), float(a.get("value_norm_beta", DEFAULT_BETA))
    if not 0.0 < beta < 1.0:
        raise ValueError(f"{BETA_KEY}: {beta} is not inside (0, 1)")
    return use, beta


class ValueNorm:
    """the device state (m, q, d) of one agent and the three launches of an update"""

    def __init__(self, beta, device):
        self.beta = float(beta)
        self.state = ops.value_norm_state(device)
        self.allreduce = None      # the trainer's allreduce_sum_: (S1, S2, c) summed over ranks, in place
        self.last = None           # (denormalised v_target, sums) of the last update, device tensors (tests, diagnostics)

    def gae_targets(self, buf, gamma, lamda, use_adv_norm):
        """-> (adv, normalised v_target) of the buffer; advances the state"""
        adv, v_raw, sums = ops.gae_advnorm_vn(buf["r"], buf["v_n"], buf["active"], buf["v_mask"], self.state, gamma, lamda, use_adv_norm)
        if self.allreduce is not None:
            self.allreduce(sums)
        ops.value_norm_update(self.state, sums, self.beta)
        self.last = (v_raw, sums)
        return adv, ops.value_norm_targets(v_raw, buf["active"], self.state)

    def entry(self):
        """the "value_norm" entry of resume bundles and model files"""
        return dict(beta=self.beta, state=self.state.cpu())

    def load_entry(self, entry):
        self.state.copy_(entry["state"])


def check_entry(agent, entry, what, check_beta=True):
    """ValueError naming the config key when a file's "value_norm" entry (None: written with the option off) is not this agent's;
    check_beta: another beta is refused too (a resume bundle would not continue its run bit for bit; weights load under any beta)"""
    theirs, mine = entry is not None, agent.value_norm is not None
    if theirs != mine:
        raise ValueError(f"{what} was written with {KEY}: {str(theirs).lower()}, this agent has {KEY}: {str(mine).lower()}")
    if mine and check_beta and float(entry["beta"]) != agent.value_norm.beta:
        raise ValueError(f"{what} was written with {BETA_KEY}: {float(entry['beta'])}, this agent has {BETA_KEY}: {agent.value_norm.beta}")
