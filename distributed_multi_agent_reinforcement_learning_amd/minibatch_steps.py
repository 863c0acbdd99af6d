"""algo.minibatch_steps of the env_3d / env_n2n trainers: one optimiser step per mini-batch instead of one per epoch (DESIGN.md section
7d; kernels: csrc/fused_adam.hpp; numpy restatement: tests/fused_adam_ref.py).

With the option on E3dMAPPO.train / N2nMAPPO.train do, for every mini-batch: zero the gradient bucket, forward + loss + backward, the
gradient SUM over ranks, and one fused clip + Adam step (trainer.FusedAdam on trainer.ParamBucket: two launches on the flat
parameters, gradients and moments).  The trainers' epoch loop then neither reduces nor steps.  With the option off (the default)
nothing here runs: torch.optim.Adam, the loop and the files are today's."""

from .options import flag

KEY = "algo.minibatch_steps"
MAX_GRAD_NORM = 5.0   # the clip of E3dMAPPO.train / N2nMAPPO.train (algo.use_grad_clip), as MAPPO.train's


def minibatch_steps_options(cfg):
    """-> minibatch_steps of cfg.algo, validated (ValueError naming the key)"""
    return flag(cfg.algo, KEY, False)


def check_entry(agent, entry, what):
    """ValueError naming the config key when a resume bundle's "minibatch_steps" entry (None: written with the option off) is not this
    agent's setting: the two optimisers' states do not convert into each other, and the run would not continue bit for bit"""
    theirs, mine = bool(entry), bool(getattr(agent, "minibatch_steps", False))
    if theirs != mine:
        raise ValueError(f"{what} was written with {KEY}: {str(theirs).lower()}, this agent has {KEY}: {str(mine).lower()}")
