"""The one device-to-host copy at the end of a train() call: the losses, the optimiser's count of skipped
steps and the sums the loss launches added to, whichever of them the call has."""
import torch

from . import ops


class BcSums:
    """the device side of the imitation metric: the two sums the bc loss launches of one train(imitation=True) call add to"""

    def __init__(self, device):
        self.sums = torch.zeros(ops.BC_SUMS, dtype=torch.float64, device=device)
        self.allreduce = None      # the trainer's allreduce_sum_: the two sums over ranks, in place


class KickSums:
    """the device side of the imitation term of teacher-regularised PPO (algo.bc_coef, algo.pathfinder_bc_coef): the three sums the fused
    loss launches of one train(kick=...) call add to"""

    def __init__(self, device):
        self.sums = torch.zeros(ops.KICK_SUMS, dtype=torch.float64, device=device)
        self.allreduce = None      # the trainer's allreduce_sum_: the three sums over ranks, in place


def read_back(*groups):
    """groups: each a tuple of scalars (Python numbers, 0-dim tensors of any dtype), a part (`.sums`, an f64 device vector, and
    `.allreduce`, the trainer's in-place sum over ranks or None) or None (a feature that is off) -> one list of Python floats per
    group, None for None, in the order given.  Every part is all-reduced once, in that order; everything reaches the host as f64
    in one copy."""
    live = [g for g in groups if g is not None]
    for g in live:
        if hasattr(g, "sums") and g.allreduce is not None:
            g.allreduce(g.sums)
    device = next((t.device for g in live for t in ([g.sums] if hasattr(g, "sums") else g) if torch.is_tensor(t)), None)
    vecs = [g.sums.double() if hasattr(g, "sums") else torch.stack([torch.as_tensor(s, dtype=torch.float64, device=device) for s in g])
            for g in live]
    flat, out = (vecs[0] if len(vecs) == 1 else torch.cat(vecs)).tolist(), []
    for g in groups:
        n = 0 if g is None else len(vecs.pop(0))
        out.append(None if g is None else flat[:n])
        flat = flat[n:]
    return out
