"""algo.update_diagnostics / algo.target_kl: what a PPO update did, measured inside the loss launches (kernels:
csrc/ppo_diag.hpp and the DIAG instances of the loss kernels; numpy restatement: tests/ppo_diag_ref.py).

Every mini-batch's loss call adds eight f64 sums over its live rows to one device tensor that train() zeroes at its start; train()
reads it in the synchronisation it already has and derives approx_kl, clip_fraction, entropy, explained_variance and ratio_mean, plus
the largest pre-clip gradient norm of the call.  Under data parallelism the sums go through one all-reduce, so every rank derives
the same values and the algo.target_kl early stop is the same decision everywhere.  Nothing here survives an iteration."""
import math

import torch

from . import ops
from .readback import read_back

KEY, KL_KEY = "algo.update_diagnostics", "algo.target_kl"
DERIVED = ("approx_kl", "clip_fraction", "entropy", "explained_variance", "ratio_mean")
LOG_KEYS = DERIVED + ("grad_norm",)


def update_diag_options(cfg):
    """-> (update_diagnostics, target_kl or None) of cfg.algo, validated (ValueError naming the key); a target turns the diagnostics on"""
    a = cfg.algo
    target = a.get("target_kl", None)
    if target is not None:
        if isinstance(target, bool) or not isinstance(target, (int, float)) or not math.isfinite(target) or not target > 0:
            raise ValueError(f"{KL_KEY}: {target!r} is not a finite number > 0 (leave the key out for no early stop)")
        target = float(target)
    return bool(a.get("update_diagnostics", False)) or target is not None, target


def derive(sums):
    """the eight sums (count, k3 KL, clipped, entropy, v_target, v_target^2, (v_target - v_now)^2, ratio) -> the five derived values"""
    c, s1, s2, s3, s4, s5, s6, s7 = (float(x) for x in sums)
    if c == 0:
        return dict.fromkeys(DERIVED, float("nan"))
    mean = s4 / c
    var = s5 / c - mean * mean
    return dict(approx_kl=s1 / c, clip_fraction=s2 / c, entropy=s3 / c, explained_variance=1.0 - (s6 / c) / var if var > 0 else float("nan"),
                ratio_mean=s7 / c)


def first_epoch_over(kls, target):
    """the early-stop rule: the index of the first epoch whose approx_kl exceeds the target, None when there is none (or no target).
    That epoch's gradient is discarded and the epochs after it are skipped, so the index is also the number of optimizer steps taken."""
    if target is None:
        return None
    for e, kl in enumerate(kls):
        if kl > target:
            return e
    return None


class UpdateDiag:
    """the device side of one agent's diagnostics: the sums of the running train() call and its largest pre-clip gradient norm"""

    def __init__(self, device):
        self.sums = torch.zeros(ops.PPO_DIAG_SUMS, dtype=torch.float64, device=device)
        self.grad_norm = torch.zeros((), dtype=torch.float32, device=device)
        self.allreduce = None      # the trainer's allreduce_sum_: the eight sums over ranks, in place (one 64-byte all-reduce per train())

    def begin(self):
        self.sums.zero_()
        self.grad_norm.zero_()
        self.noted = False

    def note_grad_norm(self, total_norm):
        """total_norm: what clip_grad_norm_ returned (the norm before clipping), a device scalar"""
        torch.maximum(self.grad_norm, total_norm.detach().to(self.grad_norm.dtype), out=self.grad_norm)
        self.noted = True

    def result(self, sums, grad_norm):
        """the eight sums (over ranks) and the gradient norm as read_back delivered them -> the diagnostics dict"""
        out = derive(sums)
        out["grad_norm"] = grad_norm if self.noted else float("nan")   # (algo.use_grad_clip: false computes no norm)
        self.last_sums = sums
        return out

    def read(self, *scalars):
        """-> (the scalars as floats, the diagnostics dict): one device-to-host copy for all of it"""
        vals, sums, (norm,) = read_back(scalars, self, (self.grad_norm,))
        return vals, self.result(sums, norm)
