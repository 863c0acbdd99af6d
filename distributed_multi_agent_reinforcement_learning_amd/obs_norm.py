"""algo.use_obs_norm of the env_3d trainer: both encoders read features normalised by a running mean / std (the reference's
`Normalization` / `RunningMeanStd`, DHGN/normalization.py, which it never applies to env_3d; kernels:
csrc/obs_norm.hpp and k_e3d_features_norm of csrc/e3d_env.hip; numpy restatement: tests/obs_norm_ref.py).

The statistics are frozen during a rollout: every tick of a training rollout normalises under the same state and adds the sums of
its live rows to per-workgroup slots in the launch that writes the features (ParticleEnv.policy_features).  Once per rollout
(E3dMAPPO.explore_env) `commit()` reduces the slots, adds the sums over ranks and merges them into the state.  Evaluation
normalises under the state and never accumulates.  The state lives on the device and never visits the host while training."""
import ctypes as C
import math

import torch

from . import e3d_env

KEY, CLIP_KEY = "algo.use_obs_norm", "algo.obs_norm_clip"
DEFAULT_CLIP = 10.0
ROW = 33   # n, mean[16], M2[16] (csrc/obs_norm.hpp)


def obs_norm_options(cfg):
    """-> (use_obs_norm, obs_norm_clip) of cfg.algo, validated (ValueError naming the key)"""
    a = cfg.algo
    use, clip = bool(a.get("use_obs_norm", False)), a.get("obs_norm_clip", DEFAULT_CLIP)
    try:
        clip = float(clip)
    except (TypeError, ValueError):
        raise ValueError(f"{CLIP_KEY}: {clip!r} is not a number") from None
    if not (math.isfinite(clip) and clip > 0.0):
        raise ValueError(f"{CLIP_KEY}: {clip} is not finite and > 0")
    return use, clip


class ObsNorm:
    """the device state (2, 33) of one agent, the slots of its training rollout and the two launches of a merge"""

    def __init__(self, clip, device):
        self.clip = float(clip)
        self.device = torch.device(device)
        self.state = torch.zeros((2, ROW), dtype=torch.float64, device=self.device)
        self.sums = torch.zeros((2, ROW), dtype=torch.float64, device=self.device)
        self.slots = None          # (e3d_obs_norm_slots(rows), 2, 33) f64, zero between rollouts
        self.allreduce = None      # the trainer's allreduce_sum_: the sums over ranks, in place
        self.L = e3d_env.load_library()

    def slots_for(self, rows):
        """the zeroed slots of a rollout over `rows` = N P feature rows per tick (allocated once per size)"""
        n = int(self.L.e3d_obs_norm_slots(int(rows)))
        if self.slots is None or self.slots.shape[0] != n:
            self.slots = torch.zeros((n, 2, ROW), dtype=torch.float64, device=self.device)
        return self.slots

    def commit(self):
        """the merge of one rollout: slots -> sums (index order) -> all-reduce -> state; the slots are zero afterwards"""
        if self.slots is None:
            return
        ptr = lambda t: C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        n = self.slots.shape[0]
        e3d_env._check(self.L.e3d_obs_norm_reduce(ptr(self.slots), n, ptr(self.sums), stream), "e3d_obs_norm_reduce")
        if self.allreduce is not None:
            self.allreduce(self.sums)
        e3d_env._check(self.L.e3d_obs_norm_update(ptr(self.state), ptr(self.sums), ptr(self.slots), n, stream), "e3d_obs_norm_update")

    def entry(self):
        """the "obs_norm" entry of resume bundles and model files"""
        return dict(clip=self.clip, state=self.state.cpu())

    def load_entry(self, entry):
        self.state.copy_(entry["state"])
        if self.slots is not None:
            self.slots.zero_()


def check_entry(agent, entry, what, check_clip=True):
    """ValueError naming the config key when a file's "obs_norm" entry (None: written with the option off) is not this agent's;
    check_clip: another clip is refused too (a resume bundle would not continue its run bit for bit)"""
    on = getattr(agent, "obs_norm", None)
    theirs, mine = entry is not None, on is not None
    if theirs != mine:
        raise ValueError(f"{what} was written with {KEY}: {str(theirs).lower()}, this agent has {KEY}: {str(mine).lower()}")
    if mine and check_clip and float(entry["clip"]) != on.clip:
        raise ValueError(f"{what} was written with {CLIP_KEY}: {float(entry['clip'])}, this agent has {CLIP_KEY}: {on.clip}")
