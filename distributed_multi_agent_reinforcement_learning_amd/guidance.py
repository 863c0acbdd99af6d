"""Scripted lead-pursuit pursuers as a yardstick policy for the env_3d / env_n2n trainers (kernels:
csrc/guidance.hpp in e3d_pursuer_guidance / n2n_pursuer_guidance; numpy restatement and specification: tests/guidance_ref.py).

A deterministic guidance law -- aim with lead at the (nearest active) evader, separate from the team-mates -- computed on the device
from the records, in the tick's lane layout, and fed to the tick where the network's actions go (`run_episode(policy="guidance")`,
`main --baseline guidance`, `runtime.eval_baseline: guidance`).  It is never trained on: it says what a sane hand-written controller
captures on the seeds the trainers evaluate on."""
from .options import distance

LEAD_KEY, SEP_RANGE_KEY, SEP_GAIN_KEY = "runtime.guidance_lead", "runtime.guidance_sep_range", "runtime.guidance_sep_gain"
BASELINE_KEY = "runtime.eval_baseline"
BASELINES = ("guidance",)
POLICIES = ("network", "guidance")
DEFAULT_LEAD, DEFAULT_SEP_GAIN = 1.0, 1.0
DEFAULT_SEP_KILL_RADII = 4.0   # guidance_sep_range defaults to this many kill radii; choices, not measurements
BASELINE_LOG_KEYS = ("baseline_return", "baseline_capture_rate", "baseline_episode_length")


def guidance_options(cfg):
    """-> (lead, sep_range, sep_gain) of cfg.runtime, validated (ValueError naming the key); sep_range is None when the key is absent
    (the environment then takes 4 x its kill_radius)"""
    rt = cfg.get("runtime", {})
    return distance(rt, LEAD_KEY, DEFAULT_LEAD), distance(rt, SEP_RANGE_KEY), distance(rt, SEP_GAIN_KEY, DEFAULT_SEP_GAIN)


def eval_baseline_options(cfg):
    """-> runtime.eval_baseline: None (absent) or "guidance", validated (ValueError naming the key)"""
    raw = cfg.get("runtime", {}).get("eval_baseline", None)
    if raw is None:
        return None
    if str(raw) not in BASELINES:
        raise ValueError(f"{BASELINE_KEY}: {raw!r} is not one of {BASELINES}")
    return str(raw)


def check_policy(policy, buf):
    """the `policy` keyword of run_episode: "network" or "guidance"; the scripted pursuers fill no buffer (nothing trains on them)"""
    if policy not in POLICIES:
        raise ValueError(f"run_episode: policy {policy!r} is not one of {POLICIES}")
    if policy == "guidance" and buf is not None:
        raise ValueError('run_episode: policy="guidance" takes no buffer (buf=None): the scripted pursuers are a yardstick, not training data')


def baseline_record(ret, captured, length):
    """the three baseline_* fields of an evaluation record from the per-environment return, captured flag and length (one read)"""
    import torch
    r, c, l = torch.stack((ret.mean(), captured.float().mean(), length.mean())).tolist()
    return dict(zip(BASELINE_LOG_KEYS, (r, c, l)))
