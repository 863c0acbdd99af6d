"""config.yaml loader keeping the reference's schema (config.yaml:13-94) without hydra/omegaconf.

The reference resolves its config with hydra (main.py:40); neither hydra nor omegaconf is needed for the hot path,
so the same yaml is read with PyYAML into an attribute dict.  An optional ``runtime`` section (ours) carries what
the reference hard-codes in main.py:42-50 (number of environments, seed, ...).
"""
import ast
import copy
import os

import yaml

SECTIONS = ("env", "sensor", "map", "attacker", "defender", "algo")


class Cfg(dict):
    """dict with attribute access, like the omegaconf nodes the reference code reads (cfg.env.max_steps ...)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def __deepcopy__(self, memo):
        return Cfg({k: copy.deepcopy(v, memo) for k, v in self.items()})


def to_cfg(d):
    if isinstance(d, dict):
        return Cfg({k: to_cfg(v) for k, v in d.items()})
    return d


DEFAULT_YAML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config.yaml")


def load_config(path=None, **overrides):
    """Reads a reference-schema config.yaml.  ``overrides`` are dotted keys, e.g. ``**{"env.num_defender": 8}``."""
    raw = yaml.safe_load(open(path or DEFAULT_YAML))
    cfg = to_cfg({k: raw[k] for k in SECTIONS if k in raw})
    cfg["runtime"] = to_cfg(raw.get("runtime") or {})
    rt = cfg.runtime
    rt.setdefault("num_envs", 16)
    rt.setdefault("seed", 0)
    rt.setdefault("tape_len", 16)
    rt.setdefault("max_path", 128)
    rt.setdefault("reference_quirks", True)
    rt.setdefault("use_graphs", True)
    rt.setdefault("device_reset", True)           # episode reset on the GPU (k_reset); False = host resetter, same results
    if rt.get("overlap_actor_critic"):
        raise ValueError("runtime.overlap_actor_critic was removed: the two-stream update could stall (DESIGN.md)")
    for k, v in overrides.items():
        node = cfg
        parts = k.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = v
    return cfg


def baseline_config(name="cfg2", **overrides):
    """The concrete configurations of BASELINE.json / SURVEY 8d."""
    base = {
        "cfg1": {"env.num_defender": 4, "map.map_size": [20, 20], "map.center": [10, 10], "map.variance": 4,
                 "map.num_obstacle_block": 2, "algo.depth": 1, "runtime.num_envs": 16},
        "cfg2": {"env.num_defender": 8, "map.map_size": [40, 40], "map.center": [20, 20], "map.variance": 10,
                 "map.num_obstacle_block": 5, "algo.depth": 0, "runtime.num_envs": 4096},
        "cfg3": {"env.num_defender": 8, "map.map_size": [40, 40], "map.center": [20, 20], "map.variance": 10,
                 "map.num_obstacle_block": 5, "algo.depth": 3, "runtime.num_envs": 4096},
        # BASELINE config 4 is a scaling configuration (16 agents, 64x64, DHGN, 8192 environments over 8 GPUs = 1024 per rank).  The
        # environment it names has no trainer in the reference, so the shapes run on the pursuit-evasion game: 16
        # defenders on a 64x64 map, DHGN depth 3.  Not pinned to reference vectors beyond the shared kernels (P > 8 takes the
        # sequential step scoring of the tick; the P = 15 shipped geometry is what the parity tests cover).
        "cfg4": {"env.num_defender": 16, "map.map_size": [64, 64], "map.center": [32, 32], "map.variance": 12,
                 "map.num_obstacle_block": 5, "algo.depth": 3, "runtime.num_envs": 1024},
        # BASELINE config 5: env_3d pursuit, 8 agents, 2048 environments over 4 GPUs = 512 per rank, GRU actor / critic.  The
        # reference has no learner for it: the package's diagonal-Gaussian MAPPO (e3d_agent.py)
        # with the reference's SLSQP evader.  No reward normalisation on this path.
        "cfg5": {"runtime.env": "e3d", "env.num_defender": 8, "env.max_steps": 200, "env.action_dim": 3, "algo.depth": 0,
                 "algo.use_reward_norm": False, "runtime.num_envs": 512, "runtime.e3d_evader": "slsqp"},
        # BASELINE config 4 on the environment it names: env_n2n, 16 pursuers, 8192 environments over 8 GPUs = 1024 per rank, the DHGN
        # actor / critic (n2n_agent.py) against the reference's SLSQP evader; max_steps = the reference's
        # episode_limit.  No reward normalisation on this path.
        "cfg4_n2n": {"runtime.env": "n2n", "env.num_defender": 16, "env.num_evader": 1, "env.max_steps": 100, "algo.depth": 3,
                     "algo.use_reward_norm": False, "runtime.num_envs": 1024, "runtime.n2n_evader": "slsqp"},
    }[name]
    ov = {"algo.use_reward_norm": True}  # the shipped `false` crashes the reference's run_episode
    ov.update(base)
    ov.update(overrides)
    return load_config(**ov)


def parse_overrides(items):
    """command-line KEY=VALUE items -> {dotted key: value}; a value Python can read as a literal (numbers, booleans, lists) becomes
    one, anything else stays a string (main and tools/bench_e3d.py)"""
    ov = {}
    for item in items:
        k, _, v = item.partition("=")
        try:
            ov[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            ov[k] = v
    return ov
