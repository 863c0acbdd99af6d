"""algo.reward_shaping of the env_3d / env_n2n trainers: potential-based shaping (Ng, Harada and Russell 1999) with the distance to
the nearest active evader as the potential, r' = r + gamma Phi(s') - Phi(s), which leaves the set of optimal policies unchanged
(DESIGN.md sections 7a, 7b; kernels: csrc/reward_shaping.hpp in the policy_record launch; numpy restatement: tests/shaping_ref.py).
Only the buffer's reward row is shaped: returns, learning curves and evaluation stay on the raw reward."""
import math

KEY, COEF_KEY = "algo.reward_shaping", "algo.shaping_coef"
MODES = ("none", "distance")
DEFAULT_COEF = 0.1   # a choice, not a measurement


def reward_shaping_options(cfg):
    """-> (reward_shaping, shaping_coef) of cfg.algo, validated (ValueError naming the key)"""
    a = cfg.algo
    mode = str(a.get("reward_shaping", "none"))
    if mode not in MODES:
        raise ValueError(f"{KEY}: {mode!r} is not one of {MODES}")
    try:
        coef = float(a.get("shaping_coef", DEFAULT_COEF))
    except (TypeError, ValueError):
        raise ValueError(f"{COEF_KEY}: {a.get('shaping_coef')!r} is not a number") from None
    if not (math.isfinite(coef) and coef > 0.0):
        raise ValueError(f"{COEF_KEY}: {coef} is not a finite number > 0")
    return mode, coef
