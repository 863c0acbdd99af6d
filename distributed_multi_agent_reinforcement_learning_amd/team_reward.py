"""algo.team_reward of the env_3d / env_n2n trainers: team reward sharing.  Both environments pay individual rewards (+1 to the pursuer
inside the kill radius in the capture step, -1 per team-mate bumped, 0 to everyone else), so the pursuers that cut off the evader's
escape routes are paid nothing for a capture.  With alpha in [0, 1] a live pursuer's reward of a training rollout becomes
m = (1 - alpha) x + alpha s, s the team's sum of x * live of the step -- a weighted sum, not a mean: at alpha = 1 every live pursuer
sees the team's total (kernels: csrc/team_reward.hpp in the policy_record launch; numpy restatement:
tests/team_reward_ref.py).  Only the buffer's reward row (and what shaping and RewardScaling receive) is shared: returns, learning
curves and evaluation stay on the raw reward.  The option is stateless; 0, the default, is the run without it."""
import math

KEY = "algo.team_reward"


def team_reward_options(cfg):
    """-> alpha of cfg.algo (0.0 when the key is absent), validated (ValueError naming the key)"""
    raw = cfg.algo.get("team_reward", 0.0)
    try:
        alpha = float(raw)
    except (TypeError, ValueError):
        raise ValueError(f"{KEY}: {raw!r} is not a number") from None
    if not (math.isfinite(alpha) and 0.0 <= alpha <= 1.0):
        raise ValueError(f"{KEY}: {alpha} is not a finite number in [0, 1]")
    return alpha
