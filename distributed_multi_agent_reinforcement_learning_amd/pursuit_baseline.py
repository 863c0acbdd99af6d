"""Scripted pursuers as a yardstick policy for `Pursuit_Env`, the flagship grid world (kernel: csrc/pe_pathfinder.hpp
in pe_pursuer_pathfinder; plain-Python restatement and specification: tests/pe_pathfinder_ref.py).

Two policies: "pathfinder" -- a distance field to the evader over the occupancy grid, candidates checked against the tick's own
static-map probe -- and "demon", the reference's straight-at-the-evader policy that is blind to walls.  Neither is trained on: an
episode of one says what a hand-written controller scores on the seeds the evaluator uses (`main --baseline pathfinder`,
`runtime.eval_baseline: pathfinder`), in the same five quantities `evaluator.evaluate(..., stats={})` reports for the network."""
import torch

from .options import distance

LEAD_KEY, SEP_RANGE_KEY, CLEARANCE_KEY = "runtime.pathfinder_lead", "runtime.pathfinder_sep_range", "runtime.pathfinder_clearance"
BASELINE_KEY = "runtime.eval_baseline"
BASELINES = ("pathfinder", "demon")
# choices, not measurements; sep_range defaults to two collision radii, taken from the configuration
DEFAULT_LEAD, DEFAULT_CLEARANCE, MAX_CLEARANCE = 0.5, 10, 1000
STAT_KEYS = ("eval_return", "eval_capture_rate", "eval_first_contact", "eval_contact_steps", "eval_collision_steps")
BASELINE_LOG_KEYS = tuple("baseline_" + k[len("eval_"):] for k in STAT_KEYS)


def pathfinder_options(cfg):
    """-> dict(lead, sep_range, clearance) of cfg.runtime, validated (ValueError naming the key); sep_range is None when the key is
    absent (the environment then takes 2 x its collision radius)"""
    rt = cfg.get("runtime", {})
    lead = distance(rt, LEAD_KEY)
    raw = rt.get("pathfinder_clearance", DEFAULT_CLEARANCE)
    if isinstance(raw, bool) or not isinstance(raw, int) and not (isinstance(raw, float) and float(raw).is_integer()):
        raise ValueError(f"{CLEARANCE_KEY}: {raw!r} is not an integer")
    if not 0 <= int(raw) <= MAX_CLEARANCE:
        raise ValueError(f"{CLEARANCE_KEY}: {int(raw)} is not in 0 .. {MAX_CLEARANCE}")
    return dict(lead=DEFAULT_LEAD if lead is None else lead, sep_range=distance(rt, SEP_RANGE_KEY), clearance=int(raw))


def eval_baseline_options(cfg):
    """-> runtime.eval_baseline on a pursuit configuration: None (absent), "pathfinder" or "demon" (ValueError naming the key)"""
    raw = cfg.get("runtime", {}).get("eval_baseline", None)
    if raw is None:
        return None
    if str(raw) not in BASELINES:
        raise ValueError(f"{BASELINE_KEY}: {raw!r} is not one of {BASELINES} (the scripted pursuers of the pursuit configurations)")
    return str(raw)


class EpisodeStats:
    """The five episode quantities, accumulated on the device from the raw reward row of every tick: in dev_step raw > 0 means the
    pursuer touches the evader, raw < 0 means its move was rejected.  No host read before result()."""

    def __init__(self, N, device):
        self.ret = torch.zeros(N, device=device)
        self.contact = torch.zeros(N, device=device)
        self.collision = torch.zeros(N, device=device)
        self.first = torch.full((N,), -1.0, device=device)

    def add(self, raw, t):
        touch = raw > 0
        self.ret += raw.sum(-1)
        self.contact += touch.sum(-1)
        self.collision += (raw < 0).sum(-1)
        self.first = torch.where((self.first < 0) & touch.any(-1), torch.full_like(self.first, float(t)), self.first)

    def result(self, status=None):
        """status: the environments' kernel status bits (pe_env.status_or), read back with the rest and raised if set"""
        got = self.first >= 0
        bits = torch.zeros((), device=self.ret.device) if status is None else status.float()
        row = torch.stack((self.ret.mean(), got.float().mean(), (self.first * got).sum(), got.sum().float(), self.contact.mean(),
                           self.collision.mean(), bits)).tolist()       # the one host read
        r, c, fs, fn, ct, cl, bits = row
        if bits:
            from . import pe_env
            raise RuntimeError("environment kernel status: " + pe_env.status_text(int(bits)))
        return dict(zip(STAT_KEYS, (r, c, fs / fn if fn else None, ct, cl)))


@torch.no_grad()
def scripted_episode(env, cfg, policy):
    """One episode of the scripted pursuers on every environment of `env`: the loop of evaluator.evaluate with the scripted actions where
    the actor's go (reset -> observe -> attacker_step -> [actions -> tick] x T, the last step through sim.step).  -> the STAT_KEYS dict."""
    if policy not in BASELINES:
        raise ValueError(f"scripted_episode: policy {policy!r} is not one of {BASELINES}")
    opts = pathfinder_options(cfg)
    env.reset()
    N, P, T = env.num_envs, env.num_defender, env.max_steps
    sim, device = env.sim, env.device
    reward = torch.zeros(N, P, device=device)
    raw = torch.zeros(N, P, device=device)
    actions = torch.zeros(N, P, dtype=torch.int32, device=device)
    obs = sim.new_obs(packed=True)
    stats = EpisodeStats(N, device)
    env.observe(obs)
    env.attacker_step()
    for step in range(T):
        if policy == "pathfinder":
            sim.pathfinder(out=actions, **opts)
        else:
            sim.demon(out=actions)
        if step + 1 < T:
            env.tick(actions, obs, reward, raw)
        else:
            sim.step(actions, reward, raw)
            env.time_step += 1
        stats.add(raw, step)
    from . import pe_env
    return stats.result(status=pe_env.status_or(sim.meta))


def eval_baseline(cfg, policy, num_eval_envs):
    """the yardstick of a training run: one scripted episode on an evaluation environment of its own (the evaluator's seed rule), as
    the baseline_* record"""
    from .pursuit_env import Pursuit_Env
    res = scripted_episode(Pursuit_Env(cfg, num_envs=int(num_eval_envs), rank=10_000), cfg, policy)
    return dict(baseline=policy, **{b: res[k] for b, k in zip(BASELINE_LOG_KEYS, STAT_KEYS)})
