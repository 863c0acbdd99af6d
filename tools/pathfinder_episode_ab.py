"""Does labelling a whole episode in one launch pay, and what does a labelled rollout cost?  (measurements 1, 2.)

    python tools/pathfinder_episode_ab.py [--configs cfg2 cfg4] [--envs 4096] [--rounds 3] [--cost-config cfg2] [--cost-rounds 8] [--out FILE.jsonl]

Measurement 1, per configuration: one pathfinder-driven closed-loop episode on reset-generated maps, the same episode for every variant
(the records are restored before each and the recorded actions drive it).  `tick`: the per-tick `pathfinder_teach` launch with the cache,
labels into row t of an (N, T, P) tensor, device events around every launch, summed.  `episode`: a `record_state` launch every tick
(events around each, summed) and one `pathfinder_label_episode` launch after the last step (events around it).  The variants alternate,
one warm-up round first; the labels of both must be equal.
Measurement 2 (--cost-config, `none` to skip): median milliseconds of `explore_env`, `explore_labelled` under both labellers, `train()`
and `train(kick=1)` on one rank, the first two rounds dropped.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_multi_agent_reinforcement_learning_amd import pe_env  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.pursuit_env import Pursuit_Env  # noqa: E402


def _pair():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def launch_ab(name, num_envs, rounds):
    cfg = baseline_config(name, **{"runtime.num_envs": num_envs})
    env = Pursuit_Env(cfg, num_envs=num_envs, rank=0)
    N, P, T = num_envs, env.num_defender, env.max_steps
    env.reset(None)
    env.sim.overlap_replan = False
    obs = env.sim.new_obs(packed=True)
    env.observe(obs)
    env.attacker_step()
    torch.cuda.synchronize()
    start = {k: v.clone() for k, v in env.sim._t.items()}
    reward, raw = torch.zeros(N, P, device="cuda"), torch.zeros(N, P, device="cuda")
    actions = torch.zeros(T, N, P, dtype=torch.int32, device="cuda")
    cache = env.pathfinder_cache()
    labels = dict(tick=torch.zeros(N, T, P, device="cuda"), episode=torch.zeros(N, T, P, device="cuda"))
    trace_def = torch.zeros((N, T, 4, P), dtype=torch.float64, device="cuda")
    trace_eva = torch.zeros((N, T, 4), dtype=torch.float64, device="cuda")
    builds = torch.zeros(N, dtype=torch.int32, device="cuda")

    def restore():
        for k, v in start.items():
            env.sim._t[k].copy_(v)
        env.time_step, env.sim.t_host = 0, 0
        cache.clear()
        cache.hits.zero_()

    restore()                                   # the episode every variant replays: the pathfinder's own
    for t in range(T):
        env.pathfinder_teach(out=actions[t], cache=cache)
        env.tick(actions[t], obs, reward, raw)

    def tick_variant():
        restore()
        ev = [_pair() for _ in range(T)]
        for t in range(T):
            ev[t][0].record()
            env.pathfinder_teach(cache=cache, a_star=labels["tick"][:, t])
            ev[t][1].record()
            env.tick(actions[t], obs, reward, raw)
        torch.cuda.synchronize()
        return dict(total=sum(a.elapsed_time(b) for a, b in ev), hit_rate=float(cache.hits.sum()) / (N * T))

    def episode_variant():
        restore()
        ev, one = [_pair() for _ in range(T)], _pair()
        for t in range(T):
            ev[t][0].record()
            env.record_state(trace_def[:, t], trace_eva[:, t])
            ev[t][1].record()
            env.tick(actions[t], obs, reward, raw)
        one[0].record()
        env.pathfinder_label_episode(trace_def, trace_eva, labels["episode"], builds=builds)
        one[1].record()
        torch.cuda.synchronize()
        rec, lab = sum(a.elapsed_time(b) for a, b in ev), one[0].elapsed_time(one[1])
        return dict(total=rec + lab, record=rec, label=lab)

    variants = dict(tick=tick_variant, episode=episode_variant)
    for run in variants.values():       # warm-up round
        run()
    rows = {k: [] for k in variants}
    for _ in range(rounds):
        for k, run in variants.items():
            rows[k].append(run())
    same = bool(torch.equal(labels["tick"], labels["episode"]))
    hit_rate = rows["tick"][-1]["hit_rate"]
    totals = {k: [r["total"] for r in v] for k, v in rows.items()}
    return dict(what="episode_ab", config=name, envs=N, ticks=T, rounds=rounds, episode_ms=totals,
                record_ms=[r["record"] for r in rows["episode"]], label_launch_ms=[r["label"] for r in rows["episode"]],
                episode_below_tick_every_round=all(e < k for e, k in zip(totals["episode"], totals["tick"])), tick_hit_rate=hit_rate,
                build_rate=float(builds.sum()) / (N * T), same_labels=same, status=int(pe_env.status_or(env.sim.meta)))


def rollout_cost(name, num_envs, rounds):
    from distributed_multi_agent_reinforcement_learning_amd.trainer import Trainer
    cfg = baseline_config(name, **{"runtime.num_envs": num_envs, "algo.pathfinder_bc_coef": 1.0})
    tr = Trainer(cfg)
    agent, env, epi = tr.agent, tr.env, int(cfg.algo.sample_epi_num)

    def timed(fn):
        torch.cuda.synchronize()
        a, b = _pair()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def labelled(labeller):
        agent.pathfinder_kick.labeller = labeller
        return agent.explore_labelled(env, epi)

    def update(buf, steps, **kw):
        with torch.enable_grad():
            return agent.train(buf, steps, return_grads=False, **kw)

    ms = {k: [] for k in ("explore_env", "explore_labelled_episode", "explore_labelled_tick", "train", "train_kick")}
    for _ in range(rounds):
        for key, fn in (("explore_env", lambda: agent.explore_env(env, epi)), ("explore_labelled_episode", lambda: labelled("episode")),
                        ("explore_labelled_tick", lambda: labelled("tick"))):
            t, (_, buf, steps) = timed(fn)
            ms[key].append(t)
            env.prefetch_reset()      # as the trainer does: the next reset runs beside what follows
        ms["train"].append(timed(lambda: update(buf, steps))[0])          # no optimiser step: the weights stay put
        ms["train_kick"].append(timed(lambda: update(buf, steps, kick=1.0))[0])
    med = lambda v: statistics.median(v[2:]) if len(v) > 2 else None
    return dict(what="rollout_cost", config=name, envs=num_envs, rounds=rounds, dropped=2, median_ms={k: med(v) for k, v in ms.items()}, all_ms=ms,
                build_rate=agent.last_build_rate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["cfg2", "cfg4"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cost-config", default="cfg2")
    ap.add_argument("--cost-rounds", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for name in args.configs:
        emit(launch_ab(name, args.envs, args.rounds))
    if args.cost_config != "none":
        emit(rollout_cost(args.cost_config, args.envs, args.cost_rounds))


if __name__ == "__main__":
    main()
