"""Does the teacher's distance-field cache pay?  (measurement 1.)

    python tools/pathfinder_cache_ab.py [--configs cfg2 cfg4] [--envs 4096] [--rounds 3] [--out FILE.jsonl]

One pathfinder-driven closed-loop episode on reset-generated maps, the same episode for every variant (the records are restored before
each): `pathfinder_teach` with the cache, `pathfinder_teach` with the cache NULL, and the plain `pathfinder`.  Device events around every
teacher launch, summed per episode; the variants alternate, one warm-up round first.  A last pass counts hits and the sweeps of the misses
(pe_diag_pathfinder_sweeps on the same records).  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_multi_agent_reinforcement_learning_amd import pe_env  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.pursuit_env import Pursuit_Env  # noqa: E402


def measure(name, num_envs, rounds):
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
    actions = torch.zeros(N, P, dtype=torch.int32, device="cuda")
    cache = env.pathfinder_cache()

    def episode(teacher, each_tick=None):
        for k, v in start.items():
            env.sim._t[k].copy_(v)
        env.time_step, env.sim.t_host = 0, 0
        cache.clear()
        cache.hits.zero_()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(T)]
        for t in range(T):
            if each_tick is not None:
                each_tick()
            ev[t][0].record()
            teacher()
            ev[t][1].record()
            env.tick(actions, obs, reward, raw)
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in ev)

    variants = dict(cached=lambda: env.pathfinder_teach(out=actions, cache=cache), uncached=lambda: env.pathfinder_teach(out=actions),
                    plain=lambda: env.pathfinder(out=actions))
    for teacher in variants.values():       # warm-up round
        episode(teacher)
    totals = {k: [] for k in variants}
    finals = {}
    for _ in range(rounds):
        for k, teacher in variants.items():
            totals[k].append(episode(teacher))
            finals[k] = (env.sim.defs.clone(), env.sim.eva.clone())
    same = all(torch.equal(a, b) for k in ("uncached", "plain") for a, b in zip(finals["cached"], finals[k]))
    # hits, and the sweeps of the misses: before every cached launch, the sweep count of the plain field on the same records
    sweeps = torch.zeros(N, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(N, P, dtype=torch.int32, device="cuda")
    prm = pe_env.pathfinder_params(env.pe_cfg)
    acc = dict(miss=torch.zeros((), dtype=torch.float64, device="cuda"), sweeps=torch.zeros((), dtype=torch.float64, device="cuda"),
               last=torch.zeros(N, dtype=torch.int32, device="cuda"), pending=None)

    def settle():
        if acc["pending"] is not None:
            miss = (cache.hits == acc["last"]).double()
            acc["miss"] += miss.sum()
            acc["sweeps"] += (miss * acc["pending"].double()).sum()
            acc["last"] = cache.hits.clone()

    def count():
        settle()
        rc = env.sim.L.pe_diag_pathfinder_sweeps(C.byref(env.pe_cfg), C.byref(env.sim.st), C.byref(prm), C.c_void_p(scratch.data_ptr()),
                                                 C.c_void_p(sweeps.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        acc["pending"] = sweeps.clone()

    episode(variants["cached"], each_tick=count)
    settle()
    misses = float(acc["miss"])
    status = int(pe_env.status_or(env.sim.meta))
    us = lambda v: 1e3 * v / T
    return dict(what="cache_ab", config=name, envs=N, ticks=T, rounds=rounds, episode_ms={k: v for k, v in totals.items()},
                per_launch_us={k: [us(x) for x in v] for k, v in totals.items()}, cached_below_uncached_every_round=all(
                    c < u for c, u in zip(totals["cached"], totals["uncached"])), hit_rate=1.0 - misses / (N * T),
                mean_sweeps_on_misses=float(acc["sweeps"]) / misses, same_final_records=bool(same), status=status)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg2", "cfg4"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for name in args.configs:
        line = json.dumps(measure(name, args.envs, args.rounds))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
