"""Times BASELINE config 4 on env_n2n (cfg4_n2n: 16 pursuers, DHGN actor / critic) on one GPU and prints one JSON line.

    python tools/bench_n2n.py [--num-envs 1024] [--warmup 2] [--steps 5] [--log-iterations 0 --log-out FILE] [KEY=VALUE ...]

KEY=VALUE: dotted config overrides as `main` takes them, e.g. algo.use_reward_scaling=True, algo.reward_shaping=distance,
algo.update_diagnostics=True, algo.target_kl=0.02.

rollout_ms / update_ms: device-event times per iteration (N2nTrainer.last_breakdown_ms); env_steps_per_s: environment steps over
the wall time of the timed iterations (host clock around work that ends in a device synchronise); slsqp_share: the SLSQP evader's
launches over the rollout time, both from one more iteration whose evader launches are bracketed by device events.  With
--log-iterations K it then trains K more iterations and writes their log records (mean return, capture rate, ...) as JSON lines."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config, parse_overrides  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--log-iterations", type=int, default=0)
    ap.add_argument("--log-out", default=None)
    ap.add_argument("overrides", nargs="*", help="dotted overrides KEY=VALUE")
    args = ap.parse_args()
    ov = parse_overrides(args.overrides)
    if not torch.cuda.is_available():
        raise SystemExit("bench_n2n needs the GPU")
    tr = N2nTrainer(baseline_config("cfg4_n2n", **{"runtime.num_envs": args.num_envs, **ov}))
    for _ in range(args.warmup):
        tr.iterate()
    torch.cuda.synchronize()
    roll, upd, steps = [], [], 0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        s, _ = tr.iterate()
        steps += s
        torch.cuda.synchronize()
        r, u = tr.last_breakdown_ms()
        roll.append(r)
        upd.append(u)
    wall = time.perf_counter() - t0
    # one more iteration with every evader launch of the rollout bracketed by events (tr.env.evader_step is the only caller)
    env, orig, pairs = tr.env, tr.env.evader_step, []

    def timed(*a, **k):
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record()
        orig(*a, **k)
        e[1].record()
        pairs.append(e)

    env.evader_step = timed
    tr.iterate()
    env.evader_step = orig
    torch.cuda.synchronize()
    slsqp_ms, slsqp_roll = sum(a.elapsed_time(b) for a, b in pairs), tr.last_breakdown_ms()[0]
    rm, um = sum(roll) / len(roll), sum(upd) / len(upd)
    print(json.dumps({"config": "cfg4_n2n", "overrides": ov, "num_envs": args.num_envs, "steps": args.steps, "rollout_ms": round(rm, 2), "update_ms": round(um, 2),
                      "env_steps_per_s": round(steps / wall, 1), "slsqp_ms_per_rollout": round(slsqp_ms, 2),
                      "slsqp_share": round(slsqp_ms / slsqp_roll, 4), "rollout_ms_all": [round(x, 2) for x in roll],
                      "update_ms_all": [round(x, 2) for x in upd]}), flush=True)
    if args.log_iterations:
        out = open(args.log_out, "w") if args.log_out else sys.stdout
        for _ in range(args.log_iterations):
            _, log = tr.iterate()
            out.write(json.dumps(log) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
