"""The imitation warm start of the flagship as one run (measurements 2 and 3).

    python tools/pathfinder_bc_run.py [--config cfg2] [--k 16] [--eval-envs 2048] [--eval-every 10] [--out FILE.jsonl] [KEY=VALUE ...]

K imitation iterations (algo.pathfinder_bc_iterations=K) and then K PPO iterations on one rank, seed 0.  One JSON line per iteration
(phase, rollout ms, update ms, the imitation log entries), a greedy evaluation with the five keys of evaluate(stats={}) before the
first iteration, every --eval-every iterations and at the end of either phase, the pathfinder's own record on the same kind of
evaluation environment, and a summary line: median rollout / update ms per phase with the first two iterations of each phase dropped."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from distributed_multi_agent_reinforcement_learning_amd import pursuit_baseline  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config, parse_overrides  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.evaluator import evaluate  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.pursuit_env import Pursuit_Env  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.trainer import Trainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--eval-envs", type=int, default=2048)
    ap.add_argument("--eval-every", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args()
    K = args.k
    cfg = baseline_config(args.config, **{"algo.pathfinder_bc_iterations": K, **parse_overrides(args.overrides)})

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    tr = Trainer(cfg)
    eval_env = Pursuit_Env(cfg, num_envs=args.eval_envs, rank=10_000)

    def evaluation(label):
        stats = {}
        with torch.no_grad():
            evaluate(eval_env, tr.agent.actor, cfg, stats=stats)
        emit(dict(what="evaluation", at=label, iteration=tr.iteration, total_steps=tr.total_steps, **stats))

    emit(dict(what="run", config=args.config, K=K, envs=tr.num_envs, eval_envs=args.eval_envs, max_train_steps=cfg.algo.max_train_steps,
              steps_per_iteration=tr.num_envs * int(cfg.env.max_steps), cache=tr.agent.pathfinder_bc.cache, bc_lr=tr.agent.pathfinder_bc.lr))
    emit(dict(what="baseline", **pursuit_baseline.eval_baseline(cfg, "pathfinder", args.eval_envs)))
    evaluation("untrained")
    times = {"imitation": [], "ppo": []}
    for it in range(2 * K):
        _, exp_r = tr.iterate()
        torch.cuda.synchronize()
        rollout_ms, update_ms = tr.last_breakdown_ms()
        phase = "imitation" if tr.last_imitation is not None else "ppo"
        times[phase].append((rollout_ms, update_ms))
        rec = dict(what="iteration", iteration=tr.iteration, phase=phase, rollout_ms=rollout_ms, update_ms=update_ms, mean_return=exp_r,
                   critic_loss=tr.last_log[0])
        if tr.last_imitation is not None:
            rec.update({k: v for k, v in tr.last_imitation.items() if k not in ("phase", "critic_loss")})
        else:
            rec["actor_loss"] = tr.last_log[1]
        emit(rec)
        if tr.iteration in (K, 2 * K):
            evaluation("end of imitation" if tr.iteration == K else "end of ppo")
        elif tr.iteration % args.eval_every == 0:
            evaluation("every")
    med = lambda rows, i: statistics.median(r[i] for r in rows[2:]) if len(rows) > 2 else None
    emit(dict(what="iteration_cost", config=args.config, envs=tr.num_envs, dropped_per_phase=2,
              **{f"{p}_{n}_ms_median": med(rows, i) for p, rows in times.items() for i, n in ((0, "rollout"), (1, "update"))}))


if __name__ == "__main__":
    main()
