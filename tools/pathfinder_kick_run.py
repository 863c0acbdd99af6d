"""Teacher-regularised PPO on the flagship as one run (measurement 3).

    python tools/pathfinder_kick_run.py [--config cfg2] [--k 16] [--coef 1.0] [--decay 0.9] [--eval-envs 2048] [--eval-every 10]
                                        [--out FILE.jsonl] [KEY=VALUE ...]

tools/pathfinder_bc_run.py's run -- K imitation iterations and then K PPO iterations on one rank, seed 0 -- with the PPO iterations
under algo.pathfinder_bc_coef (lambda_j = coef decay^j).  One JSON line per iteration (phase, rollout ms, update ms, the imitation or
kickstart log entries), a greedy evaluation with the five keys of evaluate(stats={}) before the first iteration, every --eval-every
iterations and at the end of either phase, and the pathfinder's own record on the same kind of evaluation environment."""
import argparse
import json
import os
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
    ap.add_argument("--coef", type=float, default=1.0)
    ap.add_argument("--decay", type=float, default=0.9)
    ap.add_argument("--eval-envs", type=int, default=2048)
    ap.add_argument("--eval-every", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args()
    K = args.k
    cfg = baseline_config(args.config, **{"algo.pathfinder_bc_iterations": K, "algo.pathfinder_bc_coef": args.coef,
                                          "algo.pathfinder_bc_coef_decay": args.decay, **parse_overrides(args.overrides)})

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

    kick = tr.agent.pathfinder_kick
    emit(dict(what="run", config=args.config, K=K, envs=tr.num_envs, eval_envs=args.eval_envs, max_train_steps=cfg.algo.max_train_steps,
              steps_per_iteration=tr.num_envs * int(cfg.env.max_steps), cache=tr.agent.pathfinder_bc.cache, bc_lr=tr.agent.pathfinder_bc.lr,
              coef=kick.coef, coef_decay=kick.decay, coef_iterations=kick.iterations, labeller=kick.labeller))
    emit(dict(what="baseline", **pursuit_baseline.eval_baseline(cfg, "pathfinder", args.eval_envs)))
    evaluation("untrained")
    for it in range(2 * K):
        _, exp_r = tr.iterate()
        torch.cuda.synchronize()
        rollout_ms, update_ms = tr.last_breakdown_ms()
        phase = "imitation" if tr.last_imitation is not None else "ppo"
        rec = dict(what="iteration", iteration=tr.iteration, phase=phase, rollout_ms=rollout_ms, update_ms=update_ms, mean_return=exp_r,
                   critic_loss=tr.last_log[0])
        if tr.last_imitation is not None:
            rec.update({k: v for k, v in tr.last_imitation.items() if k not in ("phase", "critic_loss")})
        else:
            rec["actor_loss"] = tr.last_log[1]
            rec.update(tr.last_kick or {})
        emit(rec)
        if tr.iteration in (K, 2 * K):
            evaluation("end of imitation" if tr.iteration == K else "end of ppo")
        elif tr.iteration % args.eval_every == 0:
            evaluation("every")


if __name__ == "__main__":
    main()
