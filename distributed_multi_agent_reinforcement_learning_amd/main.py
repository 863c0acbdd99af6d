"""Command-line entry of the training loop -- the role of the reference's main.py / MAPPO_parallel_main.py.

    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg3 --iterations 10
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m distributed_multi_agent_reinforcement_learning_amd.main

`--config` is one of the BASELINE configurations (cfg1..cfg5) or the path of a reference-schema config.yaml;
dotted overrides follow as KEY=VALUE (e.g. runtime.num_envs=1024 algo.depth=1).  cfg5 (or runtime.env=e3d) trains the
diagonal-Gaussian MAPPO on env_3d (e3d_agent.train_e3d); cfg4_n2n (or runtime.env=n2n) the DHGN MAPPO on env_n2n
(n2n_agent.train_n2n):

    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg5 --iterations 50
    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg4_n2n --iterations 5

Run protocol (all three environments): `--save-resume DIR` writes every rank's resume bundle DIR/resume_rank{r}.pt after each
iteration, `--resume DIR` continues from them.  `--evaluate CWD` (env_3d and env_n2n) loads the final weights algo.save_cwd held
(save_model), runs one greedy evaluation on --eval-envs environments, prints its JSON line and exits without training:

    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg5 --iterations 50 --save-resume ckpt
    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg5 --iterations 100 --resume ckpt --save-resume ckpt
    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg5 --evaluate ./model

`--baseline guidance` (env_3d and env_n2n) needs no model: it runs the scripted lead-pursuit pursuers (guidance.py, DESIGN.md section 7e;
runtime.guidance_lead / guidance_sep_range / guidance_sep_gain) for one episode on --eval-envs environments of the evaluation seeds and
prints the JSON keys of `--evaluate`, the yardstick to read a training log against:

    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg5 --baseline guidance --eval-envs 2048

`--baseline pathfinder` and `--baseline demon` are the same for the pursuit configurations (cfg1..cfg4): one episode of the scripted
path-finding pursuers (pursuit_baseline.py; runtime.pathfinder_lead / pathfinder_sep_range / pathfinder_clearance),
or of the reference's wall-blind `demon`, on --eval-envs environments of the evaluator's seeds; one JSON line with eval_return,
eval_capture_rate, eval_first_contact, eval_contact_steps and eval_collision_steps:

    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg2 --baseline pathfinder --eval-envs 2048
    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg2 --baseline demon --eval-envs 2048

algo.pathfinder_bc_iterations=K (cfg1..cfg4) makes the first K iterations an imitation warm start from the path-finding pursuers
(pursuit_imitation.py; algo.pathfinder_bc_beta / pathfinder_bc_beta_decay / pathfinder_bc_lr,
runtime.pathfinder_cache); each prints one JSON line with phase, bc_beta, bc_loss, bc_accuracy, critic_loss and pathfinder_hit_rate:

    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg2 algo.pathfinder_bc_iterations=60 runtime.eval_baseline=pathfinder

algo.pathfinder_bc_coef=C (cfg1..cfg4, with or without a warm start) keeps the imitation term in the PPO loss with lambda_j = C
pathfinder_bc_coef_decay^j in PPO iteration j, cut off after pathfinder_bc_coef_iterations when that is > 0 (pursuit_imitation.py, DESIGN.md
section 7p; runtime.pathfinder_labeller=episode|tick); each such iteration prints one JSON line with bc_coef, bc_aux_loss, bc_accuracy
and pathfinder_build_rate:

    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg2 algo.pathfinder_bc_iterations=16 algo.pathfinder_bc_coef=1.0 algo.pathfinder_bc_coef_decay=0.9
"""
import argparse
import json

import torch

from .config import baseline_config, load_config, parse_overrides
from . import e3d_agent, n2n_agent
from .e3d_agent import E3dTrainer, train_e3d
from .guidance import BASELINES as SCRIPTED_BASELINES
from .n2n_agent import N2nTrainer, train_n2n
from .particle_agent import episode_triple
from .pursuit_baseline import BASELINES as PURSUIT_BASELINES
from .trainer import train_agent_multiprocessing

BASELINES = ("cfg1", "cfg2", "cfg3", "cfg4", "cfg5", "cfg4_n2n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--iterations", type=int, default=None, help="stop after this many iterations (default: max_train_steps)")
    ap.add_argument("--eval-envs", type=int, default=64)
    ap.add_argument("--eval-every", type=int, default=1)
    ap.add_argument("--save-resume", metavar="DIR", default=None, help="write DIR/resume_rank{r}.pt after every iteration")
    ap.add_argument("--resume", metavar="DIR", default=None, help="load DIR/resume_rank{r}.pt before the first iteration")
    ap.add_argument("--evaluate", metavar="CWD", default=None,
                    help="env_3d / env_n2n: evaluate the weights saved under CWD on --eval-envs environments and exit")
    ap.add_argument("--baseline", choices=SCRIPTED_BASELINES + PURSUIT_BASELINES, default=None,
                    help="run the scripted pursuers on --eval-envs environments of the evaluation seeds and exit (no model): guidance on "
                         "env_3d / env_n2n, pathfinder or demon on the pursuit configurations")
    ap.add_argument("overrides", nargs="*", help="dotted overrides KEY=VALUE")
    args = ap.parse_args(argv)
    ov = parse_overrides(args.overrides)
    cfg = baseline_config(args.config, **ov) if args.config in BASELINES else load_config(args.config, **ov)
    env = str(cfg.runtime.get("env", "pursuit"))
    if args.baseline in PURSUIT_BASELINES:
        if env in ("e3d", "n2n"):
            ap.error(f"--baseline {args.baseline} is for the pursuit configurations (cfg1..cfg4); runtime.env {env} takes --baseline guidance")
        return baseline_pursuit(cfg, args.baseline, args.eval_envs)
    if args.baseline is not None:
        if env not in ("e3d", "n2n"):
            ap.error("--baseline guidance is for runtime.env e3d and n2n (cfg5, cfg4_n2n); the pursuit configurations take "
                     "--baseline pathfinder or --baseline demon")
        return baseline_guidance(cfg, env, args.eval_envs)
    if args.evaluate is not None:
        if env not in ("e3d", "n2n"):
            ap.error("--evaluate is for runtime.env e3d and n2n (cfg5, cfg4_n2n)")
        return evaluate_saved(E3dTrainer if env == "e3d" else N2nTrainer, cfg, args.evaluate, args.eval_envs)
    kw = dict(max_iterations=args.iterations, num_eval_envs=args.eval_envs, eval_every=args.eval_every)
    if args.save_resume is not None:
        kw["save_resume"] = args.save_resume
    if args.resume is not None:
        kw["resume"] = args.resume
    if env == "e3d":
        return train_e3d(cfg, **kw)
    if env == "n2n":
        return train_n2n(cfg, **kw)
    return train_agent_multiprocessing(cfg, **kw)


def evaluate_saved(trainer_cls, cfg, cwd, num_eval_envs):
    """one synchronous greedy evaluation (trainer.evaluate: the eval seeds of a training run) of the weights save_model wrote under
    cwd; rank 0 prints the eval keys as one JSON line"""
    tr = trainer_cls(cfg, num_eval_envs=num_eval_envs)
    tr.agent.load_model(cwd)
    res = tr.evaluate()
    if tr.rank == 0:
        print(json.dumps(res), flush=True)
    return res


def baseline_guidance(cfg, env_kind, num_eval_envs):
    """one episode of the scripted pursuers on num_eval_envs environments of the evaluation seeds (seed + 10^6 + n, the environments
    trainer.evaluate starts from); prints the keys of --evaluate as one JSON line.  No trainer, no model, no process group."""
    mod = e3d_agent if env_kind == "e3d" else n2n_agent
    env = mod.make_env(cfg, int(num_eval_envs), 0, "cuda", seed_offset=10 ** 6, training=False)
    ret, captured, length = episode_triple(mod.guidance_episode(env))
    r, c, l = torch.stack((ret.mean(), captured.float().mean(), length.mean())).tolist()
    res = dict(eval_return=r, eval_capture_rate=c, eval_episode_length=l)
    print(json.dumps(res), flush=True)
    return res


def baseline_pursuit(cfg, policy, num_eval_envs):
    """one episode of the scripted pursuers of a pursuit configuration on num_eval_envs environments with the evaluator's seed rule
    (Pursuit_Env(cfg, num_envs, rank=10_000), the environments EvaluatorProc starts from); prints the five keys as one JSON line.  No
    model, no process group."""
    from .pursuit_baseline import scripted_episode
    from .pursuit_env import Pursuit_Env
    res = scripted_episode(Pursuit_Env(cfg, num_envs=int(num_eval_envs), rank=10_000), cfg, policy)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
