"""Command-line entry of the training loop -- the role of the reference's main.py / MAPPO_parallel_main.py.

    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg3 --iterations 10
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m distributed_multi_agent_reinforcement_learning_amd.main

`--config` is one of the BASELINE configurations (cfg1..cfg5) or the path of a reference-schema config.yaml;
dotted overrides follow as KEY=VALUE (e.g. runtime.num_envs=1024 algo.depth=1).  cfg5 (or runtime.env=e3d) trains the
diagonal-Gaussian MAPPO on env_3d (e3d_agent.train_e3d); cfg4_n2n (or runtime.env=n2n) the DHGN MAPPO on env_n2n
(n2n_agent.train_n2n):

    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg5 --iterations 50
    python -m distributed_multi_agent_reinforcement_learning_amd.main --config cfg4_n2n --iterations 5
"""
import argparse
import ast

from .config import baseline_config, load_config
from .e3d_agent import train_e3d
from .n2n_agent import train_n2n
from .trainer import train_agent_multiprocessing

BASELINES = ("cfg1", "cfg2", "cfg3", "cfg4", "cfg5", "cfg4_n2n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--iterations", type=int, default=None, help="stop after this many iterations (default: max_train_steps)")
    ap.add_argument("--eval-envs", type=int, default=64)
    ap.add_argument("--eval-every", type=int, default=1)
    ap.add_argument("overrides", nargs="*", help="dotted overrides KEY=VALUE")
    args = ap.parse_args(argv)
    ov = {}
    for item in args.overrides:
        k, _, v = item.partition("=")
        try:
            ov[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            ov[k] = v
    cfg = baseline_config(args.config, **ov) if args.config in BASELINES else load_config(args.config, **ov)
    if str(cfg.runtime.get("env", "pursuit")) == "e3d":
        return train_e3d(cfg, max_iterations=args.iterations, num_eval_envs=args.eval_envs, eval_every=args.eval_every)
    if str(cfg.runtime.get("env", "pursuit")) == "n2n":
        return train_n2n(cfg, max_iterations=args.iterations, num_eval_envs=args.eval_envs, eval_every=args.eval_every)
    return train_agent_multiprocessing(cfg, max_iterations=args.iterations, num_eval_envs=args.eval_envs, eval_every=args.eval_every)


if __name__ == "__main__":
    main()
