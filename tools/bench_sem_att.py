"""The semantic-level attention tail (ops.sem_att_tail_train, csrc/sem_att.hpp), forward + backward, device-event times.
One process per line:
    python tools/bench_sem_att.py --shape update [--out profiles/sem_att_kernel_times.jsonl]
  --shape update: the semantic rows of tools/bench_pool.py's mini-batch (batch x steps rows, P = 8)
          tick:   one rollout tick's rows of both networks (2 x envs x P), forward only (ops.sem_att_tail against the formula and ops.encoder_tail)
Each line carries, measured in the same process on the same operands: the fused node, the plain torch formula (ops.sem_att_formula: what
CPU and float64 operands take) -- `torch_over_fused` >= 1 is the gated condition of DESIGN 7w at the update's shape --, and, recorded
only, the mean tail (ops.encoder_tail_train) with `fused_over_mean`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_multi_agent_reinforcement_learning_amd import ops  # noqa: E402


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):          # back to back
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["update", "tick"], default="update")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    P, E = 8, 128
    update = a.shape == "update"
    Rs = a.batch * a.steps * P if update else 2 * a.envs * P
    m3 = torch.randn(Rs, 3 * E, device="cuda").requires_grad_(update)
    agg, sem = torch.nn.Linear(E, E).cuda(), torch.nn.Linear(4 + 3 * E, E).cuda()
    alpha = (torch.randn(E, 1, device="cuda") / E ** 0.5).requires_grad_()
    add, g = torch.randn(Rs, E, device="cuda"), torch.randn(Rs, E, device="cuda")
    Ws = sem.weight[:, 4:]
    prm = [m3, agg.weight, agg.bias, sem.weight]
    if update:
        fns = {"fused": lambda: torch.autograd.grad(ops.sem_att_tail_train(m3, agg.weight, agg.bias, alpha, Ws, add.clone()), prm + [alpha], g),
               "torch": lambda: torch.autograd.grad(ops.sem_att_formula(m3, agg.weight, agg.bias, alpha, Ws, add.clone()), prm + [alpha], g),
               "mean": lambda: torch.autograd.grad(ops.encoder_tail_train(m3, agg.weight, agg.bias, Ws, add.clone()), prm, g)}
        assert ops.sem_att_tail_train_ok(m3, agg.weight, agg.bias, alpha, Ws, add), "the fused kernels would not run"
    else:
        fns = {"fused": lambda: ops.sem_att_tail(m3, agg.weight, agg.bias, alpha, Ws, add.clone()),
               "torch": lambda: ops.sem_att_formula(m3, agg.weight, agg.bias, alpha, Ws, add.clone()),
               "mean": lambda: ops.encoder_tail(m3, agg.weight, agg.bias, Ws, add.clone())}
    with torch.set_grad_enabled(update):
        if not update:
            assert ops.sem_att_tail_ok(m3, agg.weight, agg.bias, alpha, Ws, add), "the fused kernel would not run"
        ms = {k: timed(fn, a.warmup, a.iters) for k, fn in fns.items()}
    line = {"tool": "bench_sem_att", "shape": a.shape, "direction": "fwd+bwd" if update else "fwd", "Rs": Rs, **{k + "_ms": round(v, 4) for k, v in ms.items()},
            "torch_over_fused": round(ms["torch"] / ms["fused"], 3), "fused_over_mean": round(ms["fused"] / ms["mean"], 3),
            "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
