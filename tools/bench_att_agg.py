"""The attention aggregator (ops.att_agg3, csrc/att_agg.hpp), forward + backward, device-event times.  One process per line:
    python tools/bench_att_agg.py --shape update --mode actor [--out profiles/att_agg_kernel_times.jsonl]
  --shape update: B x T rows of the PPO update, P = 8, O = 176, q_div = T;   --shape tick: one rollout tick's rows, q_div = 1
  --mode actor: adjacency at --density;   --mode critic: ones
--density is a TOOL DEFAULT (0.1, as tools/bench_gnn_pairs.py), not a measured rollout statistic: the actor's time scales with it.
Each line carries two yardsticks measured in the same process on the same operands: the plain torch formula (ops.att_agg_formula, what
CPU and float64 operands take) and the mean aggregator ops.msg_agg3, both forward + backward."""
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
    ap.add_argument("--mode", choices=["actor", "critic"], default="actor")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    P, O, E = 8, 176, 128
    R, q_div = (a.batch * a.steps, a.steps) if a.shape == "update" else (a.envs, 1)
    critic = a.mode == "critic"
    p, e, o = torch.rand(R, P, 4, device="cuda") * 20, torch.rand(R, 1, 4, device="cuda") * 20, torch.rand(R // q_div, O, 4, device="cuda") * 20
    adj = [(torch.rand(R, P, k, device="cuda") < a.density).float() for k in (P, 1, O)]
    lins = [torch.nn.Linear(d, E).cuda() for d in (8, 4, 4)]
    prm = [t for lin in lins for t in (lin.weight, lin.bias)]
    alphas = [(torch.randn(E, 1, device="cuda") / E ** 0.5).requires_grad_() for _ in range(3)]
    d_y = torch.randn(R, P, 3, E, device="cuda")
    dense = [torch.ones_like(x) if critic else x for x in adj]
    rels = ((p, e.reshape(R, 4), 1), (e, None, 1), (o, None, q_div))

    def fused():
        torch.autograd.grad(ops.att_agg3(p, e, o, *adj, *prm, alphas, critic, None, q_div), prm + alphas, d_y)

    def formula():
        y = torch.stack([ops.att_agg_formula(p, q, ee, dense[r], lins[r].weight, lins[r].bias, alphas[r].reshape(-1), qd)
                         for r, (q, ee, qd) in enumerate(rels)], 2)
        torch.autograd.grad(y, prm + alphas, d_y)

    def mean():
        torch.autograd.grad(ops.msg_agg3(p, e, o, *adj, *prm, critic, None, q_div), prm, d_y)

    calls = ops.att_agg_calls
    ms = {"fused": timed(fused, a.warmup, a.iters)}
    assert ops.att_agg_calls == calls + a.warmup + a.iters
    ms["torch"], ms["mean"] = timed(formula, a.warmup, a.iters), timed(mean, a.warmup, a.iters)
    pairs = sum(int(x.numel() if critic else (x != 0).sum().item()) for x in adj)
    pairs8 = int(adj[0].numel() if critic else (adj[0] != 0).sum().item())
    # counted from the shapes: per pair and unit the layer (2 din), the score (2) and the weighted sum (2) forward; the backward's dm
    # (4), d_alpha (2), db (1) and dW (2 din).  The recomputation of z in the second pass and in the backward is not counted.
    flops = E * ((pairs - pairs8) * (4 * 4 + 11) + pairs8 * (4 * 8 + 11))
    line = {"tool": "bench_att_agg", "shape": a.shape, "mode": a.mode, "R": R, "P": P, "O": O, "q_div": q_div,
            "density": 1.0 if critic else a.density, "density_is_tool_default": not critic, "pairs": pairs, "fused_ms": round(ms["fused"], 4),
            "torch_ms": round(ms["torch"], 4), "mean_ms": round(ms["mean"], 4), "torch_over_fused": round(ms["torch"] / ms["fused"], 3),
            "fused_over_mean": round(ms["fused"] / ms["mean"], 3), "fused_useful_gflops": round(flops / ms["fused"] / 1e6, 1),
            "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
