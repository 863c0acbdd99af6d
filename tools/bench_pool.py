"""The max-pool aggregators (ops.pool_agg3, csrc/pool_agg.hpp; ops.fcra_pool, csrc/fcra_pool.hpp), forward + backward, device-event times.
One process per line:
    python tools/bench_pool.py --op vertex --shape update --mode actor [--out profiles/pool_kernel_times.jsonl]
  --op vertex: the operands of tools/bench_att_agg.py (update: B x T rows, P = 8, O = 176, q_div = T; tick: one rollout tick's rows; the
               actor's adjacency at --density, a TOOL DEFAULT, not a rollout statistic)
  --op fcra:   the operands of tools/bench_fcra_att.py (update: 410 episodes x 150 steps, P = 8; tick: 32 768 environments; the actor's
               adjacency at density 0.4) and the byte floor of DESIGN 7u: 2 R P E floats forward, 6 R P E forward + backward
  --mode actor | critic (ones)
Each line carries, measured in the same process on the same operands: the plain torch formula (what CPU and float64 operands take),
forward + backward -- `torch_over_fused` >= 1 is the gated condition of DESIGN 7v at the update's shape --, and, recorded only, the
`mean` and `att` kernels (the FCRA mean forward only: its gradient is the AGG GEMM's)."""
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


def vertex(a):
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

    def formula():
        y = torch.stack([ops.pool_agg_formula(p, q, ee, dense[r], lins[r].weight, lins[r].bias, qd) for r, (q, ee, qd) in enumerate(rels)], 2)
        torch.autograd.grad(y, prm, d_y)
    fns = {"fused": lambda: torch.autograd.grad(ops.pool_agg3(p, e, o, *adj, *prm, critic, None, q_div), prm, d_y), "torch": formula,
           "mean": lambda: torch.autograd.grad(ops.msg_agg3(p, e, o, *adj, *prm, critic, None, q_div), prm, d_y),
           "att": lambda: torch.autograd.grad(ops.att_agg3(p, e, o, *adj, *prm, alphas, critic, None, q_div), prm + alphas, d_y)}
    pairs = sum(int(x.numel() if critic else (x != 0).sum().item()) for x in adj)
    return fns, {"R": R, "P": P, "O": O, "q_div": q_div, "density": 1.0 if critic else a.density, "density_is_tool_default": not critic, "pairs": pairs}


def fcra(a):
    P, E = 8, 128
    R = a.episodes * a.steps_fcra if a.shape == "update" else a.envs_fcra
    y = torch.randn(R, P, E, device="cuda", requires_grad=True)
    adj = None if a.mode == "critic" else (torch.rand(R, P, P, device="cuda") < 0.4).float()
    b = (torch.randn(E, device="cuda") * 0.1).requires_grad_()
    alpha = (torch.randn(E, 1, device="cuda") / E ** 0.5).requires_grad_()
    g, yd = torch.randn(R, P, E, device="cuda"), y.detach()
    fns = {"fused": lambda: torch.autograd.grad(ops.fcra_pool(y, adj, b), (y, b), g),
           "torch": lambda: torch.autograd.grad(ops.fcra_pool_formula(y, adj, b), (y, b), g),
           "fused_fwd": lambda: ops.fcra_pool(yd, adj, b),
           "mean_fwd": lambda: ops.fcra_mean(z_critic=yd, bias=b, relu=True) if adj is None else ops.fcra_mean(z_actor=yd, adj=adj, bias=b, relu=True),
           "att": lambda: torch.autograd.grad(ops.fcra_att(y, adj, b, alpha), (y, b, alpha), g)}
    return fns, {"R": R, "P": P, "floor_bytes": 6 * R * P * E * 4, "floor_bytes_fwd": 2 * R * P * E * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", choices=["vertex", "fcra"], default="vertex")
    ap.add_argument("--shape", choices=["update", "tick"], default="update")
    ap.add_argument("--mode", choices=["actor", "critic"], default="actor")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--episodes", type=int, default=410)
    ap.add_argument("--steps-fcra", type=int, default=150)
    ap.add_argument("--envs-fcra", type=int, default=32768)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    fns, line = (vertex if a.op == "vertex" else fcra)(a)
    calls = ops.pool_agg_calls + ops.fcra_pool_calls
    ms = {"fused": timed(fns["fused"], a.warmup, a.iters)}
    assert ops.pool_agg_calls + ops.fcra_pool_calls == calls + a.warmup + a.iters, "the fused kernels did not run"
    for name in fns:
        if name != "fused":
            with torch.set_grad_enabled(not name.endswith("_fwd")):
                ms[name] = timed(fns[name], a.warmup, a.iters)
    line = {"tool": "bench_pool", "op": a.op, "shape": a.shape, "mode": a.mode, **line, **{k + "_ms": round(v, 4) for k, v in ms.items()},
            "torch_over_fused": round(ms["torch"] / ms["fused"], 3), "fused_over_att": round(ms["fused"] / ms["att"], 3)}
    if a.op == "vertex":
        line["fused_over_mean"] = round(ms["fused"] / ms["mean"], 3)
    else:
        line.update(fused_fwd_over_mean_fwd=round(ms["fused_fwd"] / ms["mean_fwd"], 3), fused_tb_s=round(line["floor_bytes"] / ms["fused"] / 1e9, 3),
                    fused_fwd_tb_s=round(line["floor_bytes_fwd"] / ms["fused_fwd"] / 1e9, 3))
    line["device"] = torch.cuda.get_device_name(0)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
