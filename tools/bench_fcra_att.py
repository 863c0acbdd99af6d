"""The FCRA hops' attention aggregator (ops.fcra_att, csrc/fcra_att.hpp), forward + backward, device-event times.  One process per line:
    python tools/bench_fcra_att.py --shape update --mode actor [--out profiles/fcra_att_kernel_times.jsonl]
  --shape update: the rows of a PPO mini-batch of BASELINE config 3 (410 episodes x 150 steps, P = 8: tools/nbr_probe.py's);
  --shape tick: one rollout tick's rows (32 768 environments)        --mode actor: adjacency at density 0.4;  --mode critic: ones
Each line carries three yardsticks measured in the same process on the same operands: the plain torch formula (ops.fcra_att_formula,
what CPU and float64 operands take), forward + backward; the mean aggregator ops.fcra_mean (forward only: it has no backward of its
own, the mean's gradient is the AGG GEMM's); and the byte floor -- forward: read y, write out; backward: read y, out, g, write dy --
as the achieved TB/s of the fused pair."""
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
    ap.add_argument("--episodes", type=int, default=410)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    P, E = 8, 128
    R = a.episodes * a.steps if a.shape == "update" else a.envs
    y = torch.randn(R, P, E, device="cuda", requires_grad=True)
    adj = None if a.mode == "critic" else (torch.rand(R, P, P, device="cuda") < 0.4).float()
    b = (torch.randn(E, device="cuda") * 0.1).requires_grad_()
    alpha = (torch.randn(E, 1, device="cuda") / E ** 0.5).requires_grad_()
    g = torch.randn(R, P, E, device="cuda")
    yd = y.detach()

    def fused():
        torch.autograd.grad(ops.fcra_att(y, adj, b, alpha), (y, b, alpha), g)

    def formula():
        torch.autograd.grad(ops.fcra_att_formula(y, adj, b, alpha), (y, b, alpha), g)

    def mean():
        ops.fcra_mean(z_critic=yd, bias=b, relu=True) if adj is None else ops.fcra_mean(z_actor=yd, adj=adj, bias=b, relu=True)

    calls = ops.fcra_att_calls
    ms = {"fused": timed(fused, a.warmup, a.iters)}
    assert ops.fcra_att_calls == calls + a.warmup + a.iters
    with torch.no_grad():
        ms["fused_fwd"] = timed(lambda: ops.fcra_att(yd, adj, b, alpha), a.warmup, a.iters)
    ms["torch"], ms["mean_fwd"] = timed(formula, a.warmup, a.iters), timed(mean, a.warmup, a.iters)
    floor_bytes = 6 * R * P * E * 4
    line = {"tool": "bench_fcra_att", "shape": a.shape, "mode": a.mode, "R": R, "P": P, "fused_ms": round(ms["fused"], 4),
            "fused_fwd_ms": round(ms["fused_fwd"], 4), "torch_ms": round(ms["torch"], 4), "mean_fwd_ms": round(ms["mean_fwd"], 4),
            "torch_over_fused": round(ms["torch"] / ms["fused"], 3), "fused_fwd_over_mean_fwd": round(ms["fused_fwd"] / ms["mean_fwd"], 3),
            "floor_bytes": floor_bytes, "fused_tb_s": round(floor_bytes / ms["fused"] / 1e9, 3),
            "fused_fwd_tb_s": round(2 * R * P * E * 4 / ms["fused_fwd"] / 1e9, 3), "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
