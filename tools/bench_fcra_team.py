"""The large-team FCRA aggregator (csrc/fcra_team.hpp through ops.fcra_att at P > 16), forward and forward + backward, device-event times.
One process per line:
    python tools/bench_fcra_team.py --P 64 --mode actor [--out profiles/fcra_team_kernel_times.jsonl]
  rows: --episodes x --steps of a PPO mini-batch (default 64 x 150);  --mode actor: adjacency at density 0.4;  --mode critic: ones
Two yardsticks on the same operands in the same process: the plain torch formula (ops.fcra_att_formula), and the bytes the kernels must
move -- forward: read y, write out; backward: read y, out, g, write dy -- as achieved TB/s.
  --vertex: instead, the price of the vertex-level `mean` through the attention kernels with a zero alpha (DHGN above 16 pursuers) against
  the `mean` message kernels, forward, at P = 16 where both exist."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_multi_agent_reinforcement_learning_amd import ops  # noqa: E402
from tools.bench_fcra_att import timed  # noqa: E402


def vertex(a, R):
    P, O, E = 16, 20, 128
    p, e, o = [torch.rand(R, k, 4, device="cuda") * 20 for k in (P, 1, O)]
    adjs = [(torch.rand(R, P, k, device="cuda") < 0.4).float() for k in (P, 1, O)]
    prm = [t for din in (8, 4, 4) for t in (torch.randn(E, din, device="cuda") * 0.1, torch.randn(E, device="cuda") * 0.1)]
    zero = torch.zeros(E, device="cuda")
    with torch.no_grad():
        mean = timed(lambda: ops.msg_agg3(p, e, o, *adjs, *prm, False), a.warmup, a.iters)
        att = timed(lambda: ops.att_agg3(p, e, o, *adjs, *prm, [zero] * 3, False), a.warmup, a.iters)
    return {"tool": "bench_fcra_team", "what": "vertex mean through att, forward", "R": R, "P": P, "mean_ms": round(mean, 4), "att_zero_alpha_ms": round(att, 4),
            "att_over_mean": round(att / mean, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=64)
    ap.add_argument("--mode", choices=["actor", "critic"], default="actor")
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--vertex", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    P, E, R = a.P, 128, a.episodes * a.steps
    if a.vertex:
        line = vertex(a, R)
    else:
        assert P > ops.FCRA_TEAM_MIN_P
        y = torch.randn(R, P, E, device="cuda", requires_grad=True)
        adj = None if a.mode == "critic" else (torch.rand(R, P, P, device="cuda") < 0.4).float()
        b = (torch.randn(E, device="cuda") * 0.1).requires_grad_()
        alpha = (torch.randn(E, 1, device="cuda") / E ** 0.5).requires_grad_()
        g, yd = torch.randn(R, P, E, device="cuda"), y.detach()
        calls = ops.fcra_team_calls
        ms = {"fused": timed(lambda: torch.autograd.grad(ops.fcra_att(y, adj, b, alpha), (y, b, alpha), g), a.warmup, a.iters)}
        assert ops.fcra_team_calls == calls + a.warmup + a.iters
        with torch.no_grad():
            ms["fwd"] = timed(lambda: ops.fcra_att(yd, adj, b, alpha), a.warmup, a.iters)
            ms["torch_fwd"] = timed(lambda: ops.fcra_att_formula(yd, adj, b, alpha), a.warmup, a.iters)
        ms["torch"] = timed(lambda: torch.autograd.grad(ops.fcra_att_formula(y, adj, b, alpha), (y, b, alpha), g), a.warmup, a.iters)
        vec = R * P * E * 4
        line = {"tool": "bench_fcra_team", "mode": a.mode, "R": R, "P": P, "fwd_ms": round(ms["fwd"], 4), "fwd_bwd_ms": round(ms["fused"], 4),
                "torch_fwd_ms": round(ms["torch_fwd"], 4), "torch_fwd_bwd_ms": round(ms["torch"], 4), "torch_over_fused": round(ms["torch"] / ms["fused"], 3),
                "fwd_tb_s": round(2 * vec / ms["fwd"] / 1e9, 3), "fwd_bwd_tb_s": round(6 * vec / ms["fused"] / 1e9, 3)}
    line["device"] = torch.cuda.get_device_name(0)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
