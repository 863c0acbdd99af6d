"""The critic's team pool (csrc/team_pool.hpp through ops.team_pool / ops.team_pool_train): forward, and forward + backward, device-event
times.  One process per line:
    python tools/bench_team_pool.py --config cfg5 --shape minibatch [--out profiles/team_pool_kernel_times.jsonl]
  --shape rollout: the groups of a tick (runtime.num_envs);  --shape minibatch: those of an update's mini-batch (round(num_envs / 10)
  episodes x env.max_steps);  --groups N / --pursuers P: any other shape;  --heads H: algo.critic_team_pool_heads (2, 4, 8: the kernels of
  csrc/team_pool_heads.hpp, with the one-head kernels on the same tensors beside them as h1_*)
Two yardsticks on the same tensors in the same process: the torch formula (ops.team_pool_formula, forward, and forward + autograd), and
the bytes the kernels must move -- forward: read feat, write out (1 KB a row); backward: read feat and g, write d feat (1.5 KB) -- as
achieved TB/s."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_multi_agent_reinforcement_learning_amd import ops  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config  # noqa: E402
from tools.bench_fcra_att import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["cfg5", "cfg4_n2n"], default="cfg5")
    ap.add_argument("--shape", choices=["rollout", "minibatch"], default="minibatch")
    ap.add_argument("--groups", type=int, default=0)
    ap.add_argument("--pursuers", type=int, default=0)
    ap.add_argument("--heads", type=int, choices=list(ops.TEAM_POOL_HEADS), default=1)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    cfg = baseline_config(a.config)
    N, P, T = int(cfg.runtime.num_envs), a.pursuers or int(cfg.env.num_defender), int(cfg.env.max_steps)
    G = a.groups or (N if a.shape == "rollout" else max(1, round(N / 10)) * T)
    E = 128
    feat = torch.randn(G, P, E, device="cuda", requires_grad=True)
    live = (torch.rand(G, P, device="cuda") < 0.8).float()
    score, gate = [(0.1 * torch.randn(E, device="cuda")).requires_grad_() for _ in range(2)]
    g, out = torch.randn(G, P, E, device="cuda"), torch.empty(G, P, E, device="cuda")
    leaves = (feat, score, gate)
    calls = ops.team_pool_calls
    H = a.heads
    ms = {"fused": timed(lambda: torch.autograd.grad(ops.team_pool_train(feat, live, score, gate, heads=H), leaves, g), a.warmup, a.iters)}
    ms["torch"] = timed(lambda: torch.autograd.grad(ops.team_pool_formula(feat, live, score, gate, heads=H), leaves, g), a.warmup, a.iters)
    if H != 1:
        ms["h1"] = timed(lambda: torch.autograd.grad(ops.team_pool_train(feat, live, score, gate), leaves, g), a.warmup, a.iters)
    with torch.no_grad():
        ms["fwd"] = timed(lambda: ops.team_pool(feat, live, score, gate, out, heads=H), a.warmup, a.iters)
        ms["torch_fwd"] = timed(lambda: ops.team_pool_formula(feat, live, score, gate, heads=H), a.warmup, a.iters)
        if H != 1:
            ms["h1_fwd"] = timed(lambda: ops.team_pool(feat, live, score, gate, out), a.warmup, a.iters)
    assert ops.team_pool_calls == calls + (2 if H == 1 else 4) * (a.warmup + a.iters)
    rows = G * P * E * 4
    line = {"tool": "bench_team_pool", "config": a.config, "shape": "groups" if a.groups else a.shape, "G": G, "P": P, "heads": H,
            "fwd_ms": round(ms["fwd"], 4), "fwd_bwd_ms": round(ms["fused"], 4), "torch_fwd_ms": round(ms["torch_fwd"], 4),
            "torch_fwd_bwd_ms": round(ms["torch"], 4), "torch_over_fused_fwd": round(ms["torch_fwd"] / ms["fwd"], 3),
            "torch_over_fused_fwd_bwd": round(ms["torch"] / ms["fused"], 3), "fwd_tb_s": round(2 * rows / ms["fwd"] / 1e9, 3),
            "fwd_bwd_tb_s": round(5 * rows / ms["fused"] / 1e9, 3), "device": torch.cuda.get_device_name(0)}
    if H != 1:
        line.update(h1_fwd_ms=round(ms["h1_fwd"], 4), h1_fwd_bwd_ms=round(ms["h1"], 4), fwd_over_h1=round(ms["fwd"] / ms["h1_fwd"], 3),
                    fwd_bwd_over_h1=round(ms["fused"] / ms["h1"], 3))
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
