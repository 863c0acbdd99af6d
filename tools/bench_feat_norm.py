"""The feature LayerNorm (csrc/layer_norm.hpp through ops.feat_norm / ops.feat_norm_train), actor and critic in one launch: forward, and
forward + backward, device-event times.  One process per line:
    python tools/bench_feat_norm.py --config cfg5 --shape rollout [--out profiles/feat_norm_kernel_times.jsonl]
  --shape rollout: the rows of a tick (runtime.num_envs x env.num_defender);  --shape minibatch: those of an update's mini-batch
  (round(num_envs / 10) episodes x env.max_steps x env.num_defender);  --rows N: any other count
Two yardsticks on the same tensors in the same process: torch's F.layer_norm (forward, and forward + autograd, per network), and the
bytes the kernels must move -- forward: read x, write y (1 KB a row and network); backward: read x and g, write dx (1.5 KB) -- as
achieved TB/s."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_multi_agent_reinforcement_learning_amd import ops  # noqa: E402
from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config  # noqa: E402
from tools.bench_fcra_att import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["cfg5", "cfg4_n2n"], default="cfg5")
    ap.add_argument("--shape", choices=["rollout", "minibatch"], default="minibatch")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    cfg = baseline_config(a.config)
    N, P, T = int(cfg.runtime.num_envs), int(cfg.env.num_defender), int(cfg.env.max_steps)
    R = a.rows or (N * P if a.shape == "rollout" else max(1, round(N / 10)) * T * P)
    E, eps, nets = 128, 1e-5, 2
    xs = [torch.randn(R, E, device="cuda", requires_grad=True) for _ in range(nets)]
    ws = [(1 + 0.1 * torch.randn(E, device="cuda")).requires_grad_() for _ in range(nets)]
    bs = [(0.1 * torch.randn(E, device="cuda")).requires_grad_() for _ in range(nets)]
    gs, outs = [torch.randn(R, E, device="cuda") for _ in range(nets)], [torch.empty(R, E, device="cuda") for _ in range(nets)]
    leaves = xs + ws + bs
    calls = ops.feat_norm_calls
    ms = {"fused": timed(lambda: torch.autograd.grad(ops.feat_norm_train(xs, ws, bs, eps), leaves, gs), a.warmup, a.iters)}
    ms["torch"] = timed(lambda: torch.autograd.grad([F.layer_norm(x, (E,), w, b, eps) for x, w, b in zip(xs, ws, bs)], leaves, gs), a.warmup, a.iters)
    with torch.no_grad():
        ms["fwd"] = timed(lambda: ops.feat_norm(xs, ws, bs, eps, outs), a.warmup, a.iters)
        ms["torch_fwd"] = timed(lambda: [F.layer_norm(x, (E,), w, b, eps) for x, w, b in zip(xs, ws, bs)], a.warmup, a.iters)
    assert ops.feat_norm_calls == calls + 2 * (a.warmup + a.iters)
    row = nets * R * E * 4
    line = {"tool": "bench_feat_norm", "config": a.config, "shape": "rows" if a.rows else a.shape, "R": R, "networks": nets,
            "fwd_ms": round(ms["fwd"], 4), "fwd_bwd_ms": round(ms["fused"], 4), "torch_fwd_ms": round(ms["torch_fwd"], 4),
            "torch_fwd_bwd_ms": round(ms["torch"], 4), "torch_over_fused_fwd": round(ms["torch_fwd"] / ms["fwd"], 3),
            "torch_over_fused_fwd_bwd": round(ms["torch"] / ms["fused"], 3), "fwd_tb_s": round(2 * row / ms["fwd"] / 1e9, 3),
            "fwd_bwd_tb_s": round(5 * row / ms["fused"] / 1e9, 3), "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
