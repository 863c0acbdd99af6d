"""A/B of the message kernels of one cfg2 mini-batch and of one rollout tick on REAL rollout data, in one process: the library's switch
(dhgn_msg_full_team) 0 = generic instantiations, 1 = full-team instantiations, alternating for three rounds, event-timed; asserts that every
output and parameter gradient is the same bits under both.   python3 tools/msg_full_team_ab.py   (profiles/r21_msg_full_ab_probe.txt)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
from distributed_multi_agent_reinforcement_learning_amd.trainer import Trainer
from distributed_multi_agent_reinforcement_learning_amd import ops

cfg = baseline_config("cfg2")
tr = Trainer(cfg)
ag, env = tr.agent, tr.env
_, rb, _ = ag.explore_env(env, 1)
batch = rb.get_training_data(ag.device) if hasattr(rb, "get_training_data") else rb.buffer
N, T, P = batch["r"].shape
mb = tr.mini_batch_size
R = mb * T
E = ag.embedding_dim
M = ag.actor.shared_net.MSG_layers
p = batch["p_state"][:mb].reshape(R, P, -1)
e = batch["e_state"][:mb].reshape(R, 1, -1)
o = rb.o_static[:mb]
adj_p = batch["p_adj"][:mb].reshape(R, P, P)
adj_e = batch["e_adj"][:mb].reshape(R, P, 1)
adj_o = batch["o_adj_bits"][:mb].reshape(R, P, -1)
print(f"R={R} P={P} K={o.shape[1]} E={E} adj_p density {adj_p.mean().item():.3f} adj_e {adj_e.mean().item():.3f}", flush=True)
L = ops.load_library()
wb = [t.detach().clone().requires_grad_(True) for t in (M[0].weight, M[0].bias, M[1].weight, M[1].bias, M[2].weight, M[2].bias)]
ga, gc = torch.randn(R, P, 3, E, device=p.device), torch.randn(R, P, 3, E, device=p.device)
st = ag._rstate
ob = st._obs()
wr = [t.detach() for t in wb]


def ev_time(fn, n):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def fwd():
    with torch.enable_grad():
        return ops.msg_agg3_pair_train(p, e, o, adj_p, adj_e, adj_o, *wb, q_div=T)


def tick():
    with torch.no_grad():
        ops.msg_agg3_pair(ob["p_state"], ob["e_state"], ob["o_state"], ob["p_adj"], ob["e_adj"], ob["o_adj_bits"], *wr, ob["o_kvalid"], 1)


res = {}
ref = None
for rnd in range(3):
    for setting in (0, 1):
        ops._msg_full_team_set = bool(setting)
        ops.MSG_FULL_TEAM = bool(setting)
        L.dhgn_msg_full_team(setting)
        out = fwd()
        g = torch.autograd.grad(out, wb, (ga, gc), retain_graph=True)
        vals = [out[0].detach().clone(), out[1].detach().clone()] + [x.clone() for x in g]
        if ref is None:
            ref = vals
        else:
            assert all(torch.equal(x, y) for x, y in zip(vals, ref)), f"setting {setting}: results differ from the generic kernels"
        t_f = ev_time(fwd, 5)
        t_b = ev_time(lambda: torch.autograd.grad(out, wb, (ga, gc), retain_graph=True), 5)
        t_t = ev_time(tick, 30)
        res.setdefault(setting, []).append((t_f, t_b, t_t))
        print(f"round {rnd} setting {setting}: update fwd (pair01 + sorted) {t_f:8.1f} us  bwd (4 kernels + reduces) {t_b:8.1f} us  rollout tick {t_t:6.1f} us", flush=True)
        del out, g
for s, v in res.items():
    v = v[1:]   # round 0 warms the allocator (the sorted kernels' tables): not in the means
    print(f"setting {s}: mean of rounds 1.. fwd {sum(x[0] for x in v) / len(v):8.1f}  bwd {sum(x[1] for x in v) / len(v):8.1f}  tick {sum(x[2] for x in v) / len(v):6.1f}")
print("bit-identical across settings: yes")
