"""The attention-pooled team context (`algo.critic_team_pool`) in plain torch, group by group: the specification the kernels of
csrc/team_pool.hpp and ops.team_pool_formula are held to.  Callable in any dtype; differentiable."""
import torch


def team_pool(feat, live, score, gate):
    """feat (G, P, E), live (G, P) non-zero = live, score / gate (E,) -> out (G, P, E):
    s_j = score . f_j, w = softmax of s over the live j (maximum subtracted), c = sum_live w_j f_j (nobody live: 0), out_i = f_i + gate c"""
    out = []
    for f, on in zip(feat, live != 0):
        c = torch.zeros_like(f[0])
        if on.any():
            fl = f[on]
            s = fl @ score
            e = torch.exp(s - s.max().detach())
            c = ((e / e.sum()).unsqueeze(-1) * fl).sum(0)
        out.append(f + gate * c)
    return torch.stack(out)
