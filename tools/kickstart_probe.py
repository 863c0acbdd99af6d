"""Launches the fused loss of algo.bc_coef and the two launches it replaces on one seeded mini-batch, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/kickstart_probe.py --kind gauss|cat [--mb --T --P --A --calls 200]

Defaults: the mini-batches of cfg5 (512 environments, direction mode) and cfg4_n2n (1024 environments); time-major mu / prob / values, a
third of the rows inactive.  Every launch writes its gradients in the forward call, so no backward pass is run."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from distributed_multi_agent_reinforcement_learning_amd import ops  # noqa: E402

DEFAULTS = {"gauss": (51, 200, 8, 4), "cat": (102, 100, 16, 9)}
EPS, ENT, COEF = 0.05, 0.05, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=tuple(DEFAULTS), required=True)
    for name in ("mb", "T", "P", "A"):
        ap.add_argument("--" + name, type=int, default=None)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kickstart_probe needs the GPU")
    mb, T, P, A = (getattr(args, n) if getattr(args, n) is not None else d for n, d in zip(("mb", "T", "P", "A"), DEFAULTS[args.kind]))
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")
    v = r(T, mb, P, 1).permute(1, 0, 2, 3)[..., 0]
    active = (torch.rand(mb, T, P, generator=g, device="cuda") < 0.67).float()
    lp_old, adv, vo, vt = r(mb, T, P) * 0.05, r(mb, T, P), v + r(mb, T, P) * 0.1, r(mb, T, P)
    tail = (active, vo, vt, EPS)
    sums, diff = torch.zeros(ops.KICK_SUMS, dtype=torch.float64, device="cuda"), 0.0
    if args.kind == "gauss":
        mu, ls = (r(T, mb, P, A) * 0.5).permute(1, 0, 2, 3), torch.zeros(A, device="cuda")
        action, target = mu + r(mb, T, P, A), mu + r(mb, T, P, A)
        lp_old = lp_old + torch.distributions.Normal(mu, torch.exp(ls)).log_prob(action).sum(-1)
        pol = dict(log_std_min=-5.0, log_std_max=2.0, squash="direction" if A == 4 else "clip")
        bc = dict(fit_std=False, wrap0=A != 4, metric="angle" if A == 4 else "mse")
        fused = lambda: ops.ppo_bc_loss_gauss(mu, ls, action, target, v, lp_old, adv, *tail, ENT, COEF, True, sums=sums, **pol, **bc)
        ppo = lambda: ops.ppo_loss_gauss_ex(mu, ls, action, v, lp_old, adv, *tail, ENT, True, **pol)
        imit = lambda: ops.bc_loss_gauss(mu, ls, target, v, *tail, True, log_std_min=-5.0, log_std_max=2.0, **bc)
    else:
        prob = (torch.rand(T, mb, P, A, generator=g, device="cuda") + 0.02).permute(1, 0, 2, 3)
        action, label = (torch.randint(0, A, (mb, T, P), generator=g, device="cuda").float() for _ in range(2))
        lp_old = lp_old + torch.log(prob / prob.sum(-1, keepdim=True)).gather(-1, action.long()[..., None])[..., 0]
        fused = lambda: ops.ppo_bc_loss_cat(prob, action, label, v, lp_old, adv, *tail, ENT, COEF, True, sums=sums)
        ppo = lambda: ops.ppo_loss_prob(prob, action, v, lp_old, adv, *tail, ENT, True)
        imit = lambda: ops.bc_loss_cat(prob, label, v, *tail, True)
    for _ in range(args.calls):
        diff = max(diff, abs(fused()[0].item() - (ppo()[0].item() + COEF * imit()[0].item())))
    print(f"{args.kind}: {mb * T * P} rows (mb {mb}, T {T}, P {P}), A {A}, {args.calls} calls of each launch; |fused - (ppo + coef bc)| <= {diff:.3e}")


if __name__ == "__main__":
    main()
