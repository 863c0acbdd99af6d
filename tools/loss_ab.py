"""A/B of the fused loss launches between two builds of libmappo_ops.so in ONE process (boxes of the pool differ by a few percent, see
tools/ab_switch.py): the public wrappers of ops run once per case on this tree's library with the C calls recorded, then the same entry
points are called on the same buffers through the other library (built from the parent commit into a scratch directory) and this one,
alternating call by call, between hip events.  The other library is loaded twice (two copies of the file): the gap between its two
medians is the noise of the method.      python tools/loss_ab.py /path/to/parent/libmappo_ops.so [pairs]
Rows: the mini-batches of the trainers (a tenth of the environments): cfg2 410 x 150 x 8, cfg5 51 x 200 x 8, cfg4_n2n 102 x 100 x 16,
as time-major views."""
import os
import shutil
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_multi_agent_reinforcement_learning_amd import ops  # noqa: E402

DEV = "cuda:0"
CFG2, CFG5, N2N = (410, 150, 8), (51, 200, 8), (102, 100, 16)


def load(path):
    ops._lib, ops.lib_path = None, (lambda: path)
    return ops.load_library()


class Recorder:
    """the library, with every loss entry point's calls noted as (name, arguments)"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not (name.endswith("_fwd_bwd") or name.endswith("_fwd_bwd_diag")):
            return fn

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def tm(rows, *tail, gen):
    """a (mb, T, P, ...) time-major view of seeded values"""
    mb, T, P = rows
    return torch.randn(T, mb, P, *tail, generator=gen).to(DEV).transpose(0, 1)


def cases():
    g = torch.Generator().manual_seed(0)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)

    def rows(r):
        return dict(v=tm(r, gen=g), lo=tm(r, gen=g).contiguous() * 0.3, adv=tm(r, gen=g).contiguous(),
                    act=(torch.rand(*r, generator=g) < 0.8).float().to(DEV), vo=tm(r, gen=g).contiguous(), vt=tm(r, gen=g).contiguous())

    def cat(r, A):
        return (tm(r, A, gen=g).abs() + 0.05, torch.randint(0, A, r, generator=g).float().to(DEV), torch.randint(0, A, r, generator=g).float().to(DEV))

    def gauss(r, A, state):
        ls = tm(r, A, gen=g) * 0.5 if state else torch.randn(A, generator=g).to(DEV) * 0.5
        return tm(r, A, gen=g), ls, tm(r, A, gen=g).contiguous(), tm(r, A, gen=g).contiguous()

    for diag in (False, True):
        d = rows(CFG2)
        yield f"ppo_loss cfg2 diag={int(diag)}", lambda d=d, diag=diag: ops.ppo_loss(d["lo"], d["adv"], d["v"], d["lo"], d["adv"], d["act"], d["vo"], d["vt"], 0.2, 0.01,
                                                                                  True, f64(8) if diag else None)
        p, a, _ = cat(CFG2, 9)
        yield f"ppo_loss_prob cfg2 A=9 diag={int(diag)}", lambda d=d, p=p, a=a, diag=diag: ops.ppo_loss_prob(p, a, d["v"], d["lo"] - 2.2, d["adv"], d["act"], d["vo"], d["vt"],
                                                                                                        0.2, 0.01, True, f64(8) if diag else None)
    d = rows(CFG5)
    mu, ls, u, t = gauss(CFG5, 3, False)
    yield "ppo_loss_gauss cfg5 A=3", lambda: ops.ppo_loss_gauss(mu, ls, u, d["v"], d["lo"] - 4, d["adv"], d["act"], d["vo"], d["vt"], 0.2, 0.01)
    yield "ppo_loss_gauss_ex cfg5 param A=3 clip", lambda: ops.ppo_loss_gauss_ex(mu, ls, u, d["v"], d["lo"] - 4, d["adv"], d["act"], d["vo"], d["vt"], 0.2, 0.01, True,
                                                                                   -1.0, 0.5, "clip")
    for A, squash in ((3, "tanh"), (4, "direction")):
        mu_s, ls_s, u_s, t_s = gauss(CFG5, A, True)
        for diag in (False, True):
            yield f"ppo_loss_gauss_ex cfg5 state A={A} {squash} diag={int(diag)}", lambda m=mu_s, l=ls_s, u_=u_s, q=squash, diag=diag: ops.ppo_loss_gauss_ex(
                m, l, u_, d["v"], d["lo"] - 4, d["adv"], d["act"], d["vo"], d["vt"], 0.2, 0.01, True, -1.0, 0.5, q, f64(8) if diag else None)
        metric = "angle" if squash == "direction" else "mse"
        yield f"bc_loss_gauss cfg5 state A={A} {metric}", lambda m=mu_s, l=ls_s, t_=t_s, me=metric: ops.bc_loss_gauss(
            m, l, t_, d["v"], d["act"], d["vo"], d["vt"], 0.2, True, -1.0, 0.5, True, me == "mse", f64(2), me)
        yield f"ppo_bc_loss_gauss cfg5 state A={A} {squash} {metric} diag=1", lambda m=mu_s, l=ls_s, u_=u_s, t_=t_s, q=squash, me=metric: ops.ppo_bc_loss_gauss(
            m, l, u_, t_, d["v"], d["lo"] - 4, d["adv"], d["act"], d["vo"], d["vt"], 0.2, 0.01, 0.3, True, -1.0, 0.5, q, True, me == "mse", me, f64(3), f64(8))
    yield "bc_loss_gauss cfg5 param A=3 mse", lambda: ops.bc_loss_gauss(mu, ls, t, d["v"], d["act"], d["vo"], d["vt"], 0.2, True, -1.0, 0.5, True, True, f64(2))
    yield "ppo_bc_loss_gauss cfg5 param A=3 clip mse diag=1", lambda: ops.ppo_bc_loss_gauss(
        mu, ls, u, t, d["v"], d["lo"] - 4, d["adv"], d["act"], d["vo"], d["vt"], 0.2, 0.01, 0.3, True, -1.0, 0.5, "clip", True, True, "mse", f64(3), f64(8))
    dn = rows(N2N)
    p, a, lab = cat(N2N, 6)
    yield "bc_loss_cat n2n A=6", lambda: ops.bc_loss_cat(p, lab, dn["v"], dn["act"], dn["vo"], dn["vt"], 0.2, True, f64(2))
    for diag in (False, True):
        yield f"ppo_bc_loss_cat n2n A=6 diag={int(diag)}", lambda diag=diag: ops.ppo_bc_loss_cat(p, a, lab, dn["v"], dn["lo"] - 1.8, dn["adv"], dn["act"], dn["vo"], dn["vt"],
                                                                                              0.2, 0.01, 0.3, True, f64(3), f64(8) if diag else None)


def main():
    parent, pairs, warm = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 200, 20
    change_path = ops.lib_path()
    with tempfile.TemporaryDirectory() as td:
        copies = [shutil.copy(parent, os.path.join(td, f"parent_{k}.so")) for k in "ab"]
        libs = {"parent": load(copies[0]), "parent'": load(copies[1]), "change": load(change_path)}
    rec = ops._lib = Recorder(libs["change"])
    ev = {k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in libs}
    order = list(libs)
    print(f"{'case':58s} {'parent us':>10s} {'parent^ us':>10s} {'change us':>10s} {'A/A':>7s} {'change/parent':>13s}   ({pairs} calls each, medians)")
    noise, worst = 0.0, []
    for name, run in cases():
        rec.calls.clear()
        out = run()                                    # (the losses keep the gradients alive; nothing is allocated until the next case)
        (cname, args), = rec.calls
        torch.cuda.synchronize()
        ms = {k: [] for k in libs}
        for it in range(warm + pairs):
            for j in range(3):
                k = order[(it + j) % 3]                 # every library takes every position in turn
                ev[k][0].record()
                rc = getattr(libs[k], cname)(*args)
                ev[k][1].record()
                assert rc == 0, (k, cname, rc)
            torch.cuda.synchronize()
            if it >= warm:
                for k in libs:
                    ms[k].append(ev[k][0].elapsed_time(ev[k][1]))
        med = {k: 1e3 * statistics.median(v) for k, v in ms.items()}
        pa, pb, ch = med["parent"], med["parent'"], med["change"]
        aa, ab = abs(pb - pa) / pa, (ch - pa) / pa
        noise = max(noise, aa)
        worst.append((name, ab))
        print(f"{name:58s} {pa:10.2f} {pb:10.2f} {ch:10.2f} {100 * aa:6.2f}% {100 * ab:+12.2f}%", flush=True)
        del out
    bad = [(n, r) for n, r in worst if abs(r) > noise]
    print(f"noise (largest A/A gap): {100 * noise:.2f}%; cases whose change/parent gap exceeds it: {[(n, f'{100 * r:+.2f}%') for n, r in bad] or 'none'}")


if __name__ == "__main__":
    main()
