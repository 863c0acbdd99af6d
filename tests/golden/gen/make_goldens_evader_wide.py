"""Golden vectors for the SLSQP evader above 16 pursuers (the PM = 32 and 64 instances of k_n2n_evader / k_e3d_evader, slsqp::sort_asc
<32> / <64>, and both launch shapes of env_3d: 64 lanes per workgroup up to P = 42, 32 from P = 43).

The samplers, the mix of kinds and the record layout are make_goldens_evader.py's; only the pursuer counts differ.  Besides the
reference's command every group carries P{k}_stable: SLSQP stops on a discrete test, so on some problems the command of ANY
implementation depends on the last bits of its arithmetic.  The reference's own e_f is therefore called a second time with every number of
the problem (positions, angles, speeds, target) moved by a relative 1e-12; the problem is stable when the two commands differ by at most
1e-7.  The mask comes from the reference alone.
The tests ask that at least 80 % of the problems of a group on which the reference calls e_f are stable.  A group that is not is sampled
again from the next seed of its own sequence (seed, P, attempt), as often as it takes; P{k}_attempt records which sample was kept, and the
run prints every rejected one.  env_n2n groups pass at once; env_3d's three-variable problems are stable at about 72 % as sampled, so
their groups are picked from many samples (the selection looks at the reference only, never at the code under test).
Usage:  python tests/golden/gen/make_goldens_evader_wide.py
"""
import os
import warnings

import numpy as np

import make_goldens_evader as base  # activates the reference loader

N2N_PS = (17, 32, 33, 64)
E3D_PS = (17, 32, 33, 42, 43, 64)
PER_P = 120
REL, STABLE_TOL = 1e-12, 1e-7
MIN_STABLE, MAX_ATTEMPTS = 0.8, 400


def _nudged(rng, *arrays):
    """every number times (1 +- 1e-12), the sign drawn per number (a common factor would only rescale the problem)"""
    return [a * (1.0 + REL * np.where(rng.random(a.shape) < 0.5, -1.0, 1.0)) for a in arrays]


def _group(rng, nudge_rng, P, problem, command, eva):
    ps, es, ts, cs, st = [], [], [], [], []
    for _ in range(PER_P):
        e, p, tg = problem(rng, P)
        cmd = command(eva, e, p, tg)
        e2, p2, t2 = _nudged(nudge_rng, e, p, tg)
        p2[:, -1], e2[-1] = p[:, -1], e[-1]   # the active flags are not coordinates
        cmd2 = command(eva, e2, p2, t2)
        ps.append(p); es.append(e); ts.append(tg); cs.append(cmd)
        st.append(bool(np.max(np.abs(np.asarray(cmd) - np.asarray(cmd2))) <= STABLE_TOL))
    ps, es, st = np.asarray(ps), np.asarray(es), np.asarray(st)
    called = (es[:, -1] > 0) & ((ps[:, :, -1] > 0).any(1) | (es.shape[1] == 5))   # env_n2n calls e_f with no pursuer left as well
    return float(st[called].mean()), {f"P{P}_p": np.asarray(ps), f"P{P}_e": np.asarray(es), f"P{P}_target": np.asarray(ts), f"P{P}_cmd": np.asarray(cs),
            f"P{P}_stable": np.asarray(st)}


def main():
    warnings.simplefilter("ignore")
    from environment.env_n2n import eva as eva2
    from environment.env_3d import eva as eva3
    for name, PS, problem, command, eva, cfg, seed in (
            ("evader_n2n_wide", N2N_PS, base.n2n_problem, base.n2n_command, eva2, base.N2N_CFG, 21),
            ("evader_e3d_wide", E3D_PS, base.e3d_problem, base.e3d_command, eva3, base.E3D_CFG, 23)):
        out = {"cfg": cfg}
        for P in PS:
            for attempt in range(MAX_ATTEMPTS):
                frac, g = _group(np.random.default_rng([seed, P, attempt]), np.random.default_rng([seed, P, attempt, 1]), P, problem,
                                 command, eva)
                print(name, P, "attempt", attempt, "stable among called %.3f" % frac, flush=True)
                if frac >= MIN_STABLE:
                    break
            else:
                raise SystemExit(f"{name} P={P}: no sample with {MIN_STABLE} of its called problems stable in {MAX_ATTEMPTS} attempts")
            out.update(g)
            out[f"P{P}_attempt"] = np.int32(attempt)
        path = os.path.join(base.OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, len(PS) * PER_P, "records,", os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
