"""Golden vectors of the reference's RewardScaling (DHGN/normalization.py:38-52) for algo.use_reward_scaling.

One RewardScaling(shape=P, gamma=0.99) per stream, called once per step with the step's whole reward vector and reset() between
episodes, as a worker of the reference's rollout does (obstacle_differ_3hop/mappo_parallel.py:517):
  n2n   the reward rows of the committed env_n2n P = 16 traces, one episode per trace,
  e3d   the reward rows of the committed env_3d P = 8 traces,
  syn   six 40-step episodes of integer rewards drawn from {-2, -1, 0, 0, 0, 1} (RandomState(0)), P = 8; the first sample is
        negative, so the first-sample quirk (std = R at n == 1) is in the fixture.
Per stream S: S_x (steps, P) f64 inputs, S_start (steps,) u8 episode starts, S_y (steps, P) f64 outputs, and the final state S_n,
S_mean, S_S, S_R.  Usage:  python tests/golden/gen/make_goldens_reward_scaling.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refload  # noqa: E402

refload.activate()
OUT = os.path.dirname(HERE)
GAMMA = 0.99
N2N_TRACES = ("n2n_p16_s2", "n2n_p16_s3", "n2n_p16_e2_s4", "n2n_p16_s5")
E3D_TRACES = ("e3d_p8_s2", "e3d_p8_s3", "e3d_p8_s4")


def episodes(kind):
    if kind == "syn":
        rng = np.random.RandomState(0)
        return [rng.choice(np.array([-2.0, -1.0, 0.0, 0.0, 0.0, 1.0]), size=(40, 8)) for _ in range(6)]
    names = N2N_TRACES if kind == "n2n" else E3D_TRACES
    return [np.load(os.path.join(OUT, n + ".npz"))["reward"].astype(np.float64) for n in names]


def drive(eps):
    from DHGN.normalization import RewardScaling
    P = eps[0].shape[1]
    rs = RewardScaling(shape=P, gamma=GAMMA)
    xs, starts, ys = [], [], []
    for ep in eps:
        rs.reset()
        for t, x in enumerate(ep):
            xs.append(x.copy()); starts.append(t == 0)
            ys.append(np.asarray(rs(x.copy()), np.float64).copy())
    ms = rs.running_ms
    return dict(x=np.stack(xs), start=np.asarray(starts, np.uint8), y=np.stack(ys), n=np.asarray(ms.n, np.int64),
                mean=np.asarray(ms.mean, np.float64), S=np.asarray(ms.S, np.float64), R=np.asarray(rs.R, np.float64))


def main():
    out = dict(gamma=np.asarray(GAMMA, np.float64))
    for kind in ("n2n", "e3d", "syn"):
        d = drive(episodes(kind))
        assert np.isfinite(d["y"]).all() and np.any(d["y"] != 0)
        print(kind, "steps", len(d["x"]), "P", d["x"].shape[1], "episodes", int(d["start"].sum()), "max |y|", float(np.abs(d["y"]).max()),
              "first x", d["x"][0].tolist())
        out.update({f"{kind}_{k}": v for k, v in d.items()})
    np.savez_compressed(os.path.join(OUT, "reward_scaling.npz"), **out)


if __name__ == "__main__":
    main()
