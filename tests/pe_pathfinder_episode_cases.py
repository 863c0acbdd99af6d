"""Synthetic episode traces for the episode labeller's tests (include/pe_env.h pe_pathfinder_label_episode), built on the host from grids:
the evader dwells inside one cell, steps to a neighbouring cell, returns, sits on a rounding tie and leaves the map; the pursuers get
random free positions and velocities every tick."""
import numpy as np


def cell(x, y, W, H):
    """pepath::cell_id: Python's round is py_round"""
    return min(max(round(x), 0), W - 1) * H + min(max(round(y), 0), H - 1)


def expected_builds(eva, W, H):
    """eva (N, T, 4) -> (N,) 1 + the ticks whose evader cell differs from the tick before (no build hits the sweep bound)"""
    out = []
    for n in range(eva.shape[0]):
        cells = [cell(eva[n, t, 0], eva[n, t, 1], W, H) for t in range(eva.shape[1])]
        out.append(1 + sum(a != b for a, b in zip(cells[1:], cells[:-1])))
    return np.array(out, np.int32)


def evader_script(rng, W, H, T):
    """(T, 4): cell A, inside A twice, the neighbour B, A again, a tie (x.5, y.5), outside the map, then a random walk over cells"""
    ax, ay = int(rng.randint(1, W - 1)), int(rng.randint(1, H - 1))
    bx = ax + 1 if ax + 1 <= W - 1 else ax - 1
    xy = [(ax, ay), (ax + 0.25, ay - 0.25), (ax - 0.125, ay + 0.375), (bx, ay), (ax, ay), (ax + 0.5, ay - 0.5),
          (-0.75, ay) if rng.randint(2) else (W - 1 + 0.625, H - 1 + 2.0)]
    x, y = float(ax), float(ay)
    while len(xy) < T:
        if rng.randint(3) == 0:       # every third tick on average a new cell, otherwise a move inside the cell
            x, y = min(max(x + rng.randint(-1, 2), 0.0), W - 1.0), min(max(y + rng.randint(-1, 2), 0.0), H - 1.0)
        xy.append((x + rng.uniform(-0.4, 0.4), y + rng.uniform(-0.4, 0.4)))
    out = np.zeros((T, 4))
    out[:, :2] = np.array(xy[:T], np.float64)
    out[:, 2:] = rng.uniform(-1.5, 1.5, (T, 2))
    return out


def pursuer_records(rng, grid, P, T):
    """(T, 4, P): random positions in free cells (a jitter of up to 0.45 around the centre, clamped to the map) and velocities"""
    W, H = grid.shape
    free = np.argwhere(grid == 0)
    out = np.zeros((T, 4, P))
    for t in range(T):
        pick = free[rng.randint(0, len(free), P)]
        out[t, 0] = np.clip(pick[:, 0] + rng.uniform(-0.45, 0.45, P), 0.0, W - 1.0)
        out[t, 1] = np.clip(pick[:, 1] + rng.uniform(-0.45, 0.45, P), 0.0, H - 1.0)
        out[t, 2:] = np.where(rng.randint(0, 3, (2, P)) > 0, rng.uniform(-2, 2, (2, P)), 0.0)
    return out


def synthetic(N, W, H, P, T, seed):
    """grids (N, W*H) u8 with densities 0 / 0.15 / 0.35 in turn, trace_def (N, T, 4, P), trace_eva (N, T, 4)"""
    grids, defs, evas = [], [], []
    for n in range(N):
        rng = np.random.RandomState(seed + n)
        g = (rng.random_sample((W, H)) < (0.0, 0.15, 0.35)[n % 3]).astype(np.uint8)
        g[rng.randint(W), rng.randint(H)] = 0          # at least one free cell
        grids.append(g.reshape(-1))
        defs.append(pursuer_records(rng, g, P, T))
        evas.append(evader_script(rng, W, H, T))
    return np.stack(grids), np.stack(defs), np.stack(evas)


def per_tick_host(pe_env, cfg, grid, trace_def, trace_eva, **kw):
    """the per-tick host twin on every tick of a trace -> actions (N, T, P) int32 and the last tick's diag"""
    N, T = trace_eva.shape[:2]
    out = np.zeros((N, T, cfg.P), np.int32)
    dg = None
    for t in range(T):
        out[:, t], dg = pe_env.pathfinder_host(cfg, grid, trace_def[:, t], trace_eva[:, t], diag=True, **kw)
    return out, dg
