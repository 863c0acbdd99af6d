"""The pathfinder law of Pursuit_Env's scripted pursuers (include/pe_env.h pe_pursuer_pathfinder) in plain Python:
floats, round(), math.sqrt and integers; no numpy arithmetic, no fused multiply-add.  The authority every pathfinder test compares to.

`cfg` is any object with W, H, P, def_tau, def_dt, def_collision_radius and action_u[9][2] (a pe_config, the oracle's config, or
`Cfg` below).  One environment at a time: grid is a flat sequence of W*H cells (cell (x, y) at x*H + y, occupied when != 0), defs the
record [x[P], y[P], vx[P], vy[P]] (4 sequences), eva (x, y, vx, vy).
"""
import math
from types import SimpleNamespace

UNREACHED = 0x7FFFFFFF
OFFS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def Cfg(W, H, P, vmax=2.0, def_tau=0.2, def_dt=0.1, radius=0.5):
    u = [[math.cos(k * math.pi / 4) * vmax, math.sin(k * math.pi / 4) * vmax] for k in range(8)] + [[0.0, 0.0]]
    return SimpleNamespace(W=W, H=H, P=P, def_tau=def_tau, def_dt=def_dt, def_collision_radius=radius, action_u=u)


def params(cfg, lead=None, sep_range=None, clearance=None):
    return SimpleNamespace(lead=0.5 if lead is None else float(lead),
                           sep_range=2.0 * cfg.def_collision_radius if sep_range is None else float(sep_range),
                           clearance=10 if clearance is None else int(clearance))


def clampi(v, hi):
    return 0 if v < 0 else (hi if v > hi else v)


def cell(cfg, x, y):
    return clampi(round(x), cfg.W - 1), clampi(round(y), cfg.H - 1)


def in_map(cfg, x, y):
    return 0 <= x < cfg.W and 0 <= y < cfg.H


def occupied(cfg, grid, x, y):
    return grid[x * cfg.H + y] != 0


def pen(cfg, grid, n, s):
    if n == s:
        return False
    return any(in_map(cfg, n[0] + dx, n[1] + dy) and occupied(cfg, grid, n[0] + dx, n[1] + dy) for dx, dy in OFFS)


def admissible(cfg, grid, c, k, s):
    """neighbour k of cell c, or None"""
    dx, dy = OFFS[k]
    n = (c[0] + dx, c[1] + dy)
    if not in_map(cfg, *n):
        return None
    if occupied(cfg, grid, *n) and n != s:
        return None
    if dx != 0 and dy != 0 and (occupied(cfg, grid, n[0], c[1]) or occupied(cfg, grid, c[0], n[1])):
        return None
    return n


def edge(cfg, grid, c, k, s, clearance):
    """(neighbour, step + pen) or None"""
    n = admissible(cfg, grid, c, k, s)
    if n is None:
        return None
    return n, (14 if k & 1 else 10) + (clearance if pen(cfg, grid, n, s) else 0)


def field(cfg, grid, eva, clearance):
    """the distance field as a flat list of W*H ints: repeated sweeps over the cells until one changes nothing"""
    W, H = cfg.W, cfg.H
    s = cell(cfg, eva[0], eva[1])
    D = [UNREACHED] * (W * H)
    D[s[0] * H + s[1]] = 0
    # pen() of every cell once (what edge() would recompute for each of a cell's eight neighbours)
    touch = [any(in_map(cfg, x + dx, y + dy) and grid[(x + dx) * H + y + dy] != 0 for dx, dy in OFFS) for x in range(W) for y in range(H)]
    items = []
    for x in range(W):
        for y in range(H):
            if (x, y) == s or grid[x * H + y] != 0:
                continue
            es = []
            for k in range(8):
                n = admissible(cfg, grid, (x, y), k, s)
                if n is not None:
                    es.append((n[0] * H + n[1], (14 if k & 1 else 10) + (clearance if n != s and touch[n[0] * H + n[1]] else 0)))
            items.append((x * H + y, es))
    changed = True
    while changed:
        changed = False
        items.reverse()     # any order reaches the same (least) fixed point; alternating directions reaches it in fewer sweeps
        for c, es in items:
            best = D[c]
            for n, w in es:
                dn = D[n]
                if dn != UNREACHED and dn + w < best:
                    best = dn + w
            if best < D[c]:
                D[c] = best
                changed = True
    return D


def walk_clear(cfg, grid, c0, c1):
    """find_attacker's Bresenham walk (agent.py:319-341) from cell c0 to cell c1: no cell of it occupied"""
    x0, y0 = c0
    x1, y1 = c1
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx = -1 if x0 > x1 else 1
    sy = -1 if y0 > y1 else 1
    err = dx - dy
    while True:
        if occupied(cfg, grid, x0, y0):
            return False
        if x0 == x1 and y0 == y1:
            return True
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x0 += sx
        if e2 < dx:
            err += dx
            y0 += sy


def clampd(v, hi):
    return 0.0 if v < 0.0 else (hi if v > hi else v)


def heading(cfg, grid, D, prm, p, eva):
    H = cfg.H
    u = cfg.action_u
    px, py = p
    ci = cell(cfg, px, py)
    dx, dy = eva[0] - px, eva[1] - py
    d = math.sqrt(dx * dx + dy * dy)
    t = d / u[0][0]
    if t > prm.lead:
        t = prm.lead
    ax, ay = clampd(eva[0] + t * eva[2], float(cfg.W - 1)), clampd(eva[1] + t * eva[3], float(cfg.H - 1))
    if occupied(cfg, grid, *cell(cfg, ax, ay)):
        ax, ay = eva[0], eva[1]
    s = cell(cfg, eva[0], eva[1])
    if D[ci[0] * H + ci[1]] == UNREACHED:
        ax, ay = eva[0], eva[1]
        direct = True
    else:
        direct = walk_clear(cfg, grid, ci, cell(cfg, ax, ay))
    if direct:
        vx, vy = ax - px, ay - py
        if vx * vx + vy * vy <= 1e-4:
            return 8
        dots = [vx * u[k][0] + vy * u[k][1] for k in range(8)]
        return dots.index(max(dots))
    best, kb = UNREACHED, 8
    for k in range(8):
        e = edge(cfg, grid, ci, k, s, prm.clearance)
        if e is None or D[e[0][0] * H + e[0][1]] == UNREACHED:
            continue
        v = D[e[0][0] * H + e[0][1]] + e[1]
        if v < best:
            best, kb = v, k
    return kb


def candidates(kstar):
    if kstar == 8:
        return [8] + list(range(8))
    return [(kstar + o) % 8 for o in (0, 1, -1, 2, -2, 3, -3, 4)] + [8]


def dynamic(cfg, x, y, vx0, vy0, ux, uy):
    """agent.py:74-104: the first-order lag under RK4, association as written (the tick's `dynamic`)"""
    tau, h = cfg.def_tau, cfg.def_dt

    def lag(v0, u):
        k1 = (u - v0) / tau
        k2 = (u - (v0 + h * k1 / 2)) / tau
        k3 = (u - (v0 + h * k2 / 2)) / tau
        k4 = (u - (v0 + h * k3)) / tau
        return v0 + (k1 + 2 * k2 + 2 * k3 + k4) * h / 6.0
    vx, vy = lag(vx0, ux), lag(vy0, uy)
    return x + vx * h, y + vy * h, vx, vy


def probe_blocked(cfg, grid, qx, qy):
    r = cfg.def_collision_radius
    for a in range(3):
        for b in range(3):
            ix, iy = round(qx + float(a - 1) * r), round(qy + float(b - 1) * r)
            if in_map(cfg, ix, iy) and occupied(cfg, grid, ix, iy):
                return True
    return False


def pursuer(cfg, grid, D, prm, defs, eva, i):
    """(action, kstar, blocked mask) of pursuer i"""
    x, y = defs[0][i], defs[1][i]
    ks = heading(cfg, grid, D, prm, (x, y), eva)
    sep2 = prm.sep_range * prm.sep_range
    blocked = crowded = 0
    for k in range(9):
        qx, qy, _, _ = dynamic(cfg, x, y, defs[2][i], defs[3][i], cfg.action_u[k][0], cfg.action_u[k][1])
        if probe_blocked(cfg, grid, qx, qy):
            blocked |= 1 << k
        for j in range(i):
            a, b, c, d = qx - defs[0][j], qy - defs[1][j], x - defs[0][j], y - defs[1][j]
            nq, no = a * a + b * b, c * c + d * d
            if nq <= sep2 and nq < no:
                crowded |= 1 << k
    order = candidates(ks)
    for k in order:
        if not ((blocked | crowded) >> k) & 1:
            return k, ks, blocked
    for k in order:
        if not (blocked >> k) & 1:
            return k, ks, blocked
    return 8, ks, blocked


def pathfinder(cfg, grid, defs, eva, lead=None, sep_range=None, clearance=None):
    """one environment -> dict(actions [P], field [W*H], kstar [P], blocked [P])"""
    prm = params(cfg, lead, sep_range, clearance)
    grid = [int(v) for v in grid]
    defs = [[float(v) for v in row] for row in defs]
    eva = [float(v) for v in eva]
    D = field(cfg, grid, eva, prm.clearance)
    rows = [pursuer(cfg, grid, D, prm, defs, eva, i) for i in range(cfg.P)]
    return dict(actions=[r[0] for r in rows], field=D, kstar=[r[1] for r in rows], blocked=[r[2] for r in rows])
