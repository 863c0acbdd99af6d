"""numpy restatement -- and the specification -- of the scripted lead-pursuit pursuers (csrc/guidance.hpp, e3d_pursuer_guidance,
n2n_pursuer_guidance; runtime.guidance_lead / guidance_sep_range / guidance_sep_gain).

Records are the device's: p (N, C, P) and e (N, C, E) f64 (env_n2n, C = 5: x, y, phi, v, active) or p (N, 7, P) and e (N, 7)
(env_3d: x, y, z, phi, gamma, v, active).  Every operation is elementwise f64 in the order of the header (plain *, +, -, /, sqrt;
squares summed left to right; products left to right), so the kernels differ from this only where the device's atan2 / cos / sin
differ from libm's, by a few ulp.

The law, for pursuer i that is active against an evader that is active (env_n2n: the nearest active one, lowest index on ties):
    r = e_pos - p_i,  d = |r|,  e_vel = the evader's velocity,  t = min(d / p_vmax, lead),  aim = r + t e_vel,
    g = aim / |aim| (0 when |aim| is 0), then for every active team-mate j != i with 0 < d_ij < sep_range, in index order,
    g += gain (p_i - p_j) / d_ij (sep_range - d_ij) / sep_range;
the command points along g at full speed.  When g is exactly 0, or the pursuer or the evader is inactive: hold."""
import numpy as np

PI = np.pi
DEFAULT_LEAD, DEFAULT_SEP_GAIN, DEFAULT_SEP_KILL_RADII = 1.0, 1.0, 4.0   # sep_range defaults to 4 x kill_radius


def default_params(kill_radius):
    """-> (lead, sep_range, sep_gain) of a configuration that names none"""
    return DEFAULT_LEAD, DEFAULT_SEP_KILL_RADII * float(kill_radius), DEFAULT_SEP_GAIN


def lead_time(d, p_vmax, lead):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = d / p_vmax
    return np.where(t < lead, t, lead)


def _unit(a):
    """a (D, ...) -> a / |a|, 0 where |a| is 0"""
    sq = a[0] * a[0] + a[1] * a[1]
    if len(a) == 3:
        sq = sq + a[2] * a[2]
    n = np.sqrt(sq)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n == 0.0, 0.0, a / n)


def e3d_direction(p, e, p_vmax, lead, sep_range, gain):
    """-> (g (N, 3, P), on (N, P)): the direction before the command, and whether pursuer and evader are both active"""
    p, e = np.asarray(p, np.float64), np.asarray(e, np.float64).reshape(len(p), 7)
    pos, p_on, e_on = p[:, :3], p[:, 6] != 0.0, e[:, 6] != 0.0
    r = e[:, :3, None] - pos                                             # (N, 3, P)
    d = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
    ephi, egam, ev = e[:, 3], e[:, 4], e[:, 5]
    cg = np.cos(egam)
    e_vel = np.stack((ev * cg * np.cos(ephi), ev * cg * np.sin(ephi), ev * np.sin(egam)), 1)   # (N, 3)
    t = lead_time(d, p_vmax, lead)
    aim = r + t[:, None, :] * e_vel[:, :, None]
    g = _unit(aim.transpose(1, 0, 2)).transpose(1, 0, 2)
    g = _add_in_order(g, pos, p_on, sep_range, gain)
    return g, p_on & e_on[:, None]


def _add_in_order(g, pos, p_on, sep_range, gain):
    """g = ((g + term_0) + term_1) + ...: a team-mate that contributes nothing leaves g as it is (no + 0.0, which would turn a -0.0)"""
    for j in range(pos.shape[2]):
        term, use = separation_from(pos, p_on, j, sep_range, gain)
        g = np.where(use[:, None, :], g + term, g)
    return g


def separation_from(pos, p_on, j, sep_range, gain):
    """-> (term (N, D, P), use (N, P)): what team-mate j adds to every pursuer i, and where it does: j active, j != i and
    0 < d_ij < sep_range.  term is 0 elsewhere."""
    N, D, P = pos.shape
    diff = pos - pos[:, :, j:j + 1]                                      # p_i - p_j
    sq = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]
    if D == 3:
        sq = sq + diff[:, 2] * diff[:, 2]
    dij = np.sqrt(sq)
    use = p_on[:, j:j + 1] & (dij > 0.0) & (dij < sep_range) & (np.arange(P)[None, :] != j)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = gain * diff / dij[:, None] * (sep_range - dij[:, None]) / sep_range
    return np.where(use[:, None, :], term, 0.0), use


def e3d_actions(p, e, p_vmax, lead, sep_range, gain):
    """-> (N, P, 3) f64 in [-1, 1]: what e3d_env_tick takes (heading / pi, pitch / (pi / 2), speed); hold rows are
    (phi_i / pi, gamma_i / (pi / 2), -1)"""
    p = np.asarray(p, np.float64)
    g, on = e3d_direction(p, e, p_vmax, lead, sep_range, gain)
    go = on & ~((g[:, 0] == 0.0) & (g[:, 1] == 0.0) & (g[:, 2] == 0.0))
    a0 = np.where(go, np.arctan2(g[:, 1], g[:, 0]) / PI, p[:, 3] / PI)
    a1 = np.where(go, np.arctan2(g[:, 2], np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])) / (PI / 2), p[:, 4] / (PI / 2))
    a2 = np.where(go, 1.0, -1.0)
    return np.clip(np.stack((a0, a1, a2), -1), -1.0, 1.0)


def hold_rows_e3d(p, e, p_vmax, lead, sep_range, gain):
    g, on = e3d_direction(p, e, p_vmax, lead, sep_range, gain)
    return ~(on & ~((g[:, 0] == 0.0) & (g[:, 1] == 0.0) & (g[:, 2] == 0.0)))


def octant(b):
    """bearing(s) b -> the action k in 1..8 whose heading k pi / 4 is nearest (rint: ties to even); 0 and -8 map to 8"""
    k = np.rint(np.asarray(b, np.float64) / (PI / 4)).astype(np.int64)
    m = np.mod(np.mod(k, 8) + 8, 8)
    return np.where(m == 0, 8, m).astype(np.int32)


def action_heading(k):
    """the heading the env_n2n tick turns towards for action k in 1..8: k pi / 4, minus 2 pi when above pi"""
    ang = np.asarray(k, np.float64) * PI / 4
    return np.where(ang > PI, ang - 2 * PI, ang)


def n2n_direction(p, e, p_vmax, lead, sep_range, gain):
    """-> (g (N, 2, P), on (N, P), target (N, P)): the direction, whether the pursuer and some evader are active, and the index of the
    evader aimed at (the nearest active one, lowest index on ties; 0 where there is none)"""
    p, e = np.asarray(p, np.float64), np.asarray(e, np.float64)
    pos, p_on, e_on = p[:, :2], p[:, 4] != 0.0, e[:, 4] != 0.0           # (N, 2, P), (N, P), (N, E)
    r = e[:, :2, None, :] - pos[:, :, :, None]                           # (N, 2, P, E): e_pos - p_i
    d = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])                   # (N, P, E)
    k = np.where(e_on[:, None, :], d, np.inf).argmin(-1)                 # first minimum = lowest index
    any_e = e_on.any(-1)
    pick = lambda a: np.take_along_axis(a, k[..., None], -1)[..., 0]     # (N, P, E) -> (N, P)
    rx, ry, dk = pick(r[:, 0]), pick(r[:, 1]), pick(d)
    ephi, ev = np.take_along_axis(e[:, 2], k, -1), np.take_along_axis(e[:, 3], k, -1)
    t = lead_time(dk, p_vmax, lead)
    aim = np.stack((rx + t * (ev * np.cos(ephi)), ry + t * (ev * np.sin(ephi))), 0)   # (2, N, P)
    g = _unit(aim).transpose(1, 0, 2)
    g = _add_in_order(g, pos, p_on, sep_range, gain)
    return g, p_on & any_e[:, None], np.where(any_e[:, None], k, 0)


def n2n_actions(p, e, p_vmax, lead, sep_range, gain, with_bearing=False):
    """-> (N, P) int32 in 0..8, as head_sample writes them: 0 (stop, keep the heading) is the hold rule.  with_bearing: also the
    bearing atan2(g_y, g_x) of every row (nan on hold rows)"""
    g, on, _ = n2n_direction(p, e, p_vmax, lead, sep_range, gain)
    go = on & ~((g[:, 0] == 0.0) & (g[:, 1] == 0.0))
    b = np.arctan2(g[:, 1], g[:, 0])
    a = np.where(go, octant(b), 0).astype(np.int32)
    return (a, np.where(go, b, np.nan)) if with_bearing else a


def near_octant_boundary(b, tol=1e-9):
    """rows whose bearing lies within tol (radians) of a boundary between two octants, (m + 1/2) pi / 4: there a last-bit difference in
    atan2 may change the action.  nan (hold rows) -> False"""
    b = np.asarray(b, np.float64)
    x = b / (PI / 4) - 0.5
    with np.errstate(invalid="ignore"):
        return np.abs(x - np.rint(x)) * (PI / 4) <= tol
