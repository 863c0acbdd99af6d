"""numpy reference of the env_n2n policy kernels (include/n2n_env.h): n2n_policy_inputs and n2n_policy_record.

Records as on the device: p (N, 5, P) and e (N, 5, E) float64 rows x, y, phi, v, active; target (N, 2).  The tick's adjacencies
pp_in (N, P, P) and pe_in (N, P, E) are fp32.  The accumulators are a dict of numpy arrays: done_before, ended, captured (uint8),
ret, length (float32)."""
import numpy as np

from tests import shaping_ref


def _rows4(rec, on):
    """(x, y, v cos phi, v sin phi) in float64, rounded to fp32; zero where `on` is false"""
    x, y, phi, v = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    out = np.stack((x, y, v * np.cos(phi), v * np.sin(phi)), -1).astype(np.float32)
    return np.where(on[..., None], out, np.float32(0))


def policy_inputs(p, e, pp_in, pe_in, done_before=None):
    """-> dict p4 (N,P,4), e4 (N,E,4), e_ref (N,4), live (N,P), pp_adj (N,P,P), pe_adj (N,P,E)"""
    N, P, E = p.shape[0], p.shape[2], e.shape[2]
    db = np.zeros(N, bool) if done_before is None else done_before.astype(bool)
    live = (p[:, 4] != 0) & ~db[:, None]
    e_on = e[:, 4] != 0
    e4 = _rows4(e, e_on)
    e_ref = np.zeros((N, 4), np.float32)
    for n in range(N):
        k = np.flatnonzero(e_on[n])
        if k.size:
            e_ref[n] = e4[n, k[0]]
    pp = np.where(live[:, :, None] & live[:, None, :], pp_in, np.float32(0)).astype(np.float32)
    pe = np.where(live[:, :, None] & e_on[:, None, :], pe_in, np.float32(0)).astype(np.float32)
    return dict(p4=_rows4(p, live), e4=e4, e_ref=e_ref, live=live.astype(np.float32), pp_adj=pp, pe_adj=pe)


def policy_record(p, e, target, reward, done, live, value, acc, kill_radius):
    """the state after the tick (records p, e), its reward (N,P) fp32 and done (N,) flags, this step's live (N,P) and value (N,P)
    -> (r, active, v, v_next_zero (N,P) bool) and the updated accumulators (a new dict)"""
    N, P = live.shape
    live = live.astype(np.float32)
    rl = (reward.astype(np.float32) * live).astype(np.float32)
    v = (value.astype(np.float32) * live).astype(np.float32)
    p_on, e_on = p[:, 4] != 0, e[:, 4] != 0
    # get_done's norm is sqrt(fma(dy, dy, dx dx)); tests/particle_config_cases.py has records on which the unfused sum decides otherwise
    reach = shaping_ref.within(np.stack((e[:, 0] - target[:, 0:1], e[:, 1] - target[:, 1:2])), kill_radius).any(-1)
    pa, ea = p_on.sum(-1), e_on.sum(-1)
    out = {k: x.copy() for k, x in acc.items()}
    db = acc["done_before"].astype(bool)
    ended = acc["ended"].astype(bool) | ((reach | (pa == 0) | (ea == 0)) & ~db)
    out["ended"] = ended.astype(np.uint8)
    out["captured"] = (acc["captured"].astype(bool) | ((ea == 0) & ~db)).astype(np.uint8)
    out["length"] = (acc["length"] + (~db).astype(np.float32)).astype(np.float32)
    s = np.zeros(N, np.float32)
    for k in range(P):                  # the agents of a step summed in order, in fp32
        s = (s + rl[:, k]).astype(np.float32)
    out["ret"] = (acc["ret"] + s).astype(np.float32)
    out["done_before"] = (db | (done != 0)).astype(np.uint8)
    v_next_zero = ~p_on | ended[:, None]
    return rl, live, v, v_next_zero, out


def ulp_close(got, want64):
    """every element within one fp32 ulp of the float64 value"""
    want32 = want64.astype(np.float32)
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    return np.all(np.abs(got.astype(np.float64) - want64) <= ulp)


def assert_policy_inputs(got, p, e, pp_in, pe_in, done_before):
    """what the GPU tests hold n2n_policy_inputs to: got, a dict of the six outputs read back, against policy_inputs() -- masks and
    adjacencies exactly, features within one fp32 ulp of the float64 value, zero rows exactly zero.  -> the reference's dict"""
    want = policy_inputs(p, e, pp_in, pe_in, done_before)
    N = p.shape[0]
    for k in ("live", "pp_adj", "pe_adj"):
        assert np.array_equal(got[k], want[k]), k
    live = want["live"].astype(bool)
    e_on = e[:, 4] != 0
    for k, rec, on in (("p4", p, live), ("e4", e, e_on)):
        f64 = np.stack((rec[:, 0], rec[:, 1], rec[:, 3] * np.cos(rec[:, 2]), rec[:, 3] * np.sin(rec[:, 2])), -1)
        assert ulp_close(got[k][on], f64[on]), k
        assert np.all(got[k][~on] == 0), k
    for n in range(N):
        k = np.flatnonzero(e_on[n])
        if k.size:
            f64 = np.array([e[n, 0, k[0]], e[n, 1, k[0]], e[n, 3, k[0]] * np.cos(e[n, 2, k[0]]), e[n, 3, k[0]] * np.sin(e[n, 2, k[0]])])
            assert ulp_close(got["e_ref"][n], f64)
        else:
            assert np.all(got["e_ref"][n] == 0)
    return want


def assert_policy_record(bufs, acc_got, p, e, target, reward, done, live, value, acc_before, kill_radius, fill=7.0):
    """what the GPU tests hold n2n_policy_record to: bufs (r, active, v, v_next read back; v_next was filled with `fill` before the
    launch) and the accumulators read back, against policy_record(), all exactly.  -> the reference's accumulators"""
    r, active, v, vz, acc_want = policy_record(p, e, target, reward, done, live, value, acc_before, kill_radius)
    assert np.array_equal(bufs["r"], r) and np.array_equal(bufs["active"], active)
    assert np.array_equal(bufs["v"], v)
    assert np.array_equal(bufs["v_next"], np.where(vz, np.float32(0), np.float32(fill)))
    for k, x in acc_want.items():
        assert np.array_equal(acc_got[k], x), k
    return acc_want


def new_accumulators(N):
    return dict(done_before=np.zeros(N, np.uint8), ended=np.zeros(N, np.uint8), captured=np.zeros(N, np.uint8),
                ret=np.zeros(N, np.float32), length=np.zeros(N, np.float32))


def random_records(rng, N, P, E, p_inactive=0.25, e_inactive=0.4):
    """records with some inactive pursuers / evaders parked at (1000, 1000) as the tick leaves them, targets in [0, 20]^2"""
    p = np.zeros((N, 5, P))
    e = np.zeros((N, 5, E))
    p[:, 0], p[:, 1] = rng.uniform(0, 20, (N, P)), rng.uniform(0, 20, (N, P))
    p[:, 2], p[:, 3] = rng.uniform(-np.pi, np.pi, (N, P)), rng.choice([0.0, 0.3], (N, P))
    p[:, 4] = (rng.random((N, P)) >= p_inactive).astype(np.float64)
    e[:, 0], e[:, 1] = rng.uniform(0, 20, (N, E)), rng.uniform(0, 20, (N, E))
    e[:, 2], e[:, 3] = rng.uniform(-np.pi, np.pi, (N, E)), 1.0
    e[:, 4] = (rng.random((N, E)) >= e_inactive).astype(np.float64)
    for rec in (p, e):
        off = rec[:, 4] == 0
        rec[:, 0][off], rec[:, 1][off], rec[:, 2][off] = 1000.0, 1000.0, 0.0
    target = rng.uniform(0, 20, (N, 2))
    # a few targets on an active evader (reach), a few environments with every evader captured
    for n in range(0, N, 7):
        on = np.flatnonzero(e[n, 4] != 0)
        if on.size:
            target[n] = e[n, :2, on[0]]
    e[3::11, 4] = 0.0
    p[5::13, 4] = 0.0
    pp_in = (rng.random((N, P, P)) < 0.5).astype(np.float32)
    pe_in = (rng.random((N, P, E)) < 0.5).astype(np.float32)
    return p, e, target, pp_in, pe_in
