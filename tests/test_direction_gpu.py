"""GPU checks of the direction-vector action head (algo.gauss_squash: direction): the rollout head, the imitation
select launch and the imitation loss with the angle metric against tests/direction_ref.py, and the E3dMAPPO agent / E3dTrainer in the
mode (buffer, rollout-update agreement, determinism, resume, the imitation phase, the checkpoint check)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import direction_ref as ref
from tests import imitation_ref

pytestmark = pytest.mark.gpu

LO, HI = -0.4, 0.3
EPS = 0.05


def _ops():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops


def _np(*ts):
    return [t.double().cpu().numpy() for t in ts]


# ---- head -------------------------------------------------------------------------------------------------------------------------
def _head_inputs(R, seed):
    g = torch.Generator().manual_seed(seed)
    feat = (torch.randn(R, 128, generator=g) * 0.3).cuda()
    W, b = (torch.randn(4, 128, generator=g) * 0.1).cuda(), (torch.randn(4, generator=g) * 0.3).cuda()
    W_ls, b_ls = (torch.randn(4, 128, generator=g) * 0.1).cuda(), (torch.randn(4, generator=g) * 0.3).cuda()
    ls = (torch.randn(4, generator=g) * 0.4).cuda()
    return feat, W, b, W_ls, b_ls, ls


def _head_call(feat, W, b, ls, seed, counter, greedy=False, squash="direction", lo=LO, hi=HI):
    R = feat.shape[0]
    out = (torch.full((R, 4), 7.0, device="cuda"), torch.full((R, 3 if squash == "direction" else 4), 7.0, dtype=torch.float64, device="cuda"),
           torch.full((R,), 7.0, device="cuda"))
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        _ops().gauss_head_sample_ex(feat, W, b, ls, seed, counter, ticket, out, greedy=greedy, log_std_min=lo, log_std_max=hi, squash=squash)
    assert int(ticket.item()) == 0
    return out


def _counter(c0):
    return torch.full((1,), c0, dtype=torch.int64, device="cuda")


# a single row, a partial wave, a full wave, one row into the next wave, one row into the next workgroup
@pytest.mark.parametrize("state", [False, True], ids=["param", "state"])
@pytest.mark.parametrize("R", [1, 5, 64, 65, 257])
def test_head_matches_reference(R, state):
    feat, W, b, W_ls, b_ls, ls = _head_inputs(R, 17 * R + state)
    src = (W_ls, b_ls) if state else ls
    seed, c0 = 0x5EED0000D1A + R, (3 << 40) + 0xFFFFFFC0        # a counter whose low word carries inside the larger launches
    f, w, bb, wl, bl, lv = _np(feat, W, b, W_ls, b_ls, ls)
    ref_src = (wl, bl) if state else lv
    for greedy in (False, True):
        counter = _counter(c0)
        u, env, lp = _head_call(feat, W, b, src, seed, counter, greedy)
        assert int(counter.item()) == c0 + R                                          # the counter advances by R
        _, _, z_r, u_r, lp_r = ref.head_sample(f, w, bb, ref_src, seed, c0, greedy, LO, HI)
        if not greedy:
            assert (z_r[:, 3] != 0).all()                                             # the fourth Philox word is used
        u64 = u.double().cpu().numpy()
        print(f"R={R} state={state} greedy={greedy}: max |u - ref| {np.abs(u64 - u_r).max():.3e}, max |logp - ref| "
              f"{np.abs(lp.double().cpu().numpy() - lp_r).max():.3e}")
        np.testing.assert_allclose(u64, u_r, rtol=0, atol=2e-5)
        np.testing.assert_allclose(lp.double().cpu().numpy(), lp_r, rtol=1e-5, atol=2e-5)
        want_env = ref.to_env(u.cpu().numpy())                                        # of the kernel's own stored fp32 u
        err = np.abs(env.cpu().numpy() - want_env).max()
        print(f"    max |env_action - to_env(u)| {err:.3e}")
        assert env.shape == (R, 3) and err <= 1e-12
        for t in (u, env, lp):
            assert not (t == 7.0).any()                                               # the pre-filled outputs are fully overwritten
        again = _head_call(feat, W, b, src, seed, _counter(c0), greedy)               # the same counter: the same bytes
        for x, y in zip((u, env, lp), again):
            assert torch.equal(x, y)
        for other in ("clip", "tanh"):                                                # the latent sample does not depend on the map
            uo = _head_call(feat, W, b, src, seed, _counter(c0), greedy, squash=other)[0]
            assert torch.equal(uo, u), other


def test_head_edge_table():
    feat = _head_inputs(3, 1)[0]
    W, ls = torch.zeros(4, 128, device="cuda"), torch.zeros(4, device="cuda")
    for k, (edge, want) in enumerate(ref.EDGES):
        b = torch.tensor(edge, dtype=torch.float32).cuda()
        u, env, lp = _head_call(feat, W, b, ls, 1, _counter(0), greedy=True, lo=-5.0, hi=2.0)
        un, en = u.cpu().numpy(), env.cpu().numpy()
        assert (un == np.array(edge, np.float32)).all()
        # exact: the bits of the specification on the stored u.  mu = 0 + b loses the sign of a -0 bias ((+0) + (-0) is +0 in the head's
        # sum, as in every mode), so row 1 of the table arrives as row 0; the signed zero itself goes through the host entry
        # (tests/test_direction_ref_cpu.py), which runs the same inline function
        assert np.array_equal(en.view(np.uint64), ref.to_env(un).view(np.uint64)), (k, en)
        if not any(x == 0 and math.copysign(1.0, x) < 0 for x in edge):
            assert np.array_equal(en.view(np.uint64), np.tile(np.array(want), (3, 1)).view(np.uint64)), (k, en)
        else:
            assert not np.signbit(un[:, 1]).any() and (en[:, 0] == 1.0).all()


def test_head_entry_refuses_other_widths():
    ops = _ops()
    for A in (3, 5):
        feat = _head_inputs(4, 2)[0]
        out = (torch.empty(4, A, device="cuda"), torch.empty(4, 3, dtype=torch.float64, device="cuda"), torch.empty(4, device="cuda"))
        with pytest.raises(AssertionError):
            ops.gauss_head_sample_ex(feat, torch.zeros(A, 128, device="cuda"), torch.zeros(A, device="cuda"), torch.zeros(A, device="cuda"), 1,
                                     _counter(0), torch.zeros(1, dtype=torch.int32, device="cuda"), out, squash="direction")
    L = ops.load_library()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    feat, W, b, ls, cnt, tk, a, e, lp = z(4, 128), z(3, 128), z(3), z(3), z(1, dt=torch.int64), z(1, dt=torch.int32), z(4, 3), z(4, 3, dt=torch.float64), z(4)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.gauss_head_sample_ex(4, 3, 128, p(feat), p(W), p(b), None, None, p(ls), -5.0, 2.0, 2, 1, p(cnt), p(tk), 0, p(a), p(e), p(lp), None)
    assert rc != 0                                                                    # the C entry itself: squash 2 needs A = 4
    rc = L.gauss_head_sample_ex(4, 3, 128, p(feat), p(W), p(b), None, None, p(ls), -5.0, 2.0, 3, 1, p(cnt), p(tk), 0, p(a), p(e), p(lp), None)
    assert rc != 0


# ---- select -----------------------------------------------------------------------------------------------------------------------
N_SEL, T_SEL, ROW = 5, 4, 2
FOLLOW = {"none": [0, 0, 0, 0, 0], "all": [1, 1, 1, 1, 1], "mixed": [1, 0, 0, 1, 0]}


@pytest.mark.parametrize("follow", list(FOLLOW))
@pytest.mark.parametrize("P", [3, 8, 9])
def test_e3d_bc_select_direction(P, follow):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_env import ParticleEnv
    env = ParticleEnv(num_envs=N_SEL)
    env.initialize(P)
    env.reset()
    guide = env.guidance_actions().clone()
    g = torch.Generator().manual_seed(P)
    action = (torch.rand(N_SEL, P, 3, generator=g, dtype=torch.float64) * 2 - 1).cuda()
    a_star = torch.full((N_SEL, T_SEL, P + 1, 4), 7.5, device="cuda")                 # rows padded by one pursuer's width
    f = torch.tensor(FOLLOW[follow], dtype=torch.uint8, device="cuda")
    before, guide0 = action.clone(), guide.clone()
    _ops().bc_select(guide, f, action, a_star[:, ROW, :P], "direction", 0.999)
    labels, executed = ref.e3d_select(guide0.cpu().numpy(), FOLLOW[follow], before.cpu().numpy())
    assert torch.equal(guide, guide0)
    assert np.array_equal(action.cpu().numpy().view(np.uint64), executed.view(np.uint64))   # exactly g where followed, else untouched
    got = a_star[:, ROW, :P].cpu().numpy()
    err = np.abs(got.astype(np.float64) - labels.astype(np.float64))
    print(f"P={P} {follow}: max label error {err.max():.3e}")
    assert (err <= np.spacing(np.abs(labels))).all()                                  # one fp32 ulp
    assert np.array_equal(got[..., 3], guide0.cpu().numpy()[..., 2].astype(np.float32))
    assert (a_star[:, ROW, P] == 7.5).all()                                           # the columns beyond 4 P of the padded row
    rest = torch.ones(T_SEL, dtype=torch.bool)
    rest[ROW] = False
    assert (a_star[:, rest] == 7.5).all()                                             # the other ticks' rows
    with pytest.raises(RuntimeError):                                                 # a row of 3 P floats is too short for the labels
        L = _ops().load_library()
        short = torch.zeros(N_SEL, P * 3, device="cuda")
        _ops()._check(L.e3d_bc_select(N_SEL, P, C.c_void_p(guide.data_ptr()), C.c_void_p(f.data_ptr()), 2, 0.999, C.c_void_p(action.data_ptr()),
                                      C.c_void_p(short.data_ptr()), P * 3, None), "e3d_bc_select")


# ---- imitation loss with the angle metric ---------------------------------------------------------------------------------------
def _r32(x):
    return x.float().double()


def _critic_inputs(g, mb, T, P):
    """the values of tests/test_imitation_gpu.py: clear of the value clip's edges and ties; about a third of the rows not live"""
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    v_tm = _r32(r(T, mb, P, 1))
    v = v_tm.permute(1, 0, 2, 3)[..., 0]
    vo = _r32(v + r(mb, T, P) * 0.1)
    vo = _r32(torch.where(((v - vo).abs() - EPS).abs() < 1e-3, vo + 0.01, vo))
    active = (torch.rand(mb, T, P, generator=g) < 0.67).double()
    active[0, 0, 0] = 1.0
    vt = _r32(r(mb, T, P))
    tie = lambda: ((v - vo).abs() > EPS) & ((((v - vo).clamp(-EPS, EPS) + vo) - vt).abs() - (v - vt).abs()).abs().lt(1e-4)
    for _ in range(3):
        vt = _r32(torch.where(tie(), vt + 0.01, vt))
    assert not tie().any() and (((v - vo).abs() - EPS).abs() >= 1e-3).all()
    return v_tm, vo, vt, active


def _angle_case(mb, T, P, state, roll, seed, zero_rows=False):
    """time-major mu / ls_raw / values as the update has them; unit-vector labels (direction_ref.label of random commands); mu[:3] at an
    angle of 5 to 175 degrees from the label and 3 to 6 long, so that no row's angle is left out and the residuals are wide against
    sigma (the log-std sums of param mode do not cancel: tests/test_imitation_gpu.py); inactive rows hold finite garbage"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    v_tm, vo, vt, active = _critic_inputs(g, mb, T, P)
    cmd = torch.stack([u(mb, T, P) * 1.998 - 0.999, u(mb, T, P) * 1.998 - 0.999, torch.where(u(mb, T, P) < 0.5, -1.0, 1.0)], -1)
    target = torch.from_numpy(ref.label(cmd.numpy())).double()
    t3 = target[..., :3]
    perp = torch.linalg.cross(t3, r(mb, T, P, 3), dim=-1)
    perp = perp / perp.norm(dim=-1, keepdim=True)
    theta = torch.deg2rad(5.0 + 170.0 * u(mb, T, P, 1))
    m3 = (3.0 + 3.0 * u(mb, T, P, 1)) * (torch.cos(theta) * t3 + torch.sin(theta) * perp)
    m4 = target[..., 3:] + torch.where(u(mb, T, P, 1) < 0.5, -1.0, 1.0) * (2.0 + 2.0 * u(mb, T, P, 1))
    mu = _r32(torch.cat((m3, m4), -1))
    if zero_rows:
        mu.view(-1, 4)[::2, :3] = 0.0                                                  # a mean that points nowhere: the row counts pi / 2
    else:
        deg = np.degrees(ref.angle(mu.numpy(), target.numpy()))
        assert deg.min() >= 1.0 and deg.max() <= 179.0
    three = torch.tensor([-0.9, -0.3, 0.8, 0.1], dtype=torch.float64).roll(roll)
    if state:
        ls_tm = r(T, mb, P, 4) * 0.6
        k = min(4, ls_tm.numel())
        ls_tm.view(-1)[:k] = three[:k]
        ls_tm = _r32(torch.where(((ls_tm - HI).abs() < 2e-3) | ((ls_tm - LO).abs() < 2e-3), ls_tm + 0.01, ls_tm))
    else:
        ls_tm = _r32(three.clone())
    dead = active == 0
    mu[dead] = _r32(r(int(dead.sum()), 4) * 40.0)
    target[dead] = _r32(r(int(dead.sum()), 4) * 40.0)
    v_tm.permute(1, 0, 2, 3)[..., 0][dead] = _r32(r(int(dead.sum())) * 30.0)
    mu_tm = mu.permute(1, 0, 2, 3).contiguous()
    return dict(mu_tm=mu_tm, ls_tm=ls_tm, target=target, v_tm=v_tm, vo=vo, vt=vt, active=active, state=state)


def _bt(t):
    return t.permute(1, 0, 2, 3) if t.dim() == 4 else t


def _gpu_bc(c, fit_std, clip, sums=None, metric="angle", wrap0=False):
    f = lambda x: x.float().cuda()
    mu_tm, ls_tm, v_tm = (f(c[k]).requires_grad_() for k in ("mu_tm", "ls_tm", "v_tm"))
    la, lc = _ops().bc_loss_gauss(_bt(mu_tm), _bt(ls_tm), f(c["target"]), v_tm.permute(1, 0, 2, 3)[..., 0], f(c["active"]),
                                  f(c["vo"]) if clip else None, f(c["vt"]), EPS, clip, log_std_min=LO, log_std_max=HI, fit_std=fit_std,
                                  wrap0=wrap0, sums=sums, metric=metric)
    (la + lc).backward()
    return la.detach(), lc.detach(), mu_tm.grad, ls_tm.grad, v_tm.grad


def _close(got, want, what):
    want = torch.as_tensor(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got.double().cpu() - want).abs().max().item()
    scale = want.abs().max().item()
    print(f"{what}: max error {err:.3e}, max |ref| {scale:.3e}")
    assert err <= 1e-5 * scale + 1e-12, (what, err, scale)


def _loss_close(got, want, what):
    print(f"{what}: {float(got):.9g} against {float(want):.9g}")
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)) + 1e-7, (what, float(got), float(want))


@pytest.mark.parametrize("fit_std", [False, True], ids=["fixed_std", "fit_std"])
@pytest.mark.parametrize("state", [False, True], ids=["param", "state"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 3), (3, 7, 5)], ids=lambda s: "x".join(map(str, s)))
def test_bc_loss_angle_metric_matches_reference(shape, state, fit_std):
    ops = _ops()
    mb, T, P = shape
    for k, clip in enumerate((True, False)):
        c = _angle_case(mb, T, P, state, k + 2 * fit_std, seed=100 * mb + 10 * state + k)
        sums = torch.tensor([3.0, 5.0], dtype=torch.float64, device="cuda")           # the call adds to what is there
        la, lc, gmu, gls, gv = _gpu_bc(c, fit_std, clip, sums, wrap0=True)            # the wrap is ignored with this metric
        mu, tgt = _bt(c["mu_tm"]).numpy(), c["target"].numpy()
        want = imitation_ref.bc_loss_gauss(mu, _bt(c["ls_tm"]).numpy(), tgt, c["v_tm"].permute(1, 0, 2, 3)[..., 0].numpy(), c["active"].numpy(),
                                           c["vo"].numpy(), c["vt"].numpy(), EPS, clip, LO, HI, fit_std, False)
        tag = f"angle {shape} state={state} fit={fit_std} clip={clip}"
        _loss_close(la, want["actor_loss"], tag + " actor")
        _loss_close(lc, want["critic_loss"], tag + " critic")
        assert gmu.stride() == c["mu_tm"].stride()
        _close(gmu, torch.from_numpy(want["g_mu"]).permute(1, 0, 2, 3), tag + " g_mu")
        _close(gls, torch.from_numpy(want["g_ls"]).permute(1, 0, 2, 3) if state else want["g_ls"], tag + " g_ls")
        _close(gv, torch.from_numpy(want["g_v"]).permute(1, 0, 2)[..., None], tag + " g_v")
        if not fit_std:
            assert not gls.any()
        s = sums.cpu().numpy()
        want_angle = (ref.angle(mu, tgt) * c["active"].numpy()).sum()
        print(f"{tag} angle sum: {s[0] - 3.0:.9g} against {want_angle:.9g}")
        assert abs((s[0] - 3.0) - want_angle) <= 1e-5 * want_angle
        assert s[1] - 5.0 == want["rows"]
        # the critic part carries the bits of the PPO launch of the mode on the same inputs
        f = lambda x: x.float().cuda()
        mu2, v2 = f(c["mu_tm"]).requires_grad_(), f(c["v_tm"]).requires_grad_()
        pa, pc = ops.ppo_loss_gauss_ex(mu2.permute(1, 0, 2, 3), torch.zeros(4, device="cuda"), f(c["target"]), v2.permute(1, 0, 2, 3)[..., 0],
                                       torch.zeros(mb, T, P, device="cuda"), torch.ones(mb, T, P, device="cuda"), f(c["active"]),
                                       f(c["vo"]) if clip else None, f(c["vt"]), EPS, 0.0, clip, squash="direction")
        (pa + pc).backward()
        assert torch.equal(lc, pc.detach()) and torch.equal(gv, v2.grad), tag
        # the metric changes neither a loss nor a gradient, and two calls give the same bits
        for metric in ("mse", "angle"):
            again = _gpu_bc(c, fit_std, clip, metric=metric)
            for x, y in zip((la, lc, gmu, gls, gv), again):
                assert torch.equal(x, y), (tag, metric)


def test_bc_loss_angle_metric_counts_a_zero_mean_as_a_right_angle():
    c = _angle_case(3, 7, 5, False, 0, seed=9, zero_rows=True)
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    _gpu_bc(c, False, True, sums)
    mu, tgt, act = _bt(c["mu_tm"]).numpy(), c["target"].numpy(), c["active"].numpy()
    zero = (mu[..., :3] == 0).all(-1) & (act != 0)
    assert zero.sum() >= 10 and ((act != 0) & ~zero).sum() >= 10
    want = (ref.angle(mu, tgt) * act).sum()
    assert want > zero.sum() * np.pi / 2
    s = sums.cpu().numpy()
    assert abs(s[0] - want) <= 1e-5 * want and s[1] == act.sum()
    only = dict(c, active=torch.from_numpy(zero.astype(np.float64)))                  # the zero rows alone: pi / 2 each (fp32's)
    sums.zero_()
    _gpu_bc(only, False, True, sums)
    assert sums[0].item() == zero.sum() * float(np.float32(np.pi / 2))


def _raw_old_entry(c, A, fit_std, wrap0, clip):
    """bc_loss_gauss_fwd_bwd itself (the entry of before, through ctypes) on contiguous batch-major tensors -> outputs and sums"""
    ops = _ops()
    L = ops.load_library()
    f = lambda x: x.float().cuda().contiguous()
    mu, ls, tgt, v = f(_bt(c["mu_tm"])[..., :A]), f(c["ls_tm"])[:A].contiguous(), f(c["target"][..., :A]), f(c["v_tm"].permute(1, 0, 2, 3)[..., 0])
    act, vo, vt = f(c["active"]), f(c["vo"]), f(c["vt"])
    mb, T, P = act.shape
    n = mb * T * P
    asum = act.sum().reshape(1)
    losses, g_mu, g_ls, g_v = torch.empty(2, device="cuda"), torch.empty_like(mu), torch.empty(A, device="cuda"), torch.empty_like(v)
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    ws = torch.empty(L.bc_loss_workspace(), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.bc_loss_gauss_fwd_bwd(n, A, p(mu), p(g_mu), T, P, T * P * A, P * A, A, p(ls), p(g_ls), 0, 0, 0, LO, HI, int(fit_std), int(wrap0), p(tgt),
                                 p(act), p(v), T * P, P, 1, p(vo) if clip else None, p(vt), p(asum), EPS, int(clip), p(losses), p(g_v), p(sums),
                                 p(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    new_sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    mu2, ls2, v2 = mu.clone().requires_grad_(), ls.clone().requires_grad_(), v.clone().requires_grad_()
    la, lc = ops.bc_loss_gauss(mu2, ls2, tgt, v2, act, vo if clip else None, vt, EPS, clip, log_std_min=LO, log_std_max=HI, fit_std=fit_std,
                               wrap0=wrap0, sums=new_sums, metric="mse")
    (la + lc).backward()
    return (losses[0], losses[1], g_mu, g_ls, g_v, sums), (la.detach(), lc.detach(), mu2.grad, ls2.grad, v2.grad, new_sums)


@pytest.mark.parametrize("A,fit_std,wrap0,clip", [(3, False, True, True), (3, True, False, False), (4, True, True, True)])
def test_old_bc_entry_and_new_entry_with_metric_0_give_the_same_bits(A, fit_std, wrap0, clip):
    c = _angle_case(3, 7, 5, False, 1, seed=A)
    old, new = _raw_old_entry(c, A, fit_std, wrap0, clip)
    for k, (x, y) in enumerate(zip(old, new)):
        assert torch.equal(x, y), k
    want = imitation_ref.bc_loss_gauss(_bt(c["mu_tm"]).numpy()[..., :A], c["ls_tm"].numpy()[:A], c["target"].numpy()[..., :A],
                                       c["v_tm"].permute(1, 0, 2, 3)[..., 0].numpy(), c["active"].numpy(), c["vo"].numpy(), c["vt"].numpy(), EPS, clip,
                                       LO, HI, fit_std, wrap0)
    _loss_close(old[0], want["actor_loss"], "old entry actor")                        # and they are still 7f's numbers: sum d^2, wrapped
    _loss_close(old[5][0].item(), want["sq_sum"], "old entry sum d^2")


# ---- agent and trainer ------------------------------------------------------------------------------------------------------------
N_ENVS, T, P_NUM = 16, 20, 3
DIRECTION = {"algo.gauss_squash": "direction"}
BC = {"algo.bc_iterations": 3, "algo.epochs": 2}


def _cfg(**ov):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    return baseline_config("cfg5", **{"runtime.num_envs": N_ENVS, "env.max_steps": T, "env.num_defender": P_NUM, "runtime.e3d_evader": "rule",
                                      **DIRECTION, **ov})


def _agent(cfg, seed=0):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO, make_env
    env = make_env(cfg, N_ENVS)
    torch.manual_seed(seed)
    return E3dMAPPO(cfg, N_ENVS, max(1, round(N_ENVS / 10))), env


def _trainer(cfg, **kw):
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dTrainer
    return E3dTrainer(cfg, num_eval_envs=4, **kw)


def _weights(tr):
    return {f"{n}.{k}": v.clone() for n, m in (("actor", tr.agent.actor), ("critic", tr.agent.critic)) for k, v in m.state_dict().items()}


def _adam_steps(agent):
    return float(next(iter(agent.ac_optimizer.state.values()))["step"])


@pytest.mark.parametrize("std", ["param", "state"])
def test_agent_buffer_and_rollout_update_agreement(std):
    agent, env = _agent(_cfg(**{"algo.gauss_std": std}))
    assert agent.policy_ex and agent.latent_dim == 4 and agent.action_dim == 3 and agent.actor.Mean.weight.shape == (4, 128)
    assert (agent.actor.LogStd.weight.shape == (4, 128)) if std == "state" else (agent.actor.log_std.shape == (4,))
    mean_r, buf, steps, stats = agent.explore_env(env)
    assert steps == N_ENVS * T and buf["a_n"].shape == (N_ENVS, T, P_NUM, 4) and "a_star" not in buf
    assert torch.isfinite(buf["a_n"]).all() and torch.isfinite(buf["a_logprob_n"]).all()
    st = agent._state(env)
    assert st.action.shape == (N_ENVS, P_NUM, 4) and st.env_action.shape == (N_ENVS, P_NUM, 3)
    # the environment received to_env of the stored u: the last tick's pair is still in the rollout state
    assert torch.equal(st.action, buf["a_n"][:, T - 1])
    want = ref.to_env(st.action.cpu().numpy())
    assert np.abs(st.env_action.cpu().numpy() - want).max() <= 1e-12
    with torch.no_grad():
        mu, values, ls_raw = agent.sequence_forward(buf["feat_a"], buf["feat_c"], N_ENVS, T, return_ls_raw=True)
        ls = ls_raw.clamp(agent.log_std_min, agent.log_std_max)
        lp = torch.distributions.Normal(mu, torch.exp(ls)).log_prob(buf["a_n"]).sum(-1)                # no Jacobian term
    live = buf["active"] == 1
    assert live.sum() > 0 and mu.shape == (N_ENVS, T, P_NUM, 4)
    assert (lp - buf["a_logprob_n"])[live].abs().max().item() <= 1e-4
    assert (values - buf["v_n"][:, :T])[live].abs().max().item() <= 1e-4
    with torch.enable_grad():
        agent.train(buf, steps)                                                        # the update runs on the four latent dimensions
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in agent.ac_parameters)


@pytest.mark.timeout(300)
def test_trainer_determinism_and_resume(tmp_path):
    cfg = _cfg(**{"algo.save_cwd": str(tmp_path / "model")})
    path = str(tmp_path / "resume.pt")
    runs = []
    for save in (True, False):
        tr = _trainer(cfg, eval_every=1)
        logs = []
        for it in range(2):
            logs.append(tr.iterate()[1])
            if save and it == 0:
                tr.save_resume(path)
        runs.append((tr, logs))
    (a, logs_a), (b, logs_b) = runs
    assert logs_a == logs_b and all(np.isfinite(log["mean_return"]) and "eval_return" in log for log in logs_a)
    bundle = torch.load(path, map_location="cpu", weights_only=False)
    assert bundle["policy"] == dict(gauss_std="param", gauss_squash="direction", log_std_min=-5.0, log_std_max=2.0)
    c = _trainer(cfg, eval_every=1)
    c.load_resume(path)
    assert c.iterate()[1] == logs_a[1]                                                 # iteration 2 bit for bit
    wa, wc = _weights(a), _weights(c)
    assert list(wa) == list(wc) and all(torch.equal(wa[k], wc[k]) for k in wa)
    assert torch.equal(a.agent._state(a.env).counter, c.agent._state(c.env).counter)
    # another mode's trainer refuses the bundle by the key, before any tensor shape is looked at
    for other in ("clip", "tanh"):
        d = _trainer(_cfg(**{"algo.gauss_squash": other, "algo.save_cwd": str(tmp_path / "model")}))
        with pytest.raises(ValueError, match=r"algo\.gauss_squash"):
            d.load_resume(path)


@pytest.mark.timeout(300)
def test_checkpoints_of_another_mode_are_refused(tmp_path):
    clip_dir, dir_dir = str(tmp_path / "clip"), str(tmp_path / "direction")
    clip, _ = _agent(_cfg(**{"algo.gauss_squash": "clip"}))
    direction, _ = _agent(_cfg())
    clip.save_model(clip_dir)
    direction.save_model(dir_dir)
    assert set(torch.load(clip_dir + "/e3d_state_dicts.pt", map_location="cpu")) == {"actor", "critic"}      # the default file as it was
    sd = torch.load(dir_dir + "/e3d_state_dicts.pt", map_location="cpu")
    assert sd["policy"]["gauss_squash"] == "direction" and sd["actor"]["Mean.weight"].shape == (4, 128)
    with pytest.raises(ValueError, match=r"algo\.gauss_squash"):
        direction.load_model(clip_dir)
    with pytest.raises(ValueError, match=r"algo\.gauss_squash"):
        clip.load_model(dir_dir)
    direction.load_model(dir_dir)


@pytest.mark.timeout(300)
def test_imitation_phase_in_direction_mode():
    cfg = _cfg(**BC, **{"algo.bc_beta": 0.75, "algo.bc_lr": 1e-3, "algo.bc_heading_wrap": True, "algo.bc_target_bound": 0.5})   # read and ignored
    tr = _trainer(cfg, eval_every=1)
    logs = []
    for it in range(4):
        if it == 3:
            assert _adam_steps(tr.agent) == 3 * 2
        logs.append(tr.iterate()[1])
    assert _adam_steps(tr.agent) == 2                                                  # Adam restarted with the first PPO iteration
    buf = tr.agent.buffer
    assert buf["a_star"].shape == (N_ENVS, T, P_NUM, 4) and buf["a_n"].shape == (N_ENVS, T, P_NUM, 4)
    for log in logs[:3]:
        assert log["phase"] == "imitation" and "bc_angle_deg" in log and "bc_action_mse" not in log
        assert 0.0 < log["bc_angle_deg"] < 180.0 and log["bc_loss"] == log["actor_loss"] and np.isfinite(log["bc_loss"])
    assert "bc_angle_deg" not in logs[3] and "phase" not in logs[3]
    assert not tr.agent.bc_wrap0


@pytest.mark.timeout(300)
def test_imitation_labels_and_a_loss_that_falls_on_a_fixed_buffer(monkeypatch):
    agent, env = _agent(_cfg(**BC))
    guides = []
    step = env.step
    monkeypatch.setattr(env, "step", lambda action: (guides.append(env._guidance_out.clone()), step(action))[1])
    _, buf, steps, _ = agent.explore_expert(env, 1.0)
    guides = torch.stack(guides, 1).cpu().numpy()                                      # (N, T, P, 3)
    want = ref.label(guides)
    got = buf["a_star"].cpu().numpy()
    assert got.shape == (N_ENVS, T, P_NUM, 4) and (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    losses, angles = [], []
    for _ in range(30):
        with torch.enable_grad():
            _, bc_loss = agent.train(buf, steps, imitation=True)
        agent.ac_optimizer.step()
        losses.append(bc_loss)
        angles.append(agent.bc_metric(*agent.last_bc))
    # (the ratio is a record, not a criterion)
    print(f"direction: bc_loss {losses[0]:.6g} -> {losses[-1]:.6g} (ratio {losses[-1] / losses[0]:.4f}), bc_angle_deg {angles[0]:.4g} -> {angles[-1]:.4g}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert agent.BC_METRIC == "bc_angle_deg" and 0.0 < angles[-1] < 180.0
