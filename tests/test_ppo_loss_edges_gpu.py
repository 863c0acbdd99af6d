"""The four PPO loss launches (k_ppo_loss, k_ppo_loss_prob, k_ppo_loss_gauss, k_ppo_loss_gauss_ex) and the teacher launches that
inline the same row against the f64 restatements, on the inputs of tests/ppo_edges_cases.py: rows exactly on every closed-interval
decision of ppo_elem and of the two hand-written clamp rules (compared element by element), random rows at every row count, view and
action count, upstream gradients other than 1, and repeatability.  tests/test_ppo_edges_cases_cpu.py holds the same inputs and the
restatement to torch autograd without a GPU."""
import numpy as np
import pytest
import torch

from tests import gauss_sd_ref as gs
from tests import ppo_edges_cases as pc

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD = 5                 # a column block [..., 2:2 + A] of a (.., A + PAD) buffer
# view -> the storage of (the policy's operand, a per-row ls_raw, values_now)
LAYOUTS = {"time_major": ("tm", "tm", "tm"), "batch_major": ("bm", "bm", "bm"), "column_block": ("block", "block", "tm"),
           "value_slice": ("tm", "tm", "slice"), "mixed": ("tm", "bm", "bm")}


def _ops():
    from distributed_multi_agent_reinforcement_learning_amd import ops
    return ops


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _operand(x, layout):
    """(d0, d1, d2, K) numpy -> (leaf, the view of that shape the loss gets, a function -> its gradient in that shape).  What lies
    around a column block or a slice is NaN: a read outside the view would show, and its gradient has to stay 0."""
    K = x.shape[-1]
    if layout == "tm":
        leaf = _dev(np.swapaxes(x, 0, 1)).requires_grad_()
        return leaf, leaf.transpose(0, 1), lambda: leaf.grad.transpose(0, 1)
    if layout == "bm":
        leaf = _dev(x).requires_grad_()
        return leaf, leaf, lambda: leaf.grad
    lo, width = (2, K + PAD) if layout == "block" else (1, 3)
    buf = np.full(x.shape[:3] + (width,), np.nan, F32)
    buf[..., lo:lo + K] = x
    leaf = _dev(buf).requires_grad_()

    def grad():
        g = leaf.grad
        assert not g[..., :lo].any() and not g[..., lo + K:].any()
        return g[..., lo:lo + K]
    return leaf, leaf[..., lo:lo + K], grad


def _values(x, layout):
    leaf, view, grad = _operand(x[..., None], layout)
    return leaf, view[..., 0], lambda: grad()[..., 0]


def _run(c, value_clip, view="time_major", diag=None, scale=(1.0, 1.0), teacher=False):
    """one loss call on fresh leaves -> dict: la, lc, grads (device tensors in the logical shape, in the order of
    ppo_edges_cases.reference), leaves"""
    ops, kind = _ops(), c["kind"]
    pol, lsl, vl = LAYOUTS[view]
    d = {k: _dev(c[k]) for k in ("adv", "v_old", "v_tgt", "active", "lp_old")}
    tail = (d["lp_old"], d["adv"], d["active"], d["v_old"] if value_clip else None, d["v_tgt"], float(c["eps"]), float(c["ent_coef"]))
    kw = {} if diag is None else {"diag": diag}
    if kind == "plain":
        leaves = [_dev(c[k]).requires_grad_() for k in ("lp_now", "ent", "v_now")]
        grads = [lambda t=t: t.grad for t in leaves]
        la, lc = ops.ppo_loss(*leaves, *tail, value_clip, **kw)
    else:
        v_leaf, v, g_v = _values(c["v_now"], vl)
        action = _dev(c["action"])
        if kind == "prob":
            leaf, p, g_p = _operand(c["prob"], pol)
            leaves, grads = [leaf, v_leaf], [g_p, g_v]
            if teacher:
                la, lc = ops.ppo_bc_loss_cat(p, action, action, v, *tail, 0.0, value_clip)
            else:
                la, lc = ops.ppo_loss_prob(p, action, v, *tail, value_clip, **kw)
        else:
            m_leaf, mu, g_mu = _operand(c["mu"], pol)
            if c["state"]:
                l_leaf, ls, g_ls = _operand(c["ls"], lsl)
            else:
                l_leaf = ls = _dev(c["ls"]).requires_grad_()
                g_ls = lambda: l_leaf.grad
            leaves, grads = [m_leaf, l_leaf, v_leaf], [g_mu, g_ls, g_v]
            pk = dict(log_std_min=c["lo"], log_std_max=c["hi"], squash=c["squash"])
            if teacher:
                la, lc = ops.ppo_bc_loss_gauss(mu, ls, action, action, v, *tail, 0.0, value_clip, **pk)
            elif kind == "gauss":
                la, lc = ops.ppo_loss_gauss(mu, ls, action, v, *tail, value_clip, **kw)
            else:
                la, lc = ops.ppo_loss_gauss_ex(mu, ls, action, v, *tail, value_clip, **pk, **kw)
    (scale[0] * la + scale[1] * lc).backward()
    return dict(la=la.detach(), lc=lc.detach(), grads=[g() for g in grads], leaves=leaves)


def _np64(t):
    return t.detach().double().cpu().numpy()


def _flat(out):
    return [out["la"], out["lc"]] + out["grads"]


def _same_bits(a, b, tag):
    for x, y in zip(_flat(a), _flat(b)):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), tag


def _each(got, want, tag):
    """element by element: |got - want| <= 1e-5 |want| + 1e-12, and an exact 0 where the reference is exactly 0.  A factor 1/2 on one
    edge row cannot hide behind a larger neighbour."""
    got, want = _np64(got) if torch.is_tensor(got) else np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err, bound = np.abs(got - want), 1e-5 * np.abs(want) + 1e-12
    k = np.argmax(err / bound)
    print(f"{tag}: closest to its bound, element {k}: got {got.reshape(-1)[k]:.9g} want {want.reshape(-1)[k]:.9g} (err {err.reshape(-1)[k]:.3e}, bound {bound.reshape(-1)[k]:.3e})")
    assert np.all(err <= bound), (tag, int(k), got.reshape(-1)[k], want.reshape(-1)[k])
    assert np.all(got[want == 0] == 0), tag


def _each_all(out, ref, tag):
    _each(out["la"], ref["la"], tag + " actor loss")
    _each(out["lc"], ref["lc"], tag + " critic loss")
    for k, (g, w) in enumerate(zip(out["grads"], ref["grads"])):
        _each(g, w, f"{tag} gradient {k}")


def _loss_close(got, want, tag):
    print(f"{tag}: {float(got):.9g} against {float(want):.9g}")
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)) + 1e-7, (tag, float(got), float(want))


def _close(got, want, tag):
    got, want = _np64(got), _np64(want) if torch.is_tensor(want) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f"{tag}: max error {err:.3e}, max |ref| {scale:.3e}")
    assert err <= 1e-5 * scale + 1e-12, (tag, err, scale)
    return err, scale


def _bulk_check(c, out, ref, tag, scale=(1.0, 1.0)):
    """the project's tolerances: losses to 1e-5 |want| + 1e-7, a gradient's largest error to 1e-5 max |ref| + 1e-12; the gradient rows
    of inactive rows exactly 0"""
    _loss_close(out["la"], ref["la"], tag + " actor loss")
    _loss_close(out["lc"], ref["lc"], tag + " critic loss")
    dead = _dev(c["active"]) == 0
    n = len(ref["grads"])
    for k, (g, w) in enumerate(zip(out["grads"], ref["grads"])):
        _close(g, np.asarray(w) * (scale[1] if k == n - 1 else scale[0]), f"{tag} gradient {k}")
        if g.dim() >= 3:                                   # (the log_std vector of param mode has no rows)
            assert not g[dead].any(), (tag, k, "an inactive row has a gradient")


def _strides_kept(out, tag):
    for leaf in out["leaves"]:                              # (the stride over a dimension of one entry says nothing)
        assert leaf.grad.shape == leaf.shape, tag
        assert all(g == s for n, g, s in zip(leaf.shape, leaf.grad.stride(), leaf.stride()) if n > 1), (tag, leaf.grad.stride(), leaf.stride())


def _diag_and_repeat(c, value_clip, out, tag, view="time_major"):
    """the diag= form carries the plain call's bytes, and a second plain launch gives the same bits"""
    _same_bits(out, _run(c, value_clip, view), tag + " repeat")
    if not (c["kind"] == "gauss_ex" and c["state"] and c["A"] > 8):
        diag = torch.zeros(8, dtype=torch.float64, device="cuda")
        _same_bits(out, _run(c, value_clip, view, diag=diag), tag + " diag")
        assert diag[0].item() == float((c["active"] != 0).sum())


def _teacher(c, value_clip, out, tag, ref=None):
    """ppo_bc_loss_gauss / ppo_bc_loss_cat at coef 0 on the same rows: the critic loss and g_v are the PPO launch's bytes, the actor
    outputs lie within the tolerances of checks 2-3 of tests/test_kickstart_gpu.py; with ref, they are also held to the restatement
    element by element (the two clamp rules are the PPO launch's: cat_pass, gauss_ls_pass)"""
    t = _run(c, value_clip, teacher=True)
    if ref is not None:
        _each_all(t, ref, tag + " teacher")
    assert torch.equal(t["lc"], out["lc"]) and torch.equal(t["grads"][-1], out["grads"][-1]), tag
    _loss_close(t["la"], out["la"].double(), tag + " teacher actor loss")
    for k, (g, w) in enumerate(zip(t["grads"][:-1], out["grads"][:-1])):
        _close(g, w, f"{tag} teacher gradient {k}")
    _same_bits(t, _run(c, value_clip, teacher=True), tag + " teacher repeat")


# ---- (a) the edge batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", pc.POLICY_EDGES)
def test_policy_clip_edges(d):
    """ratio == 1 + eps (d > 0) or 1 - eps (d < 0) exactly, with eps taken from the device's own expf(d)"""
    lrs = pc.policy_clip_lrs(d)
    lr, ratios = _ops().ppo_ratio(_dev(lrs), torch.zeros(len(lrs), device="cuda"))
    assert np.array_equal(lr.cpu().numpy(), lrs)
    c = pc.policy_clip_batch(d, ratios.cpu().numpy())
    live = c["active"].reshape(-1) != 0
    seen = {s: int(((c["side"] == s) & live).sum()) for s in (-1, 0, 1)}
    print(f"d = {d}: eps = {c['eps']!r}, rows inside / on / outside the edge: {seen}")
    assert all(seen.values())                                   # the steps of d reached both sides of the edge
    for value_clip in (True, False):
        out, ref = _run(c, value_clip), pc.reference(c, value_clip)
        tag = f"policy clip d={d} clip={value_clip}"
        _each_all(out, ref, tag)
        g_lp = _np64(out["grads"][0]).reshape(-1)
        blocked = (c["side"] == 1) & (c["factor"] == 0)
        assert blocked.any() and np.all(g_lp[blocked] == 0) and np.all(g_lp[(c["side"] == 0) & live & (c["adv"].reshape(-1) != 0)] != 0)
        _diag_and_repeat(c, value_clip, out, tag)


VALUE_EDGE_VARIANTS = {"plain": ("plain", 0, False, "clip"), "prob": ("prob", 5, False, "clip"), "gauss": ("gauss", 3, False, "clip"),
                       "ex_param_clip": ("gauss_ex", 4, False, "clip"), "ex_state_tanh": ("gauss_ex", 3, True, "tanh")}


@pytest.mark.parametrize("value_clip", [True, False])
@pytest.mark.parametrize("name", list(VALUE_EDGE_VARIANTS))
def test_value_clip_edges(name, value_clip):
    """v_now - v_old == -+eps exactly, one fp32 step to either side, and the qa == qb tie outside the clip range, in every kernel"""
    c = pc.value_clip_case(*VALUE_EDGE_VARIANTS[name])
    out, ref = _run(c, value_clip), pc.reference(c, value_clip)
    tag = f"value clip {name} clip={value_clip}"
    _each(out["lc"], ref["lc"], tag + " critic loss")
    _each(out["grads"][-1], ref["grads"][-1], tag + " g_v")
    _diag_and_repeat(c, value_clip, out, tag)
    if name != "plain":
        _teacher(c, value_clip, out, tag)


@pytest.mark.parametrize("ent_coef", [0.0, pc.CAT_ENT])
@pytest.mark.parametrize("A", [2, 16])
def test_categorical_clamp_edges(A, ent_coef):
    """probabilities exactly on finfo(float32).eps and 1 - eps32 (the gradient passes) and half an eps beyond (blocked)"""
    c = pc.categorical_case(A, ent_coef)
    out, ref = _run(c, True), pc.reference(c, True)
    tag = f"categorical clamp A={A} ent={ent_coef}"
    _each_all(out, ref, tag)
    _diag_and_repeat(c, True, out, tag)
    _teacher(c, True, out, tag, ref)


@pytest.mark.parametrize("squash", ["clip", "tanh"])
@pytest.mark.parametrize("state", [False, True], ids=["param", "state"])
def test_log_std_bound_edges(state, squash):
    """ls_raw exactly on log_std_min and log_std_max (the gradient flows) and one fp32 step to either side of each"""
    c = pc.log_std_case(state, squash)
    out, ref = _run(c, True), pc.reference(c, True)
    tag = f"log-std bounds state={state} {squash}"
    _each_all(out, ref, tag)
    _diag_and_repeat(c, True, out, tag)
    _teacher(c, True, out, tag, ref)


# ---- (b) bulk: every row count, every view -------------------------------------------------------------------------------------------------
def _key(name, shape):
    kind, A, state, squash = pc.VARIANTS[name]
    return (kind, shape, A, state, squash)


@pytest.mark.parametrize("value_clip", [True, False])
@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", list(pc.VARIANTS))
def test_bulk_rows(name, shape, value_clip):
    key = _key(name, shape)
    c, ref = pc.bulk_case(*key), pc.bulk_reference(value_clip, *key)
    out = _run(c, value_clip)
    _bulk_check(c, out, ref, f"{name} {shape} clip={value_clip}")
    _strides_kept(out, name)


@pytest.mark.parametrize("shape", pc.VIEW_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("view", pc.VIEWS)
@pytest.mark.parametrize("name", [n for n in pc.VARIANTS if n != "plain"])
def test_bulk_views(name, view, shape):
    key = _key(name, shape)
    value_clip = pc.VIEWS.index(view) % 2 == 0
    c, ref = pc.bulk_case(*key), pc.bulk_reference(value_clip, *key)
    out = _run(c, value_clip, view)
    _bulk_check(c, out, ref, f"{name} {shape} {view} clip={value_clip}")
    _strides_kept(out, name)
    _same_bits(out, _run(c, value_clip, "time_major"), f"{name} {view}: the bytes do not depend on the storage")


@pytest.mark.parametrize("value_clip", [True, False])
@pytest.mark.parametrize("shape", pc.VIEW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sharp_probabilities_against_f64(shape, value_clip):
    """k_ppo_loss_prob at logits of scale 40: probabilities below eps32, where the clamp blocks the gradient, and at 1.  Beside the
    kernel's error stands that of torch's own fp32 op-by-op graph on the device against the same f64 reference."""
    key = ("prob", shape, 9, False, "clip", pc.SHARP)
    c, ref = pc.bulk_case(*key), pc.bulk_reference(value_clip, *key)
    out = _run(c, value_clip)
    tag = f"sharp prob {shape} clip={value_clip}"
    leaf, p, g_p = _operand(c["prob"], "tm")
    v_leaf, v, g_v = _values(c["v_now"], "tm")
    d = {k: _dev(c[k]) for k in ("adv", "v_old", "v_tgt", "active", "lp_old", "action")}
    dist = torch.distributions.Categorical(p, validate_args=False)          # (prob is unnormalised: Categorical renormalises, as the kernel)
    la, lc = gs.torch_ppo_rows(torch.exp(dist.log_prob(d["action"]) - d["lp_old"]), dist.entropy(), v, d["adv"], d["active"],
                               d["v_old"] if value_clip else None, d["v_tgt"], c["eps"], c["ent_coef"], value_clip)
    (la + lc).backward()
    want = np.asarray(ref["grads"][0])
    e_torch, e_kernel = np.abs(_np64(g_p()) - want).max(), np.abs(_np64(out["grads"][0]) - want).max()
    print(f"{tag}: g_prob error of the kernel {e_kernel:.3e}, of torch's fp32 graph {e_torch:.3e}, max |ref| {np.abs(want).max():.3e}")
    _bulk_check(c, out, ref, tag)


# ---- (c) every compiled action count ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", range(1, 17))
@pytest.mark.parametrize("name", list(pc.A_VARIANTS))
def test_every_action_count(name, A):
    kind, state, squash = pc.A_VARIANTS[name]
    for k, shape in enumerate(pc.A_SHAPES):
        key = (kind, shape, A, state, squash)
        value_clip = (A + k) % 2 == 0
        c, ref = pc.bulk_case(*key), pc.bulk_reference(value_clip, *key)
        out = _run(c, value_clip)
        tag = f"{name} A={A} {shape} clip={value_clip}"
        _bulk_check(c, out, ref, tag)
        if state and A <= 8:                                # the DIAG instances of state mode: the same bytes
            _same_bits(out, _run(c, value_clip, diag=torch.zeros(8, dtype=torch.float64, device="cuda")), tag + " diag")
        elif state:                                         # beyond the head's action count: refused, no launch
            with pytest.raises(RuntimeError, match="bad argument"):
                _run(c, value_clip, diag=torch.zeros(8, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("state", [False, True], ids=["param", "state"])
def test_direction_mode_at_four_latent_dimensions(state):
    for k, shape in enumerate(pc.A_SHAPES):
        key = ("gauss_ex", shape, 4, state, "direction")
        c, ref = pc.bulk_case(*key), pc.bulk_reference(k == 0, *key)
        out = _run(c, k == 0)
        _bulk_check(c, out, ref, f"direction state={state} {shape}")
        clip = dict(c, squash="clip")                       # the clip instance: no Jacobian term
        _same_bits(out, _run(clip, k == 0), "direction is the clip instance")


# ---- (e) upstream gradients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.VARIANTS))
def test_upstream_gradients_scale_the_saved_ones(name):
    """(2 la - 3 lc).backward(): the autograd functions scale the launch's gradients by the upstream ones"""
    key = _key(name, (3, 17, 5))
    c, ref = pc.bulk_case(*key), pc.bulk_reference(True, *key)
    out = _run(c, True, scale=(2.0, -3.0))
    _bulk_check(c, out, ref, f"{name} upstream (2, -3)", scale=(2.0, -3.0))
    one = _run(c, True)
    n = len(one["grads"])
    for k, (g, w) in enumerate(zip(out["grads"], one["grads"])):
        assert torch.equal(g, w * (-3.0 if k == n - 1 else 2.0)), (name, k)      # exact: a power of two, and 3 x in one rounding
