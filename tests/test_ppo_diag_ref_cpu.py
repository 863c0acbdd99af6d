"""CPU checks of the update diagnostics: the identities of tests/ppo_diag_ref.py, csrc/ppo_diag.hpp compiled for the host against it bit
for bit, the parsing of algo.update_diagnostics / algo.target_kl, and the early-stop rule."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import ppo_diag_ref as ref

EPS = 0.2


def _rows(n, seed, lr_scale=0.1):
    rng = np.random.default_rng(seed)
    lp_old = rng.standard_normal(n).astype(np.float32) * 3
    lp_now = (lp_old + rng.standard_normal(n).astype(np.float32) * np.float32(lr_scale)).astype(np.float32)
    lr = (lp_now - lp_old).astype(np.float32)
    ratio = np.exp(lr.astype(np.float64)).astype(np.float32)
    ent = rng.standard_normal(n).astype(np.float32) + 2
    v_tgt = (rng.standard_normal(n) * 3 + 1).astype(np.float32)
    v_now = (v_tgt + rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    active = (rng.random(n) > 0.3).astype(np.float32)
    return dict(lr=lr, ratio=ratio, ent=ent, v_now=v_now, v_tgt=v_tgt, active=active)


def _terms(r, eps=EPS):
    return ref.row_terms(r["lr"], r["ratio"], r["ent"], r["v_now"], r["v_tgt"], r["active"], eps)


# ---- the restatement's identities ---------------------------------------------------------------------------------------------------------
def test_same_policy_gives_zero_kl_no_clip_and_ratio_one():
    r = _rows(1000, 0)
    r["lr"] = np.zeros_like(r["lr"])
    r["ratio"] = np.ones_like(r["ratio"])
    s = ref.sums(_terms(r))
    assert s[1] == 0 and s[2] == 0 and s[7] == s[0] == (r["active"] != 0).sum()
    d = ref.derive(s)
    assert d["approx_kl"] == 0 and d["clip_fraction"] == 0 and d["ratio_mean"] == 1


def test_perfect_critic_explains_all_variance():
    r = _rows(1000, 1)
    r["v_now"] = r["v_tgt"].copy()
    assert ref.derive(ref.sums(_terms(r)))["explained_variance"] == 1.0
    r["v_tgt"][:] = 2.5                       # no variance in the targets: NaN
    assert math.isnan(ref.derive(ref.sums(_terms(r)))["explained_variance"])


@pytest.mark.parametrize("scale", [1e-8, 1e-3, 0.1, 5.0])
def test_k3_is_non_negative(scale):
    t = _terms(_rows(2000, 2, scale))
    assert (t[:, 1] >= 0).all() and ref.sums(t)[1] >= 0
    if scale <= 1e-3:                          # f64 expm1: lr^2 / 2 survives where exp(lr) - 1 - lr in fp32 would be 0 or noise
        live = t[:, 0] != 0
        x = _rows(2000, 2, scale)["lr"].astype(np.float64)[live]
        np.testing.assert_allclose(t[live, 1], x * x / 2, rtol=1e-2 if scale > 1e-6 else 1e-6, atol=1e-300)


def test_inactive_rows_change_nothing():
    r = _rows(500, 3)
    live = r["active"] != 0
    kept = {k: v[live] for k, v in r.items()}
    a, b = _terms(r), _terms(kept)
    assert np.array_equal(a[live], b) and not a[~live].any()
    r2 = {k: v.copy() for k, v in r.items()}
    for k in ("lr", "ratio", "ent", "v_now", "v_tgt"):
        r2[k][~live] = 1e30                    # whatever an inactive row holds
    assert np.array_equal(_terms(r2), a)
    r["active"] = r["active"] * 7.0            # a live row counts once, it is not weighted by active
    assert np.array_equal(_terms(r), a)


def test_no_live_row_gives_nans():
    r = _rows(64, 4)
    r["active"][:] = 0
    s = ref.sums(_terms(r))
    assert not s.any() and all(math.isnan(v) for v in ref.derive(s).values())
    from distributed_multi_agent_reinforcement_learning_amd.update_diag import derive
    assert all(math.isnan(v) for v in derive(s).values())


def test_package_derive_is_the_restatement():
    from distributed_multi_agent_reinforcement_learning_amd.update_diag import DERIVED, derive
    s = ref.sums(_terms(_rows(777, 5)))
    assert derive(s) == ref.derive(s) and tuple(derive(s)) == DERIVED


# ---- csrc/ppo_diag.hpp on the host ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-8, 1e-5, 0.05, 1.0, 20.0])
def test_host_row_step_matches_the_restatement_bit_for_bit(scale):
    from distributed_multi_agent_reinforcement_learning_amd import ops
    L = ops.load_library()
    n = 4096
    r = _rows(n, 6, 1.0)
    rng = np.random.default_rng(7)
    # |lr| around the given scale, or (20.0) log-uniform from 1e-8 all the way up to 20
    mag = scale * rng.uniform(0.5, 1.0, n) if scale != 20.0 else 10.0 ** rng.uniform(-8.0, math.log10(20.0), n)
    r["lr"] = (np.sign(rng.standard_normal(n)) * mag).astype(np.float32)
    r["ratio"] = np.exp(r["lr"].astype(np.float64)).astype(np.float32)
    assert np.abs(r["lr"]).max() <= 20.0 and (scale != 20.0 or (np.abs(r["lr"]).max() > 10 and np.abs(r["lr"]).min() < 1e-7))
    out = np.empty((n, ref.NSUM))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.ppo_diag_rows_host(n, ptr(r["lr"]), ptr(r["ratio"]), ptr(r["ent"]), ptr(r["v_now"]), ptr(r["v_tgt"]), ptr(r["active"]), EPS, ptr(out))
    assert rc == 0
    want = _terms(r, np.float32(EPS))
    assert (want[:, 2] != 0).any() == (scale >= 1.0)          # the large steps leave the clip range, the small ones never do
    assert np.array_equal(out.view(np.uint64), want.view(np.uint64))


# ---- options ------------------------------------------------------------------------------------------------------------------------------
def _agents():
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO
    return (("cfg5", E3dMAPPO), ("cfg4_n2n", N2nMAPPO))


def test_options_parse_and_default_to_off():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config, load_config, parse_overrides
    from distributed_multi_agent_reinforcement_learning_amd.update_diag import update_diag_options
    assert "update_diagnostics" not in load_config().algo and "target_kl" not in load_config().algo      # config.yaml stays as it is
    for name in ("cfg5", "cfg4_n2n", "cfg1"):
        assert update_diag_options(baseline_config(name)) == (False, None)
        assert update_diag_options(baseline_config(name, **parse_overrides(["algo.update_diagnostics=True"]))) == (True, None)
        assert update_diag_options(baseline_config(name, **parse_overrides(["algo.target_kl=0.02"]))) == (True, 0.02)      # implies diagnostics
        assert update_diag_options(baseline_config(name, **{"algo.update_diagnostics": False, "algo.target_kl": 1})) == (True, 1.0)


@pytest.mark.parametrize("bad", [0, 0.0, -0.01, float("inf"), float("nan"), "0.02", "abc", True])
def test_bad_target_kl_raises_naming_the_key(bad):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    for name, Agent in _agents():
        with pytest.raises(ValueError, match="algo.target_kl"):
            Agent(baseline_config(name, **{"algo.target_kl": bad}), 8, 1, device="cpu")     # raised before the device check


def test_pursuit_refuses_target_kl():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
    with pytest.raises(ValueError, match="algo.target_kl"):
        MAPPO(baseline_config("cfg1", **{"algo.target_kl": 0.02}), 4, 2, "Learner")


# ---- the stop rule --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kls,target,want", [
    ([0.0, 0.01, 0.03, 0.05], 0.02, 2),          # the first epoch over the target; two optimizer steps were taken
    ([0.0, 0.01, 0.02, 0.02], 0.02, None),       # equal is not over
    ([0.5], 0.02, 0),                            # over at once: no step at all
    ([0.0, 0.03, 0.01], 0.02, 1),                # the first one, whatever follows
    ([0.0, 0.01], None, None),                   # no target
    ([], 0.02, None),
    ([0.0, math.nan, 0.03], 0.02, 2),            # no live row (NaN) is not over
])
def test_stop_rule(kls, target, want):
    from distributed_multi_agent_reinforcement_learning_amd.update_diag import first_epoch_over
    assert first_epoch_over(kls, target) == want and ref.stop_epoch(kls, target) == want
