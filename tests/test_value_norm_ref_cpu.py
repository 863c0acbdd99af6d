"""CPU checks of algo.use_value_norm: tests/value_norm_ref.py behaves as the specification says (identity before the first update,
the first update's statistics, the variance floor, the empty batch, additivity of the sums over ranks, the masked
denormalisation), and the option is parsed / refused where it should be."""
import numpy as np
import pytest

from tests import value_norm_ref as ref

EPS = 2.0 ** -52   # f64 machine epsilon


def _batch(seed, shape=(6, 11, 4), mean=3.0, std=2.5):
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(shape) * std + mean).astype(np.float32)
    active = (rng.random(shape) < 0.8).astype(np.float32)
    return y, active


def test_identity_before_any_update():
    st = ref.new_state()
    assert ref.stats(st) == (0.0, 1.0)
    y, active = _batch(0)
    assert np.array_equal(ref.denormalise(st, y, active), np.where(active != 0, y.astype(np.float64), 0.0))
    assert np.array_equal(ref.targets(st, y, active), np.where(active != 0, y.astype(np.float64), 0.0))


@pytest.mark.parametrize("beta", [0.99999, 0.9, 0.5])
def test_first_update_gives_the_batch_statistics(beta):
    """after one update from the zero state the debiased mean IS the batch mean and the variance the batch variance (floored):
    m / d = (1 - beta) mean / (1 - beta).  Each of m / d and q / d is two roundings of an exact ratio -> within a few eps."""
    y, active = _batch(1)
    live = y.astype(np.float64)[active != 0]
    st = ref.update(ref.new_state(), ref.sums(y, active), beta)
    mean, sd = ref.stats(st)
    assert abs(mean - live.mean()) <= 4 * EPS * np.abs(live).mean()
    var = (live ** 2).mean() - live.mean() ** 2
    assert var > ref.VAR_MIN
    assert abs(sd - np.sqrt(var)) <= 8 * EPS * (live ** 2).mean() / np.sqrt(var)
    assert st[2] == np.float64(1.0) - np.float64(beta)


def test_variance_floor():
    y = np.full((2, 3, 4), 7.0, np.float32) + np.float32(0.01) * np.arange(24, dtype=np.float32).reshape(2, 3, 4) / 24
    active = np.ones_like(y)
    st = ref.update(ref.new_state(), ref.sums(y, active), 0.99)
    mean, sd = ref.stats(st)
    assert sd == np.sqrt(1e-2) and abs(mean - y.astype(np.float64).mean()) < 1e-12


def test_empty_batch_changes_nothing():
    y, active = _batch(2)
    st = ref.update(ref.new_state(), ref.sums(y, active), 0.999)
    before = st.copy()
    ref.update(st, ref.sums(y, np.zeros_like(active)), 0.999)
    assert np.array_equal(st.view(np.uint64), before.view(np.uint64))
    z = ref.update(ref.new_state(), np.zeros(3), 0.999)
    assert not z.any() and ref.stats(z) == (0.0, 1.0)


def test_sums_of_two_halves_give_the_state_of_the_whole():
    """the multi-rank rule: (S1, S2, c) of the ranks are added, then one update"""
    y, active = _batch(3, shape=(8, 9, 4))
    s_full = ref.sums(y, active)
    s_sum = ref.sums(y[:4], active[:4]) + ref.sums(y[4:], active[4:])
    assert s_sum[2] == s_full[2]
    a = ref.update(ref.update(ref.new_state(), s_full, 0.99), s_full, 0.99)
    b = ref.update(ref.update(ref.new_state(), s_sum, 0.99), s_sum, 0.99)
    n = s_full[2]
    assert np.all(np.abs(a - b) <= n * EPS * np.abs(a))
    assert ref.stats(a)[0] == pytest.approx(ref.stats(b)[0], rel=1e-13)


def test_masked_denormalisation_keeps_zeroed_rows_at_zero():
    st = ref.update(ref.new_state(), np.array([50.0, 350.0, 10.0]), 0.9)   # mean 5, var 10
    mean, sd = ref.stats(st)
    assert mean == pytest.approx(5.0) and sd == pytest.approx(np.sqrt(10.0))
    N, T, P = 3, 5, 2
    rng = np.random.default_rng(4)
    active = np.ones((N, T, P), np.float32)
    active[1, 3:] = 0                    # an episode that ended after step 2
    active[2, :, 1] = 0                  # a pursuer dead from the start
    vmask = np.array([[1, 1], [0, 0], [1, 0]], np.float32)
    v = rng.standard_normal((N, T + 1, P)).astype(np.float32) * ref.value_masks(active, vmask)
    r = rng.standard_normal((N, T, P)).astype(np.float32) * active
    adv, vt = ref.gae(st, r, v, active, vmask, 0.99, 0.95, use_adv_norm=False)
    assert np.all(adv[active == 0] == 0) and np.all(vt[active == 0] == 0)
    # the last live step of episode 1 bootstraps from 0, not from the mean: delta = r - v_denorm
    d = r[1, 2].astype(np.float64) - (v[1, 2].astype(np.float64) * sd + mean)
    assert np.allclose(adv[1, 2], d, rtol=0, atol=1e-12)
    # and the targets are 0 off the live rows, (y - mean) / std on them
    tg = ref.targets(st, vt, active)
    assert np.all(tg[active == 0] == 0) and np.allclose(tg[active != 0] * sd + mean, vt[active != 0])


def test_option_parses_and_defaults_to_off():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config, load_config, parse_overrides
    from distributed_multi_agent_reinforcement_learning_amd.value_norm import value_norm_options
    assert "use_value_norm" not in load_config().algo and "value_norm_beta" not in load_config().algo   # config.yaml stays as it is
    for name in ("cfg5", "cfg4_n2n"):
        assert value_norm_options(baseline_config(name)) == (False, 0.99999)
        ov = parse_overrides(["algo.use_value_norm=True", "algo.value_norm_beta=0.999"])
        assert ov == {"algo.use_value_norm": True, "algo.value_norm_beta": 0.999}
        assert value_norm_options(baseline_config(name, **ov)) == (True, 0.999)


@pytest.mark.parametrize("beta", [0.0, 1.0, -0.5, 1.5])
@pytest.mark.parametrize("use", [False, True])
def test_bad_beta_raises_on_both_agents_before_the_device_check(beta, use):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO
    ov = {"algo.use_value_norm": use, "algo.value_norm_beta": beta}
    with pytest.raises(ValueError, match="algo.value_norm_beta"):
        E3dMAPPO(baseline_config("cfg5", **ov), 8, 1, device="cpu")
    with pytest.raises(ValueError, match="algo.value_norm_beta"):
        N2nMAPPO(baseline_config("cfg4_n2n", **ov), 8, 1, device="cpu")


def test_pursuit_refuses_the_option():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
    with pytest.raises(ValueError, match="algo.use_value_norm"):
        MAPPO(baseline_config("cfg1", **{"algo.use_value_norm": True}), 4, 2, "Learner")
