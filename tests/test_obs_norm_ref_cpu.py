"""CPU checks of algo.use_obs_norm: tests/obs_norm_ref.py behaves as the specification says (the merge is the mean / population
variance of the concatenation, identity before the first merge, the clip, zero rows, the empty batch), csrc/obs_norm.hpp compiled
for the host reproduces it bit for bit, and the option is parsed / refused where it should be."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import obs_norm_ref as ref
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "distributed_multi_agent_reinforcement_learning_amd", "csrc")


def _features(seed, rows, hard=False):
    """raw fp32 features (rows, 16) of both networks with the scales of the real ones: positions with a large offset, angles, flags;
    column 5 is constant (std 0; 0.75, whose sums are exact).  hard: column 7 has mean 1e3 and std 1e-3 -- about the zero mean of an
    empty state its Q - A delta cancels 12 of 16 digits, which the arithmetic must still reproduce bit for bit"""
    rng = np.random.default_rng(seed)
    scale = np.array([5, 5, 5, 3, 1.5, 0.3, 8, 1e-3 if hard else 8, 8, 3, 1.5, 0.3, 0.5, 4, 4, 4])
    offset = np.array([10, 10, 10, 0, 0, 0.7, 0, 1e3 if hard else 0, 0, 0, 0, 0, 0.5, 0, 0, 0])
    out = []
    for _ in range(2):
        x = rng.standard_normal((rows, 16)) * scale + offset
        x[:, 5] = 0.75
        out.append(x.astype(np.float32))
    return out


def _state_after(batches):
    st = ref.new_state()
    for xa, xc in batches:
        ref.merge(st, ref.sums(st, xa, xc, np.ones(len(xa))))
    return st


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_merging_two_batches_gives_the_statistics_of_their_concatenation():
    """rtol 1e-12 on well-conditioned columns: Q - A delta about a mean m off by o loses a factor (o^2 + var) / var, here <= 5"""
    a, b = _features(0, 700), _features(1, 333)
    st = _state_after([a, b])
    for k in range(2):
        x = np.concatenate([a[k], b[k]]).astype(np.float64)
        n, mean, M2 = ref.split(st[k])
        assert n == 1033
        np.testing.assert_allclose(mean, x.mean(0), rtol=1e-12, atol=0)
        var = x.var(0)
        np.testing.assert_allclose(M2 / n, var, rtol=1e-12, atol=0)      # (column 5 is constant: exactly 0 both ways)
        assert M2[5] == 0.0 and var[5] == 0.0
        np.testing.assert_allclose(ref.stats(st[k])[1], x.std(0), rtol=1e-12, atol=0)


def test_identity_before_the_first_merge():
    xa, xc = _features(2, 50)
    on = np.ones(50)
    ya, yc = ref.normalise(ref.new_state(), xa, xc, on, 10.0)
    assert np.array_equal(ya.view(np.uint32), xa.view(np.uint32)) and np.array_equal(yc.view(np.uint32), xc.view(np.uint32))
    # one network merged, the other not: the identity holds per network
    st = _state_after([_features(3, 40)])
    st[1] = 0
    ya, yc = ref.normalise(st, xa, xc, on, 10.0)
    assert not np.array_equal(ya, xa) and np.array_equal(yc.view(np.uint32), xc.view(np.uint32))


def test_clip_acts_at_plus_minus_clip():
    st = _state_after([_features(4, 500)])
    xa, xc = _features(5, 200)
    xa[:, 0] += np.float32(1000.0) * np.sign(xa[:, 0] - 10)      # far outside on both sides
    for clip in (10.0, 2.5):
        ya, yc = ref.normalise(st, xa, xc, np.ones(200), clip)
        assert ya.max() == np.float32(clip) and ya.min() == np.float32(-clip) and np.abs(yc).max() <= np.float32(clip)
        assert set(np.unique(ya[:, 0])) == {np.float32(-clip), np.float32(clip)}
        # the constant column: x == mean gives 0, anything else is over std + 1e-8 = 1e-8 and clipped
        assert np.all(ya[:, 5] == 0)
    inside = np.abs(ref.normalise(st, xa, xc, np.ones(200), 1e6)[1]) < 10
    assert np.array_equal(ref.normalise(st, xa, xc, np.ones(200), 10.0)[1][inside], ref.normalise(st, xa, xc, np.ones(200), 1e6)[1][inside])


def test_zero_rows_stay_zero():
    st = _state_after([_features(6, 300)])
    xa, xc = _features(7, 64)
    on = (np.arange(64) % 3 != 0).astype(np.float64)
    xa[on == 0] = 0
    xc[on == 0] = 0
    ya, yc = ref.normalise(st, xa, xc, on, 10.0)
    assert not ya[on == 0].any() and not yc[on == 0].any() and ya[on != 0].any()
    assert np.abs(-ref.split(st[0])[1] / (ref.stats(st[0])[1] + ref.EPS)).max() > 1      # ... which is not what -mean / std gives


def test_empty_batch_changes_nothing():
    st = _state_after([_features(8, 100)])
    before = st.copy()
    xa, xc = _features(9, 30)
    s = ref.sums(st, xa, xc, np.zeros(30))
    assert not s.any()
    ref.merge(st, s)
    assert np.array_equal(st.view(np.uint64), before.view(np.uint64))
    assert not ref.merge(ref.new_state(), np.zeros((2, ref.ROW))).any()


def test_sums_add_over_ticks_and_ranks():
    """the multi-rank rule: the (2, 33) sums of the parts are added, then one merge -- the state of the whole within f64 summation"""
    st = _state_after([_features(10, 200)])
    xa, xc = _features(11, 400)
    counted = (np.arange(400) % 5 != 0)
    whole = ref.sums(st, xa, xc, counted)
    parts = ref.sums(st, xa[:150], xc[:150], counted[:150]) + ref.sums(st, xa[150:], xc[150:], counted[150:])
    assert np.array_equal(parts[:, 0], whole[:, 0]) and whole[0, 0] == counted.sum()
    a, b = ref.merge(st.copy(), whole), ref.merge(st.copy(), parts)
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)


# ---- csrc/obs_norm.hpp on the host ----------------------------------------------------------------------------------------------------------
HOST_SRC = r"""
#include "obs_norm.hpp"
extern "C" {
void on_normalise(long rows, const float *x, const double *row, double clip, float *y) {
    for (long r = 0; r < rows; r++)
        for (int k = 0; k < obsnorm::COLS; k++)
            y[r * obsnorm::COLS + k] = obsnorm::normalise(x[r * obsnorm::COLS + k], row[0], row[1 + k], row[1 + obsnorm::COLS + k], clip);
}
void on_merge(double *row, const double *s) {
    for (int k = 0; k < obsnorm::COLS; k++)
        obsnorm::merge(row[0], s[0], s[1 + k], s[1 + obsnorm::COLS + k], row[1 + k], row[1 + obsnorm::COLS + k]);
    row[0] = row[0] + s[0];
}
}
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    td = tmp_path_factory.mktemp("obs_norm_host")
    src, lib = td / "obs_norm_host.cpp", td / "libobs_norm_host.so"
    src.write_text(HOST_SRC)
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no system C++ compiler"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + CSRC, str(src), "-o", str(lib)])
    L = C.CDLL(str(lib))
    L.on_normalise.argtypes = [C.c_long, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    L.on_merge.argtypes = [C.c_void_p, C.c_void_p]
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_host_header_matches_the_restatement_bit_for_bit(host_lib):
    st, mine = ref.new_state(), ref.new_state()
    on = np.ones(257)
    for it in range(4):
        xa, xc = _features(20 + it, 257, hard=True)
        # normalise under the state in force (the first pass: n == 0, the identity)
        want = ref.normalise(st, xa, xc, on, 10.0)
        for k, x in enumerate((xa, xc)):
            y = np.empty_like(x)
            host_lib.on_normalise(x.shape[0], _ptr(np.ascontiguousarray(x)), _ptr(mine[k]), 10.0, _ptr(y))
            assert np.array_equal(y.view(np.uint32), want[k].view(np.uint32)), (it, k)
        # merge this batch's sums (the last one is empty: C == 0)
        counted = np.zeros(257) if it == 3 else (np.arange(257) % 7 != it)
        s = ref.sums(st, xa, xc, counted)
        ref.merge(st, s)
        for k in range(2):
            host_lib.on_merge(_ptr(mine[k]), _ptr(np.ascontiguousarray(s[k])))
        assert np.array_equal(mine.view(np.uint64), st.view(np.uint64)), it
    assert st[0, 0] > 0 and st[0, 1 + ref.COLS + 5] == 0.0                 # the constant column: std 0
    mean, sd = ref.stats(st[0])
    assert abs(mean[7] - 1e3) < 1e-2 and sd[7] < 1e-2                    # the column with mean 1e3, std 1e-3 (in fp32 steps of 6e-5)


# ---- options ------------------------------------------------------------------------------------------------------------------------------
def test_option_parses_and_defaults_to_off():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config, load_config, parse_overrides
    from distributed_multi_agent_reinforcement_learning_amd.obs_norm import obs_norm_options
    assert "use_obs_norm" not in load_config().algo and "obs_norm_clip" not in load_config().algo   # config.yaml stays as it is
    assert obs_norm_options(baseline_config("cfg5")) == (False, 10.0)
    ov = parse_overrides(["algo.use_obs_norm=True", "algo.obs_norm_clip=5"])
    assert ov == {"algo.use_obs_norm": True, "algo.obs_norm_clip": 5}
    assert obs_norm_options(baseline_config("cfg5", **ov)) == (True, 5.0)


@pytest.mark.parametrize("clip", [0, 0.0, -1.0, float("inf"), float("nan"), "abc"])
@pytest.mark.parametrize("use", [False, True])
def test_bad_clip_raises_before_the_device_check(clip, use):
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    from distributed_multi_agent_reinforcement_learning_amd.obs_norm import obs_norm_options
    cfg = baseline_config("cfg5", **{"algo.use_obs_norm": use, "algo.obs_norm_clip": clip})
    with pytest.raises(ValueError, match="algo.obs_norm_clip"):
        obs_norm_options(cfg)
    with pytest.raises(ValueError, match="algo.obs_norm_clip"):
        E3dMAPPO(cfg, 8, 1, device="cpu")


def test_e3d_agent_accepts_the_option_up_to_the_device_check():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.e3d_agent import E3dMAPPO
    with pytest.raises(RuntimeError, match="GPU only"):
        E3dMAPPO(baseline_config("cfg5", **{"algo.use_obs_norm": True}), 8, 1, device="cpu")


def test_pursuit_and_n2n_refuse_the_option():
    from distributed_multi_agent_reinforcement_learning_amd.config import baseline_config
    from distributed_multi_agent_reinforcement_learning_amd.mappo import MAPPO
    from distributed_multi_agent_reinforcement_learning_amd.n2n_agent import N2nMAPPO
    with pytest.raises(ValueError, match="algo.use_obs_norm"):
        MAPPO(baseline_config("cfg1", **{"algo.use_obs_norm": True}), 4, 2, "Learner")
    with pytest.raises(ValueError, match="algo.use_obs_norm"):
        N2nMAPPO(baseline_config("cfg4_n2n", **{"algo.use_obs_norm": True}), 8, 1, device="cpu")
    N2n_off = baseline_config("cfg4_n2n", **{"algo.use_obs_norm": False})
    with pytest.raises(RuntimeError, match="GPU only"):       # off: the agent goes on to its device check
        N2nMAPPO(N2n_off, 8, 1, device="cpu")
