"""The host sampling reference (tests/sampling_ref.py) itself: Philox4x32-10 against the Random123 known-answer vectors, the top draws
the GPU tests place rows on, and the inverse CDF's handling of zero-probability bins."""
import numpy as np
import pytest

from tests import sampling_ref as sr

# counter | key | output of philox4x32_10 (Random123, kat_vectors)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(w) for w in sr.philox4x32_10_words(*ctr, *key)) == out


def test_philox_word0_form_is_the_kernels_call():
    """c0 / c1 = low / high counter word, c2 = c3 = 0, k0 / k1 = low / high seed word, vectorised over counters"""
    ctr = np.array([0, 1, 0xFFFFFFFF, 1 << 32, (1 << 40) + 5, 0x500FCD3FEFA], np.uint64)
    seed = 0xDEADBEEF12345678
    got = sr.philox4x32_10(ctr, seed)
    for c, g in zip(ctr.tolist(), got.tolist()):
        assert g == int(sr.philox4x32_10_words(c & 0xFFFFFFFF, c >> 32, 0, 0, seed & 0xFFFFFFFF, seed >> 32)[0])
    # both seed words and both counter words reach the output
    assert sr.philox4x32_10(ctr, 1 << 32).tolist() != sr.philox4x32_10(ctr, 0).tolist()
    assert sr.philox4x32_10(np.array([1 << 32], np.uint64), 3)[0] != sr.philox4x32_10(np.array([0], np.uint64), 3)[0]


@pytest.mark.parametrize("seed,top", [(3, 2350790), (77, 3895978), (3, 0x10000634706), (0xDEADBEEF12345678, 0x500FCD3FEFA)])
def test_top_draws(seed, top):
    """the (seed, counter) pairs of the GPU top-draw tests give o0 >> 8 == 0xFFFFFF, which the kernels' fp32 u rounds to tot itself"""
    o = int(sr.philox4x32_10(np.array([top], np.uint64), seed)[0])
    assert o >> 8 == 0xFFFFFF
    assert (np.float32(o >> 8) + np.float32(0.5)) * np.float32(1.0 / 16777216.0) == np.float32(1.0)   # ties to even: 2^24
    assert sr.uniform(np.array([top], np.uint64), seed)[0] == 1.0 - 2.0 ** -25


def test_uniform_grid():
    x = sr.uniform(np.arange(1 << 16, dtype=np.uint64), 5)
    assert x.min() > 0 and x.max() < 1
    assert np.all(np.modf(x * 2 ** 24)[0] == 0.5)


def test_inverse_cdf_never_returns_a_zero_probability_bin():
    rng = np.random.default_rng(0)
    R, A = 20000, 7
    p = rng.random((R, A)).astype(np.float32)
    p[rng.random((R, A)) < 0.5] = 0
    one = np.arange(R) % 5 == 0                     # all but one zero
    p[one] = 0
    p[one, rng.integers(0, A, one.sum())] = rng.random(one.sum()).astype(np.float32) + 0.1
    p[p.sum(1) == 0, 3] = 1.0
    ctr = np.arange(R, dtype=np.uint64) + np.uint64((1 << 40) - 100)
    a, amb = sr.inverse_cdf(p, ctr, 9, sr.fp32_band)
    assert np.all(p[np.arange(R), a] > 0)
    assert np.all(a[one] == np.argmax(p[one] > 0, 1))
    assert amb.mean() < 1e-3
    # a top draw on rows whose trailing bins are empty: the last positive bin
    top = 0x10000634706
    q = np.array([[0.2, 0.3, 0, 0], [0.5, 0, 0.5, 0], [0, 0, 0, 1.0], [0, 1.0, 0, 0]], np.float32)
    a, amb = sr.inverse_cdf(q, np.full(4, top, np.uint64), 3, 1e-6)
    assert a.tolist() == [1, 2, 3, 1] and amb.all()
    # all-zero rows stay at A - 1 (out of the samplers' contract, as in the kernels)
    a, _ = sr.inverse_cdf(np.zeros((2, 4), np.float32), np.arange(2, dtype=np.uint64), 3, 0.0)
    assert a.tolist() == [3, 3]


def test_inverse_cdf_follows_the_probabilities():
    """frequencies of the reference's draws match p (a wrong bin mapping would shift them), and the first bin edge above u wins"""
    R = 200000
    p = np.tile(np.array([0.1, 0.0, 0.25, 0.05, 0.6], np.float32), (R, 1))
    a, _ = sr.inverse_cdf(p, np.arange(R, dtype=np.uint64), 11, 0.0)
    freq = np.bincount(a, minlength=5) / R
    assert np.abs(freq - p[0]).max() < 4e-3 and freq[1] == 0
    x = sr.uniform(np.arange(R, dtype=np.uint64), 11)
    assert np.array_equal(a, np.searchsorted(np.cumsum(p[0].astype(np.float64)), x, side="right"))


def test_logp_ref_is_categorical_log_prob():
    import torch
    p = np.array([[0.2, 0.3, 0.5], [1e-9, 0.5, 0.5], [2.0, 0.0, 2.0], [1.0, 0, 0]], np.float32)
    a = np.array([2, 0, 1, 0])
    want = torch.distributions.Categorical(probs=torch.from_numpy(p), validate_args=False).log_prob(torch.from_numpy(a))
    # torch normalises the fp32 probs and clamps to the fp32 epsilon, in fp32
    np.testing.assert_allclose(sr.logp_ref(p, a), want.numpy(), rtol=1e-6, atol=1e-7)
