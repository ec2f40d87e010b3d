"""The numpy restatement of rt_denoise (tests/denoise_ref.py) against what it must reduce to (no GPU needed).

With all stops off, one pass, non-negative data and a pixel at least 2 from the border, the filter is the plain
convolution with K (x) K: 25 products, 25 sums and one quotient per channel, each rounding by at most 2^-24
relative, all terms non-negative -- so the restatement must equal an f64 convolution within 64 * 2^-24 relative
(51 roundings, rounded up).  And the host side of the colour stop: ic0 = 1.0f / SigmaColor and every
ic = ic0 * 2^i are exact power-of-two multiples of ic0."""
import numpy as np
import pytest

import denoise_ref as dr

F = np.float32
REL = 64 * 2.0 ** -24


def planes(h, w, seed, one_key=True):
    rng = np.random.default_rng(seed)
    mean = np.zeros((h, w, 4), np.float32)
    mean[..., :3] = rng.random((h, w, 3), dtype=np.float32) * F(4.0)
    mean[..., 3] = rng.random((h, w), dtype=np.float32)
    key = np.full((h, w), 7, np.uint32) if one_key else rng.integers(0, 3, (h, w)).astype(np.uint32)
    t = (rng.random((h, w), dtype=np.float32) * F(49.5) + F(0.5)).astype(np.float32)
    return mean, key, t


@pytest.mark.parametrize("miss", [False, True], ids=["hit", "miss"])
@pytest.mark.parametrize("h,w", [(5, 5), (17, 33), (41, 75)])
def test_all_stops_off_is_the_f64_convolution(h, w, miss):
    mean, key, t = planes(h, w, seed=h * w)
    if miss:
        key[:] = dr.HIT_MISS
    got = dr.passes(mean, key, t, iterations=1)[0]
    assert got.dtype == np.float32 and got.shape == (h, w, 3)
    k2 = np.outer(dr.K.astype(np.float64), dr.K.astype(np.float64))
    assert k2.sum() == 1.0
    m = mean[..., :3].astype(np.float64)
    want = np.zeros((h - 4, w - 4, 3))
    for dy in range(5):
        for dx in range(5):
            want += k2[dy, dx] * m[dy:dy + h - 4, dx:dx + w - 4]
    err = np.abs(got[2:-2, 2:-2].astype(np.float64) - want) / want
    print(f"{h}x{w}: largest relative error {err.max():.3e} (bound {REL:.3e})")
    assert err.max() <= REL
    # and the w channel is Mean's, bit for bit
    out, rgba = dr.denoise(mean, key, t, iterations=1)
    assert rgba is None and np.array_equal(out[..., 3].view(np.uint32), mean[..., 3].view(np.uint32))
    assert np.array_equal(out[..., :3].view(np.uint32), got.view(np.uint32))


def test_border_taps_are_skipped_and_the_weights_renormalised():
    """A constant image stays constant to the last bit but one rounding chain: every pixel's result is
    (sum of w c) / (sum of w) over the taps inside, within the same bound; a 1 x 1 image is its own result."""
    mean, key, t = planes(9, 7, seed=3)
    mean[..., :3] = F(1.5)
    got = dr.passes(mean, key, t, iterations=3)
    for g in got:
        assert np.abs(g.astype(np.float64) - 1.5).max() <= 1.5 * REL
    one, k1, t1 = planes(1, 1, seed=4)
    out = dr.passes(one, k1, t1, iterations=4)[-1]
    # the centre alone: (9/64 c) / (9/64), two roundings
    assert np.abs(out.astype(np.float64) - one[..., :3]).max() <= one[..., :3].max() * 2 * 2.0 ** -24


def test_another_key_never_enters():
    mean, key, t = planes(12, 12, seed=5, one_key=False)
    mean[key == 1, :3] = np.nan
    mean[key == 2, :3] = np.inf
    out = dr.passes(mean, key, t, iterations=2)[-1]
    assert np.isfinite(out[key == 0]).all()
    assert np.isnan(out[key == 1]).all() and np.isinf(out[key == 2]).all()


@pytest.mark.parametrize("sigma", [0.5, 4.0, 3.0, 0.3, 1e-3, 7.0])
def test_host_ic_values_are_exact_power_of_two_multiples(sigma):
    ics = dr.host_ic(sigma, 8)
    ic0 = F(1.0) / F(sigma)
    assert all(type(v) is np.float32 for v in ics) and ics[0] == ic0
    for i, v in enumerate(ics):
        assert float(v) == float(ic0) * 2 ** i  # exact in f64, and representable: the product did not round
