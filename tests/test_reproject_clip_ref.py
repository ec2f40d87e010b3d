"""The numpy restatement of rt_reproject_clip (tests/reproject_clip_ref.py) against what it must reduce to, and the
quality the clamp was added for (no GPU needed).

The unit cases use the same camera twice, so that pixel (x, y) gathers exactly history pixel (x, y) (sx = x, sy = y to
the bit is not needed: a constant history makes H the constant whatever the weights are, see test_reproject_ref.py).
Means are small integers or quarters, so the window's sums and the band are exact and written down by hand.

The quality claim runs the 24-move sequence of tests/reproject_clip_seq.py on the oracle's means at Radius 2, Gamma 1,
the setting the claim was made for (its 0.52 on scene 0 is that column of the prototype).  Measured with this
definition, mean of moves 13..24 before any filter, over the raw 1-spp MSE, plain rt_reproject -> clipped: scene 0
0.668 -> 0.357 (0.53 of it), scene 1 prefix 64 0.641 -> 0.617, scene 2 0.269 -> 0.263
(profiles/reproject_clip_defaults.txt).  The library's defaults (Radius 1, Gamma 0.5) were chosen after rt_denoise;
before any filter they give 0.367, 0.613 and 0.273: on scene 2 that is 1.5 % above plain rt_reproject, which the
test prints and DESIGN.md says."""
import numpy as np
import pytest

import reproject_clip_ref as rc
import reproject_clip_seq as cseq
import reproject_ref as rr
import reproject_seq as seq
from test_reproject_ref import Orbit, flat

F = np.float32
W, H = 33, 17


@pytest.fixture(scope="module")
def cams(orc):
    o = Orbit()
    return dict(here=orc.camera(o, W, H), step=orc.camera(o, W, H, x_angle=o.x_angle + 1.0 / 16.0))


def both(p, cam, prev, radius, gamma, **kw):
    kw.setdefault("max_history", 8)
    planes = (p["mean"], p["key"], p["t"], cam, prev, p["hist"], p["hist_key"], p["hist_t"], p["hist_count"])
    return rr.reproject(*planes, **kw), rc.reproject_clip(*planes, radius=radius, gamma=gamma, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def textured(w, h, seed):
    """A mean of quarters in [0, 4): every sum of up to 49 values and squares is exact in f32."""
    p = flat(w, h)
    rng = np.random.default_rng(seed)
    p["mean"][..., :3] = rng.integers(0, 16, (h, w, 3)).astype(np.float32) * F(0.25)
    return p


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_history_inside_the_band_is_untouched(cams, radius):
    """A constant history of 2 (a power of two: H = acc / ws is 2 to the bit, test_reproject_ref.py) under a mean of
    quarters in [0, 4) and a wide band: wherever 2 lies in the band, Out is rt_reproject's, bit for bit."""
    p = textured(W, H, 5)
    wide = 8.0
    lo, hi, nf = rc.band(p["mean"], p["key"], radius, wide)
    assert (nf >= (radius + 1) ** 2).all() and (hi > lo).mean() > 0.9
    (out_p, cnt_p, _), (out_c, cnt_c, _) = both(p, cams["here"], cams["step"], radius, wide)
    inside = ((lo <= F(2.0)) & (F(2.0) <= hi)).all(axis=2)
    assert inside.mean() > 0.9 and (cnt_p == 2).mean() > 0.5
    assert np.array_equal(bits(out_c)[inside], bits(out_p)[inside]) and np.array_equal(cnt_c, cnt_p)
    # and a tight band does bind on the same planes: the check above is not vacuous
    _, (out_t, _, _) = both(p, cams["here"], cams["step"], radius, 0.01)
    assert (bits(out_t)[cnt_p == 2] != bits(out_p)[cnt_p == 2]).any()


def test_a_history_outside_the_band_lands_exactly_on_lo_or_hi(cams):
    """A 2 x 2 checker of 1 and 3 in x: a 3 x 3 window inside the image holds six of one and three of the other."""
    p = flat(W, H)
    xs = np.arange(W)
    p["mean"][..., :3] = np.where(xs % 2 == 0, F(1.0), F(3.0))[None, :, None]
    lo, hi, nf = rc.band(p["mean"], p["key"], 1, 1.0)
    assert nf[5, 5] == 9 and nf[0, 0] == 4 and nf[0, 5] == 6 and nf[H - 1, W - 1] == 4
    # centre on an odd column: s1 = 6 * 1 + 3 * 3 = 15, s2 = 6 + 27 = 33 -> m = 15/9, v = 33/9 - m*m
    m = F(15.0) / F(9.0)
    sd = np.sqrt(F(33.0) / F(9.0) - m * m)
    assert lo[5, 5, 0] == m - F(1.0) * sd and hi[5, 5, 1] == m + F(1.0) * sd
    a = F(1.0) / (F(1.0) + F(1.0))
    for hist, bound in ((F(100.0), hi), (F(-100.0), lo)):
        p["hist"][..., :3] = hist
        _, (out, cnt, _) = both(p, cams["here"], cams["here"], 1, 1.0)
        kept = cnt == 2
        assert kept[2:-2, 2:-2].all()
        want = bound + (p["mean"][..., :3] - bound) * a
        assert np.array_equal(bits(out[..., :3])[kept], bits(want)[kept])
        assert np.array_equal(bits(out[..., 3]), bits(p["mean"][..., 3]))


def test_the_window_is_cut_by_the_image_edge_and_by_a_key_boundary():
    w, h = 9, 7
    mean = np.ones((h, w, 4), np.float32)
    key = np.full((h, w), 7, np.uint32)
    for r in (1, 2, 3):
        _, _, nf = rc.band(mean, key, r, 1.0)
        ys, xs = np.mgrid[0:h, 0:w]
        nx = np.minimum(xs, r) + np.minimum(w - 1 - xs, r) + 1
        ny = np.minimum(ys, r) + np.minimum(h - 1 - ys, r) + 1
        assert np.array_equal(nf, (nx * ny).astype(np.float32))
    # a key boundary at x = 4: the whole word is compared, bit 31 included, and a miss is a key like any other
    for other in (np.uint32(8), np.uint32(7) | rr.HIT_INSIDE, rr.HIT_MISS):
        k2 = key.copy()
        k2[:, 4:] = other
        _, _, nf = rc.band(mean, k2, 2, 1.0)
        # rows x columns of the pixel's own side: (3, 3) sees columns 1..3, (3, 2) 0..3, (3, 4) 4..6, (3, 6) 4..8
        assert nf[3, 3] == 5 * 3 and nf[3, 2] == 5 * 4 and nf[3, 4] == 5 * 3 and nf[3, 6] == 5 * 5 and nf[0, 3] == 3 * 3
    # 1 x 1: the centre alone
    _, _, nf = rc.band(mean[:1, :1], key[:1, :1], 3, 1.0)
    assert nf.shape == (1, 1) and nf[0, 0] == 1


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_neighbour_is_skipped(cams, bad):
    p = textured(W, H, 9)
    q = {k: v.copy() for k, v in p.items()}
    q["mean"][6, 10, 1] = bad
    lo_p, hi_p, nf_p = rc.band(p["mean"], p["key"], 2, 1.0)
    lo_q, hi_q, nf_q = rc.band(q["mean"], q["key"], 2, 1.0)
    near = np.zeros((H, W), bool)
    near[4:9, 8:13] = True
    assert np.array_equal(nf_q[near], nf_p[near] - 1) and np.array_equal(nf_q[~near], nf_p[~near])
    assert np.isfinite(lo_q).all() and np.isfinite(hi_q).all()
    # the same band as with the pixel behind another key (which removes it from its neighbours' windows alike)
    k = {kk: v.copy() for kk, v in p.items()}
    k["key"][6, 10] = 99
    lo_k, hi_k, _ = rc.band(k["mean"], k["key"], 2, 1.0)
    others = near.copy()
    others[6, 10] = False
    assert np.array_equal(bits(lo_q)[others], bits(lo_k)[others]) and np.array_equal(bits(hi_q)[others], bits(hi_k)[others])
    # the pixel itself: its centre is dropped too; its Out carries Mean's non-finite channel through the fold, as rt_reproject's does
    (out_p, _, _), (out_c, _, _) = both(q, cams["here"], cams["here"], 2, 1.0)
    others = np.ones((H, W), bool)
    others[6, 10] = False
    assert np.isfinite(out_c[others]).all()
    assert not np.isfinite(out_c[6, 10, 1]) and not np.isfinite(out_p[6, 10, 1])


def test_an_isolated_pixel_keeps_its_fresh_value(cams):
    p = textured(W, H, 11)
    p["hist"][..., :3] = F(100.0)
    for y, x in ((8, 16), (0, 0), (H - 1, 5)):
        p["key"][y, x] = 1000 + x
        p["hist_key"][y, x] = 1000 + x
    lo, hi, nf = rc.band(p["mean"], p["key"], 3, 2.0)
    (out_p, cnt_p, _), (out_c, cnt_c, _) = both(p, cams["here"], cams["here"], 3, 2.0)
    for y, x in ((8, 16), (0, 0), (H - 1, 5)):
        assert nf[y, x] == 1 and np.array_equal(lo[y, x], p["mean"][y, x, :3]) and np.array_equal(hi[y, x], p["mean"][y, x, :3])
        assert cnt_c[y, x] == 2 and cnt_p[y, x] == 2                       # it did take its history ...
        assert np.array_equal(bits(out_c[y, x]), bits(p["mean"][y, x]))   # ... clamped onto the fresh value
        assert not np.array_equal(out_p[y, x, :3], p["mean"][y, x, :3])


def test_a_nan_bound_clamps_nothing_and_overflowed_squares_open_the_band():
    hc = np.array([-5.0, 0.0, 5.0, np.inf], np.float32)
    nan, one = np.full(4, np.nan, np.float32), np.ones(4, np.float32)
    assert np.array_equal(bits(rc.clamp(hc, nan, nan, one)), bits(hc))
    assert np.array_equal(rc.clamp(hc, nan, F(1.0) * one, one), np.array([-5, 0, 1, 1], np.float32))
    assert np.array_equal(rc.clamp(hc, F(-1.0) * one, nan, one), np.array([-1, 0, 5, np.inf], np.float32))
    assert np.array_equal(bits(rc.clamp(hc, one, -one, 0 * one)), bits(hc))  # nf == 0: no clamp
    # squares that overflow under a mean whose square does not: s2 = inf, sd = inf, the band is (-inf, +inf)
    c = F(1e30)
    mean = np.zeros((3, 3, 4), np.float32)
    mean[..., :3] = np.array([[c, -c, c], [-c, 0, -c], [c, -c, c]], np.float32)[..., None]
    lo, hi, nf = rc.band(mean, np.zeros((3, 3), np.uint32), 1, 1.0)
    assert nf[1, 1] == 9 and np.isneginf(lo[1, 1]).all() and np.isposinf(hi[1, 1]).all()
    assert np.array_equal(bits(rc.clamp(hc, lo[1, 1, 0] * one, hi[1, 1, 0] * one, one)), bits(hc))
    # ... and where m * m overflows too, v = pos(inf - inf) = 0: the band is the point m (what the header says)
    mean[..., :3] = c
    lo, hi, nf = rc.band(mean, np.zeros((3, 3), np.uint32), 1, 1.0)
    assert np.array_equal(bits(lo), bits(hi)) and np.isfinite(lo).all() and (np.abs(lo / c - 1) < 1e-6).all()


def test_out_count_is_rt_reprojects_on_every_input(cams):
    """Random keys, counts, misses, non-finite values, both camera pairs, with and without history."""
    rng = np.random.default_rng(3)
    for trial in range(4):
        p = textured(W, H, 20 + trial)
        p["key"] = rng.integers(0, 4, (H, W)).astype(np.uint32)
        p["key"][rng.random((H, W)) < 0.1] = rr.HIT_MISS
        p["hist_key"] = np.where(rng.random((H, W)) < 0.8, p["key"], np.uint32(2)).astype(np.uint32)
        p["hist_count"] = rng.choice(np.array([0, 1, 3, 8, 50], np.uint32), (H, W)).astype(np.uint32)
        p["hist"][..., :3] = rng.random((H, W, 3), dtype=np.float32) * F(8.0)
        for img in (p["mean"], p["hist"]):
            img[rng.integers(0, H, 6), rng.integers(0, W, 6), rng.integers(0, 3, 6)] = [np.nan, np.inf, -np.inf, 1e-41, -2.0, 3e38]
        for prev in ("here", "step"):
            (out_p, cnt_p, _), (out_c, cnt_c, _) = both(p, cams["here"], cams[prev], 1 + trial % 3, (0.5, 1.0, 2.0, 1e-3)[trial],
                                                        depth_tolerance=0.1 * (trial % 2), frames=1 + trial % 2)
            assert np.array_equal(cnt_c, cnt_p) and (cnt_c > 1).any() and (cnt_c == 1 + trial % 2).any()
            assert np.array_equal(bits(out_c[..., 3]), bits(out_p[..., 3]))
            fresh = cnt_c == 1 + trial % 2
            assert np.array_equal(bits(out_c)[fresh], bits(p["mean"])[fresh])  # (a fold's count is above Frames)
    # no history: the mean itself
    out, cnt, rgba = rc.reproject_clip(p["mean"], p["key"], p["t"], cams["here"], cams["step"], max_history=8, radius=2, gamma=1.0)
    assert rgba is None and np.array_equal(bits(out), bits(p["mean"])) and (cnt == 1).all()


@pytest.fixture(scope="module")
def sequences(orc):
    return {name: seq.oracle_inputs(orc, index, prefix, moves=cseq.MOVES) for name, (index, prefix) in seq.SCENES.items()}


@pytest.mark.timeout(280)
@pytest.mark.parametrize("name,bound", [("0 RGB Glass", 0.75), ("1 prefix 64", 1.0), ("2 RTWeekend", 1.0)])
def test_quality_24_moves_the_clamp_beats_plain_reprojection(sequences, name, bound):
    """Mean of moves 13..24, before any filter, MaxHistory 8, DepthTolerance 0.1, Radius 2 and Gamma 1: the clipped
    MSE is below plain rt_reproject's on every scene, and at most 0.75 of it on scene 0.  The yardstick is
    tests/reproject_ref.py on the same inputs.  The library's defaults are printed beside it."""
    cams_, fresh, hits, refs = sequences[name]
    kw = dict(max_history=8, depth_tolerance=0.1)
    plain = cseq.tail(a for a, _, _ in cseq.run(cams_, fresh, hits, refs, cseq.plain(**kw)))
    clip = cseq.tail(a for a, _, _ in cseq.run(cams_, fresh, hits, refs, cseq.clipped(2, 1.0, **kw)))
    dflt = cseq.tail(a for a, _, _ in cseq.run(cams_, fresh, hits, refs, cseq.clipped(1, 0.5, **kw)))
    raw = cseq.tail(seq.mse(fresh[i + 1], refs[i]) for i in range(cseq.MOVES))
    print(f"scene {name}: moves 13..24 over the raw 1-spp MSE: rt_reproject {plain / raw:.3f}, clipped R 2 gamma 1 "
          f"{clip / raw:.3f} (clipped / plain {clip / plain:.3f}); the defaults R 1 gamma 0.5 {dflt / raw:.3f}, recorded")
    assert clip < plain, (name, clip, plain)
    assert clip <= bound * plain, (name, clip, plain, bound)
