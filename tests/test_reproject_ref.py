"""The numpy restatement of rt_reproject (tests/reproject_ref.py) against what it must reduce to (no GPU needed).

Cameras come from the oracle's camera set-up (the 24-float record); first hits from an f64 ray cast at the pixel
centre.  A constant history H with a constant mean M makes the fold checkable to the bit: every kept weight w gives
acc = H * ws exactly when H is a power of two, so acc / ws is H and Out is H + (M - H) * a in f32."""
import numpy as np
import pytest

import reproject_ref as rr
import reproject_seq as seq

F = np.float32
W, H = 33, 17
STEP = 1.0 / 16.0


class Orbit:
    """What oracle.camera reads of a scene: the look-at point and the default orbit."""

    def __init__(self, distance=8.0, x_angle=0.3, y_height=1.0):
        self.look_at = np.zeros(4, np.float32)
        self.distance, self.x_angle, self.y_height = distance, x_angle, y_height


def flat(w, h, key=7, t=5.0, mean=4.0, hist=2.0, count=1):
    """Constant planes: one key, one distance, a constant mean and a constant history."""
    m = np.full((h, w, 4), mean, np.float32)
    m[..., 3] = F(0.25)
    hs = np.full((h, w, 4), hist, np.float32)
    hs[..., 3] = F(0.75)
    return dict(mean=m, key=np.full((h, w), key, np.uint32), t=np.full((h, w), t, np.float32), hist=hs,
                hist_key=np.full((h, w), key, np.uint32), hist_t=np.full((h, w), t, np.float32),
                hist_count=np.full((h, w), count, np.uint32))


def call(p, cam, prev, **kw):
    kw.setdefault("max_history", 8)
    return rr.reproject(p["mean"], p["key"], p["t"], cam, prev, p["hist"], p["hist_key"], p["hist_t"], p["hist_count"], **kw)


@pytest.fixture(scope="module")
def cams(orc):
    o = Orbit()
    return dict(here=orc.camera(o, W, H), step=orc.camera(o, W, H, x_angle=o.x_angle + STEP),
                close=orc.camera(o, W, H, distance=o.distance / 4))


def test_no_history_is_the_mean(cams):
    rng = np.random.default_rng(1)
    p = flat(W, H)
    p["mean"][..., :3] = rng.random((H, W, 3), dtype=np.float32)
    p["mean"][3, 4, 1], p["mean"][5, 6, 0], p["mean"][7, 8, 2] = np.nan, np.inf, F(1e-41)
    for frames in (1, 3):
        out, cnt, rgba = rr.reproject(p["mean"], p["key"], p["t"], cams["here"], cams["step"], frames=frames, max_history=8)
        assert rgba is None and out.dtype == np.float32 and cnt.dtype == np.uint32
        assert np.array_equal(out.view(np.uint32), p["mean"].view(np.uint32)) and (cnt == frames).all()


def test_a_miss_and_a_point_behind_the_previous_camera_are_fresh(cams):
    p = flat(W, H)
    p["key"][:, :10] = rr.HIT_MISS
    p["t"][:, :10] = F(1e30)
    p["hist_key"][:, :10] = rr.HIT_MISS  # the history has misses in the same place: a miss still takes none
    out, cnt, _ = call(p, cams["here"], cams["here"])
    assert (cnt[:, :10] == 1).all() and np.array_equal(out[:, :10].view(np.uint32), p["mean"][:, :10].view(np.uint32))
    assert (cnt[2:-2, 12:-2] == 2).all()  # (the hits of the same frame do fold)
    # the previous camera four times closer: a point 5 away from the new camera (8 from the look-at point) lies
    # behind the previous one (2 from it)
    q = flat(W, H)
    pr = rr.project(cams["here"], cams["close"], q["key"], q["t"])
    assert (pr["d"] <= 0).all() and not pr["ok"].any()
    out, cnt, _ = call(q, cams["here"], cams["close"])
    assert (cnt == 1).all() and np.array_equal(out.view(np.uint32), q["mean"].view(np.uint32))


def test_a_key_that_differs_in_bit_31_rejects_the_tap(cams):
    p = flat(W, H)
    _, cnt, _ = call(p, cams["here"], cams["step"])
    assert (cnt == 2).mean() > 0.5
    p["hist_key"] ^= rr.HIT_INSIDE
    out, cnt, _ = call(p, cams["here"], cams["step"])
    assert (cnt == 1).all() and np.array_equal(out.view(np.uint32), p["mean"].view(np.uint32))


def test_the_depth_test_rejects_the_far_side_of_a_sphere(orc):
    """One sphere of radius 1 at the look-at point, the camera 5 away, the previous camera half an orbit on: what
    the new camera sees is the far side for the previous one, behind the pixels where that camera saw the near side
    of the same sphere.  Without the depth test every such pixel takes that history; with it, none whose point is
    more than the tolerance further than what the previous camera saw."""
    w, h = 48, 36
    o = Orbit(distance=5.0, x_angle=0.0, y_height=0.0)
    sphere = np.zeros((1, 20), np.float32)
    sphere[0, 4] = 1.0
    cam, prev = orc.camera(o, w, h), orc.camera(o, w, h, x_angle=float(F(np.pi)))
    key, t = seq.hit_planes_f64(cam, sphere, w, h)
    pkey, pt = seq.hit_planes_f64(prev, sphere, w, h)
    front = (key == 0) & (t < F(4.3))  # well inside the silhouette
    assert front.sum() > 50 and (pkey == 0).sum() > 50
    mean = np.full((h, w, 4), 4.0, np.float32)
    hist = np.full((h, w, 4), 2.0, np.float32)
    one = np.ones((h, w), np.uint32)
    _, cnt_off, _ = rr.reproject(mean, key, t, cam, prev, hist, pkey, pt, one, max_history=8, depth_tolerance=0.0)
    _, cnt_on, _ = rr.reproject(mean, key, t, cam, prev, hist, pkey, pt, one, max_history=8, depth_tolerance=0.1)
    assert (cnt_off[front] == 2).all()
    assert (cnt_on[front] == 1).all()
    # and the same camera twice keeps its history under the same tolerance
    _, cnt_same, _ = rr.reproject(mean, key, t, cam, cam, hist, key, t, one, max_history=8, depth_tolerance=0.1)
    assert (cnt_same[front] == 2).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_history_tap_is_skipped_and_the_others_fold(cams, bad):
    """A non-finite channel removes the tap exactly as a count of 0 does, and pixels that lose a tap still fold."""
    p = flat(W, H)
    base_out, base_cnt, _ = call(p, cams["here"], cams["step"])
    holes = [(5, 9, 0), (8, 20, 1), (11, 14, 2)]
    a, b = flat(W, H), flat(W, H)
    for y, x, ch in holes:
        a["hist"][y, x, ch] = bad
        b["hist_count"][y, x] = 0
    out_a, cnt_a, _ = call(a, cams["here"], cams["step"])
    out_b, cnt_b, _ = call(b, cams["here"], cams["step"])
    assert np.isfinite(out_a).all()
    assert np.array_equal(out_a.view(np.uint32), out_b.view(np.uint32)) and np.array_equal(cnt_a, cnt_b)
    # the constant history hides a lost tap in Out; the count plane of a varied history shows it
    c = flat(W, H)
    c["hist_count"][:] = 5
    for y, x, _ in holes:
        c["hist_count"][y, x] = 1
    _, cnt_low, _ = call(c, cams["here"], cams["step"])
    for y, x, ch in holes:
        c["hist"][y, x, ch] = bad
    _, cnt_skipped, _ = call(c, cams["here"], cams["step"])
    used = cnt_low == 2  # pixels that took one of the three taps
    assert used.sum() >= 3 and (cnt_skipped[used] != 2).all()
    assert (cnt_skipped[used] == 6).sum() >= 3  # their other taps still folded
    assert (base_cnt == 2).mean() > 0.5 and np.isfinite(base_out).all()


@pytest.mark.parametrize("frames,cap,count,n_after,total", [(1, 8, 1, 1, 2), (1, 8, 7, 7, 8), (1, 8, 8, 8, 8), (1, 8, 100, 8, 8),
                                                            (3, 8, 4, 4, 7), (3, 8, 7, 7, 8), (3, 3, 9, 3, 3),
                                                            (2, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)])
def test_the_count_rules_at_the_cap(cams, frames, cap, count, n_after, total):
    p = flat(W, H, count=count)
    out, cnt, _ = call(p, cams["here"], cams["step"], frames=frames, max_history=cap)
    folded = cnt != frames if total != frames else np.zeros((H, W), bool)
    if total != frames:
        assert folded.mean() > 0.5 and (cnt[folded] == total).all()
    else:
        assert (cnt == total).all()
        folded = out[..., 0] != F(4.0)
    a = F(frames) / (F(n_after) + F(frames))
    want = F(2.0) + (F(4.0) - F(2.0)) * a
    assert (out[folded][:, :3] == want).all() and (out[~folded][:, :3] == F(4.0)).all()
    assert (out[..., 3] == F(0.25)).all()  # Out.w is Mean's
    # a history count of 0 is no history
    z = flat(W, H, count=0)
    out, cnt, _ = call(z, cams["here"], cams["step"], frames=frames, max_history=cap)
    assert (cnt == frames).all() and np.array_equal(out.view(np.uint32), z["mean"].view(np.uint32))


@pytest.fixture(scope="module")
def scene0(orc):
    return seq.oracle_inputs(orc, 0, None)


def test_projection_agrees_with_f64_on_scene_0(orc, scene0):
    """(sx, sy) of every hit pixel against the same projection in f64 (the f64 ray, the f64 distance): within 1e-2
    pixel."""
    from test_gpu_first_hit import first_hit_f64
    cams_, _, hits, _ = scene0
    sc = orc.scene_builtin(0)
    cam, prev = cams_[1].astype(np.float64), cams_[0].astype(np.float64)
    f = first_hit_f64(cams_[1], sc.spheres, seq.W, seq.H)
    hit = f["win"] >= 0
    x = cam[0:3] + f["d"] * np.where(hit, f["t"], 0.0)[:, None]
    v = x - prev[0:3]
    fv = prev[16:19] - prev[0:3]
    d = v @ fv
    sx = ((v @ prev[8:11]) / d * (fv @ fv) * 2 / prev[20] + 1) * (seq.W / 2)
    sy = ((v @ prev[12:15]) / d * (fv @ fv) * 2 / prev[21] + 1) * (seq.H / 2)
    pr = rr.project(cams_[1], cams_[0], hits[1][0], hits[1][1])
    assert hit.sum() > 1000 and (d[hit] > 0).all()
    ex = np.abs(pr["sx"].reshape(-1).astype(np.float64) - sx)[hit].max()
    ey = np.abs(pr["sy"].reshape(-1).astype(np.float64) - sy)[hit].max()
    print(f"projection: largest |sx - f64| {ex:.3e}, |sy - f64| {ey:.3e} pixel over {hit.sum()} hit pixels")
    assert ex <= 1e-2 and ey <= 1e-2
    # one key step moves the image: the projection is not the identity
    ys, xs = np.mgrid[0:seq.H, 0:seq.W]
    assert np.abs(pr["sx"] - xs)[hit.reshape(seq.H, seq.W)].mean() > 0.5


def test_six_moves_on_scene_0_beat_the_raw_frame(scene0):
    """The sequence of tests/reproject_seq.py from the oracle's means under the library's defaults (MaxHistory 8,
    DepthTolerance 0.1): the reprojected MSE is strictly below the raw 1-spp MSE at every move from the second on
    (scripts/reproject_defaults.py gives 0.62 and lower; the first move has one frame of history)."""
    cams_, fresh, hits, refs = scene0
    res = seq.run(cams_, fresh, hits, refs, max_history=8, depth_tolerance=0.1)
    print("scene 0 ratios:", " ".join(f"{a / b:.3f}" for a, b in res))
    assert len(res) == seq.MOVES
    for move, (rep, raw) in enumerate(res, 1):
        if move >= 2:
            assert rep < raw, (move, rep, raw)
