"""GPU checks of rt_reproject: the running mean carried across a camera move.

The checker is tests/reproject_ref.py, the numpy restatement of the definition in include/rt_trace.h.  Out, OutCount
and Rgba8 must equal it bit for bit wherever it is not NaN and be NaN where it is (NaN payloads are not part of the
contract): no tolerance, no pixel excluded.  Rgba8 is compared with the oracle's RGBA8 encoding of the
restatement's Out on every pixel (both encode a NaN channel as 0).

  synthetic planes  numpy with a fixed seed: Key a handful of discs over a miss background, some with
                    RT_HIT_INSIDE, the history's keys the same discs with a few words changed (another sphere, bit 31
                    alone, a miss); T around the orbit's distance, smooth for half of the pixels and random up to three
                    times it for the rest, the history's T the smooth field with noise, so that the depth test keeps some taps and
                    rejects others; counts from 0 to beyond the cap; a mean and a history in [0, 4] with denormals,
                    negatives, inf and NaN.  1x1, 3x2, 33x17, 75x41 and 136x104.  Camera pairs from rt_camera_setup
                    around scene 1's look-at point: the same camera, one key step in angle, in distance and in height
                    (rt_on_render's steps), half an orbit and a camera four times closer (d <= 0 for the points behind them).
                    Per pair: no depth test, the default tolerance, Frames 3 with the pow flag and a tight
                    tolerance, and no history.
  real planes       scene 0 at 72x40 and scene 1 prefix 64 at 136x104: rt_trace at one frame and rt_trace_first_hit
                    at the pixel centre for two cameras one key step apart; the first frame without history, the
                    second carried from it; the downloaded planes restated.
  what is written   every plane lies in one arena that starts from test_gpu_tiles.POISON, with poisoned gaps: after a
                    call the inputs and the gaps are unchanged and a plane that was not passed (Rgba8) is still
                    poison.  A following rt_trace of the unchanged key has CullPassRan == 0.
  quality           the six-move sequence of tests/reproject_seq.py on scenes 0 and 2 with the GPU's means, first
                    hits and reprojection under the library's defaults: the reprojected MSE is strictly below the
                    raw 1-spp MSE, against the GPU's mean of frames 1..256 at that camera, at every move from the
                    second on.  Scene 1 prefix 64 (half the spheres are perfect mirrors, whose image a surface
                    reprojection cannot follow) is printed, not asserted.  Chosen on the CPU first
                    (scripts/reproject_defaults.py): 0.62 and lower on scene 0, 0.36 and lower on scene 2.
                    Measured on an MI355X: profiles/reproject_quality.txt."""
import numpy as np
import pytest

import reproject_ref as rr
import reproject_seq as seq
from test_gpu_tiles import POISON, POISON_I32

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (33, 17), (75, 41), (136, 104)]
PAIRS = ("same", "angle", "distance", "height", "half_orbit", "closer")
KEY_STEP = 1.0 / 16.0           # rt_on_render: x_angle += 1/16, distance and y_height += 1.0 * WorldScale = 1/16
CAP = 8
CONFIGS = {  # name: (DepthTolerance, Frames, MaxHistory, Flags, history, Rgba8)
    "no_depth": (0.0, 1, CAP, 0, True, True),
    "default_tolerance": (0.1, 1, CAP, 0, True, False),
    "tight_frames3_pow": (0.02, 3, CAP, rr.SRGB_POW, True, True),
    "no_history": (0.1, 1, CAP, 0, False, True),
}
GAP = 64  # poisoned words between two planes of the arena


def camera_pair(rt, w, h, pair):
    """(new camera, previous camera) around scene 1's look-at point."""
    s = rt.scene_builtin(1)
    d, a, y = s.DefaultDistanceFromLookAt, s.DefaultXAngle, s.DefaultYHeight
    prev = {"same": (d, a, y), "angle": (d, a - KEY_STEP, y), "distance": (d + KEY_STEP, a, y), "height": (d, a, y - KEY_STEP),
            "half_orbit": (d, a + float(np.float32(np.pi)), y), "closer": (d / 4, a, y)}[pair]
    return rt.camera_setup(s, w, h), rt.camera_setup(s, w, h, *prev), d


def synthetic(w, h, seed, distance):
    rng = np.random.default_rng(seed)
    n = w * h
    ys, xs = np.mgrid[0:h, 0:w]
    key = np.full((h, w), rr.HIT_MISS, np.uint32)
    for i in range(7):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.15, 0.45) * max(min(w, h), 2)
        k = np.uint32(rng.integers(0, 300)) | (rr.HIT_INSIDE if i % 3 == 2 else np.uint32(0))
        key[(xs - cx) ** 2 + (ys - cy) ** 2 < r * r] = k
    if n < 8:
        key[:] = 5  # (the smallest images are one surface: a miss alone would test nothing)
    miss = key == rr.HIT_MISS
    # T: around the orbit's distance, so that the points lie near the look-at point and project into the previous image
    smooth = (distance * (0.8 + 0.4 * (xs + 0.6 * ys) / max(w + h, 2))).astype(np.float32)
    rough = (distance * rng.uniform(0.5, 3.0, (h, w))).astype(np.float32)  # (beyond 2: behind a camera half an orbit on)
    field = np.where(rng.random((h, w)) < 0.5, smooth, rough).astype(np.float32)
    t = np.where(miss, np.float32(1e30), field).astype(np.float32)
    # the history: the same discs with a few words changed, and T the same field with 0.1 %, 5 % or 30 % of noise
    hist_key = key.copy()
    pick = rng.random((h, w))
    hist_key[pick < 0.04] = 3
    flip = (pick >= 0.04) & (pick < 0.08) & ~miss
    hist_key[flip] ^= rr.HIT_INSIDE
    hist_key[(pick >= 0.08) & (pick < 0.10)] = rr.HIT_MISS
    noise = rng.choice(np.array([0.001, 0.05, 0.3]), (h, w)) * rng.uniform(-1, 1, (h, w))
    hist_t = np.where(hist_key == rr.HIT_MISS, np.float32(1e30), smooth * (1 + noise)).astype(np.float32)
    hist_count = rng.choice(np.array([0, 1, 2, 5, CAP - 1, CAP, CAP + 3, 1000, 0xFFFFFFFF], np.uint32), (h, w)).astype(np.uint32)
    specials = [np.float32(1e-41), np.float32(-1e-42), np.float32(-0.75), np.float32(-3.0), np.float32(np.inf),
                np.float32(-np.inf), np.float32(np.nan), np.float32(0.0), np.float32(-0.0)]
    images = []
    for _ in range(2):
        img = np.zeros((h, w, 4), np.float32)
        img[..., :3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(4.0)
        img[..., 3] = rng.random((h, w), dtype=np.float32)
        flat = img.reshape(n, 4)
        if n >= 64:
            for i, p in enumerate(rng.choice(n, size=min(n // 16, 4 * len(specials)), replace=False)):
                flat[p, i % 3] = specials[i % len(specials)]
        elif n > 1:
            flat[n - 1, 1] = np.float32(1e-41)
        images.append(img)
    return dict(mean=images[0], hit=pack_hit(key, t), history=images[1], history_hit=pack_hit(hist_key, hist_t),
                history_count=hist_count)


def pack_hit(key, t):
    hit = np.zeros(key.shape + (2,), np.uint32)
    hit[..., 0] = key
    hit[..., 1] = t.view(np.uint32)
    return hit


class Arena:
    """Every plane of a call in one poisoned device buffer with poisoned gaps."""
    ORDER = (("mean", 4), ("hit", 2), ("history", 4), ("history_hit", 2), ("history_count", 1), ("out", 4), ("out_count", 1),
             ("rgba8", 1))
    INPUTS = ("mean", "hit", "history", "history_hit", "history_count")

    def __init__(self, torch, w, h, planes):
        self.torch, self.w, self.h = torch, w, h
        n, at, self.off = w * h, GAP, {}
        for name, words in self.ORDER:
            self.off[name] = (at, n * words)
            at += (n * words + GAP + 3) // 4 * 4  # (every plane 16-byte aligned)
        host = np.full(at, POISON, np.uint32)
        for name in self.INPUTS:
            o, m = self.off[name]
            host[o:o + m] = np.ascontiguousarray(planes[name]).view(np.uint32).reshape(-1)
        self.before = host
        self.buf = torch.from_numpy(host.view(np.int32).copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self, name):
        return self.buf.data_ptr() + 4 * self.off[name][0]

    def after(self):
        self.torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(np.uint32)

    def plane(self, words, name):
        o, m = self.off[name]
        return words[o:o + m]


def assert_same_bits(got_u32, want_f32, what):
    """Bit for bit where the restatement is not NaN, NaN where it is."""
    want = np.ascontiguousarray(want_f32, np.float32).reshape(-1)
    got = got_u32.reshape(-1)
    nan = np.isnan(want)
    assert np.isnan(got.view(np.float32)[nan]).all(), f"{what}: a NaN of the restatement is a number on the GPU"
    bad = np.flatnonzero(got[~nan] != want.view(np.uint32)[~nan])
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} words differ from the restatement, first at word "
                           f"{np.flatnonzero(~nan)[bad[0]]}: GPU {got[~nan][bad[0]]:#010x}, restatement "
                           f"{want.view(np.uint32)[~nan][bad[0]]:#010x}")


def run_and_check(rt, orc, torch, w, h, planes, cam, prev, *, tol, frames, cap, flags, history=True, pass_rgba8=True, label=""):
    """One call in a poisoned arena against the restatement; returns the restatement's (Out, OutCount)."""
    ar = Arena(torch, w, h, planes)
    hist = dict(history_ptr=ar.ptr("history"), history_hit_ptr=ar.ptr("history_hit"),
                history_count_ptr=ar.ptr("history_count")) if history else {}
    rt.reproject(w, h, cam, prev, ar.ptr("mean"), ar.ptr("hit"), ar.ptr("out"), ar.ptr("out_count"),
                 rgba8_ptr=ar.ptr("rgba8") if pass_rgba8 else 0, frames=frames, max_history=cap, depth_tolerance=tol,
                 srgb_pow=bool(flags & rr.SRGB_POW), stream=torch.cuda.current_stream().cuda_stream, **hist)
    words = ar.after()
    key, t = planes["hit"][..., 0], planes["hit"][..., 1].view(np.float32)
    given = (planes["history"], planes["history_hit"][..., 0], planes["history_hit"][..., 1].view(np.float32),
             planes["history_count"]) if history else (None, None, None, None)
    want, want_count, want_rgba = rr.reproject(planes["mean"], key, t, rt.camera_floats(cam), rt.camera_floats(prev), *given,
                                               frames=frames, max_history=cap, depth_tolerance=tol, flags=flags,
                                               encode=orc.encode_rgba8)
    assert_same_bits(ar.plane(words, "out"), want, f"{label} Out")
    assert np.array_equal(ar.plane(words, "out_count"), want_count.reshape(-1)), f"{label}: OutCount differs"
    if pass_rgba8:
        assert np.array_equal(ar.plane(words, "rgba8"), want_rgba.reshape(-1)), f"{label}: Rgba8 differs"
    # nothing else is written: the inputs, the gaps and a plane that was not passed
    written = np.zeros(words.size, bool)
    for name in ("out", "out_count") + (("rgba8",) if pass_rgba8 else ()):
        o, m = ar.off[name]
        written[o:o + m] = True
    assert np.array_equal(words[~written], ar.before[~written]), f"{label}: a word outside Out, OutCount and Rgba8 was written"
    o, m = ar.off["out"]
    assert not (words[o:o + m].reshape(-1, 4) == POISON).all(axis=1).any(), f"{label}: a pixel of Out was not written"
    assert not (ar.plane(words, "out_count") == POISON).any(), f"{label}: a pixel of OutCount was not written"
    return want, want_count


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic_planes_match_the_restatement(rt, orc, torch_cuda, w, h, pair):
    cam, prev, distance = camera_pair(rt, w, h, pair)
    planes = synthetic(w, h, seed=1000 * w + h, distance=distance)
    if w * h >= 64:  # the planes are what the check is designed on
        key, hkey = planes["hit"][..., 0], planes["history_hit"][..., 0]
        assert len(np.unique(key)) >= 4 and (key == rr.HIT_MISS).any() and (((key & rr.HIT_INSIDE) != 0) & (key != rr.HIT_MISS)).any()
        assert ((key ^ hkey) == rr.HIT_INSIDE).any() and (hkey != key).mean() < 0.2
        for img in (planes["mean"][..., :3], planes["history"][..., :3]):
            assert np.isnan(img).any() and np.isinf(img).any() and (img < 0).any() and ((img != 0) & (np.abs(img) < 1e-38)).any()
        assert (planes["history_count"] == 0).any() and (planes["history_count"] > CAP).any()
    for name, (tol, frames, cap, flags, history, rgba8) in CONFIGS.items():
        run_and_check(rt, orc, torch_cuda, w, h, planes, cam, prev, tol=tol, frames=frames, cap=cap, flags=flags,
                      history=history, pass_rgba8=rgba8, label=f"{w}x{h} {pair} {name}")


def test_every_rejection_path_runs_on_the_synthetic_planes(rt):
    """What the restatement does on the planes above, so that a kernel that ignored a rule would not pass: per
    camera pair some pixels fold and some hits are fresh, the depth test removes history, every count rule
    appears, and the half orbit and the closer camera leave the image or the front of the previous camera."""
    w, h = 75, 41
    folded = {}
    for pair in PAIRS:
        cam, prev, distance = camera_pair(rt, w, h, pair)
        p = synthetic(w, h, seed=1000 * w + h, distance=distance)
        key, t = p["hit"][..., 0], p["hit"][..., 1].view(np.float32)
        given = (p["history"], p["history_hit"][..., 0], p["history_hit"][..., 1].view(np.float32), p["history_count"])
        counts = {}
        for tol in (0.0, 0.1, 0.02):
            _, counts[tol], _ = rr.reproject(p["mean"], key, t, rt.camera_floats(cam), rt.camera_floats(prev), *given,
                                             frames=1, max_history=CAP, depth_tolerance=tol)
        folded[pair] = {tol: int((c != 1).sum()) for tol, c in counts.items()}
        pr = rr.project(rt.camera_floats(cam), rt.camera_floats(prev), key, t)
        hits = key != rr.HIT_MISS
        if pair in ("same", "angle", "distance", "height"):
            assert folded[pair][0.0] > folded[pair][0.1] > folded[pair][0.02] > 20, (pair, folded[pair])
            assert ((counts[0.02] == 1) & hits).sum() > 20  # hits without usable history
            assert {2, 3, 6, CAP}.issubset(set(np.unique(counts[0.0]))), np.unique(counts[0.0])
        if pair in ("half_orbit", "closer"):  # points behind the previous camera, and points outside its image
            assert (pr["d"][hits] <= 0).mean() > 0.05 and (~pr["ok"][hits] & (pr["d"][hits] > 0)).mean() > 0.05
    assert folded["same"] != folded["angle"] != folded["distance"] != folded["height"]


class Loop:
    """One device and one built-in scene: rt_trace at one frame, the mean of later frames and rt_trace_first_hit at
    the pixel centre, per camera, downloaded."""

    def __init__(self, rt, torch, scene_index, prefix, w, h, max_bounce=8):
        self.rt, self.torch, self.w, self.h = rt, torch, w, h
        s = rt.scene_builtin(scene_index)
        self.scene = rt.scene_prefix(s, prefix) if prefix else s
        self.dev = rt.Device(0)
        self.dev.upload_scene(self.scene)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.max_bounce = max_bounce

    def camera(self, x_angle=None):
        return self.rt.camera_setup(self.scene, self.w, self.h, x_angle=x_angle)

    def trace(self, cam, frames=1, prev_count=0, prev=None):
        """The running mean after `frames` more frames (H, W, 4) f32."""
        torch, w, h = self.torch, self.w, self.h
        buf = torch.zeros((w * h, 4), dtype=torch.float32, device="cuda") if prev is None else torch.from_numpy(
            np.ascontiguousarray(prev).reshape(w * h, 4)).cuda()
        cur = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.dev.trace(cam, width=w, height=h, prev_ptr=buf.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
                       prev_count=prev_count, frames=frames, max_bounce=self.max_bounce, stream=self.stream)
        torch.cuda.synchronize()
        return buf.cpu().numpy().reshape(h, w, 4)

    def first_hit(self, cam):
        """The Hit plane at the pixel centre (H, W, 2) u32."""
        torch, w, h = self.torch, self.w, self.h
        hit = torch.full((w * h, 2), POISON_I32, dtype=torch.int32, device="cuda")
        self.dev.trace_first_hit(cam, width=w, height=h, centre=True, hit_ptr=hit.data_ptr(), stream=self.stream)
        torch.cuda.synchronize()
        return hit.cpu().numpy().view(np.uint32).reshape(h, w, 2)


@pytest.mark.parametrize("name,scene,prefix,w,h", [("s1p64_136x104", 1, 64, 136, 104), ("s0_72x40", 0, None, 72, 40)])
def test_real_planes_match_the_restatement(rt, orc, torch_cuda, name, scene, prefix, w, h):
    lp = Loop(rt, torch_cuda, scene, prefix, w, h)
    try:
        d = rt.reproject_defaults()
        cam0 = lp.camera()
        cam1 = lp.camera(x_angle=lp.scene.DefaultXAngle + KEY_STEP)
        mean0, hit0, mean1, hit1 = lp.trace(cam0), lp.first_hit(cam0), lp.trace(cam1), lp.first_hit(cam1)
        assert (hit1[..., 0] == rr.HIT_MISS).any() and len(np.unique(hit1[..., 0])) >= 4
        none = dict(history=mean0, history_hit=hit0, history_count=np.zeros((h, w), np.uint32))  # (uploaded, not passed)
        out0, count0 = run_and_check(rt, orc, torch_cuda, w, h, dict(mean=mean0, hit=hit0, **none), cam0, cam0,
                                     tol=d["depth_tolerance"], frames=1, cap=d["max_history"], flags=0, history=False,
                                     label=f"{name} first frame")
        assert np.array_equal(out0.view(np.uint32), mean0.view(np.uint32)) and (count0 == 1).all()
        planes = dict(mean=mean1, hit=hit1, history=out0, history_hit=hit0, history_count=count0)
        for tol in (d["depth_tolerance"], 0.0):
            out1, count1 = run_and_check(rt, orc, torch_cuda, w, h, planes, cam1, cam0, tol=tol, frames=1,
                                         cap=d["max_history"], flags=0, label=f"{name} tol={tol}")
            hits = hit1[..., 0] != rr.HIT_MISS
            carried = (count1 == 2)
            print(f"{name} tol {tol}: {carried.sum()} of {hits.sum()} hit pixels carried their history")
            assert carried[hits].mean() > 0.5 and not carried[~hits].any()
        # the pass has no effect on tracing: the next launch of the unchanged key runs no cull pass
        before = lp.dev.last_info()
        lp.trace(cam1, prev_count=1)
        info = lp.dev.last_info()
        assert info["CullPassRan"] == 0, (before, info)
    finally:
        lp.dev.close()


def gpu_sequence(rt, torch, scene_index, prefix):
    """tests/reproject_seq.py's sequence with the library's own planes: (cams, fresh, hits, refs, reproject)."""
    lp = Loop(rt, torch, scene_index, prefix, seq.W, seq.H, max_bounce=seq.BOUNCES)
    try:
        cams, fresh, hits, refs = [], [], [], []
        for i, ang in enumerate(seq.angles(lp.scene.DefaultXAngle)):
            cam = lp.camera(x_angle=float(ang))
            m0 = lp.trace(cam)
            cams.append(cam)
            fresh.append(m0)
            hit = lp.first_hit(cam)
            hits.append((hit[..., 0].copy(), hit[..., 1].view(np.float32).copy()))
            if i:
                refs.append(seq.mean_without_frame_0(m0, lp.trace(cam, frames=seq.REF_FRAMES, prev_count=1, prev=m0),
                                                     seq.REF_FRAMES))
    finally:
        lp.dev.close()

    def reproject(mean, key, t, cam, prev, history=None, hist_key=None, hist_t=None, hist_count=None, *, max_history,
                  depth_tolerance):
        h, w = key.shape
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        d_mean, d_hit = up(mean), up(pack_hit(key, t).view(np.int32))
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        count = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        kw, keep = {}, []
        if history is not None:
            keep = [up(history), up(pack_hit(hist_key, hist_t).view(np.int32)), up(hist_count.view(np.int32))]
            kw = dict(history_ptr=keep[0].data_ptr(), history_hit_ptr=keep[1].data_ptr(), history_count_ptr=keep[2].data_ptr())
        rt.reproject(w, h, cam, prev, d_mean.data_ptr(), d_hit.data_ptr(), out.data_ptr(), count.data_ptr(),
                     max_history=max_history, depth_tolerance=depth_tolerance, stream=torch.cuda.current_stream().cuda_stream,
                     **kw)
        torch.cuda.synchronize()
        return out.cpu().numpy(), count.cpu().numpy().view(np.uint32), None

    return cams, fresh, hits, refs, reproject


@pytest.mark.parametrize("name,asserted", [("0 RGB Glass", True), ("2 RTWeekend", True), ("1 prefix 64", False)])
def test_quality_six_moves_beat_the_raw_frame(rt, torch_cuda, name, asserted):
    index, prefix = seq.SCENES[name]
    d = rt.reproject_defaults()
    cams, fresh, hits, refs, reproject = gpu_sequence(rt, torch_cuda, index, prefix)
    res = seq.run(cams, fresh, hits, refs, max_history=d["max_history"], depth_tolerance=d["depth_tolerance"],
                  reproject=reproject)
    print(f"quality: scene {name}, defaults {d}: reprojected MSE / raw 1-spp MSE per move " +
          " ".join(f"{a / b:.3f}" for a, b in res) + "; raw MSE " + " ".join(f"{b:.4e}" for _, b in res) +
          ("" if asserted else " (recorded, not asserted)"))
    assert len(res) == seq.MOVES
    if asserted:
        for move, (rep, raw) in enumerate(res, 1):
            if move >= 2:
                assert rep < raw, (name, move, rep, raw)
