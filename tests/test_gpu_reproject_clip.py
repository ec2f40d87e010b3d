"""GPU checks of rt_reproject_clip: rt_reproject with the history clamped to the fresh neighbourhood's band.

The checker is tests/reproject_clip_ref.py, the numpy restatement of the definition in include/rt_trace.h.  Out,
OutCount and Rgba8 must equal it bit for bit wherever it is not NaN and be NaN where it is: no tolerance, no pixel
excluded.

  synthetic planes  numpy with a fixed seed: Key in runs along x of a few spheres (some with RT_HIT_INSIDE), blocks of
                    misses, and isolated pixels whose key no neighbour has; T a smooth field around the orbit's
                    distance; the history's keys the same with a few words changed, counts from 0 to beyond the cap.
                    Mean is a colour per sphere plus noise; History is, per pixel, near that colour (inside the
                    band), or far outside it on either side; both carry +-inf, NaN, denormals and negatives.
                    1x1, 33x9, 70x13 and 136x104 (none a multiple of the 32x8 tile) at Radius 1, 2 and 3:
                    one key step in angle with Rgba8 and the pow flag, the same camera twice without Rgba8 under
                    the default tolerance, and no history.
  never binding     one sphere, a noisy mean and a Gamma of 1e30: the band is wider than any history (checked on
                    the restatement's band), and Out, OutCount and Rgba8 equal rt_reproject's of the same planes.
  what is written   every plane lies in one arena that starts from test_gpu_tiles.POISON, with poisoned gaps
                    (test_gpu_reproject.Arena): after a call the inputs and the gaps are unchanged and a plane that
                    was not passed is still poison; every pixel of Out and OutCount is written.
  traced planes     the six-move sequence of tests/reproject_seq.py on scene 0 with the library's own 1-spp means
                    and first-hit planes, carried by rt_reproject_clip at the library's defaults: every move equals
                    the restatement on the same planes."""
import numpy as np
import pytest

import reproject_clip_ref as rc
import reproject_ref as rr
import reproject_seq as seq
from test_gpu_reproject import Arena, assert_same_bits, camera_pair, gpu_sequence, pack_hit
from test_gpu_tiles import POISON

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (33, 9), (70, 13), (136, 104)]
CAP = 8
CONFIGS = {  # name: (camera pair, DepthTolerance, Frames, Flags, Gamma, history, Rgba8)
    "angle_pow_rgba8": ("angle", 0.0, 1, rr.SRGB_POW, 1.0, True, True),
    "same_tolerance": ("same", 0.1, 3, 0, 0.5, True, False),
    "no_history": ("angle", 0.1, 1, 0, 2.0, False, True),
}
SPECIALS = [np.float32(v) for v in (1e-41, -1e-42, -0.75, -3.0, np.inf, -np.inf, np.nan, 0.0, -0.0, 3e38, 1e20)]


def synthetic(w, h, seed, distance):
    rng = np.random.default_rng(seed)
    n = w * h
    ys, xs = np.mgrid[0:h, 0:w]
    palette = np.array([3, 17, 40 | int(rr.HIT_INSIDE), 255, 256], np.uint32)
    key = np.zeros((h, w), np.uint32)
    for y in range(h):  # runs along x, 1 to 12 pixels long; a row starts where the row above did, half of the time
        x = 0
        while x < w:
            run = int(rng.integers(1, 13))
            k = palette[rng.integers(0, len(palette))]
            if y and rng.random() < 0.5:
                k = key[y - 1, x]
            key[y, x:x + run] = k
            x += run
    for _ in range(max(1, n // 400)):  # blocks of misses
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        key[y0:y0 + 5, x0:x0 + 9] = rr.HIT_MISS
    isolated = rng.random((h, w)) < 0.02
    key[isolated] = (1000 + np.arange(int(isolated.sum()))).astype(np.uint32)  # keys no other pixel has
    if n == 1:
        key[:] = 5
    miss = key == rr.HIT_MISS
    smooth = (distance * (0.8 + 0.4 * (xs + 0.6 * ys) / max(w + h, 2))).astype(np.float32)
    t = np.where(miss, np.float32(1e30), smooth).astype(np.float32)
    hist_key = key.copy()
    pick = rng.random((h, w))
    hist_key[pick < 0.03] = 3
    flip = (pick >= 0.03) & (pick < 0.05) & ~miss
    hist_key[flip] ^= rr.HIT_INSIDE
    hist_t = np.where(hist_key == rr.HIT_MISS, np.float32(1e30),
                      smooth * (1 + 0.01 * rng.uniform(-1, 1, (h, w)))).astype(np.float32)
    hist_count = rng.choice(np.array([0, 1, 2, 5, CAP - 1, CAP, CAP + 3, 0xFFFFFFFF], np.uint32), (h, w),
                            p=[0.05, 0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05]).astype(np.uint32)
    # Mean: a colour per sphere plus noise; History: near it, or far outside the band on either side
    colour = (np.stack([(key * np.uint32(m) % np.uint32(97)) for m in (7, 13, 29)], axis=-1) / 97.0 * 3.0).astype(np.float32)
    mean = np.zeros((h, w, 4), np.float32)
    mean[..., :3] = colour + rng.random((h, w, 3), dtype=np.float32) * np.float32(0.5)
    mean[..., 3] = rng.random((h, w), dtype=np.float32)
    history = np.zeros((h, w, 4), np.float32)
    where = ((xs // 6 + ys // 3) % 4)[..., None]  # in blocks, so that the taps of a gather mostly agree
    far = np.where(where == 0, np.float32(40.0), np.where(where == 2, np.float32(-40.0), np.float32(0.0)))
    history[..., :3] = colour + np.float32(0.22) + rng.random((h, w, 3), dtype=np.float32) * np.float32(0.06) + far
    history[..., 3] = rng.random((h, w), dtype=np.float32)
    for img in (mean, history):
        flat = img.reshape(n, 4)
        if n >= 64:
            for i, p in enumerate(rng.choice(n, size=min(n // 12, 4 * len(SPECIALS)), replace=False)):
                flat[p, i % 3] = SPECIALS[i % len(SPECIALS)]
    return dict(mean=mean, hit=pack_hit(key, t), history=history, history_hit=pack_hit(hist_key, hist_t),
                history_count=hist_count)


def restate(rt, orc, planes, cam, prev, *, tol, frames, flags, history, radius, gamma, clip=True):
    key, t = planes["hit"][..., 0], planes["hit"][..., 1].view(np.float32)
    given = (planes["history"], planes["history_hit"][..., 0], planes["history_hit"][..., 1].view(np.float32),
             planes["history_count"]) if history else (None, None, None, None)
    kw = dict(frames=frames, max_history=CAP, depth_tolerance=tol, flags=flags, encode=orc.encode_rgba8)
    if clip:
        return rc.reproject_clip(planes["mean"], key, t, rt.camera_floats(cam), rt.camera_floats(prev), *given,
                                 radius=radius, gamma=gamma, **kw)
    return rr.reproject(planes["mean"], key, t, rt.camera_floats(cam), rt.camera_floats(prev), *given, **kw)


def run_and_check(rt, torch, w, h, planes, cam, prev, want, *, tol, frames, flags, history, pass_rgba8, radius, gamma,
                  label, clip=True):
    """One call in a poisoned arena against the restatement's (Out, OutCount, Rgba8); returns the arena's words."""
    ar = Arena(torch, w, h, planes)
    hist = dict(history_ptr=ar.ptr("history"), history_hit_ptr=ar.ptr("history_hit"),
                history_count_ptr=ar.ptr("history_count")) if history else {}
    call, extra = (rt.reproject_clip, dict(radius=radius, gamma=gamma)) if clip else (rt.reproject, {})
    call(w, h, cam, prev, ar.ptr("mean"), ar.ptr("hit"), ar.ptr("out"), ar.ptr("out_count"),
         rgba8_ptr=ar.ptr("rgba8") if pass_rgba8 else 0, frames=frames, max_history=CAP, depth_tolerance=tol,
         srgb_pow=bool(flags & rr.SRGB_POW), stream=torch.cuda.current_stream().cuda_stream, **hist, **extra)
    words = ar.after()
    want_out, want_count, want_rgba = want
    assert_same_bits(ar.plane(words, "out"), want_out, f"{label} Out")
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
    return ar, words


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic_planes_match_the_restatement(rt, orc, torch_cuda, w, h, radius):
    for name, (pair, tol, frames, flags, gamma, history, rgba8) in CONFIGS.items():
        cam, prev, distance = camera_pair(rt, w, h, pair)
        planes = synthetic(w, h, seed=1000 * w + h, distance=distance)
        kw = dict(tol=tol, frames=frames, flags=flags, history=history, radius=radius, gamma=gamma)
        want = restate(rt, orc, planes, cam, prev, **kw)
        if history and w * h >= 64:  # the planes are what the check is designed on
            plain = restate(rt, orc, planes, cam, prev, clip=False, **kw)
            key = planes["hit"][..., 0]
            folded = want[1] != frames
            moved = (want[0].view(np.uint32) != plain[0].view(np.uint32)).any(axis=2)
            assert np.array_equal(want[1], plain[1]) and folded.mean() > 0.3
            assert (moved & folded).sum() > 0.2 * folded.sum() and (~moved & folded).sum() > 0.05 * folded.sum(), name
            assert not moved[~folded].any() and (key == rr.HIT_MISS).any() and ((key >= 1000) & (key < 100000)).any()
            for img in (planes["mean"][..., :3], planes["history"][..., :3]):
                assert np.isnan(img).any() and np.isposinf(img).any() and np.isneginf(img).any()
        run_and_check(rt, torch_cuda, w, h, planes, cam, prev, want, pass_rgba8=rgba8, label=f"{w}x{h} R{radius} {name}", **kw)


@pytest.mark.parametrize("w,h,radius", [(70, 13, 3), (136, 104, 1), (136, 104, 2)])
def test_a_band_that_never_binds_gives_rt_reprojects_bits(rt, orc, torch_cuda, w, h, radius):
    cam, prev, distance = camera_pair(rt, w, h, "angle")
    planes = synthetic(w, h, seed=77, distance=distance)
    rng = np.random.default_rng(78)
    for name in ("hit", "history_hit"):  # one sphere and a block of misses, at a smooth distance
        planes[name][..., 0] = 9
        planes[name][2:6, 3:30, 0] = rr.HIT_MISS
    for name in ("mean", "history"):
        planes[name][..., :3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(4.0)
    gamma = 1e30
    lo, hi, nf = rc.band(planes["mean"], planes["hit"][..., 0], radius, gamma)
    surface = planes["hit"][..., 0] != rr.HIT_MISS
    assert (nf[surface] >= 4).all() and (lo[surface] < -1e20).all() and (hi[surface] > 1e20).all()
    kw = dict(tol=0.1, frames=1, flags=0, history=True, radius=radius, gamma=gamma)
    want_plain = restate(rt, orc, planes, cam, prev, clip=False, **kw)
    want = restate(rt, orc, planes, cam, prev, **kw)
    assert (want_plain[1] == 2).mean() > 0.5
    assert_same_bits(want[0].view(np.uint32), want_plain[0], "the restatements")
    ar, words = run_and_check(rt, torch_cuda, w, h, planes, cam, prev, want_plain, pass_rgba8=True, clip=False,
                              label=f"{w}x{h} rt_reproject", **kw)
    written = {name: ar.plane(words, name).copy() for name in ("out", "out_count", "rgba8")}
    ar, words = run_and_check(rt, torch_cuda, w, h, planes, cam, prev, want, pass_rgba8=True,
                              label=f"{w}x{h} R{radius} never binding", **kw)
    for name, plane in written.items():  # the two calls' own bytes, NaN payloads included
        assert np.array_equal(ar.plane(words, name), plane), f"{name} differs from rt_reproject's"


def test_six_moves_on_scene_0_with_the_librarys_planes_match_the_restatement(rt, torch_cuda):
    torch = torch_cuda
    d = rt.reproject_clip_defaults()
    cams, fresh, hits, refs, _ = gpu_sequence(rt, torch, *seq.SCENES["0 RGB Glass"])
    floats = [rt.camera_floats(c) for c in cams]
    w, h = seq.W, seq.H
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    hist, cnt = fresh[0].copy(), np.ones((h, w), np.uint32)
    plain_hist, plain_cnt = hist, cnt
    ratios = []
    for i in range(1, len(cams)):
        kw = dict(max_history=d["max_history"], depth_tolerance=d["depth_tolerance"])
        given = (hist, hits[i - 1][0], hits[i - 1][1], cnt)
        want, want_cnt, _ = rc.reproject_clip(fresh[i], hits[i][0], hits[i][1], floats[i], floats[i - 1], *given,
                                              radius=d["radius"], gamma=d["gamma"], **kw)
        plain_hist, plain_cnt, _ = rr.reproject(fresh[i], hits[i][0], hits[i][1], floats[i], floats[i - 1], plain_hist,
                                                hits[i - 1][0], hits[i - 1][1], plain_cnt, **kw)
        planes = [up(fresh[i]), up(pack_hit(*hits[i]).view(np.int32)), up(hist), up(pack_hit(*hits[i - 1]).view(np.int32)),
                  up(cnt.view(np.int32))]
        out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        count = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        rt.reproject_clip(w, h, cams[i], cams[i - 1], planes[0].data_ptr(), planes[1].data_ptr(), out.data_ptr(),
                          count.data_ptr(), history_ptr=planes[2].data_ptr(), history_hit_ptr=planes[3].data_ptr(),
                          history_count_ptr=planes[4].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert_same_bits(out.cpu().numpy().view(np.uint32), want, f"move {i} Out")
        assert np.array_equal(count.cpu().numpy().view(np.uint32), want_cnt), f"move {i}: OutCount differs"
        hits_i = hits[i][0] != rr.HIT_MISS
        assert (want_cnt[hits_i] > 1).mean() > 0.5 and (want.view(np.uint32) != plain_hist.view(np.uint32)).any()
        hist, cnt = want, want_cnt
        ratios.append((seq.mse(hist, refs[i - 1]), seq.mse(plain_hist, refs[i - 1]), seq.mse(fresh[i], refs[i - 1])))
    print(f"scene 0, defaults {d}: MSE / raw 1-spp MSE per move, clipped " + " ".join(f"{a / c:.3f}" for a, _, c in ratios) +
          "; rt_reproject " + " ".join(f"{b / c:.3f}" for _, b, c in ratios))
