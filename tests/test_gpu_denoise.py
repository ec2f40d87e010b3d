"""GPU checks of rt_denoise: the a-trous filter over a running mean and rt_trace_first_hit's planes.

The checker is tests/denoise_ref.py, the numpy restatement of the definition in include/rt_trace.h.  Out and
Rgba8 must equal it bit for bit wherever it is not NaN and be NaN where it is (NaN payloads are not part of the
contract): no tolerance, no pixel excluded.  Rgba8 is compared with the oracle's RGBA8 encoding of the
restatement's Out on every pixel (both encode a NaN channel as 0).

  synthetic planes  numpy with a fixed seed: Key a handful of discs over a miss background, some with
                    RT_HIT_INSIDE; T in [0.5, 50], 1e30 on a miss; unit normals with a few zero vectors; albedo
                    with channels at 0 and below 0.01; a mean in [0, 4] with a few denormals, negatives, inf and
                    NaN.  1x1, 3x2, 33x17, 75x41 and 136x104; Iterations 1, 2, 5 and 6 (step 32 exceeds the small
                    images); each stop alone, all together, both flags, one run with Normal == NULL.
  real planes       scene 1 prefix 64 at 136x104 and scene 0 at 72x40: rt_trace at Frames = 1 and
                    rt_trace_first_hit of the same frame, denoised under the defaults and under DEMODULATE; the
                    downloaded planes restated.
  what is written   every plane lies in one arena that starts from test_gpu_tiles.POISON, with poisoned gaps:
                    after a call the inputs and the gaps are unchanged, Scratch is still poison at Iterations == 1,
                    and a plane that was not passed (Rgba8) is still poison.  A following rt_trace of the unchanged
                    key has CullPassRan == 0.
  quality           scene 1 prefix 64, 136x104, 8 bounces: the denoised 4-spp mean has a strictly lower MSE, on
                    channels clamped to [0, 1], against the GPU's 1024-spp mean than the raw 4-spp mean.  Chosen on
                    the CPU first (the oracle's means, an f64 first hit, the restatement): ratio 0.721 under the
                    defaults.  Measured on an MI355X with the library's own planes: ratio 0.7336 (denoised MSE
                    9.1204e-04, raw 1.2432e-03; profiles/denoise_quality.txt)."""
import numpy as np
import pytest

import denoise_ref as dr
from test_gpu_tiles import POISON, POISON_I32

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (33, 17), (75, 41), (136, 104)]
ITERATIONS = (1, 2, 5, 6)
CONFIGS = {  # name: (NormalPower, SigmaDepth, SigmaColor, Flags, pass Normal)
    "no_stop": (0, 0.0, 0.0, 0, True),
    "normal": (3, 0.0, 0.0, 0, True),
    "normal_k8": (8, 0.0, 0.0, 0, True),
    "depth": (0, 0.3, 0.0, 0, True),
    "colour": (0, 0.0, 1.5, 0, True),
    "all": (2, 0.25, 0.5, 0, True),
    "demodulate": (0, 0.0, 0.75, dr.DEMODULATE, True),
    "both_flags": (2, 0.25, 0.5, dr.DEMODULATE | dr.SRGB_POW, True),
    "pow": (1, 0.1, 0.0, dr.SRGB_POW, True),
    "normal_null": (0, 0.25, 0.5, 0, False),
}
GAP = 64  # poisoned words between two planes of the arena


def synthetic(w, h, seed):
    rng = np.random.default_rng(seed)
    n = w * h
    ys, xs = np.mgrid[0:h, 0:w]
    key = np.full((h, w), dr.HIT_MISS, np.uint32)
    for i in range(7):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.15, 0.45) * max(min(w, h), 2)
        k = np.uint32(rng.integers(0, 300)) | (np.uint32(0x80000000) if i % 3 == 2 else np.uint32(0))
        key[(xs - cx) ** 2 + (ys - cy) ** 2 < r * r] = k
    miss = key == dr.HIT_MISS
    t = np.where(miss, np.float32(1e30), rng.uniform(0.5, 50.0, (h, w)).astype(np.float32)).astype(np.float32)
    # depth varies smoothly inside a disc for half of the pixels, so that the depth stop has every weight to form
    smooth = (10.0 + 0.05 * xs + 0.03 * ys).astype(np.float32)
    t = np.where(~miss & (rng.random((h, w)) < 0.5), smooth, t).astype(np.float32)
    v = rng.normal(size=(h, w, 3))
    v[..., 2] += 2.0  # (mostly one hemisphere: the normal stop passes many taps, and stops some)
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    normal = np.zeros((h, w, 4), np.float32)
    normal[..., :3] = v
    normal[rng.random((h, w)) < 0.03] = 0.0
    normal[miss] = 0.0
    albedo = np.zeros((h, w, 4), np.float32)
    albedo[..., :3] = rng.random((h, w, 3), dtype=np.float32)
    albedo[..., :3][rng.random((h, w, 3)) < 0.05] = 0.0
    albedo[..., :3][rng.random((h, w, 3)) < 0.05] = np.float32(0.004)
    albedo[..., 3] = 1.0
    albedo[miss] = 0.0
    mean = np.zeros((h, w, 4), np.float32)
    mean[..., :3] = rng.random((h, w, 3), dtype=np.float32) * np.float32(4.0)
    mean[..., 3] = rng.random((h, w), dtype=np.float32)
    flat = mean.reshape(n, 4)
    specials = [np.float32(1e-41), np.float32(-1e-42), np.float32(-0.75), np.float32(-3.0), np.float32(np.inf),
                np.float32(-np.inf), np.float32(np.nan), np.float32(0.0), np.float32(-0.0)]
    if n >= 64:
        for i, p in enumerate(rng.choice(n, size=min(n // 16, 4 * len(specials)), replace=False)):
            flat[p, i % 3] = specials[i % len(specials)]
    elif n > 1:
        flat[n - 1, 1] = np.float32(1e-41)
    hit = np.zeros((h, w, 2), np.uint32)
    hit[..., 0] = key
    hit[..., 1] = t.view(np.uint32)
    return dict(mean=mean, hit=hit, normal=normal, albedo=albedo)


class Arena:
    """Mean, Hit, Normal, Albedo, Out, Scratch and Rgba8 in one poisoned device buffer with poisoned gaps."""
    ORDER = (("mean", 4), ("hit", 2), ("normal", 4), ("albedo", 4), ("out", 4), ("scratch", 4), ("rgba8", 1))

    def __init__(self, torch, w, h, planes):
        self.torch, self.w, self.h = torch, w, h
        n, at, self.off = w * h, GAP, {}
        for name, words in self.ORDER:
            self.off[name] = (at, n * words)
            at += (n * words + GAP + 3) // 4 * 4  # (every plane 16-byte aligned)
        host = np.full(at, POISON, np.uint32)
        for name in ("mean", "hit", "normal", "albedo"):
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


def run_and_check(rt, orc, torch, w, h, planes, *, iterations, normal_power, sigma_depth, sigma_color, flags,
                  pass_normal=True, pass_rgba8=True, label=""):
    ar = Arena(torch, w, h, planes)
    rt.denoise(w, h, ar.ptr("mean"), ar.ptr("hit"), ar.ptr("out"), scratch_ptr=ar.ptr("scratch"),
               normal_ptr=ar.ptr("normal") if pass_normal else 0, albedo_ptr=ar.ptr("albedo") if flags & dr.DEMODULATE else 0,
               rgba8_ptr=ar.ptr("rgba8") if pass_rgba8 else 0, iterations=iterations, normal_power=normal_power,
               sigma_depth=sigma_depth, sigma_color=sigma_color, demodulate=bool(flags & dr.DEMODULATE),
               srgb_pow=bool(flags & dr.SRGB_POW), stream=torch.cuda.current_stream().cuda_stream)
    words = ar.after()
    key, t = planes["hit"][..., 0], planes["hit"][..., 1].view(np.float32)
    want, want_rgba = dr.denoise(planes["mean"], key, t, planes["normal"], planes["albedo"], iterations=iterations,
                                 normal_power=normal_power, sigma_depth=sigma_depth, sigma_color=sigma_color, flags=flags,
                                 encode=orc.encode_rgba8)
    assert_same_bits(ar.plane(words, "out"), want, f"{label} Out")
    if pass_rgba8:
        assert np.array_equal(ar.plane(words, "rgba8"), want_rgba.reshape(-1)), f"{label}: Rgba8 differs"
    # nothing else is written: the inputs, the gaps, a plane that was not passed, and Scratch of a single pass
    written = np.zeros(words.size, bool)
    for name in ("out",) + (("scratch",) if iterations > 1 else ()) + (("rgba8",) if pass_rgba8 else ()):
        o, m = ar.off[name]
        written[o:o + m] = True
    assert np.array_equal(words[~written], ar.before[~written]), f"{label}: a word outside Out, Scratch and Rgba8 was written"
    o, m = ar.off["out"]
    assert not (words[o:o + m].reshape(-1, 4) == POISON).all(axis=1).any(), f"{label}: a pixel of Out was not written"
    return want


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic_planes_match_the_restatement(rt, orc, torch_cuda, w, h, config):
    k, sd, sc, flags, pass_normal = CONFIGS[config]
    planes = synthetic(w, h, seed=1000 * w + h)
    if w * h >= 64:  # the planes are what the check is designed on
        key = planes["hit"][..., 0]
        assert len(np.unique(key)) >= 4 and (key == dr.HIT_MISS).any() and (((key & 0x80000000) != 0) & (key != dr.HIT_MISS)).any()
        m = planes["mean"][..., :3]
        assert np.isnan(m).any() and np.isinf(m).any() and (m < 0).any() and ((m != 0) & (np.abs(m) < 1e-38)).any()
        a = planes["albedo"][key != dr.HIT_MISS][:, :3]
        assert (a == 0).any() and ((a > 0) & (a < 0.01)).any()
    for it in ITERATIONS:
        run_and_check(rt, orc, torch_cuda, w, h, planes, iterations=it, normal_power=k, sigma_depth=sd, sigma_color=sc,
                      flags=flags, pass_normal=pass_normal, pass_rgba8=it != 2, label=f"{w}x{h} {config} n={it}")


def test_the_stops_are_not_ignored(rt, orc, torch_cuda):
    """Each stop and each flag changes the restatement's result on the synthetic planes, so a kernel that
    parsed and ignored one would not pass the test above."""
    w, h = 75, 41
    planes = synthetic(w, h, seed=1000 * w + h)
    key, t = planes["hit"][..., 0], planes["hit"][..., 1].view(np.float32)
    outs = {}
    for name, (k, sd, sc, flags, _) in CONFIGS.items():
        outs[name], _ = dr.denoise(planes["mean"], key, t, planes["normal"], planes["albedo"], iterations=2, normal_power=k,
                                   sigma_depth=sd, sigma_color=sc, flags=flags)
    base = outs["no_stop"].view(np.uint32)
    for name in ("normal", "depth", "colour", "all", "demodulate"):
        assert (outs[name].view(np.uint32) != base).mean() > 0.05, name
    assert (outs["normal_k8"].view(np.uint32) != outs["normal"].view(np.uint32)).mean() > 0.05


class Traced:
    """rt_trace at `frames` and rt_trace_first_hit of frame 0 for one built-in input, downloaded."""

    def __init__(self, rt, torch, scene_index, prefix, w, h, frames, max_bounce=8):
        self.rt, self.torch, self.w, self.h = rt, torch, w, h
        s = rt.scene_builtin(scene_index)
        self.scene = rt.scene_prefix(s, prefix) if prefix else s
        self.cam = rt.camera_setup(self.scene, w, h)
        self.dev = rt.Device(0)
        self.dev.upload_scene(self.scene)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.max_bounce = max_bounce
        self.mean = self.trace(frames)
        hit = torch.full((w * h, 2), POISON_I32, dtype=torch.int32, device="cuda")
        normal = torch.full((w * h, 4), POISON_I32, dtype=torch.int32, device="cuda")
        albedo = torch.full((w * h, 4), POISON_I32, dtype=torch.int32, device="cuda")
        self.dev.trace_first_hit(self.cam, width=w, height=h, frame=0, hit_ptr=hit.data_ptr(), normal_ptr=normal.data_ptr(),
                                 albedo_ptr=albedo.data_ptr(), stream=self.stream)
        torch.cuda.synchronize()
        self.planes = dict(mean=self.mean, hit=hit.cpu().numpy().view(np.uint32).reshape(h, w, 2),
                           normal=normal.cpu().numpy().view(np.float32).reshape(h, w, 4),
                           albedo=albedo.cpu().numpy().view(np.float32).reshape(h, w, 4))

    def trace(self, frames, prev_count=0):
        torch, w, h = self.torch, self.w, self.h
        prev = torch.zeros((w * h, 4), dtype=torch.float32, device="cuda")
        cur = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.dev.trace(self.cam, width=w, height=h, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
                       prev_count=prev_count, frames=frames, max_bounce=self.max_bounce, stream=self.stream)
        torch.cuda.synchronize()
        return prev.cpu().numpy().reshape(h, w, 4)


@pytest.mark.parametrize("name,scene,prefix,w,h", [("s1p64_136x104", 1, 64, 136, 104), ("s0_72x40", 0, None, 72, 40)])
def test_real_planes_match_the_restatement(rt, orc, torch_cuda, name, scene, prefix, w, h):
    tr = Traced(rt, torch_cuda, scene, prefix, w, h, frames=1)
    try:
        d = rt.denoise_defaults()
        key = tr.planes["hit"][..., 0]
        assert (key == dr.HIT_MISS).any() and len(np.unique(key)) >= 4
        for flags in (0, dr.DEMODULATE):
            out = run_and_check(rt, orc, torch_cuda, w, h, tr.planes, iterations=d["iterations"],
                                normal_power=d["normal_power"], sigma_depth=d["sigma_depth"], sigma_color=d["sigma_color"],
                                flags=flags, label=f"{name} flags={flags}")
            changed = (out[..., :3].view(np.uint32) != tr.mean[..., :3].view(np.uint32)).mean()
            assert changed > 0.01, f"{name}: the filter changed {changed:.3f} of the channels only"
        # the pass has no effect on tracing: the next launch of the unchanged key runs no cull pass
        before = tr.dev.last_info()
        tr.trace(1, prev_count=1)
        info = tr.dev.last_info()
        assert info["CullPassRan"] == 0, (before, info)
    finally:
        tr.dev.close()


def test_quality_denoised_4spp_is_closer_to_1024spp_than_raw_4spp(rt, orc, torch_cuda):
    w, h = 136, 104
    tr = Traced(rt, torch_cuda, 1, 64, w, h, frames=4)
    try:
        ref = tr.trace(1024)
        d = rt.denoise_defaults()
        ar = Arena(torch_cuda, w, h, tr.planes)
        rt.denoise(w, h, ar.ptr("mean"), ar.ptr("hit"), ar.ptr("out"), scratch_ptr=ar.ptr("scratch"),
                   normal_ptr=ar.ptr("normal"), stream=tr.stream)
        out = ar.plane(ar.after(), "out").view(np.float32).reshape(h, w, 4)

        def mse(a):
            return float(((np.clip(a[..., :3], 0, 1).astype(np.float64) - np.clip(ref[..., :3], 0, 1)) ** 2).mean())

        raw, den = mse(tr.mean), mse(out)
        print(f"quality: defaults {d}: denoised MSE {den:.4e}, raw 4-spp MSE {raw:.4e}, ratio {den / raw:.4f}")
        assert den < raw
    finally:
        tr.dev.close()
