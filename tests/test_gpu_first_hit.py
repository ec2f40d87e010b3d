"""GPU checks of rt_trace_first_hit: what every pixel's primary ray sees -- sphere, depth, normal, albedo.

The sphere index is checked bit-exactly against the oracle as it stands, with no tolerance and no pixel
excluded.  The oracle renders a *coded* copy of the scene: every material (the `spheres` rows and the
`materials` rows) has Color = 0, Specular = 0, IndexOfRefraction = 0 and Emissive = (i + 1, 0, 0) for sphere i,
rendered with use_sky = False, max_bounce = 1, frames = 1, prev_count = k.  The running mean's x is then
(i + 1) / (k + 1) for the sphere the reference's first segment selects and 0 on a miss -- exact for
k in {0, 1, 3, 7}: k + 1 is a power of two, the attenuation is 1 and the previous mean is 0.  The GPU traces
the unmodified scene: the pass reads no material for Key.

T, Normal, the inside flag and Albedo are checked in centre mode against an f64 restatement of the first hit
(first_hit_f64), on every pixel that restatement can decide: a pixel is *ambiguous* when a sphere in front of
the winner has |dist/r^2 - 1| < 1e-4, when the two nearest accepted t are within 1e-4 relative, or when a
candidate t is within 1e-5 of eps.  Ambiguous pixels, together with those whose winner has dist/r^2 > 1 - 1e-3
(X = sqrt(r^2 - dist) is ill-conditioned there for any f32 evaluation, the reference's included; excluded from
the T and Normal checks only), are at most 0.5 % of each input.

The tolerance for T is no chosen number: for the same pixels the f64 direction rounded to f32 and the camera
position go through the oracle's own f32 sequence (or_group_test), and the largest |t_f32 - t_f64| relative to
|C| + r is the reference's own error.  The GPU's limit is 4 times that (its direction comes from f32 film
arithmetic, not from a rounded f64 one: about another ulp per operation), and Normal's follows from T's by
|dN| <= dT / r + 4 * 2^-23.  Measured reference error (|t_f32 - t_f64| / (|C| + r)) and the limit it gives:
  scene 1 prefix 64, 136 x 104, centre      reference 5.02e-07   limit 2.01e-06   (0 ambiguous, 4 ill-conditioned)
  scene 0, 72 x 40, centre                  reference 6.93e-07   limit 2.77e-06   (1 ambiguous, 4 ill-conditioned)
  seed 2 "inside" camera, 72 x 40, centre   reference 9.24e-08   limit 3.70e-07   (0, 0)
  seed 18 "inside" camera, 72 x 40, centre  reference 3.71e-07   limit 1.48e-06   (1, 0)   1,060 spheres, 9 mask words
  seed 2 "outside" camera, 72 x 40, centre  reference 5.03e-07   limit 2.01e-06   (3, 3)   115 spheres, 60 of them seen
  scene 0, 72 x 40, frame 3's jitters       reference 7.03e-07   limit 2.81e-06   (1, 5)
Each test prints these beside the GPU's own error; on an MI355X that was, in the same order, 1.62e-06, 7.11e-07,
1.25e-07, 3.07e-07, 7.29e-07 and 6.50e-07 (the same under both rule sets), and Normal's error at most 0.80 of its
limit.  Normal is the reference's Normalize, which returns zero where len^2 <= 1e-4: the 115 pixels of the seed 2
"outside" input whose winner has r^2 < 1e-4 must hold exactly that, and |Normal| = 1 is asked of the others.
Scene 2 (RTWeekend) at 136 x 104 has 10 ambiguous pixels, but
122 more whose winner is ill-conditioned -- the rays that meet the ground sphere (r = 1000) near its horizon -- which
together break the 0.5 % cap: it is a badly chosen input for the T and Normal check, so there it serves the checks
of Key, Albedo, the inside flag and Normal's side and length alone, with the cap on its ambiguous pixels.

Planes start from the poison pattern of test_gpu_tiles.py, so an untouched word is recognisable."""
import ctypes

import numpy as np
import pytest

import random_scenes
from test_gpu_tiles import LISTS, POISON, POISON_I32, tile_mask

pytestmark = pytest.mark.gpu

EINVAL = -22
EPS = 1e-4
FRAMES = (0, 1, 3, 7)
BUILTIN = {  # name: (scene index, prefix or None, W, H)
    "s1p64_136x104": (1, 64, 136, 104),   # ragged right and bottom reference tiles, 8 px wide and tall
    "s1p64_75x41": (1, 64, 75, 41),       # wave tiles clipped by the image in both directions
    "s0_72x40": (0, None, 72, 40),        # 5 spheres: a last group with padding lanes
    "s1p3_72x40": (1, 3, 72, 40),
    "s2_136x104": (2, None, 136, 104),    # RTWeekend: 482 spheres, 4 mask words
}
# tests/random_scenes.py seeds: 18 is a scene of 1,060 spheres (more than 256), 2 a "cloud" scene; each brings
# its four cameras (outside, inside, on_surface, grazing with add_grazing_spheres: seed 18 is at the generator's
# largest scene already, so its extras are cut off again and seed 2's grazing camera is the one with tangent spheres)
RANDOM_SEEDS = (18, 2)
RW, RH = 72, 40
KINDS = ("outside", "inside", "on_surface", "grazing")
BASE = "s1p64_136x104"
INSIDE = "r2_inside"           # 115 spheres; the camera's sphere fills the image
INSIDE_MANY = "r18_inside"     # 1,060 spheres, 9 mask words; the camera's sphere wins 2,066 of 2,880 pixels, four others the rest


class Input:
    def __init__(self, name, s, o, w, h, rt, orc):
        self.name, self.s, self.o, self.w, self.h = name, s, o, w, h
        self.cam, self.ocam = rt.camera_setup(s, w, h), orc.camera(o, w, h)
        self.camf = rt.camera_floats(self.cam)
        n = len(o.spheres)
        sp, ma = o.spheres.copy(), o.materials.copy()
        sp[:, 8:20] = 0.0
        ma[:, :] = 0.0
        sp[:, 12] = np.arange(1, n + 1, dtype=np.float32)   # Emissive.x of the sphere's own material
        # and of the materials row MaterialIndex names: every row, since the SIMD rules test all four lanes of the
        # last group and a prefix scene's padding lanes hold real spheres (MaterialIndex up to 4 * groups - 1)
        ma[:, 4] = np.arange(1, len(ma) + 1, dtype=np.float32)
        self.coded = orc.Scene(sp, o.groups, ma, look_at=tuple(o.look_at[:3]), use_sky=False, distance=o.distance,
                               x_angle=o.x_angle, y_height=o.y_height)
        self._index = {}
        self._orc = orc

    def oracle_index(self, k, simd):
        """(H*W,) int: the sphere the reference's first segment of frame k selects, -1 on a miss (read-only)."""
        if (k, simd) not in self._index:
            op, _, _ = self._orc.render(self.coded, self.ocam, self.w, self.h, prev_count=k, frames=1, max_bounce=1,
                                        simd=simd)
            v = op[:, 0].astype(np.float64) * (k + 1)
            assert np.array_equal(v, np.round(v)) and v.min() >= 0 and v.max() <= len(self.coded.materials), self.name
            idx = v.astype(np.int64) - 1
            idx.setflags(write=False)
            self._index[(k, simd)] = idx
        return self._index[(k, simd)]


@pytest.fixture(scope="module")
def inputs(rt, orc):
    cache = {}
    # the random inputs are what they are chosen for: a scene of more than 256 spheres, a cloud scene, four cameras each
    specs = {seed: random_scenes.make(seed) for seed in RANDOM_SEEDS}
    assert any(s["n"] > 256 for s in specs.values()) and any(s["cloud"] for s in specs.values())
    assert all(tuple(c[4] for c in s["cameras"]) == KINDS for s in specs.values())

    def get(name):
        if name in cache:
            return cache[name]
        if name in BUILTIN:
            idx, prefix, w, h = BUILTIN[name]
            s, o = rt.scene_builtin(idx), orc.scene_builtin(idx)
            if prefix:
                s, o = rt.scene_prefix(s, prefix), o.prefix(prefix)
            cache[name] = Input(name, s, o, w, h, rt, orc)
            return cache[name]
        seed, kind = int(name[1:name.index("_")]), name[name.index("_") + 1:]
        spec = random_scenes.make(seed)
        spheres = random_scenes.add_grazing_spheres(rt, spec, RW, RH, seed=seed)
        for look, dist, ang, yh, k in spec["cameras"]:
            s, o = random_scenes.build(rt, orc, spheres, spec["use_sky"], look, dist, ang, yh)
            cache[f"r{seed}_{k}"] = Input(f"r{seed}_{k}", s, o, RW, RH, rt, orc)
        return cache[name]

    return get


class Dev:
    """One device; the scene of the input in use is uploaded when it changes."""

    def __init__(self, rt, options=None):
        self.dev, self.current = rt.Device(0, options=options), None

    def use(self, inp):
        if self.current != inp.name.split("_")[0] + str(len(inp.o.spheres)):
            self.dev.upload_scene(inp.s)
            self.current = inp.name.split("_")[0] + str(len(inp.o.spheres))
        return self.dev


@pytest.fixture(scope="module")
def fdev(rt, torch_cuda):
    d = Dev(rt)
    yield d
    d.dev.close()


class Planes:
    """The three device planes, poisoned."""

    def __init__(self, torch, w, h):
        self.torch, self.w, self.h = torch, w, h
        self.hit = torch.full((w * h, 2), POISON_I32, dtype=torch.int32, device="cuda")
        self.normal = torch.full((w * h, 4), POISON_I32, dtype=torch.int32, device="cuda")
        self.albedo = torch.full((w * h, 4), POISON_I32, dtype=torch.int32, device="cuda")

    def ptrs(self, hit=True, normal=True, albedo=True):
        return dict(hit_ptr=self.hit.data_ptr() if hit else 0, normal_ptr=self.normal.data_ptr() if normal else 0,
                    albedo_ptr=self.albedo.data_ptr() if albedo else 0)

    def words(self):
        """(hit (n, 2), normal (n, 4), albedo (n, 4)) u32 after a device sync."""
        self.torch.cuda.synchronize()
        return tuple(t.cpu().numpy().view(np.uint32) for t in (self.hit, self.normal, self.albedo))


def first_hit(dev, torch, inp, *, frame=0, simd=True, centre=False, tiles=None, which=(True, True, True)):
    pl = Planes(torch, inp.w, inp.h)
    dev.trace_first_hit(inp.cam, width=inp.w, height=inp.h, frame=frame, simd=simd, centre=centre, tiles=tiles,
                        stream=torch.cuda.current_stream().cuda_stream, **pl.ptrs(*which))
    return pl


# ------------------------------------------------- 1. Key against the oracle, bit for bit, every pixel
def assert_key_parity(rt, torch, dev, inp, k, simd):
    hit, _, _ = first_hit(dev, torch, inp, frame=k, simd=simd).words()
    want = inp.oracle_index(k, simd)
    key = hit[:, 0]
    got = np.where(key == rt.HIT_MISS, -1, (key & ~np.uint32(rt.HIT_INSIDE)).astype(np.int64))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{inp.name} k={k} simd={simd}: {bad.size} pixels see another sphere, first pixel {bad[0]}: "
                           f"GPU {got[bad[0]]}, oracle {want[bad[0]]}")
    miss = want < 0
    assert np.all(hit[miss, 0] == rt.HIT_MISS) and np.all(hit[miss, 1] == np.float32(1e30).view(np.uint32))
    assert not np.any(hit[~miss, 1] == np.float32(1e30).view(np.uint32))
    return int((~miss).sum()), len(set(want[~miss].tolist()))


@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
@pytest.mark.parametrize("name", list(BUILTIN))
def test_key_matches_the_oracle_builtin(rt, torch_cuda, inputs, fdev, name, simd):
    inp = inputs(name)
    dev = fdev.use(inp)
    seen = [assert_key_parity(rt, torch_cuda, dev, inp, k, simd) for k in FRAMES]
    print(f"{name} simd={simd}: (hit pixels, distinct spheres) per frame {seen}")
    if name == BASE:
        # the input is what the check was designed on: a third of the pixels hit, two dozen spheres are seen,
        # and consecutive frames differ, so a wrong frame index cannot pass
        assert all(4300 <= h <= 4500 and 24 <= d <= 30 for h, d in seen), seen
        assert int((inp.oracle_index(0, simd) != inp.oracle_index(1, simd)).sum()) > 100


@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_key_matches_the_oracle_random(rt, torch_cuda, inputs, fdev, seed, kind, simd):
    inp = inputs(f"r{seed}_{kind}")
    dev = fdev.use(inp)
    for k in (0, 3):
        assert_key_parity(rt, torch_cuda, dev, inp, k, simd)


# ------------------------------------------------- 2. Cull off
@pytest.mark.parametrize("name", [BASE, INSIDE])
def test_cull_off_writes_the_same_bytes(rt, torch_cuda, inputs, fdev, name):
    inp = inputs(name)
    off = Dev(rt, options={"Cull": rt.RT_OPT_OFF})
    try:
        for simd, centre, k in ((True, False, 0), (False, False, 3), (True, True, 0)):
            a = first_hit(fdev.use(inp), torch_cuda, inp, frame=k, simd=simd, centre=centre).words()
            b = first_hit(off.use(inp), torch_cuda, inp, frame=k, simd=simd, centre=centre).words()
            for pa, pb, plane in zip(a, b, ("Hit", "Normal", "Albedo")):
                assert np.array_equal(pa, pb), f"{name} simd={simd} centre={centre}: {plane} differs with Cull off"
                assert not np.any(np.all(pa == POISON, axis=1)), plane  # (every pixel of the image was written)
    finally:
        off.dev.close()


# ------------------------------------------------- 3. tile lists
@pytest.mark.parametrize("name", ["7", "19", "right_column", "descending", "all_but_7"])
def test_tile_lists_write_the_listed_pixels_only(rt, torch_cuda, inputs, fdev, name):
    inp = inputs(BASE)
    dev = fdev.use(inp)
    whole = first_hit(dev, torch_cuda, inp, frame=1).words()
    m = tile_mask(inp.w, inp.h, LISTS[name])
    assert m.any() and not m.all()
    part = first_hit(dev, torch_cuda, inp, frame=1, tiles=LISTS[name]).words()
    for pw, pp, plane in zip(whole, part, ("Hit", "Normal", "Albedo")):
        assert np.array_equal(pp[m], pw[m]), f"{name}: listed pixels of {plane} differ from the whole-image call"
        assert np.all(pp[~m] == POISON), f"{name}: {int((pp[~m] != POISON).any(1).sum())} unlisted pixels of {plane} written"
    # a plane passed as NULL is not written: the buffer exists, poisoned, and is not passed
    for skip in range(3):
        which = tuple(i != skip for i in range(3))
        got = first_hit(dev, torch_cuda, inp, frame=1, tiles=LISTS[name], which=which).words()
        for i, (pg, pw) in enumerate(zip(got, whole)):
            if i == skip:
                assert np.all(pg == POISON), f"{name}: the plane that was not passed was written"
            else:
                assert np.array_equal(pg[m], pw[m]) and np.all(pg[~m] == POISON)
    # a list of no tiles: RT_OK, nothing written
    none = first_hit(dev, torch_cuda, inp, frame=1, tiles=[]).words()
    assert all(np.all(p == POISON) for p in none)


def test_reserve_covers_a_listed_call_and_upload_waits_for_the_pass(rt, torch_cuda, inputs, fdev):
    """rt_device_reserve sizes the pass's bitmap, so the first listed call allocates no device memory; and
    rt_scene_upload waits for a pass still in flight, so its planes hold the scene it was launched with."""
    torch = torch_cuda
    a, b = inputs(BASE), inputs("s2_136x104")
    want_a = first_hit(fdev.use(a), torch, a, frame=1).words()
    want_b = first_hit(fdev.use(b), torch, b, frame=1).words()
    dev = rt.Device(0)
    try:
        dev.upload_scene(a.s)
        dev.reserve(a.w, a.h)
        pl = Planes(torch, a.w, a.h)
        pb = Planes(torch, b.w, b.h)
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info()[0]
        stream = torch.cuda.current_stream().cuda_stream
        dev.trace_first_hit(a.cam, width=a.w, height=a.h, frame=1, tiles=LISTS["all_but_7"], stream=stream, **pl.ptrs())
        assert torch.cuda.mem_get_info()[0] == free, "the first listed call after rt_device_reserve allocated device memory"
        dev.trace_first_hit(a.cam, width=a.w, height=a.h, frame=1, tiles=[7], stream=stream, **pl.ptrs())
        dev.upload_scene(b.s)  # no wait of the caller's in between: the upload's own
        dev.trace_first_hit(b.cam, width=b.w, height=b.h, frame=1, stream=stream, **pb.ptrs())
        for got, want in ((pl.words(), want_a), (pb.words(), want_b)):
            for pg, pw in zip(got, want):
                assert np.array_equal(pg, pw)
    finally:
        dev.close()


# ------------------------------------------------- 4. no effect on tracing
def test_no_effect_on_tracing(rt, orc, torch_cuda, inputs):
    torch = torch_cuda
    inp = inputs(BASE)
    w, h = inp.w, inp.h
    dev = rt.Device(0)
    try:
        dev.upload_scene(inp.s)
        for simd in (True, False):
            prev = torch.zeros((w * h, 4), dtype=torch.float32, device="cuda")
            cur = torch.zeros(w * h, dtype=torch.int32, device="cuda")
            rays = torch.zeros(1, dtype=torch.int64, device="cuda")
            args = dict(width=w, height=h, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
                        frames=8, max_bounce=8, simd=simd, stream=torch.cuda.current_stream().cuda_stream)
            dev.trace(inp.cam, prev_count=0, **args)
            before = dev.last_info()
            pl = first_hit(dev, torch, inp, frame=5, simd=simd, tiles=[7, 3])
            after = dev.last_info()
            assert after == before, (before, after)
            dev.trace(inp.cam, prev_count=8, **args)
            info = dev.last_info()
            assert info["CullPassRan"] == 0 and info["TileCounts"] == 0, info
            torch.cuda.synchronize()
            op, oc, orays = orc.render(inp.o, inp.ocam, w, h, frames=16, max_bounce=8, simd=simd)
            assert np.array_equal(prev.cpu().numpy().view(np.uint32), op.view(np.uint32).reshape(-1, 4))
            assert np.array_equal(cur.cpu().numpy().view(np.uint32), oc)
            assert int(rays.item()) == orays
            assert not np.all(pl.words()[0] == POISON)  # (the pass did run)
    finally:
        dev.close()


# ------------------------------------------------- 5. T, Normal, inside flag and Albedo against f64
def first_hit_f64(camf, spheres, w, h, jx=None, jy=None):
    """The first hit of every pixel's primary ray in f64 (eps = 1e-4; T - X, else T + X): dict of (h*w,) arrays --
    win (-1: miss), t, inside (T - X < eps of the winner), ambiguous, illcond, and d (n, 3), n_out (n, 3), cr (|C| + r)."""
    c = camf.astype(np.float64)
    cp, cx, cy, fc, fw, fh = c[0:3], c[8:11], c[12:15], c[16:19], c[20], c[21]
    ys, xs = np.mgrid[0:h, 0:w]
    px = xs.ravel().astype(np.float64) + (0.0 if jx is None else jx)
    py = ys.ravel().astype(np.float64) + (0.0 if jy is None else jy)
    ax = (-1.0 + (px * 2.0) / w) * fw * 0.5
    ay = (-1.0 + (py * 2.0) / h) * fh * 0.5
    v = (fc + ax[:, None] * cx + ay[:, None] * cy) - cp
    d = v / np.linalg.norm(v, axis=1, keepdims=True)
    s = spheres[:, 0:3].astype(np.float64)
    r = spheres[:, 4].astype(np.float64)
    r2 = r * r
    cc = s - cp                      # C = S - O: the camera is every ray's origin
    cc2 = (cc * cc).sum(1)
    n = w * h
    out = dict(win=np.full(n, -1, np.int64), t=np.full(n, np.inf), inside=np.zeros(n, bool), ambiguous=np.zeros(n, bool),
               illcond=np.zeros(n, bool), d=d)
    for lo in range(0, n, 2048):
        dd = d[lo:lo + 2048]
        T = dd @ cc.T
        q = cc[None, :, :] - dd[:, None, :] * T[:, :, None]
        dist = (q * q).sum(2)
        del q
        hit = dist < r2
        X = np.sqrt(np.maximum(r2 - dist, 0.0))
        t0 = T - X
        ins = t0 < EPS
        t = np.where(ins, T + X, t0)
        tt = np.where(hit & (t > EPS), t, np.inf)
        win = tt.argmin(1)
        rows = np.arange(len(dd))
        tw = tt[rows, win]
        found = np.isfinite(tw)
        two = np.partition(tt, 1, axis=1)[:, :2] if tt.shape[1] > 1 else np.concatenate([tt, np.full_like(tt, np.inf)], 1)
        second = np.where(np.isfinite(two[:, 1]), two[:, 1], 0.0)
        close = np.isfinite(two[:, 1]) & (second - two[:, 0] <= 1e-4 * two[:, 0])
        graze = (np.abs(dist / r2 - 1.0) < 1e-4) & (T + X > EPS) & (T - X < tw[:, None])
        near_eps = hit & ((np.abs(t0 - EPS) < 1e-5) | (np.abs(T + X - EPS) < 1e-5))
        sl = slice(lo, lo + len(dd))
        out["win"][sl] = np.where(found, win, -1)
        out["t"][sl] = tw
        out["inside"][sl] = found & ins[rows, win]
        out["ambiguous"][sl] = close | graze.any(1) | near_eps.any(1)
        out["illcond"][sl] = found & (dist[rows, win] / r2[win] > 1.0 - 1e-3)
    wi = np.maximum(out["win"], 0)
    tf = np.where(np.isfinite(out["t"]), out["t"], 0.0)
    out["n_out"] = (cp + d * tf[:, None] - s[wi]) / r[wi][:, None]
    out["cr"] = np.sqrt(cc2[wi]) + r[wi]
    out["r"] = r[wi]
    return out


def reference_error(orc, inp, f, pixels):
    """max |t_f32 - t_f64| / (|C| + r) over `pixels`: the f64 direction rounded to f32 and the camera position
    through the oracle's own f32 group test (or_group_test)."""
    L = orc.lib()
    o32 = np.ascontiguousarray(inp.camf[0:3], np.float32)
    dist4, t4 = np.zeros(4, np.float32), np.zeros(4, np.float32)
    worst = 0.0
    for p in pixels:
        d32 = np.ascontiguousarray(f["d"][p], np.float32)
        g = np.ascontiguousarray(inp.o.groups[f["win"][p] // 4])
        L.or_group_test(o32.ctypes.data, d32.ctypes.data, g.ctypes.data, dist4.ctypes.data, t4.ctypes.data)
        worst = max(worst, abs(float(t4[f["win"][p] % 4]) - f["t"][p]) / f["cr"][p])
    return worst


def check_planes_against_f64(rt, orc, inp, planes, f, simd, label, check_t=True):
    """check_t False: an input whose ill-conditioned winners break the cap (the module's docstring): no T and
    Normal tolerance check, and the cap holds for its ambiguous pixels."""
    hit, normal, albedo = planes
    n = inp.w * inp.h
    key, t_gpu = hit[:, 0], hit[:, 1].view(np.float32).astype(np.float64)
    decided = ~f["ambiguous"]
    checked_t = decided & ~f["illcond"] & (f["win"] >= 0)
    left_out = int((f["ambiguous"] | (f["illcond"] & (f["win"] >= 0) & check_t)).sum())
    assert left_out <= 0.005 * n, f"{label}: {left_out} of {n} pixels ambiguous or ill-conditioned (cap 0.5 %)"
    got = np.where(key == rt.HIT_MISS, -1, (key & ~np.uint32(rt.HIT_INSIDE)).astype(np.int64))
    bad = np.flatnonzero(decided & (got != f["win"]))
    assert bad.size == 0, f"{label}: {bad.size} decided pixels see another sphere than f64, first {bad[0]}"
    miss, hitp = decided & (f["win"] < 0), decided & (f["win"] >= 0)
    assert np.all(key[miss] == rt.HIT_MISS) and np.all(hit[miss, 1] == np.float32(1e30).view(np.uint32))
    assert np.all(normal[miss] == 0) and np.all(albedo[miss] == 0)
    # Albedo: the winner's Color bit for bit, w = 1
    color = np.ascontiguousarray(inp.o.spheres[:, 8:11]).view(np.uint32)
    assert np.array_equal(albedo[hitp, :3], color[f["win"][hitp]]), f"{label}: Albedo is not the winner's Color"
    assert np.all(albedo[hitp, 3] == np.float32(1.0).view(np.uint32))
    flag = ((key & np.uint32(rt.HIT_INSIDE)) != 0) & (key != rt.HIT_MISS)  # (RT_HIT_MISS has every bit set)
    if not simd:  # the scalar rules' flag is the winner's own
        assert np.array_equal(flag[hitp], f["inside"][hitp]), f"{label}: RT_HIT_INSIDE differs from T - X < eps"
    # Normal is the reference's Normalize of HitNormal = D T - C, whose length is the winner's radius: zero where
    # len^2 <= 1e-4 (x64_math.h:234-245), a unit vector else.  A winner whose r^2 is within 1e-3 of that threshold
    # (far more than T's limit moves len^2) is held to neither.
    r2w = f["r"] ** 2
    tiny, unit = hitp & (r2w < 1e-4 * (1 - 1e-3)), hitp & (r2w > 1e-4 * (1 + 1e-3))
    assert int((hitp & ~tiny & ~unit).sum()) <= 0.005 * n
    assert np.all(normal[tiny] == 0), f"{label}: Normal of a sphere with r^2 <= 1e-4 is not Normalize's zero"
    checked_n = checked_t & unit
    # |Normal| = 1 (l2 carries 2.5 ulp at most, the square root and each quotient half an ulp: below 4 * 2^-23),
    # w = 0, and it points against the outward normal exactly where the flag is set
    nv = normal[:, :3].view(np.float32).astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(nv[unit], axis=1) - 1.0) <= 4 * 2.0 ** -23) and np.all(normal[hitp, 3] == 0)
    against = (nv * f["n_out"]).sum(1) < 0
    assert np.array_equal(against[checked_n], flag[checked_n]), f"{label}: Normal's side differs from the flag"
    if not check_t:
        return flag, hitp
    # T and Normal within 4 times the reference's own error
    px = np.flatnonzero(checked_t)
    ref = reference_error(orc, inp, f, px)
    limit = 4.0 * ref
    err_t = np.abs(t_gpu[px] - f["t"][px]) / f["cr"][px]
    pn = np.flatnonzero(checked_n)
    n64 = np.where(flag[pn, None], -f["n_out"][pn], f["n_out"][pn])
    err_n = np.linalg.norm(nv[pn] - n64, axis=1)
    lim_n = limit * f["cr"][pn] / f["r"][pn] + 4 * 2.0 ** -23
    print(f"{label}: {px.size} pixels checked, {left_out} left out; reference error {ref:.3e}, limit {limit:.3e}, "
          f"GPU T error {err_t.max():.3e}; Normal error / its limit at worst {float((err_n / lim_n).max()):.3f}")
    assert err_t.max() <= limit, f"{label}: T error {err_t.max():.3e} above 4 x the reference's {ref:.3e}"
    assert np.all(err_n <= lim_n), f"{label}: Normal error above dT / r + 4 * 2^-23 at {int((err_n > lim_n).sum())} pixels"
    return flag, hitp


@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
@pytest.mark.parametrize("name", [BASE, "s0_72x40", "s2_136x104", INSIDE, INSIDE_MANY, "r2_outside"])
def test_centre_planes_against_f64(rt, orc, torch_cuda, inputs, fdev, name, simd):
    inp = inputs(name)
    f = first_hit_f64(inp.camf, inp.o.spheres, inp.w, inp.h)
    planes = first_hit(fdev.use(inp), torch_cuda, inp, simd=simd, centre=True).words()
    flag, hitp = check_planes_against_f64(rt, orc, inp, planes, f, simd, f"{name} {'simd' if simd else 'scalar'} centre",
                                          check_t=name != "s2_136x104")
    if simd and name not in (INSIDE, INSIDE_MANY):  # an outside camera: no candidate ever has T - X < eps
        assert not flag.any(), f"{name}: RT_HIT_INSIDE set on {int(flag.sum())} pixels of an outside camera"
    if simd and name in (INSIDE, INSIDE_MANY):  # sticky per class, so checked only where the winner encloses the camera
        s = inp.o.spheres.astype(np.float64)
        encl = np.linalg.norm(s[:, 0:3] - inp.camf[0:3].astype(np.float64), axis=1) < s[:, 4]
        seen = hitp & encl[np.maximum(f["win"], 0)]
        assert seen.any() and flag[seen].all(), "RT_HIT_INSIDE missing where the enclosing sphere wins"


# ------------------------------------------------- 6. the jittered planes belong to the jittered ray
def test_jittered_t_belongs_to_the_jittered_ray(rt, orc, torch_cuda, inputs, fdev):
    inp = inputs("s0_72x40")
    w, h, k = inp.w, inp.h, 3
    L = orc.lib()
    jx, jy = np.zeros(w * h), np.zeros(w * h)
    for y in range(h):
        for x in range(w):
            st = ctypes.c_uint64(rt.pixel_seed(x, y, k, w, h))
            jx[y * w + x] = L.or_random_float(ctypes.byref(st), -0.5, 0.5)
            jy[y * w + x] = L.or_random_float(ctypes.byref(st), -0.5, 0.5)
    assert np.abs(jx).max() > 0.4 and np.abs(jy).max() > 0.4
    f = first_hit_f64(inp.camf, inp.o.spheres, w, h, jx, jy)
    for simd in (True, False):
        planes = first_hit(fdev.use(inp), torch_cuda, inp, frame=k, simd=simd).words()
        check_planes_against_f64(rt, orc, inp, planes, f, simd, f"s0_72x40 {'simd' if simd else 'scalar'} frame 3")
    # and not to the centre ray: against the centre's f64 depths the same plane is far outside the limit
    fc = first_hit_f64(inp.camf, inp.o.spheres, w, h)
    both = (f["win"] >= 0) & (fc["win"] == f["win"]) & ~f["ambiguous"] & ~fc["ambiguous"]
    t_gpu = planes[0][:, 1].view(np.float32).astype(np.float64)
    assert (np.abs(t_gpu[both] - fc["t"][both]) / fc["cr"][both]).max() > 1e-3


# ------------------------------------------------- 7. the centre flag is not parsed and ignored
def test_centre_differs_from_frame_0(rt, torch_cuda, inputs, fdev):
    inp = inputs(BASE)
    dev = fdev.use(inp)
    for simd in (True, False):
        jit = first_hit(dev, torch_cuda, inp, frame=0, simd=simd).words()[0][:, 0]
        cen = first_hit(dev, torch_cuda, inp, frame=0, simd=simd, centre=True).words()[0][:, 0]
        differ = int((jit != cen).sum())
        assert 1 <= differ < 0.1 * jit.size, differ
        # centre mode reads no frame index
        assert np.array_equal(cen, first_hit(dev, torch_cuda, inp, frame=7, simd=simd, centre=True).words()[0][:, 0])


# ------------------------------------------------- refusals through the binding (CPU-side return codes)
def test_refusals_with_a_device(rt, torch_cuda, inputs):
    inp = inputs("s1p3_72x40")
    L = rt.lib()
    pl = Planes(torch_cuda, inp.w, inp.h)
    hit, normal, albedo = pl.hit.data_ptr(), pl.normal.data_ptr(), pl.albedo.data_ptr()
    dev = rt.Device(0)
    try:
        def call(*, handle=dev.handle, cam=inp.cam, desc=None, tiles=None, n_tiles=0, flags=0, planes="default", **kw):
            d = rt.RtTraceDesc(inp.w, inp.h, 0, 0, 0, 1, rt.RT_SEED_PIXEL, 0, 1, 0, 0)
            for k, v in kw.items():
                setattr(d, k, v)
            p = rt.RtFirstHitPlanes(32, hit, normal, albedo) if planes == "default" else planes
            arr = (ctypes.c_uint32 * max(len(tiles), 1))(*tiles) if tiles is not None else None
            return L.rt_trace_first_hit(handle, ctypes.byref(cam) if cam is not None else None,
                                        None if desc == "null" else ctypes.byref(d), arr, n_tiles, flags,
                                        ctypes.byref(p) if p is not None else None, None)

        assert call() == EINVAL and b"no scene uploaded" in L.rt_last_error()  # before any upload
        dev.upload_scene(inp.s)
        assert call() == 0  # (the rsqrt table is the built-in one here; the pass does not need it either way)
        assert call(handle=None) == EINVAL
        assert call(cam=None) == EINVAL and call(desc="null") == EINVAL and call(planes=None) == EINVAL
        assert call(planes=rt.RtFirstHitPlanes(24, hit, normal, albedo)) == EINVAL and b"Size" in L.rt_last_error()
        assert call(planes=rt.RtFirstHitPlanes(32, None, None, None)) == EINVAL and b"every plane" in L.rt_last_error()
        assert call(planes=rt.RtFirstHitPlanes(32, hit + 4, None, None)) == EINVAL and b"8-byte" in L.rt_last_error()
        assert call(planes=rt.RtFirstHitPlanes(32, None, normal + 8, None)) == EINVAL and b"16-byte" in L.rt_last_error()
        assert call(planes=rt.RtFirstHitPlanes(32, None, None, albedo + 8)) == EINVAL and b"16-byte" in L.rt_last_error()
        assert call(flags=2) == EINVAL and b"flags" in L.rt_last_error()
        assert call(SeedMode=0) == EINVAL and b"RT_SEED_PIXEL" in L.rt_last_error()
        assert call(BandCount=2) == EINVAL and call(BandIndex=1) == EINVAL and call(BandCount=0) == 0
        assert call(Width=0) == EINVAL and call(Height=65537) == EINVAL and b"bad image size" in L.rt_last_error()
        n = rt.tile_count(inp.w, inp.h)
        assert call(tiles=None, n_tiles=2) == EINVAL and b"tiles is NULL" in L.rt_last_error()
        assert call(tiles=[0, n], n_tiles=2) == EINVAL and b"the image has" in L.rt_last_error()
        assert call(tiles=[1, 1], n_tiles=2) == EINVAL and b"listed twice" in L.rt_last_error()
        assert call(tiles=[0], n_tiles=0) == 0  # a list of none: nothing to do
        # Frames, MaxBounce and Flags of the descriptor are not read
        assert call(Frames=0xFFFFFFFF, PreviousRayCount=0xFFFFFFFF, MaxBounce=0, Flags=0xFFFFFFFF) == 0
        torch_cuda.cuda.synchronize()
    finally:
        dev.close()
