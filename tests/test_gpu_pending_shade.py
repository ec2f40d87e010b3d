"""GPU parity of the pending shade: a lane whose segment hit keeps the hit and shades it at
the start of its next round (a secondary round, or a merged round beside lanes starting
samples), and a hit at the bounce limit adds its emission term alone.  The cases are the
bounce limits at which each of these paths is the only one or the last one taken, hand-built
scenes whose last-bounce emission is visible in the frame, mixed materials in one wave,
merged rounds, the sky right after a shade, pixel-slot advance, the brute-force routing and
invalid lanes beside lanes carrying hits.  Every case is bit-exact against the oracle:
running mean, RGBA8 and ray count."""
import numpy as np
import pytest

import random_scenes
from test_gpu_parity import assert_same, gpu_render

pytestmark = pytest.mark.gpu

F = np.float32
OFF = -1
BRUTE = {"Cull": OFF, "Prefilter": OFF}


@pytest.fixture(scope="module")
def devices(rt, torch_cuda):
    """Devices by option set, opened on first use and closed with the module."""
    opened = {}

    def get(options):
        key = tuple(sorted(options.items()))
        if key not in opened:
            opened[key] = rt.Device(0, options=options)
        return opened[key]

    yield get
    for dev in opened.values():
        dev.close()


@pytest.fixture(params=["lanes4", "auto"])
def lanes(request):
    """lanes4: four lanes per pixel at every frame count (the walk-specialised kernels' shape);
    auto: the host's own choice (2 spp: two lanes per pixel, the run-time kernel)."""
    return {"LanesPerPixel": 4} if request.param == "lanes4" else {}


_oracle_frames = {}


def _oracle(orc, key, o, W, H, **kw):
    """The oracle's (mean, RGBA8, rays) of a case, rendered once and shared by the device variants."""
    if key not in _oracle_frames:
        r = orc.render(o, orc.camera(o, W, H), W, H, **kw)
        for a in r[:2]:
            a.setflags(write=False)
        _oracle_frames[key] = r
    return _oracle_frames[key]


def _check(rt, orc, torch, dev, key, s, o, W, H, spp, B, simd):
    g = gpu_render(rt, torch, dev, s, rt.camera_setup(s, W, H), W, H, frames=spp, bounces=B, simd=simd)
    r = _oracle(orc, (key, W, H, spp, B, simd), o, W, H, frames=spp, max_bounce=B, simd=simd)
    assert_same(*g, *r)
    return r


def _builtin(rt, orc, index, n):
    return rt.scene_prefix(rt.scene_builtin(index), n), orc.scene_builtin(index).prefix(n)


def _sphere(pos, radius, color, ior=0.0, specular=0.0, emissive=(0.0, 0.0, 0.0)):
    row = np.zeros(20, F)
    row[0:3] = pos
    row[4] = radius
    row[8:11] = color   # Material: Color(4) Emissive(4) Specular IOR pad pad
    row[12:15] = emissive
    row[16], row[17] = specular, ior
    return row


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("spp", [2, 4])
@pytest.mark.parametrize("B", [1, 2, 3, 8])
def test_bounce_limits(rt, orc, torch_cuda, devices, lanes, B, spp, simd):
    """B = 1: every hit takes the emission-only path and no shade runs.  B = 2: a primary hit is
    shaded at the start of a secondary round whose own hit is at the limit.  B = 3: a secondary
    hit is carried into another secondary round.  B = 8: the headline's limit."""
    s, o = _builtin(rt, orc, 1, 64)
    _check(rt, orc, torch_cuda, devices(lanes), "floating64", s, o, 32, 32, spp, B, simd)


def _lit_scene(rt, orc):
    """A red diffuse sphere below an emissive grey one, a green diffuse one beside them (paths of
    three hits that end on the light) and fillers that make it a scene of split rounds.  No sky:
    all light is emission, attenuated by the colours of the hits before it."""
    spheres = np.array([
        _sphere((0.0, 0.0, 0.0), 1.0, (0.8, 0.3, 0.2)),
        _sphere((0.0, 2.2, 0.0), 1.0, (0.6, 0.6, 0.9), emissive=(4.0, 3.0, 2.0)),
        _sphere((0.3, 1.0, 2.1), 0.9, (0.2, 0.9, 0.4)),
        *[_sphere((-3.0 - i, -1.5, 2.0 - i), 0.4, (0.3, 0.5 + 0.05 * i, 0.7)) for i in range(6)],
    ], F)
    return random_scenes.build(rt, orc, spheres, False, (0.0, 1.1, 0.0), 3.5, 0.3, 0.5)


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("B", [2, 3])
def test_emission_at_the_bounce_limit_with_attenuation(rt, orc, torch_cuda, devices, lanes, B, simd):
    """Hits at the limit that reach the emissive sphere through coloured diffuse ones: the
    emission-only term must use the attenuation the earlier shades left.  The oracle's frame
    at B differs from its frame at B - 1 only through such hits, so the case exercises them."""
    s, o = _lit_scene(rt, orc)
    W = H = 16
    r = _check(rt, orc, torch_cuda, devices(lanes), "lit", s, o, W, H, 4, B, simd)
    below = _oracle(orc, ("lit", W, H, 4, B - 1, simd), o, W, H, frames=4, max_bounce=B - 1, simd=simd)
    lit = np.any(r[0].reshape(-1, 4)[:, :3] != below[0].reshape(-1, 4)[:, :3], axis=1)
    assert lit.any(), f"no pixel gains light at hit {B}"
    # (and the light arrives attenuated: not the emissive sphere's own (4, 3, 2) ratio on every such pixel)
    gain = (r[0].reshape(-1, 4) - below[0].reshape(-1, 4))[lit][:, :3]
    assert np.any(np.abs(gain[:, 0] * 3.0 - gain[:, 1] * 4.0) > 1e-3 * np.abs(gain[:, 0]))


@pytest.mark.parametrize("simd", [True, False])
def test_glass_in_front_of_diffuse_spheres(rt, orc, torch_cuda, devices, lanes, simd):
    """The camera outside a glass sphere with diffuse, specular and emissive spheres behind and
    beside it: dielectric and diffuse shades in the same round of a wave."""
    spheres = np.array([
        _sphere((0.0, 0.0, 0.0), 1.0, (1.0, 1.0, 1.0), ior=1.5),
        _sphere((-2.5, 0.0, -0.8), 0.9, (0.9, 0.2, 0.2)),
        _sphere((-2.0, 1.4, 0.6), 0.6, (0.2, 0.8, 0.3), specular=0.7),
        _sphere((-1.8, -1.2, -1.6), 0.7, (0.3, 0.3, 0.9), emissive=(1.0, 2.0, 0.5)),
        _sphere((0.4, 1.5, -1.0), 0.5, (0.8, 0.8, 0.1)),
        _sphere((0.2, -1.4, 1.2), 0.5, (0.6, 0.2, 0.7)),
        *[_sphere((-4.0 - i, 0.5 * i - 1.0, 1.5 - i), 0.5, (0.3, 0.5 + 0.05 * i, 0.7)) for i in range(4)],
    ], F)
    s, o = random_scenes.build(rt, orc, spheres, True, (0.0, 0.0, 0.0), 4.0, 0.3, 0.5)
    _check(rt, orc, torch_cuda, devices(lanes), "glass_front", s, o, 16, 16, 4, 8, simd)


def _with_glass(rt, orc, n):
    """The first n Floating Spheres from the scene's own camera, the one nearest the camera made
    of glass and the farthest one emissive, under the sky (without them most of the frame is black)."""
    ref = rt.scene_builtin(1)
    look = (float(ref.LookAt.x), float(ref.LookAt.y), float(ref.LookAt.z))
    dist, ang, yh = float(ref.DefaultDistanceFromLookAt), float(ref.DefaultXAngle), float(ref.DefaultYHeight)
    spheres = rt.scene_arrays(ref)[0][:n].copy()
    gap = np.linalg.norm(spheres[:, 0:3] - random_scenes._camera_pos(look, dist, ang, yh), axis=1) - spheres[:, 4]
    spheres[int(np.argmin(gap)), 17] = 1.5
    spheres[int(np.argmax(gap)), 12:15] = (3.0, 2.0, 1.0)
    return random_scenes.build(rt, orc, spheres, True, look, dist, ang, yh)


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("n", [5, 8])
def test_merged_rounds(rt, orc, torch_cuda, devices, lanes, n, B, simd):
    """Scenes of one and two groups trace every round merged: lanes shading a pending hit and
    lanes starting a sample in the same round."""
    s, o = _with_glass(rt, orc, n)
    _check(rt, orc, torch_cuda, devices(lanes), f"glass{n}", s, o, 32, 32, 2, B, simd)


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("B", [1, 3])
def test_sky_after_a_pending_shade(rt, orc, torch_cuda, devices, lanes, B, simd):
    """The first 64 RTWeekend spheres: segments that miss right after their shade take the sky
    term with the shaded attenuation and direction."""
    s, o = _builtin(rt, orc, 2, 64)
    assert o.use_sky
    _check(rt, orc, torch_cuda, devices(lanes), "rtw64", s, o, 32, 32, 2, B, simd)


@pytest.mark.parametrize("simd", [True, False])
def test_one_frame_per_launch_carries_no_hit_to_the_next_pixel(rt, orc, torch_cuda, devices, lanes, simd):
    """frames = 1 on a running mean (the host's own choice gives each lane four pixel slots):
    a lane that completes a pixel moves to its next slot with no pending hit.  Then a second
    launch continues the mean."""
    torch = torch_cuda
    s, o = _builtin(rt, orc, 1, 64)
    W, H, B = 64, 48, 5
    dev = devices(lanes)
    cam, ocam = rt.camera_setup(s, W, H), orc.camera(o, W, H)
    mean = np.random.default_rng(9).uniform(0.0, 2.0, (W * H, 4)).astype(F)
    prev = torch.from_numpy(mean.copy()).to("cuda")
    omean = mean
    for count in (7, 8):
        g = gpu_render(rt, torch, dev, s, cam, W, H, frames=1, bounces=B, simd=simd, prev_count=count, prev=prev)
        if not lanes:
            assert dev.last_info()["PixelsPerLane"] == 4, dev.last_info()
        key = ("floating64_mean", count, simd)
        if key not in _oracle_frames:
            _oracle_frames[key] = orc.render(o, ocam, W, H, prev_count=count, frames=1, max_bounce=B, simd=simd,
                                             prev=omean.copy())
        r = _oracle_frames[key]
        assert_same(*g, *r)
        prev, omean = g[0], r[0].reshape(-1, 4)


@pytest.mark.parametrize("simd", [True, False])
def test_brute_force_routing(rt, orc, torch_cuda, devices, lanes, simd):
    """No cull pass and no prefilter: every round runs the exact all-groups loop."""
    s, o = _builtin(rt, orc, 1, 64)
    _check(rt, orc, torch_cuda, devices({**BRUTE, **lanes}), "floating64", s, o, 32, 32, 2, 2, simd)


@pytest.mark.parametrize("simd", [True, False])
def test_image_edge_inside_a_wave_tile(rt, orc, torch_cuda, devices, lanes, simd):
    """36 x 20: wave tiles cut by the right and the bottom edge, lanes outside the image beside
    lanes carrying hits."""
    s, o = _builtin(rt, orc, 1, 64)
    _check(rt, orc, torch_cuda, devices(lanes), "floating64", s, o, 36, 20, 4, 8, simd)
