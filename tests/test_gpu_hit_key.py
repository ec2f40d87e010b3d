"""GPU parity of the per-class hit key, and of the sample seeds at the far end of the frame index.

A lane keeps, per residue class of the sphere index, the nearest hit's t and one key
(4 g + L) | inside << 31 (csrc/rtk_walk.h Hit); the hit select takes the minimum of the four t and the
key of the lowest class that holds it, and that key is the word a pending hit carries.  The cases are
the ones in which a wrong key shows in the frame:
- the sticky inside flag of the SIMD rules (main.cpp:425): a class whose earlier candidate was hit from
  inside keeps the flag when a nearer sphere of the class replaces it, so exchanging two spheres of
  one class changes the frame under the SIMD rules and not under the scalar ones;
- a tie between two classes: two identical spheres with different emission, where the lower class
  wins under the SIMD rules and the later sphere under the scalar ones;
and each runs through the default routing, the run-time kernel, 1, 4 and 16 lanes per pixel and the
four-wave kernels.  The seed cases put the frame index next to 2^32 and give the tiles of one launch
different counts.  Every comparison is bit for bit with the oracle: v4 mean, RGBA8 and ray count."""
import numpy as np
import pytest

import random_scenes
from test_gpu_parity import assert_same, gpu_render
from test_gpu_tile_work import Images, Oracle, assert_work, launch

pytestmark = pytest.mark.gpu

F = np.float32
OFF, ON = -1, 1
W, H, SPP, B = 96, 54, 4, 3
VARIANTS = {
    "default": {},
    "run_time_kernel": {"WalkAny": ON},
    "lanes1": {"LanesPerPixel": 1},
    "lanes4": {"LanesPerPixel": 4},
    "lanes16": {"LanesPerPixel": 16},
    "four_wave": {"OneWaveGroups": OFF},
}
# what rt_trace_last_info must say of a launch of each variant: a case routed to another kernel fails
ROUTED = {
    "default": lambda i: i["OneWaveGroups"] == 1,
    "run_time_kernel": lambda i: i["OneWaveGroups"] == 1 and i["Walk"] == 0,
    "lanes1": lambda i: i["LanesPerPixel"] == 1 and i["PixelsPerLane"] == 1,
    "lanes4": lambda i: i["LanesPerPixel"] == 4,
    "lanes16": lambda i: i["LanesPerPixel"] == 16,
    "four_wave": lambda i: i["OneWaveGroups"] == 0,
}


@pytest.fixture(scope="module")
def devices(rt, torch_cuda):
    """Devices by variant, opened on first use and closed with the module."""
    opened = {}

    def get(name):
        if name not in opened:
            opened[name] = rt.Device(0, options=VARIANTS[name])
        return opened[name]

    yield get
    for dev in opened.values():
        dev.close()


def _floating(rt, n):
    """The first n Floating Spheres and the scene's own camera parameters."""
    ref = rt.scene_builtin(1)
    look = (float(ref.LookAt.x), float(ref.LookAt.y), float(ref.LookAt.z))
    view = (look, float(ref.DefaultDistanceFromLookAt), float(ref.DefaultXAngle), float(ref.DefaultYHeight))
    return rt.scene_arrays(ref)[0][:n].copy(), view


def sticky_spheres(rt, n, exchanged):
    """The first n Floating Spheres with an r = 50 sphere centred on the look-at point in slot 0: the
    camera is inside it, so its candidate sets class 0's inside flag on every ray.  It is emissive (the
    scene has no sky: the paths that leave the cloud end on it and carry light back).  exchanged: slots 0
    and 4 (class 0 of groups 0 and 1) trade places."""
    sp, view = _floating(rt, n)
    sp[0, 0:3] = view[0]
    sp[0, 4] = 50.0
    sp[0, 12:15] = (1.0, 0.9, 0.8)
    if exchanged:
        sp[[0, 4]] = sp[[4, 0]]
    return sp, view


def tie_spheres(rt, n, exchanged):
    """The first n Floating Spheres with slot 2 moved onto slot 1 (same centre, same radius) and the two
    given different emission.  exchanged: the two trade materials."""
    sp, view = _floating(rt, n)
    sp[2, 0:8] = sp[1, 0:8]
    sp[1, 12:15] = (4.0, 1.0, 0.25)
    sp[2, 12:15] = (0.25, 1.0, 4.0)
    if exchanged:
        sp[[1, 2], 8:20] = sp[[2, 1], 8:20]
    return sp, view


SCENES = {
    "sticky8": lambda rt, x: sticky_spheres(rt, 8, x),     # two groups: merged rounds, the exact loop
    "sticky64": lambda rt, x: sticky_spheres(rt, 64, x),   # sixteen groups: split rounds, a cluster walk
    "tie12": lambda rt, x: tie_spheres(rt, 12, x),
    "tie64": lambda rt, x: tie_spheres(rt, 64, x),
}

_built = {}
_frames = {}


def _scene(rt, orc, name, exchanged):
    key = (name, exchanged)
    if key not in _built:
        sp, (look, dist, ang, yh) = SCENES[name](rt, exchanged)
        _built[key] = random_scenes.build(rt, orc, sp, False, look, dist, ang, yh)
    return _built[key]


def _oracle(rt, orc, name, exchanged, simd):
    """The oracle's (mean, RGBA8, rays) of a case, rendered once, read-only, shared by the variants."""
    key = (name, exchanged, simd)
    if key not in _frames:
        o = _scene(rt, orc, name, exchanged)[1]
        r = orc.render(o, orc.camera(o, W, H), W, H, frames=SPP, max_bounce=B, simd=simd)
        for a in r[:2]:
            a.setflags(write=False)
        _frames[key] = r
    return _frames[key]


def _differing(a, b):
    return int(np.any(a[0].reshape(-1, 4).view(np.uint32) != b[0].reshape(-1, 4).view(np.uint32), axis=1).sum())


@pytest.mark.parametrize("name", ["sticky8", "sticky64"])
def test_oracle_sticky_flag_shows_under_simd_rules_only(rt, orc, name):
    """What makes the sticky scenes a test of the key's bit 31: with slots 0 and 4 exchanged the big
    sphere's inside flag is set after the class's nearer candidate instead of before it, which the SIMD
    rules' OR keeps and the scalar rules never see."""
    n_simd = _differing(_oracle(rt, orc, name, False, True), _oracle(rt, orc, name, True, True))
    n_scalar = _differing(_oracle(rt, orc, name, False, False), _oracle(rt, orc, name, True, False))
    print(name, "pixels that differ: SIMD rules", n_simd, "scalar rules", n_scalar, "of", W * H)
    assert n_simd > 0 and n_scalar == 0


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("name", ["tie12", "tie64"])
def test_oracle_tie_shows_in_the_frame(rt, orc, name, simd):
    """Exchanging the materials of the two coincident spheres changes the frame: the tie is seen."""
    n = _differing(_oracle(rt, orc, name, False, simd), _oracle(rt, orc, name, True, simd))
    print(name, "simd", simd, "pixels that differ", n, "of", W * H)
    assert n > 0


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("exchanged", [False, True])
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_hit_key_matches_oracle(rt, orc, torch_cuda, devices, variant, name, exchanged, simd):
    s = _scene(rt, orc, name, exchanged)[0]
    g = gpu_render(rt, torch_cuda, devices(variant), s, rt.camera_setup(s, W, H), W, H, frames=SPP, bounces=B,
                   simd=simd)
    info = devices(variant).last_info()
    assert ROUTED[variant](info), (variant, info)
    print(variant, name, "walk", info["Walk"], "clustered", info["ClusteredWalk"], "lanes", info["LanesPerPixel"])
    assert_same(*g, *_oracle(rt, orc, name, exchanged, simd))


# ------------------------------------------------------------------ seeds
SW, SH, SPREV = 33, 5, 4294967000
SMEAN = np.random.default_rng(33).uniform(0.25, 2.0, (SW * SH, 4)).astype(F)
SMEAN.setflags(write=False)


@pytest.fixture(scope="module")
def seed_scene(rt, orc):
    s, o = rt.scene_prefix(rt.scene_builtin(1), 64), orc.scene_builtin(1).prefix(64)
    return s, o


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_seeds_next_to_the_last_frame_index(rt, orc, torch_cuda, devices, seed_scene, variant, simd):
    """33 x 5, frames 4,294,967,000 ... 4,294,967,003 on a running mean: the seed index
    (frame H + y) W + x (main.cpp:668) lies above 2^39, its product with the seed multiplier wraps 2^64
    many times over, and the width is no multiple of 64 (the mixer's shifts read the index modulo 64)."""
    s, o = seed_scene
    prev = torch_cuda.from_numpy(SMEAN.copy()).to("cuda")
    g = gpu_render(rt, torch_cuda, devices(variant), s, rt.camera_setup(s, SW, SH), SW, SH, frames=4, bounces=B,
                   simd=simd, prev_count=SPREV, prev=prev)
    assert ROUTED[variant](devices(variant).last_info()), (variant, devices(variant).last_info())
    key = ("seed", simd)
    if key not in _frames:
        _frames[key] = orc.render(o, orc.camera(o, SW, SH), SW, SH, prev_count=SPREV, frames=4, max_bounce=B, simd=simd,
                                  prev=SMEAN.copy())
    assert_same(*g, *_frames[key])


@pytest.mark.parametrize("simd", [True, False])
def test_seeds_of_tiles_with_their_own_counts(rt, orc, torch_cuda, seed_scene, simd):
    """One rt_trace_tile_work launch over the image's two reference tiles (32 and 1 pixels wide), each
    with its own (PreviousRayCount, Frames): a wave's frame index comes from its tile's pair.  The
    oracle counts rays per image, not per tile, so the launch runs a second time with the pairs
    exchanged: the two launches together trace each pair over the whole image once."""
    s, o = seed_scene
    pairs = [(SPREV, 4), (7, 3)]
    oracle = Oracle(orc, o, orc.camera(o, SW, SH), SW, SH, SMEAN, B)
    dev = rt.Device(0)
    rays = []
    try:
        dev.upload_scene(s)
        for work in ({0: pairs[0], 1: pairs[1]}, {0: pairs[1], 1: pairs[0]}):
            img = Images(torch_cuda, SW, SH, SMEAN)
            launch(dev, torch_cuda, rt.camera_setup(s, SW, SH), work, img, bounces=B, simd=simd)
            rays.append(assert_work(img, oracle.expected(work, simd=simd), f"pairs {work}"))
            assert dev.last_info()["TileCounts"] == 1
    finally:
        dev.close()
    want = [oracle.render(p, simd)[2] for p in pairs]
    print("rays", rays, "oracle, whole image per pair", want)
    assert sum(rays) == sum(want)


@pytest.mark.parametrize("simd", [True, False])
def test_seeds_with_four_pixels_per_lane(rt, orc, torch_cuda, seed_scene, simd):
    """One frame per launch, four pixel slots per lane: a lane seeds each slot's sample from that slot's
    own pixel, and carries no hit key over from the slot before.  A lane's four slots are the four 8 x 8
    quadrants of a 16 x 16 block tile and a lane moves on only when its pixel is complete, so the case takes
    one frame (the shape the host itself picks only at one frame) at 96 x 54, where whole block tiles and
    tiles cut by both edges occur; 33 x 5 has no row in a tile's lower quadrants."""
    s, o = seed_scene
    dev = rt.Device(0, options={"LanesPerPixel": 1, "PixelsPerLane": 4})
    try:
        mean = np.random.default_rng(4).uniform(0.25, 2.0, (W * H, 4)).astype(F)
        prev = torch_cuda.from_numpy(mean.copy()).to("cuda")
        g = gpu_render(rt, torch_cuda, dev, s, rt.camera_setup(s, W, H), W, H, frames=1, bounces=B, simd=simd,
                       prev_count=SPREV, prev=prev)
        assert dev.last_info()["PixelsPerLane"] == 4, dev.last_info()
    finally:
        dev.close()
    r = orc.render(o, orc.camera(o, W, H), W, H, prev_count=SPREV, frames=1, max_bounce=B, simd=simd, prev=mean.copy())
    assert_same(*g, *r)
