"""GPU parity of the cluster walk's own-sphere rule ("the sphere a ray leaves"): a lane
leaves the sphere its ray starts on out of its own member flags when it has proven that it cannot
accept it (tests/test_own_sphere_skip.py checks the proof's claim on the CPU).  Every case is bit-exact
against the oracle: running mean, RGBA8 and ray count."""
import numpy as np
import pytest

import random_scenes
from test_gpu_parity import assert_same, gpu_render
from test_gpu_tile_work import Images, Oracle, assert_work, launch

pytestmark = pytest.mark.gpu

F = np.float32
ON, OFF = 1, -1
W, H, SPP, B = 96, 64, 4, 8


def _c2(rt, orc, n=64):
    return rt.scene_prefix(rt.scene_builtin(1), n), orc.scene_builtin(1).prefix(n)


def _check(rt, orc, torch, dev, s, o, w, h, spp, bounces, simd, distance=None):
    g = gpu_render(rt, torch, dev, s, rt.camera_setup(s, w, h, distance=distance), w, h, frames=spp, bounces=bounces,
                   simd=simd)
    r = orc.render(o, orc.camera(o, w, h, distance=distance), w, h, frames=spp, max_bounce=bounces, simd=simd)
    assert_same(*g, *r)
    return dev.last_info()


@pytest.fixture(scope="module")
def odev(rt, torch_cuda):
    dev = rt.Device(0)
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def c2_oracle(rt, orc):
    """The first case's oracle frames per rule set, rendered once and shared read-only."""
    s, o = _c2(rt, orc)
    out = {}
    for simd in (True, False):
        r = orc.render(o, orc.camera(o, W, H), W, H, frames=SPP, max_bounce=B, simd=simd)
        r[0].setflags(write=False)
        r[1].setflags(write=False)
        out[simd] = r
    return s, o, out


@pytest.mark.parametrize("simd", [True, False])
def test_c2_scene(rt, torch_cuda, odev, c2_oracle, simd):
    s, _, ref = c2_oracle
    assert np.all(np.isfinite(rt.scene_own_sphere(s, simd))), "the rule is on for every sphere of this scene"
    g = gpu_render(rt, torch_cuda, odev, s, rt.camera_setup(s, W, H), W, H, frames=SPP, bounces=B, simd=simd)
    assert_same(*g, *ref[simd])
    info = odev.last_info()
    assert info["ClusteredWalk"] == 1 and info["Walk"] == 2, info  # kWalkCl1


@pytest.mark.parametrize("distance", [1.0, 200.0])
def test_c2_scene_from_inside_the_cloud_and_from_afar(rt, orc, torch_cuda, odev, distance):
    s, o = _c2(rt, orc)
    _check(rt, orc, torch_cuda, odev, s, o, W, H, SPP, B, True, distance)


def test_rgb_glass(rt, orc, torch_cuda, odev):
    """Dielectrics: rays that continue inside the sphere they hit, and leave it from inside."""
    _check(rt, orc, torch_cuda, odev, rt.scene_builtin(0), orc.scene_builtin(0), 64, 48, 8, 5, True)


@pytest.mark.parametrize("simd", [True, False])
def test_rule_off_beside_live_spheres(rt, orc, torch_cuda, odev, simd):
    """16 spheres, one of radius 50 and four of radius 1e-3 (outside the rule's radius range: rho = +inf)
    beside ordinary ones."""
    sp = rt.scene_arrays(rt.scene_prefix(rt.scene_builtin(1), 16))[0].copy()
    ref = rt.scene_builtin(1)
    look = (float(ref.LookAt.x), float(ref.LookAt.y), float(ref.LookAt.z))
    sp[0, 0:3] = (look[0], look[1] - 52.0, look[2])
    sp[0, 4] = 50.0
    sp[5:9, 4] = 1e-3
    s, o = random_scenes.build(rt, orc, sp, True, look, float(ref.DefaultDistanceFromLookAt), float(ref.DefaultXAngle),
                               float(ref.DefaultYHeight))
    rho = rt.scene_own_sphere(s, simd)
    assert np.isposinf(rho[0]) and np.all(np.isposinf(rho[5:9]))
    _check(rt, orc, torch_cuda, odev, s, o, 64, 48, 4, 8, simd)


@pytest.mark.parametrize("simd", [True, False])
def test_rule_off_for_one_sphere_of_a_scene_wide_table(rt, orc, torch_cuda, odev, simd):
    """(The scene above takes per-lane tables, where the rule is off throughout.)  32 spheres, one of
    radius 1e-3 and in view: the table stays scene-wide and that one sphere alone has rho = +inf."""
    sp = rt.scene_arrays(rt.scene_prefix(rt.scene_builtin(1), 32))[0].copy()
    ref = rt.scene_builtin(1)
    look = (float(ref.LookAt.x), float(ref.LookAt.y), float(ref.LookAt.z))
    sp[6, 4] = 1e-3
    s, o = random_scenes.build(rt, orc, sp, True, look, float(ref.DefaultDistanceFromLookAt), float(ref.DefaultXAngle),
                               float(ref.DefaultYHeight))
    rho = rt.scene_own_sphere(s, simd)
    assert np.isposinf(rho[6]) and np.all(np.isfinite(np.delete(rho, 6)))
    info = _check(rt, orc, torch_cuda, odev, s, o, 64, 48, 4, 8, simd)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == 2, info


def test_two_word_walk(rt, orc, torch_cuda, odev):
    s, o = _c2(rt, orc, 256)
    info = _check(rt, orc, torch_cuda, odev, s, o, 64, 48, 2, 16, True)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == 3, info  # kWalkCl2


@pytest.mark.parametrize("options", [{"OneWaveGroups": OFF, "Clusters": ON}, {"WalkAny": ON, "Clusters": ON},
                                     {"LanesPerPixel": 16, "Clusters": ON}],
                         ids=["four_wave", "walk_any", "lanes16"])
def test_every_unit_that_holds_the_rule(rt, torch_cuda, c2_oracle, options):
    """The first case through the four-wave kernels, the run-time kernel and the P = 16 unit."""
    s, _, ref = c2_oracle
    dev = rt.Device(0, options=options)
    try:
        g = gpu_render(rt, torch_cuda, dev, s, rt.camera_setup(s, W, H), W, H, frames=SPP, bounces=B, simd=True)
        assert_same(*g, *ref[True])
        info = dev.last_info()
        assert info["ClusteredWalk"] == 1, info
        if "WalkAny" in options or "OneWaveGroups" in options:
            assert info["Walk"] == 0, info
        if "LanesPerPixel" in options:
            assert info["LanesPerPixel"] == 16, info
    finally:
        dev.close()


def test_per_tile_counts_unit(rt, orc, torch_cuda):
    """The first case through rt_trace_tile_work with two different counts (one per tile row)."""
    s, o = _c2(rt, orc)
    cam, ocam = rt.camera_setup(s, W, H), orc.camera(o, W, H)
    mean = np.random.default_rng(7).uniform(0.25, 2.0, (W * H, 4)).astype(F)
    pairs = [(0, 4), (3, 6)]
    work = {t: pairs[t // 3] for t in range(6)}  # 3 x 2 reference tiles
    dev = rt.Device(0)
    try:
        dev.upload_scene(s)
        img = Images(torch_cuda, W, H, mean)
        launch(dev, torch_cuda, cam, work, img, bounces=B)
        rays = assert_work(img, Oracle(orc, o, ocam, W, H, mean, B).expected(work), "own sphere")
        want = sum(orc.render(o, ocam, W, H, prev_count=p, frames=f, max_bounce=B, prev=mean.copy(),
                              rows=(32 * r, 32 * r + 32))[2] for r, (p, f) in enumerate(pairs))
        assert rays == want
        assert dev.last_info()["TileCounts"] == 1
    finally:
        dev.close()
