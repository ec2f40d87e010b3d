"""GPU parity of the expanded prefilter ("the expanded prefilter"): the scene-wide
walk-specialised kernels test cluster and member pairs in 7 packed FMAs on the recentred table
(tests/test_expanded_prefilter.py checks the skip proof on the CPU).  Every case is bit-exact against
the oracle -- running mean, RGBA8 and ray count -- and asserts the walk the launch reports."""
import numpy as np
import pytest

import random_scenes
from test_expanded_prefilter import translated
from test_gpu_parity import assert_same, gpu_render
from test_gpu_tile_work import Images, Oracle, assert_work, launch

pytestmark = pytest.mark.gpu

F = np.float32
ON = 1
CL1, CL2, CL4 = 2, 3, 4  # rt_kernel.h kWalkCl1 / kWalkCl2 / kWalkCl4
W, H, SPP, B = 128, 96, 8, 8


def _c2(rt, orc, n=64):
    return rt.scene_prefix(rt.scene_builtin(1), n), orc.scene_builtin(1).prefix(n)


def _check(rt, orc, torch, dev, s, o, w, h, spp, bounces, simd):
    g = gpu_render(rt, torch, dev, s, rt.camera_setup(s, w, h), w, h, frames=spp, bounces=bounces, simd=simd)
    r = orc.render(o, orc.camera(o, w, h), w, h, frames=spp, max_bounce=bounces, simd=simd)
    assert_same(*g, *r)
    return dev.last_info()


@pytest.fixture(scope="module")
def xdev(rt, torch_cuda):
    dev = rt.Device(0)
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def c2_oracle(rt, orc):
    """The 64-sphere case's oracle frames per rule set, rendered once and shared read-only."""
    s, o = _c2(rt, orc)
    out = {}
    for simd in (True, False):
        r = orc.render(o, orc.camera(o, W, H), W, H, frames=SPP, max_bounce=B, simd=simd)
        r[0].setflags(write=False)
        r[1].setflags(write=False)
        out[simd] = r
    return s, o, out


@pytest.mark.parametrize("simd", [True, False])
def test_one_word_walk(rt, torch_cuda, xdev, c2_oracle, simd):
    s, _, ref = c2_oracle
    assert rt.scene_clusters_expanded(s, simd)[2]
    g = gpu_render(rt, torch_cuda, xdev, s, rt.camera_setup(s, W, H), W, H, frames=SPP, bounces=B, simd=simd)
    assert_same(*g, *ref[simd])
    info = xdev.last_info()
    assert info["ClusteredWalk"] == 1 and info["Walk"] == CL1, info


def test_two_word_walk(rt, orc, torch_cuda, xdev):
    s, o = _c2(rt, orc, 256)
    info = _check(rt, orc, torch_cuda, xdev, s, o, 64, 48, 4, 16, True)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == CL2, info


def four_word_scene(rt, orc):
    """More than 64 groups under a scene-wide table: random_scenes.make draws no such scene (its large
    scenes all take per-lane thresholds), so this builds one through random_scenes.build from the 256
    Floating Spheres and 44 of them again, moved up by 2.5."""
    ref = rt.scene_builtin(1)
    sp = rt.scene_arrays(ref)[0]
    more = sp[:44].copy()
    more[:, 1] += F(2.5)
    look = (float(ref.LookAt.x), float(ref.LookAt.y), float(ref.LookAt.z))
    return random_scenes.build(rt, orc, np.concatenate([sp, more]), False, look, float(ref.DefaultDistanceFromLookAt),
                               float(ref.DefaultXAngle), float(ref.DefaultYHeight))


def test_four_word_walk(rt, orc, torch_cuda, xdev):
    s, o = four_word_scene(rt, orc)
    assert s.SIMDSpheres.Count > 64 and rt.scene_clusters_expanded(s, True)[2]
    info = _check(rt, orc, torch_cuda, xdev, s, o, 64, 48, 4, 8, True)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == CL4, info


@pytest.mark.parametrize("lanes", [8, 16])
def test_lanes_per_pixel(rt, torch_cuda, c2_oracle, lanes):
    s, _, ref = c2_oracle
    dev = rt.Device(0, options={"LanesPerPixel": lanes, "Clusters": ON})
    try:
        g = gpu_render(rt, torch_cuda, dev, s, rt.camera_setup(s, W, H), W, H, frames=SPP, bounces=B, simd=True)
        assert_same(*g, *ref[True])
        info = dev.last_info()
        assert info["LanesPerPixel"] == lanes and info["Walk"] == CL1, info
    finally:
        dev.close()


def test_per_tile_counts(rt, orc, torch_cuda):
    """One rt_trace_tile_work call over two tiles at different (PreviousRayCount, Frames)."""
    s, o = _c2(rt, orc)
    w, h = 64, 32
    cam, ocam = rt.camera_setup(s, w, h), orc.camera(o, w, h)
    mean = np.random.default_rng(13).uniform(0.25, 2.0, (w * h, 4)).astype(F)
    work = {0: (0, 4), 1: (3, 6)}
    dev = rt.Device(0)
    try:
        dev.upload_scene(s)
        img = Images(torch_cuda, w, h, mean)
        launch(dev, torch_cuda, cam, work, img, bounces=B)
        assert_work(img, Oracle(orc, o, ocam, w, h, mean, B).expected(work), "expanded prefilter")
        info = dev.last_info()
        assert info["TileCounts"] == 1 and info["Walk"] == CL1, info
    finally:
        dev.close()


@pytest.mark.parametrize("simd", [True, False])
def test_scene_far_from_its_origin_runs_the_run_time_kernel(rt, orc, torch_cuda, xdev, simd):
    s = translated(rt, _c2(rt, orc)[0], 1e4)
    assert not rt.scene_clusters_expanded(s, simd)[2]
    sp = rt.scene_arrays(s)[0]
    ref = rt.scene_builtin(1)
    look = (float(ref.LookAt.x) + 1e4, float(ref.LookAt.y), float(ref.LookAt.z))
    s, o = random_scenes.build(rt, orc, sp, False, look, float(ref.DefaultDistanceFromLookAt), float(ref.DefaultXAngle),
                               float(ref.DefaultYHeight))
    info = _check(rt, orc, torch_cuda, xdev, s, o, 64, 48, 4, 8, simd)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == 0, info
