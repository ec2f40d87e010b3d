"""GPU parity of the direction walk ("the direction table"): the one-word scene-wide
walk-specialised kernels choose their member entries by a per-sphere direction table
(tests/test_direction_table.py checks the table's claim on the CPU).  Every case is bit-exact against the
oracle -- running mean, RGBA8 and ray count -- with the table on and off, and asserts what
rt_trace_last_direction_table reports: 1 where the launch fact holds, 0 where it does not."""
import itertools

import numpy as np
import pytest

import random_scenes
import test_gpu_tile_work as tw
import test_gpu_tiles as tt
from test_expanded_prefilter import translated
from test_gpu_parity import assert_same, gpu_render

pytestmark = pytest.mark.gpu

F = np.float32
ON, OFF = 1, -1
CL1 = 2  # rt_kernel.h kWalkCl1: the walk the launch reports with and without the table
W, H, SPP, B = 128, 96, 8, 8


@pytest.fixture(scope="module")
def floating(rt, orc):
    """Floating Spheres prefixes and their oracle frames per rule set, rendered once and shared read-only."""
    cache = {}

    def get(n, simd):
        if (n, simd) not in cache:
            s, o = rt.scene_prefix(rt.scene_builtin(1), n), orc.scene_builtin(1).prefix(n)
            r = orc.render(o, orc.camera(o, W, H), W, H, frames=SPP, max_bounce=B, simd=simd)
            r[0].setflags(write=False)
            r[1].setflags(write=False)
            cache[(n, simd)] = (s, r)
        return cache[(n, simd)]

    return get


def render_with(rt, torch, s, options, simd, ref, w=W, h=H, spp=SPP, bounces=B):
    dev = rt.Device(0, options=options)
    try:
        g = gpu_render(rt, torch, dev, s, rt.camera_setup(s, w, h), w, h, frames=spp, bounces=bounces, simd=simd)
        assert_same(*g, *ref)
        return dev.last_info()
    finally:
        dev.close()


@pytest.mark.parametrize("lanes", [4, 8, 16])
@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("n", [16, 33, 64, 128])
def test_table_on_and_off_give_the_oracle_bits(rt, torch_cuda, floating, n, simd, lanes):
    s, ref = floating(n, simd)
    assert rt.scene_direction_table(s, simd)[0] is not None
    on = render_with(rt, torch_cuda, s, {"LanesPerPixel": lanes, "DirectionTable": ON}, simd, ref)
    assert on["DirectionTable"] == 1 and on["Walk"] == CL1 and on["ClusteredWalk"] == 1 and on["LanesPerPixel"] == lanes, on
    off = render_with(rt, torch_cuda, s, {"LanesPerPixel": lanes, "DirectionTable": OFF}, simd, ref)
    assert off["DirectionTable"] == 0 and off["Walk"] == CL1 and off["ClusteredWalk"] == 1, off
    # the default: the direction walk up to 8 lanes per pixel; the 16-lane shape (the 8-rank band share's, measured
    # slower with it) takes it only when asked
    dflt = render_with(rt, torch_cuda, s, {"LanesPerPixel": lanes}, simd, ref)
    assert dflt["DirectionTable"] == (1 if lanes <= 8 else 0) and dflt["Walk"] == CL1, dflt


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("options", [{"WalkAny": ON}, {"Cull": OFF}], ids=["walk_any", "cull_off"])
def test_without_the_fact_the_old_walk_runs(rt, torch_cuda, floating, options, simd):
    s, ref = floating(64, simd)
    info = render_with(rt, torch_cuda, s, options, simd, ref)
    assert info["DirectionTable"] == 0 and info["ClusteredWalk"] == 1, info


@pytest.mark.parametrize("simd", [True, False])
def test_two_word_scene_has_no_direction_walk(rt, orc, torch_cuda, simd):
    """132 spheres, 33 whole groups: two mask words.  (At 129 spheres -- a ragged 33rd group -- the two-word kernels'
    ray count under the SIMD rules is 1 short of the oracle's 17,488 with both images equal, with the parent commit's
    library as with this one: not this walk's, and recorded in DESIGN_HISTORY.)"""
    s, o = rt.scene_prefix(rt.scene_builtin(1), 132), orc.scene_builtin(1).prefix(132)
    assert rt.scene_direction_table(s, simd)[0] is None
    ref = orc.render(o, orc.camera(o, 64, 48), 64, 48, frames=4, max_bounce=B, simd=simd)
    info = render_with(rt, torch_cuda, s, None, simd, ref, 64, 48, 4)
    assert info["DirectionTable"] == 0 and info["Walk"] == 3, info  # kWalkCl2


@pytest.mark.parametrize("simd", [True, False])
def test_scene_far_from_its_origin_keeps_the_run_time_kernel(rt, orc, torch_cuda, simd):
    far = translated(rt, rt.scene_prefix(rt.scene_builtin(1), 64), 1e4)
    assert rt.scene_direction_table(far, simd)[0] is None
    ref_scene = rt.scene_builtin(1)
    look = (float(ref_scene.LookAt.x) + 1e4, float(ref_scene.LookAt.y), float(ref_scene.LookAt.z))
    s, o = random_scenes.build(rt, orc, rt.scene_arrays(far)[0], False, look, float(ref_scene.DefaultDistanceFromLookAt),
                               float(ref_scene.DefaultXAngle), float(ref_scene.DefaultYHeight))
    ref = orc.render(o, orc.camera(o, 64, 48), 64, 48, frames=4, max_bounce=B, simd=simd)
    info = render_with(rt, torch_cuda, s, None, simd, ref, 64, 48, 4)
    assert info["DirectionTable"] == 0 and info["Walk"] == 0, info


@pytest.mark.parametrize("camera", [0, 1], ids=["outside", "inside"])
def test_adversarial_scene_with_dielectrics(rt, orc, torch_cuda, camera):
    """Seed 4015 of the generator: 50 spheres (13 groups) under a one-word scene-wide table, some of them
    dielectric, so paths continue inside spheres; seen from outside the cloud and from inside its largest sphere."""
    spec = random_scenes.make(4015, n_max=300)
    sp = spec["spheres"]
    assert len(sp) > 8 and np.count_nonzero(sp[:, 17]) >= 3
    look, dist, ang, yh, _ = spec["cameras"][camera]
    s, o = random_scenes.build(rt, orc, sp, spec["use_sky"], look, dist, ang, yh)
    for simd in (True, False):
        assert rt.scene_direction_table(s, simd)[0] is not None
        ref = orc.render(o, orc.camera(o, 96, 64), 96, 64, frames=6, max_bounce=B, simd=simd)
        info = render_with(rt, torch_cuda, s, None, simd, ref, 96, 64, 6)
        assert info["DirectionTable"] == 1, info


def test_reflections_on_cell_borders(rt, orc, torch_cuda):
    """A mirror sphere at the origin with small spheres along the 26 axis, edge and corner directions of the
    direction grid's cube: the rays the mirror sends to them run along face centres, face edges and corners,
    where components tie and cells meet."""
    rows = [np.zeros(20, F)]
    rows[0][4] = 1.0
    rows[0][8:11] = 0.9
    rows[0][16] = 1.0  # Specular
    for k, v in enumerate(itertools.product((-1.0, 0.0, 1.0), repeat=3)):
        if not any(v):
            continue
        r = np.zeros(20, F)
        r[0:3] = 2.5 * np.array(v) / np.linalg.norm(v)
        r[4] = 0.3
        r[8:11] = (0.3 + 0.05 * (k % 7), 0.9 - 0.07 * (k % 5), 0.5)
        r[12:15] = 1.5 if k % 3 == 0 else 0.0  # (a third of them emit, so the image is not black without a sky)
        rows.append(r)
    s, o = random_scenes.build(rt, orc, np.array(rows, F), True, (0.0, 0.0, 0.0), 6.0, 0.7, 1.0)
    for simd in (True, False):
        assert rt.scene_direction_table(s, simd)[0] is not None
        ref = orc.render(o, orc.camera(o, 96, 64), 96, 64, frames=6, max_bounce=B, simd=simd)
        info = render_with(rt, torch_cuda, s, None, simd, ref, 96, 64, 6)
        assert info["DirectionTable"] == 1, info


def test_per_tile_counts(rt, orc, torch_cuda):
    """One rt_trace_tile_work call over two tiles at different (PreviousRayCount, Frames)."""
    s, o = rt.scene_prefix(rt.scene_builtin(1), 64), orc.scene_builtin(1).prefix(64)
    w, h = 64, 32
    cam, ocam = rt.camera_setup(s, w, h), orc.camera(o, w, h)
    mean = np.random.default_rng(13).uniform(0.25, 2.0, (w * h, 4)).astype(F)
    work = {0: (0, 4), 1: (3, 6)}
    dev = rt.Device(0)
    try:
        dev.upload_scene(s)
        img = tw.Images(torch_cuda, w, h, mean)
        tw.launch(dev, torch_cuda, cam, work, img, bounces=B)
        tw.assert_work(img, tw.Oracle(orc, o, ocam, w, h, mean, B).expected(work), "direction walk")
        info = dev.last_info()
        assert info["TileCounts"] == 1 and info["DirectionTable"] == 1 and info["Walk"] == CL1, info
    finally:
        dev.close()


def test_tile_list(rt, orc, torch_cuda):
    """One rt_trace_tiles call over three of the twelve tiles of the 128 x 96 frame."""
    s, o = rt.scene_prefix(rt.scene_builtin(1), 64), orc.scene_builtin(1).prefix(64)
    oprev, ocur, _ = orc.render(o, orc.camera(o, W, H), W, H, frames=SPP, max_bounce=B)
    dev = rt.Device(0)
    try:
        dev.upload_scene(s)
        img = tt.Images(torch_cuda, W, H)
        tiles = [1, 5, 6]
        tt.launch(dev, torch_cuda, rt.camera_setup(s, W, H), tiles, img, frames=SPP, bounces=B)
        tt.assert_tiles(img, tiles, oprev, ocur)
        assert dev.last_info()["DirectionTable"] == 1
    finally:
        dev.close()
