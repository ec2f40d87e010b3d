"""Frames from inside one huge sphere: the scenes that take the kernel's math layer to the edges of its ranges
(tests/test_gpu_math_layer.py traces them on the GPU), and, here on the CPU, the oracle held to the reference's
own compiled code at those radii.

The scene is the 16-sphere prefix of Floating Spheres whose last sphere becomes a diffuse, emissive sphere
centred on the look-at point, so the camera is inside it and every path ends on it or bounces off it.  Its
radius R is 2^29, 2^31, 2^45, 2^62, 2^63.5 or float32(2^63.99): r^2 = 2^58 keeps the host's short-sqrt proof
(r^2 <= 2^60, rt_pack.cpp sqrt_range_ok), every larger one clears it; the hit normal's |N|^2 ~ r^2 runs from
inside sqrt_rn's stated range [2^-60, 2^60] to the top of f32, and its length from below to far above the
2^40 at which normalize leaves its short division.

test_oracle_matches_patched_reference_inside_huge_sphere renders the twelve frames (six radii, both rule sets)
through the reference's RenderTile / RenderTileScalar in pixel-seed mode (the `refpix` fixture) and compares
running mean, RGBA8 and ray count with the oracle bit for bit: the oracle stays the truth the GPU is held to.
It skips where the compiled reference is absent."""
import numpy as np
import pytest

import random_scenes
from conftest import host_is_intel

F = np.float32
W, H, FRAMES, B = 48, 32, 4, 8
N_PREFIX = 16
RADII = {"2^29": F(2.0 ** 29), "2^31": F(2.0 ** 31), "2^45": F(2.0 ** 45), "2^62": F(2.0 ** 62),
         "2^63.5": F(2.0 ** 63.5), "2^63.99": F(2.0 ** 63.99)}
COLOR, EMISSIVE = (0.75, 0.5, 0.25), (0.5, 0.75, 1.0)


def huge_sphere_scene(rt, orc, radius):
    """(rt scene, oracle scene): Floating Spheres' first 16 spheres, the last one replaced (docstring)."""
    base = rt.scene_prefix(rt.scene_builtin(1), N_PREFIX)
    spheres, _, _ = rt.scene_arrays(base)
    look = (base.LookAt.x, base.LookAt.y, base.LookAt.z)
    row = np.zeros(20, F)
    row[0:3] = look
    row[4] = radius
    row[8:11] = COLOR
    row[12:15] = EMISSIVE   # Specular (16) and IOR (17) stay 0: diffuse
    spheres[N_PREFIX - 1] = row
    return random_scenes.build(rt, orc, spheres, bool(base.UseSkyColor), look, base.DefaultDistanceFromLookAt,
                               base.DefaultXAngle, base.DefaultYHeight)


def oracle_frame(orc, o, simd):
    """The oracle's frame, and the two facts that let it be compared bit for bit with no NaN rule and no pixel
    left out: every value finite, no pixel all zero; and some path bounced."""
    prev, cur, rays = orc.render(o, orc.camera(o, W, H), W, H, frames=FRAMES, max_bounce=B, simd=simd)
    assert np.isfinite(prev).all(), f"{np.count_nonzero(~np.isfinite(prev))} NaN or inf values in the oracle's frame"
    assert np.all(np.any(prev[:, :3] != 0, axis=1)), "an all-zero pixel in the oracle's frame"
    assert rays > W * H * FRAMES, "no path bounced"
    prev.setflags(write=False)
    cur.setflags(write=False)
    return prev, cur, rays


@pytest.mark.skipif(not host_is_intel(), reason="the oracle's rsqrtss table is Intel's")
@pytest.mark.parametrize("simd", [True, False], ids=["RenderTile", "RenderTileScalar"])
@pytest.mark.parametrize("radius", list(RADII), ids=list(RADII))
def test_oracle_matches_patched_reference_inside_huge_sphere(rt, orc, refpix, radius, simd):
    _, o = huge_sphere_scene(rt, orc, RADII[radius])
    cam = orc.camera(o, W, H)
    oprev, ocur, orays = oracle_frame(orc, o, simd)
    prev = np.zeros((W * H, 4), F)
    cur = np.zeros(W * H, np.uint32)
    rays = np.zeros(1, np.uint64)
    state = np.zeros(1, np.uint64)
    refpix.ref_set_patch(B, 1)
    try:
        refpix.ref_render(o.spheres.ctypes.data, len(o.spheres), o.groups.ctypes.data, len(o.groups),
                          o.materials.ctypes.data, len(o.materials), int(o.use_sky), cam.ctypes.data, W, H, 0, FRAMES,
                          int(simd), state.ctypes.data, prev.ctypes.data, cur.ctypes.data, rays.ctypes.data)
    finally:
        refpix.ref_set_patch(5, 0)
    assert int(rays[0]) == orays, (int(rays[0]), orays)
    bad = np.flatnonzero(np.any(prev.view(np.uint32) != oprev.view(np.uint32), axis=1))
    assert bad.size == 0, (len(bad), bad[:5], oprev[bad[:3]], prev[bad[:3]])
    assert np.array_equal(cur, ocur)
