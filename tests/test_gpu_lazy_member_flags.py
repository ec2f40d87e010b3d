"""GPU parity of the cluster walk's lazy member flags (the clusters item): a member-pair entry
takes its behind and own-sphere compares and its mask merge only where some lane is near one of its two
spheres.  Every scene-wide walk, which holds the branch -- one, two and four mask words -- and the per-lane
walk beside it, whose loop has no such branch, through the walk-specialised kernels and the run-time kernel
(Walk 0), under both rule sets, bit-exact against the oracle: running mean, RGBA8 and ray count.  The
Floating Spheres camera stands at distance 1.0, inside the cloud: origins lie inside and beside spheres, so
the behind rule and the own-sphere rule both fire.

Mask words follow the group count (rt_kernel.h: one word up to 32 groups, two up to 64, else four), so of the
Floating Spheres prefixes 16, 64 and 100 spheres walk one word and 256 two; the four-word scene-wide walk is
the 264-sphere cloud (the 256 and eight shifted copies), RTWeekend's 121 groups the four-word per-lane one."""
import numpy as np
import pytest

import random_scenes
from test_gpu_parity import assert_same, gpu_render

pytestmark = pytest.mark.gpu

ON = 1
W, H, SPP, B = 64, 32, 8, 8
# walk kernels (rt_kernel.h kWalk*): the run-time kernel, then one / two / four words, scene-wide and per-lane
ANY, CL1, CL2, CL4, CL4REL = 0, 2, 3, 4, 7
# adversarial scenes (tests/random_scenes.py: seed, camera) whose table is scene-wide under both rule sets:
# 36 spheres seen from outside (one word), 243 spheres seen from inside the largest one (two words)
SCENE_WIDE = ((9, 0), (6, 1))

# name -> (builder, the walk kernel of its table under either rule set)
CASES = {
    "fs16": (lambda rt, orc: _floating(rt, orc, 16), CL1),
    "fs64": (lambda rt, orc: _floating(rt, orc, 64), CL1),
    "fs100": (lambda rt, orc: _floating(rt, orc, 100), CL1),
    "fs256": (lambda rt, orc: _floating(rt, orc, 256), CL2),
    "fs264": (lambda rt, orc: _floating_and_copies(rt, orc), CL4),
    "rtweekend": (lambda rt, orc: _builtin(rt, orc, 2), CL4REL),
    "random_a": (lambda rt, orc: _random(rt, orc, *SCENE_WIDE[0]), CL1),
    "random_b": (lambda rt, orc: _random(rt, orc, *SCENE_WIDE[1]), CL2),
}


def _floating(rt, orc, n):
    s, o = rt.scene_prefix(rt.scene_builtin(1), n), orc.scene_builtin(1).prefix(n)
    return s, o, rt.camera_setup(s, W, H, distance=1.0), orc.camera(o, W, H, distance=1.0)


def _floating_and_copies(rt, orc):
    """Floating Spheres and eight of them again, shifted: 66 groups, a four-word table that stays scene-wide."""
    ref = rt.scene_builtin(1)
    sp = rt.scene_arrays(ref)[0].copy()
    extra = sp[:8].copy()
    extra[:, 0:3] += np.float32(0.37)
    look = (float(ref.LookAt.x), float(ref.LookAt.y), float(ref.LookAt.z))
    s, o = random_scenes.build(rt, orc, np.concatenate([sp, extra]), True, look, float(ref.DefaultDistanceFromLookAt),
                               float(ref.DefaultXAngle), float(ref.DefaultYHeight))
    return s, o, rt.camera_setup(s, W, H, distance=1.0), orc.camera(o, W, H, distance=1.0)


def _builtin(rt, orc, index):
    s, o = rt.scene_builtin(index), orc.scene_builtin(index)
    return s, o, rt.camera_setup(s, W, H), orc.camera(o, W, H)


def _random(rt, orc, seed, camera):
    spec = random_scenes.make(seed)
    look, dist, ang, yh, _ = spec["cameras"][camera]
    s, o = random_scenes.build(rt, orc, spec["spheres"], spec["use_sky"], look, dist, ang, yh)
    return s, o, rt.camera_setup(s, W, H), orc.camera(o, W, H)


@pytest.fixture(scope="module")
def devices(rt, torch_cuda):
    """The default routing (a walk-specialised kernel per table) and the run-time kernel forced."""
    devs = {"walk": rt.Device(0), "any": rt.Device(0, options={"WalkAny": ON, "Clusters": ON})}
    yield devs
    for d in devs.values():
        d.close()


_frames = {}


def _reference(rt, orc, name, simd):
    """A case's scene, cameras and oracle frames, rendered once and shared read-only by both kernels."""
    if (name, simd) not in _frames:
        s, o, cam, ocam = CASES[name][0](rt, orc)
        ref = orc.render(o, ocam, W, H, frames=SPP, max_bounce=B, simd=simd)
        ref[0].setflags(write=False)
        ref[1].setflags(write=False)
        _frames[(name, simd)] = (s, cam, ref)
    return _frames[(name, simd)]


@pytest.mark.parametrize("kernel", ["walk", "any"])
@pytest.mark.parametrize("simd", [True, False], ids=["simd", "scalar"])
@pytest.mark.parametrize("name", list(CASES))
def test_lazy_member_flags_match_oracle(rt, orc, torch_cuda, devices, name, simd, kernel):
    s, cam, ref = _reference(rt, orc, name, simd)
    assert rt.scene_clusters(s, simd)[1] > 0, "the case walks a cluster table"
    per_lane = bool((rt.scene_prefilter(s, simd)[2] >> 2) & 1)
    assert per_lane == (name == "rtweekend"), "every table but RTWeekend's is scene-wide"
    dev = devices[kernel]
    g = gpu_render(rt, torch_cuda, dev, s, cam, W, H, frames=SPP, bounces=B, simd=simd)
    assert_same(*g, *ref)
    info = dev.last_info()
    assert info["ClusteredWalk"] == 1, info
    assert info["Walk"] == (ANY if kernel == "any" else CASES[name][1]), info
