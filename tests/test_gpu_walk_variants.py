"""GPU parity of every secondary-walk variant the trace kernel compiles: the
one-, two- and four-word cluster walks (one scalar load per table entry, the
one-word mask merge), the table's edge sizes, the run-time kernel that keeps
the IEEE candidate square root, and the candidate acceptance rules (ties and
the sticky inside flag).  Every case is bit-exact against the oracle: running
mean, RGBA8 and ray count."""
import numpy as np
import pytest

import random_scenes
from test_gpu_parity import assert_same, gpu_render

pytestmark = pytest.mark.gpu

F = np.float32
# rt_kernel.h kWalk*: the walk compiled into the launched kernel (rt_trace_info.Walk)
WALK_ANY, WALK_CL1, WALK_CL2, WALK_CL4_REL = 0, 2, 3, 7


@pytest.fixture(scope="module")
def wdev(rt, torch_cuda):
    dev = rt.Device(0)
    yield dev
    dev.close()


def _builtin(rt, orc, index, n=None):
    s, o = rt.scene_builtin(index), orc.scene_builtin(index)
    if n is not None:
        s, o = rt.scene_prefix(s, n), o.prefix(n)
    return s, o


def _check(rt, orc, torch, dev, s, o, W, H, spp, B, simd, distance=None):
    cam = rt.camera_setup(s, W, H, distance=distance)
    g = gpu_render(rt, torch, dev, s, cam, W, H, frames=spp, bounces=B, simd=simd)
    r = orc.render(o, orc.camera(o, W, H, distance=distance), W, H, frames=spp, max_bounce=B, simd=simd)
    assert_same(*g, *r)
    return dev.last_info()


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("distance", [None, 1.0])
def test_one_word_table(rt, orc, torch_cuda, wdev, simd, distance):
    """64 spheres (16 groups, one mask word), from the default camera and from inside the
    cloud (distance 1.0: members of several clusters are flagged in one round)."""
    s, o = _builtin(rt, orc, 1, 64)
    info = _check(rt, orc, torch_cuda, wdev, s, o, 64, 48, 4, 8, simd, distance)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == WALK_CL1, info


def test_two_word_table(rt, orc, torch_cuda, wdev):
    s, o = _builtin(rt, orc, 1, 256)
    info = _check(rt, orc, torch_cuda, wdev, s, o, 32, 32, 2, 16, True)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == WALK_CL2, info


def test_four_word_per_lane_table(rt, orc, torch_cuda, wdev):
    s, o = _builtin(rt, orc, 2)  # RTWeekend: 482 spheres, sky
    info = _check(rt, orc, torch_cuda, wdev, s, o, 32, 32, 2, 8, True)
    assert info["ClusteredWalk"] == 1 and info["Walk"] == WALK_CL4_REL, info


@pytest.mark.parametrize("simd", [True, False])
@pytest.mark.parametrize("n", [5, 9, 33])
def test_table_edges(rt, orc, torch_cuda, wdev, n, simd):
    """One- and two-group scenes (merged rounds), an odd cluster count whose last pair
    entry carries a padding cluster, and the first size past eight groups."""
    s, o = _builtin(rt, orc, 1, n)
    _check(rt, orc, torch_cuda, wdev, s, o, 32, 32, 2, 8, simd)


def _sphere(pos, radius, color, ior=0.0, specular=0.0):
    row = np.zeros(20, F)
    row[0:3] = pos
    row[4] = radius
    row[8:11] = color   # Material: Color(4) Emissive(4) Specular IOR pad pad
    row[16], row[17] = specular, ior
    return row


@pytest.mark.parametrize("simd", [True, False])
def test_ieee_sqrt_kernel(rt, orc, torch_cuda, wdev, simd):
    """A sphere of radius 1e-7 (r^2 = 1e-14, below 2^-36) beside normal ones and in view: the
    host clears the short-sqrt flag and launches the run-time kernel, whose candidate
    sites keep the IEEE square root."""
    base = rt.scene_arrays(rt.scene_builtin(1))[0][:11]
    look = (float(rt.scene_builtin(1).LookAt.x), float(rt.scene_builtin(1).LookAt.y), float(rt.scene_builtin(1).LookAt.z))
    tiny = _sphere(look, 1e-7, (0.9, 0.2, 0.2))
    spheres = np.concatenate([base, tiny[None, :]])
    ref = rt.scene_builtin(1)
    s, o = random_scenes.build(rt, orc, spheres, True, look, float(ref.DefaultDistanceFromLookAt),
                               float(ref.DefaultXAngle), float(ref.DefaultYHeight))
    assert rt.scene_prefilter(s, simd)[2] & 2 == 0, "the scene must leave the short sqrt's proven range"
    assert rt.scene_prefilter(rt.scene_prefix(rt.scene_builtin(1), 11), simd)[2] & 2, "(and only the tiny sphere does it)"
    info = _check(rt, orc, torch_cuda, wdev, s, o, 32, 32, 2, 8, simd)
    assert info["Walk"] == WALK_ANY, info


def _fillers():
    return [_sphere((3.0 + i, -2.0, 4.0 - i), 0.4, (0.3, 0.5 + 0.05 * i, 0.7)) for i in range(3)]


@pytest.mark.parametrize("simd", [True, False])
def test_tie_between_identical_spheres(rt, orc, torch_cuda, wdev, simd):
    """Spheres 0 and 4 are identical (the same lane of groups 0 and 1) with different
    colours: the SIMD rules keep the earlier group on a tie (strict <), the scalar
    rules take the later sphere (<=)."""
    a = _sphere((0.0, 0.0, 0.0), 1.0, (0.9, 0.1, 0.1))
    b = _sphere((0.0, 0.0, 0.0), 1.0, (0.1, 0.9, 0.1))
    spheres = np.array([a, *_fillers(), b, *_fillers()], F)
    s, o = random_scenes.build(rt, orc, spheres, True, (0.0, 0.0, 0.0), 4.0, 0.3, 0.5)
    _check(rt, orc, torch_cuda, wdev, s, o, 16, 16, 4, 4, simd)


@pytest.mark.parametrize("simd", [True, False])
def test_sticky_inside_flag(rt, orc, torch_cuda, wdev, simd):
    """The camera sits inside glass sphere 0; sphere 4 (the same lane, the next group)
    lies in front of it and a further one beyond: the nearer hit supersedes the inside
    candidate, whose bit stays set under the SIMD rules (sticky OR) and not under the
    scalar ones."""
    glass = _sphere((0.0, 0.0, 0.0), 2.0, (1.0, 1.0, 1.0), ior=1.5)
    near = _sphere((0.0, 0.0, 0.0), 0.3, (0.2, 0.4, 0.9))
    far = _sphere((-3.5, 0.0, 0.0), 0.8, (0.9, 0.8, 0.2))
    spheres = np.array([glass, *_fillers(), near, *_fillers(), far], F)
    s, o = random_scenes.build(rt, orc, spheres, True, (0.0, 0.0, 0.0), 1.0, 0.0, 0.0)
    _check(rt, orc, torch_cuda, wdev, s, o, 16, 16, 4, 4, simd)
