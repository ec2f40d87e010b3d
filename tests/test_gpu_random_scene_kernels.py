"""GPU parity of every trace kernel and every forced device option on the adversarial random
scenes (tests/random_scenes.py), bit-exact against the oracle: running mean, RGBA8 and ray count,
no tolerance and no excluded pixel.

tests/test_gpu_random_scenes.py traces these scenes at Frames = 2 only, where the 960-pixel launch
runs at 2 lanes per pixel: one template, the run-time dispatch kernel.  Here the same scenes -- 56
seeds and the sized inputs below, 4 cameras (outside, inside a sphere, on a surface, grazing), both
rule sets, 40 x 24 (ragged against the 16 x 16 block tile both ways), MaxBounce 6, 8-row bands --
run at the launch shapes that have walk-specialised kernels, and under the forced options.

Launch shapes on a default device (test_launch_shapes_match_oracle): Frames 1 gives 4 pixels per lane,
Frames 4 / 8 / 16 give that many lanes per pixel (asserted from last_info()).  At Frames 4 and 16 a
second launch of the same key continues the mean with prev_count = Frames in the same buffers and is
compared with the oracle at 2 x Frames rendered from zero.  The first launch of a key measures its
costs and re-sorts (OrderLaunches: the first four launches of a key do), so the second already runs in
the learned heaviest-first order with its block tiles' pixels dealt by cost: OrderedLaunches >= 1 and
PixelsSorted == 1 are asserted on it, and no third launch is needed (a first launch splits only from
32 frames per lane on, SplitFirstLaunch, so none of these does).  Where the camera sees no live tile
(every pixel provably black: TilesTraced == 0) there is no order to learn, and the two fields are not looked at.

Walk (rt_trace_info.Walk)                    reached by (default device)
  0 run-time dispatch                        tiny (r^2 = 4e-12 leaves the short square root's range), every shape
  1 per-group loops                          seeds without a table: 13, 29 (2 groups), 18, 47 (265 groups); wide130 ..
  2 one word, scene-wide, direction table    one-level clouds (seeds 0, 2, 3, 9, 17 ..) at 4 pixels per lane, 4 and 8 lanes
  2 one word, scene-wide, no direction table the same clouds at 16 lanes
  3 two words, scene-wide                    clouds of 33..64 groups: seeds 6, 10, 22, 27, 31, 43, 44, 46; cloud2w
  4 four words, scene-wide                   cloud4w (101 groups)
  5 one word, per-lane thresholds            wide seeds of up to 32 groups (1, 4, 5, 7 ..), cloud seed 14
  6 two words, per-lane thresholds           wide seeds 8, 30, 41
  7 four words, per-lane thresholds          wide400 (101 groups)
No Walk value is exempt.  The mask words follow the rule set's group count (1 up to 32 groups, 2 up to 64,
4 up to 128: rt_pack.cpp cluster_table), and no table is built past 128 groups, so wide130 / cloud130 /
wide165 / cloud165 and seeds 18, 47 run the per-group loops whatever Clusters says.

Forced options (test_forced_options_match_oracle, one device per option set, closed in finally) on
OPTION_INPUTS at Frames 1 and 8; what shows that the option took effect, read from last_info():
  PrefilterRelative ON                  Walk 5 on the one-level cloud seed3 (per-lane walk on cloud geometry)
  PrefilterRelative OFF                 ClusteredWalk 0 and Walk 1 on the small wide seed1 (its prefilter is off)
  Prefilter ON                          ClusteredWalk 1 on seed3 (a table is walked only with the prefilter)
  Prefilter OFF                         ClusteredWalk 0 everywhere
  Clusters ON                           ClusteredWalk 1 on seed3, cloud4w; 0 on wide130 / cloud130 (no table past 128 groups)
  Clusters OFF                          ClusteredWalk 0 everywhere
  Clusters ON, SubClusterSpheres 1      Walk 4 on cloud4w, Walk 7 on wide400 (*)
  ClusterCount 3, SubClusterSpheres 2   Walk 3 on the two-level cloud seed31, Walk 4 on cloud4w (*)
  WalkAny ON, Clusters ON               Walk 0 everywhere
  Cull OFF (also with Prefilter OFF)    CullPassRan 0 and SegmentsFolded 0 everywhere
  OneWaveGroups OFF (also Clusters ON)  OneWaveGroups 0 everywhere (165-group scenes: beyond the LDS image)
  SphereSourceLds ON                    OneWaveGroups 0 everywhere
  SceneInHbm ON                         OneWaveGroups 1: a one-wave device keeps no LDS image, the option is inert
  OneWaveGroups OFF, SceneInHbm ON      OneWaveGroups 0 everywhere (the four-wave kernels reading HBM)
  DirectionTable ON, LanesPerPixel 16   DirectionTable 1 at 16 lanes on seed3
  DirectionTable OFF                    DirectionTable 0 everywhere
  LanesPerPixel 32                      LanesPerPixel 32 everywhere
  LanesPerPixel 1, PixelsPerLane 4      PixelsPerLane 4 at Frames 8
  PixelsPerLane 1                       PixelsPerLane 1 at Frames 1
  PixelSegment 4                        a second launch of each key at Frames 8 (prev_count 8, against the oracle at 16):
                                        PixelsSorted 1 wherever a tile is live.  The segment size only shapes the pixel
                                        permutation a launch builds for the NEXT launch of its key, so a cold launch
                                        alone would run the default device's path
  Interleave ON                         the same second launch: OrderedLaunches >= 1 but PixelsSorted 0 (interleaved wave
                                        tiles are not dealt by cost)
  MergeRounds ON + Clusters OFF, MergeRounds OFF, SecondaryThreshold 1, EncodePass OFF
                                        they change the kernel arguments of every cold launch, but rt_trace_info has no
                                        field that shows it: EFFECTS holds an explicit empty list, and the device reports
                                        the options back (rt_device_get_options), as for every set
(*) These values are the default device's too (the mask words follow the group count): they show that the table
built with another K and sub-cluster size is still walked by the multi-word kernels and gives the oracle's bits,
not that K or the size changed -- no query takes options, so that cannot be read back.  Likewise ClusteredWalk 1 on
seed3 under Clusters ON / Prefilter ON is the default's value.
Host-only schedule options (XcdGroup, WaveOrder, TileOrder, PixelSort) add no device code that reads scene
geometry and stay with test_gpu_parity.py::test_kernel_variants_match_oracle.

Oracle results are computed once per (input, camera, rule set, frames), by a small thread pool that
renders the next input while the GPU traces this one, and shared by both tests.

Measured on an MI355X (profiles/random_scene_kernels_pytest_gpu.log): the 93 tests of this file take 10.6 s run
alone (64 launch-shape tests of 48 launches each, at most 0.42 s, seed47; 27 option tests of 208 launches each, 312
with the second launches, at most 0.53 s); the whole GPU suite went from 788 tests in 43.9 s to 881 in 52.0 s.  Every comparison passed on the
first run: no case was reduced, and there is no regression test of a kernel bug to keep.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import random_scenes

pytestmark = pytest.mark.gpu

ON, OFF = 1, -1
W, H, B, BAND = 40, 24, 6, 8
FRAMES = (1, 4, 8, 16)
WARM = (4, 16)                      # a second launch of the key continues these to 2 x Frames
INPUTS = random_scenes.SEED_NAMES + random_scenes.NAMED
KINDS = ("outside", "inside", "on_surface", "grazing")

OPTION_INPUTS = random_scenes.OPTION_INPUTS
OPTION_FRAMES = (1, 8)
OPTION_WARM_FRAMES = 8              # option sets in OPTION_WARM launch each key a second time at this frame count
OPTION_SETS = [
    {"PrefilterRelative": ON}, {"PrefilterRelative": OFF},
    {"Prefilter": ON}, {"Prefilter": OFF},
    {"Clusters": ON}, {"Clusters": OFF},
    {"Clusters": ON, "SubClusterSpheres": 1}, {"ClusterCount": 3, "SubClusterSpheres": 2},
    {"WalkAny": ON, "Clusters": ON},
    {"Cull": OFF}, {"Cull": OFF, "Prefilter": OFF},
    {"OneWaveGroups": OFF}, {"OneWaveGroups": OFF, "Clusters": ON}, {"SphereSourceLds": ON}, {"SceneInHbm": ON},
    {"OneWaveGroups": OFF, "SceneInHbm": ON},
    {"DirectionTable": ON, "LanesPerPixel": 16}, {"DirectionTable": OFF},
    {"LanesPerPixel": 32}, {"LanesPerPixel": 1, "PixelsPerLane": 4}, {"PixelsPerLane": 1},
    {"MergeRounds": ON, "Clusters": OFF}, {"MergeRounds": OFF},
    {"Interleave": ON}, {"SecondaryThreshold": 1}, {"EncodePass": OFF}, {"PixelSegment": 4},
]


def _option_id(options):
    return ",".join(f"{k}={v}" for k, v in options.items())


# ---------------------------------------------------------------- inputs and their oracle results, built once
_inputs = {}   # name -> (spheres, [(kind, rt scene, rt camera, oracle scene, oracle camera)])
_oracle = {}   # (name, camera index, simd, frames) -> future of (mean as u32 (N, 4), RGBA8, rays)
_pool = ThreadPoolExecutor(max(1, min(8, len(os.sched_getaffinity(0)))))
_launches = []  # (option id or "", input, camera kind, frames, last_info()) of every launch of this file


def _input(rt, orc, name):
    if name not in _inputs:
        spec, grazing_seed = random_scenes.named(name)
        spheres = random_scenes.add_grazing_spheres(rt, spec, W, H, seed=grazing_seed)
        views = []
        for look, dist, ang, yh, kind in spec["cameras"]:
            s, o = random_scenes.build(rt, orc, spheres, spec["use_sky"], look, dist, ang, yh)
            views.append((kind, s, rt.camera_setup(s, W, H), o, orc.camera(o, W, H)))
        _inputs[name] = (spheres, views)
    return _inputs[name]


def _render(orc, o, ocam, simd, frames):
    prev, cur, rays = orc.render(o, ocam, W, H, frames=frames, max_bounce=B, simd=simd)
    return prev.view(np.uint32).reshape(-1, 4), cur, rays


def _request(rt, orc, name, frames):
    """Queues the oracle renders of an input that nobody asked for yet (each from zero)."""
    _, views = _input(rt, orc, name)
    for ci, (_, _, _, o, ocam) in enumerate(views):
        for simd in (True, False):
            for f in frames:
                if (name, ci, simd, f) not in _oracle:
                    _oracle[(name, ci, simd, f)] = _pool.submit(_render, orc, o, ocam, simd, f)


def _expected(name, ci, simd, frames):
    return _oracle[(name, ci, simd, frames)].result()


def _launch(torch, dev, cam, simd, frames, bufs=None):
    """One launch; with `bufs` of an earlier launch it continues their mean from prev_count = frames."""
    prev_count = 0 if bufs is None else frames
    if bufs is None:
        bufs = (torch.zeros((W * H, 4), dtype=torch.float32, device="cuda"),
                torch.zeros(W * H, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    prev, cur, rays = bufs
    dev.trace(cam, width=W, height=H, prev_ptr=prev.data_ptr(), cur_ptr=cur.data_ptr(), rays_ptr=rays.data_ptr(),
              prev_count=prev_count, frames=frames, max_bounce=B, simd=simd, band_rows=BAND,
              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return bufs


def _assert_same(bufs, want, what):
    """The three bit-for-bit comparisons (a continued launch adds to the ray count, as the oracle's
    count from zero does)."""
    prev, cur, rays = bufs
    oprev, ocur, orays = want
    gp = prev.cpu().numpy().view(np.uint32).reshape(-1, 4)
    bad = np.argwhere(gp != oprev)
    assert bad.size == 0, f"{what}: {len(bad)} accumulation words differ, first {bad[:3].tolist()}"
    assert np.array_equal(cur.cpu().numpy().view(np.uint32), ocur), f"{what}: RGBA8 differs"
    assert int(rays.item()) == orays, f"{what}: {int(rays.item())} segments, the oracle counts {orays}"


@pytest.fixture(scope="module")
def kdev(rt, torch_cuda):
    dev = rt.Device(0)
    yield dev
    dev.close()


# ---------------------------------------------------------------- part 2: launch shapes on a default device
@pytest.mark.parametrize("name", INPUTS)
def test_launch_shapes_match_oracle(rt, orc, torch_cuda, kdev, name):
    """Every launch shape of a default device on one input: Frames 1 (4 pixels per lane), 4, 8 and 16
    (that many lanes per pixel), and the warm second launch of the key at Frames 4 and 16, which runs in
    the learned order (module docstring)."""
    torch = torch_cuda
    all_frames = tuple(sorted(set(FRAMES) | {2 * f for f in WARM}))
    _request(rt, orc, name, all_frames)
    if INPUTS.index(name) + 1 < len(INPUTS):  # the pool renders the next input while this one is traced
        _request(rt, orc, INPUTS[INPUTS.index(name) + 1], all_frames)
    _, views = _input(rt, orc, name)
    kdev.upload_scene(views[0][1])
    for ci, (kind, _, cam, _, _) in enumerate(views):
        for simd in (True, False):
            for frames in FRAMES:
                what = f"{name} {kind} simd={simd} Frames={frames}"
                bufs = _launch(torch, kdev, cam, simd, frames)
                info = dict(kdev.last_info(), Warm=0)
                _launches.append(("", name, kind, frames, info))
                _assert_same(bufs, _expected(name, ci, simd, frames), what)
                if frames == 1:
                    assert info["PixelsPerLane"] == 4 and info["LanesPerPixel"] == 1, (what, info)
                else:
                    assert info["PixelsPerLane"] == 1 and info["LanesPerPixel"] == frames, (what, info)
                assert info["CullPassRan"] == 1 and info["OrderedLaunches"] == 0 and info["PixelsSorted"] == 0, (what, info)
                if frames in WARM:
                    _launch(torch, kdev, cam, simd, frames, bufs)
                    warm = dict(kdev.last_info(), Warm=1)
                    _launches.append(("", name, kind, frames, warm))
                    _assert_same(bufs, _expected(name, ci, simd, 2 * frames), what + " (second launch)")
                    assert warm["CullPassRan"] == 0 and warm["LanesPerPixel"] == frames, (what, warm)
                    if warm["TilesTraced"] > 0:  # (no live tile: there is no order to learn)
                        assert warm["OrderedLaunches"] >= 1 and warm["PixelsSorted"] == 1, (what, warm)


# ---------------------------------------------------------------- part 3: forced options on the same scenes
def _everywhere(field, value):
    return lambda runs: all(info[field] == value for _, _, _, info in runs)


def _on(name, **fields):
    """Every launch of input `name` (optionally at frames=) shows these last_info() values."""
    frames = fields.pop("frames", None)

    def check(runs):
        hit = [info for n, _, f, info in runs if n == name and frames in (None, f)]
        return bool(hit) and all(info[k] == v for info in hit for k, v in fields.items())
    return check


def _warm(pixels_sorted):
    """Second launches of a key with a live tile exist, and each ran in the learned order, its pixels dealt
    by cost or not as given."""
    def check(runs):
        hit = [info for _, _, _, info in runs if info["Warm"] and info["TilesTraced"] > 0]
        return bool(hit) and all(info["CullPassRan"] == 0 and info["OrderedLaunches"] >= 1 and
                                 info["PixelsSorted"] == pixels_sorted for info in hit)
    return check


NO_FIELD = []  # the option changes kernel arguments, but rt_trace_info has no field that shows it
EFFECTS = {
    "PrefilterRelative=1": [_on("seed3", Walk=5, ClusteredWalk=1)],
    "PrefilterRelative=-1": [_on("seed1", Walk=1, ClusteredWalk=0)],
    "Prefilter=1": [_on("seed3", ClusteredWalk=1)],
    "Prefilter=-1": [_everywhere("ClusteredWalk", 0)],
    "Clusters=1": [_on("seed3", ClusteredWalk=1), _on("cloud4w", ClusteredWalk=1), _on("wide130", ClusteredWalk=0),
                   _on("cloud130", ClusteredWalk=0)],
    "Clusters=-1": [_everywhere("ClusteredWalk", 0)],
    "Clusters=1,SubClusterSpheres=1": [_on("cloud4w", Walk=4, ClusteredWalk=1), _on("wide400", Walk=7, ClusteredWalk=1)],
    "ClusterCount=3,SubClusterSpheres=2": [_on("seed31", Walk=3, ClusteredWalk=1), _on("cloud4w", Walk=4, ClusteredWalk=1)],
    "WalkAny=1,Clusters=1": [_everywhere("Walk", 0), _on("seed3", ClusteredWalk=1)],
    "Cull=-1": [_everywhere("CullPassRan", 0), _everywhere("SegmentsFolded", 0)],
    "Cull=-1,Prefilter=-1": [_everywhere("CullPassRan", 0), _everywhere("SegmentsFolded", 0),
                             _everywhere("ClusteredWalk", 0)],
    "OneWaveGroups=-1": [_everywhere("OneWaveGroups", 0)],
    "OneWaveGroups=-1,Clusters=1": [_everywhere("OneWaveGroups", 0), _on("seed3", ClusteredWalk=1)],
    "SphereSourceLds=1": [_everywhere("OneWaveGroups", 0)],
    "SceneInHbm=1": [_everywhere("OneWaveGroups", 1)],
    "OneWaveGroups=-1,SceneInHbm=1": [_everywhere("OneWaveGroups", 0)],
    "DirectionTable=1,LanesPerPixel=16": [_everywhere("LanesPerPixel", 16), _on("seed3", DirectionTable=1, Walk=2)],
    "DirectionTable=-1": [_everywhere("DirectionTable", 0), _on("seed3", Walk=2)],
    "LanesPerPixel=32": [_everywhere("LanesPerPixel", 32)],
    "LanesPerPixel=1,PixelsPerLane=4": [_everywhere("PixelsPerLane", 4), _everywhere("LanesPerPixel", 1)],
    "PixelsPerLane=1": [_everywhere("PixelsPerLane", 1)],
    "MergeRounds=1,Clusters=-1": [_everywhere("ClusteredWalk", 0)],
    "MergeRounds=-1": NO_FIELD,
    "Interleave=1": [_warm(0)],
    "SecondaryThreshold=1": NO_FIELD,
    "EncodePass=-1": NO_FIELD,
    "PixelSegment=4": [_warm(1)],
}
OPTION_WARM = ("Interleave=1", "PixelSegment=4")


@pytest.mark.parametrize("options", OPTION_SETS, ids=_option_id)
def test_forced_options_match_oracle(rt, orc, torch_cuda, options):
    """One forced option set, on a device of its own, over OPTION_INPUTS x 4 cameras x both rule sets at
    Frames 1 and 8 (the sets of OPTION_WARM: and a second launch of the key at 8); then what shows that the
    option took effect (module docstring)."""
    torch = torch_cuda
    warm_set = _option_id(options) in OPTION_WARM
    for name in OPTION_INPUTS:
        _request(rt, orc, name, OPTION_FRAMES + ((2 * OPTION_WARM_FRAMES,) if warm_set else ()))
    runs = []
    dev = rt.Device(0, options=options)
    try:
        assert dev.options() == options
        for name in OPTION_INPUTS:
            _, views = _input(rt, orc, name)
            dev.upload_scene(views[0][1])
            for ci, (kind, _, cam, _, _) in enumerate(views):
                for simd in (True, False):
                    for frames in OPTION_FRAMES:
                        bufs = _launch(torch, dev, cam, simd, frames)
                        what = f"{_option_id(options)}: {name} {kind} simd={simd} Frames={frames}"
                        info = dict(dev.last_info(), Warm=0)
                        runs.append((name, kind, frames, info))
                        _launches.append((_option_id(options), name, kind, frames, info))
                        _assert_same(bufs, _expected(name, ci, simd, frames), what)
                        if warm_set and frames == OPTION_WARM_FRAMES:
                            _launch(torch, dev, cam, simd, frames, bufs)
                            warm = dict(dev.last_info(), Warm=1)
                            runs.append((name, kind, frames, warm))
                            _launches.append((_option_id(options), name, kind, frames, warm))
                            _assert_same(bufs, _expected(name, ci, simd, 2 * frames), what + " (second launch)")
    finally:
        dev.close()
    shown = ("Walk", "ClusteredWalk", "DirectionTable", "OneWaveGroups", "LanesPerPixel", "PixelsPerLane", "CullPassRan",
             "Warm", "OrderedLaunches", "PixelsSorted")
    for i, effect in enumerate(EFFECTS[_option_id(options)]):  # (every set has an entry: test_every_option_set_has_effects)
        assert effect(runs), f"{_option_id(options)}: effect {i} not seen; (input, camera, Frames, {shown}): " \
                             f"{sorted({(n, k, f) + tuple(info[s] for s in shown) for n, k, f, info in runs})}"


def test_every_option_set_has_effects():
    """EFFECTS is indexed directly: a renamed or new option set cannot lose its checks unnoticed."""
    assert set(EFFECTS) == {_option_id(o) for o in OPTION_SETS} and set(OPTION_WARM) <= set(EFFECTS)


# ---------------------------------------------------------------- what the set exercised
def test_random_scene_kernels_exercise_every_walk():
    """Per camera kind, on the default device: Walk 1, Walk 2 with and without the direction table (the
    latter at 16 lanes), Walk 5, Walk 0 on `tiny` at every shape, and a dead-tile fold -- except from the
    inside camera, where no tile can be dead and the absence of a fold is asserted instead -- and second
    launches at Frames 4 and 16 that did run ordered and sorted.  Over the
    whole file, the forced options' devices included: every Walk value 1-7."""
    default = [r for r in _launches if r[0] == ""]
    if {r[1] for r in default} != set(INPUTS):
        pytest.skip("run with the per-input tests")
    missing = []
    for kind in KINDS:
        runs = [(name, frames, info) for _, name, k, frames, info in default if k == kind]
        seen = {
            "walk 1": any(i["Walk"] == 1 and not i["ClusteredWalk"] for _, _, i in runs),
            "walk 2, direction table": any(i["Walk"] == 2 and i["ClusteredWalk"] and i["DirectionTable"] for _, _, i in runs),
            "walk 2, no direction table, 16 lanes": any(i["Walk"] == 2 and i["ClusteredWalk"] and not i["DirectionTable"] and
                                                        i["LanesPerPixel"] == 16 for _, _, i in runs),
            "walk 5": any(i["Walk"] == 5 and i["ClusteredWalk"] for _, _, i in runs),
        }
        for frames in FRAMES:
            tiny = [i for n, f, i in runs if n == "tiny" and f == frames]
            seen[f"walk 0 on tiny at Frames {frames}"] = bool(tiny) and all(i["Walk"] == 0 for i in tiny)
        # the warm launches assert the learned order only where a tile is live: some must have been
        for frames in WARM:
            seen[f"ordered and sorted second launch at Frames {frames}"] = any(
                i["Warm"] and f == frames and i["TilesTraced"] > 0 and i["OrderedLaunches"] >= 1 and i["PixelsSorted"] == 1
                for _, f, i in runs)
        folds = sorted({n for n, _, i in runs if i["SegmentsFolded"] > 0})
        if kind == "inside":
            # the camera is strictly inside the largest sphere, so every primary ray hits it and no tile
            # can be dead: a fold from this camera would be a wrong cull, not coverage
            seen["no dead tile from inside a sphere"] = not folds
        else:
            seen["dead-tile fold"] = bool(folds)
        print(kind, "folds on", folds)
        missing += [(kind, what) for what, ok in seen.items() if not ok]
    assert not missing, missing
    by_walk = {w: sorted({r[1] for r in default if r[4]["Walk"] == w}) for w in range(8)}
    print({w: names[:12] for w, names in by_walk.items()})
    seen = {r[4]["Walk"] for r in _launches}
    assert seen >= set(range(1, 8)), sorted(seen)
