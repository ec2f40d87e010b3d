"""simd_ray_tracer_amd — Python mirror of the reference trace path's interface.

Thin ctypes layer over the in-tree C-ABI library ``librt_trace.so`` (HIP
kernels for gfx950 + C++ host, see ``include/rt_trace.h``).  It mirrors the
reference's names and argument meaning:

* ``scene_builtin`` / ``scene_prefix``  — Scenes[] of main.cpp:93-268
* ``camera_setup``                      — the camera block of OnRender, main.cpp:776-838
* ``Device.trace``                      — WorkQueueStart(RenderTile|RenderTileScalar, ...), main.cpp:851-856
* ``on_init`` / ``on_render``           — OnInit / OnRender, base.h:163-164

The library is REQUIRED: every entry point raises if it is missing or if no
HIP device is present.  There is no CPU fallback on this path (the CPU
restatement under ``oracle/`` is test infrastructure, never imported here).
"""
from __future__ import annotations

import ctypes
import os
import pathlib
from ctypes import POINTER, c_bool, c_char_p, c_double, c_float, c_int, c_uint32, c_uint64, c_void_p
from typing import Optional

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
# RT_TRACE_LIB selects an alternative in-tree build (kernel A/B experiments)
LIB_PATH = _HERE / os.environ.get("RT_TRACE_LIB", "librt_trace.so")

RT_SEED_PIXEL = 1
RT_MAX_SPHERES = 16384
RT_FLAG_ACCUM_ZERO = 1
RT_FLAG_SRGB_POW = 2
RT_FORMAT_R32B32G32A32_F32 = 1
RT_FORMAT_R8G8B8A8_U32 = 2
KEY_FORWARD, KEY_BACK, KEY_RIGHT, KEY_LEFT, KEY_UP, KEY_DOWN, KEY_RESET = (1, 2, 4, 8, 16, 32, 64)


# ----------------------------------------------------------- C structs
class RtV3(ctypes.Structure):
    _fields_ = [("x", c_float), ("y", c_float), ("z", c_float), ("_w", c_float)]


class RtMaterial(ctypes.Structure):  # main.cpp:11-16, 48 B (16-byte aligned in C)
    _fields_ = [("Color", RtV3), ("Emissive", RtV3), ("Specular", c_float), ("IndexOfRefraction", c_float),
                ("_pad", c_float * 2)]


class RtScalarSphere(ctypes.Structure):  # main.cpp:17-21, 80 B
    _fields_ = [("Position", RtV3), ("Radius", c_float), ("_pad", c_float * 3), ("Material", RtMaterial)]


class RtSphereGroup(ctypes.Structure):  # main.cpp:23-26, 64 B
    _fields_ = [("X", c_float * 4), ("Y", c_float * 4), ("Z", c_float * 4), ("Radii", c_float * 4)]


class RtArray(ctypes.Structure):  # main.cpp:28-40
    _fields_ = [("Data", c_void_p), ("Count", c_uint32)]


class RtScene(ctypes.Structure):  # main.cpp:42-51, 80 B
    _fields_ = [("LookAt", RtV3), ("UseSkyColor", c_bool), ("DefaultDistanceFromLookAt", c_float),
                ("DefaultXAngle", c_float), ("DefaultYHeight", c_float), ("ScalarSpheres", RtArray),
                ("SIMDSpheres", RtArray), ("Materials", RtArray)]


class RtImage(ctypes.Structure):  # base.h:132-136
    _fields_ = [("Data", c_void_p), ("Width", c_uint32), ("Height", c_uint32), ("Format", c_uint32)]


class RtCameraInfo(ctypes.Structure):  # main.cpp:270-282, 144 B
    _fields_ = [("CameraPosition", RtV3), ("CameraZ", RtV3), ("CameraX", RtV3), ("CameraY", RtV3),
                ("FilmCenter", RtV3), ("FilmW", c_float), ("FilmH", c_float), ("TilesX", c_uint32),
                ("CurrentImage", RtImage), ("PreviousImage", RtImage)]


class RtRenderParams(ctypes.Structure):  # base.h:157-161
    _fields_ = [("ThreadCount", c_uint32), ("EnableSIMD", c_bool), ("SceneIndex", c_uint32)]


class RtInitParams(ctypes.Structure):  # base.h:152-155
    _fields_ = [("WindowWidth", c_uint32), ("WindowHeight", c_uint32), ("WindowTitle", c_char_p),
                ("WindowTitleSize", c_uint32)]


class RtTraceDesc(ctypes.Structure):
    _fields_ = [(n, c_uint32) for n in ("Width", "Height", "PreviousRayCount", "Frames", "MaxBounce", "EnableSIMD",
                                        "SeedMode", "BandRows", "BandCount", "BandIndex", "Flags")]


class RtTraceInfo(ctypes.Structure):  # rt_trace_last_info
    _fields_ = [("SegmentsFolded", c_uint64)] + [(n, c_uint32) for n in (
        "LanesPerPixel", "TilesTotal", "TilesTraced", "CullPassRan", "OrderedLaunches", "ClusteredWalk",
        "GroupsPerRuleSet", "SplitHeadFrames", "OneWaveGroups", "Walk", "PixelsPerLane", "PixelsSorted", "BufferGrowths",
        "TilesSelected")]


class RtTileWork(ctypes.Structure):  # rt_tile_work: one entry of rt_trace_tile_work's queue
    _fields_ = [("Tile", c_uint32), ("PreviousRayCount", c_uint32), ("Frames", c_uint32)]


class RtTileDelta(ctypes.Structure):  # rt_tile_delta: one tile's RGBA8 change statistics, 16 B
    _fields_ = [("Changed", c_uint32), ("MaxDelta", c_uint32), ("SumDelta", c_uint32), ("SumSquares", c_uint32)]


# a copied-back rt_tile_delta array: np.frombuffer(bytes, tile_delta_dtype) or array.view(tile_delta_dtype)
tile_delta_dtype = np.dtype([(n, "<u4") for n, _ in RtTileDelta._fields_])


class RtTileCounts(ctypes.Structure):  # rt_tile_counts: one tile's entry of rt_trace_tile_counts' device table, 8 B
    _fields_ = [("PreviousRayCount", c_uint32), ("Frames", c_uint32)]


class RtTileRule(ctypes.Structure):  # rt_tile_rule: rt_tile_counts_step's stopping rule, 20 B
    _fields_ = [(n, c_uint32) for n in ("Size", "MaxRoundFrames", "MaxTileFrames", "RestMaxDelta", "RestSumSquares")]


class RtTileStepSummary(ctypes.Structure):  # rt_tile_step_summary: what rt_tile_counts_step decided, 16 B
    _fields_ = [("NextFrames", c_uint64), ("ActiveTiles", c_uint32), ("RestedNow", c_uint32)]


# a device table's host image: np.zeros(tile_count(w, h), tile_counts_dtype), or a (n, 2) uint32 array viewed so
tile_counts_dtype = np.dtype([(n, "<u4") for n, _ in RtTileCounts._fields_])
tile_step_summary_dtype = np.dtype([("NextFrames", "<u8"), ("ActiveTiles", "<u4"), ("RestedNow", "<u4")])


class RtFirstHit(ctypes.Structure):  # rt_first_hit: one pixel of rt_trace_first_hit's Hit plane, 8 B
    _fields_ = [("Key", c_uint32), ("T", c_float)]


class RtFirstHitPlanes(ctypes.Structure):  # rt_first_hit_planes: the device planes rt_trace_first_hit writes, 32 B
    _fields_ = [("Size", c_uint32), ("Hit", c_void_p), ("Normal", c_void_p), ("Albedo", c_void_p)]


# a copied-back Hit plane: np.frombuffer(bytes, first_hit_dtype).reshape(height, width)
first_hit_dtype = np.dtype([("Key", "<u4"), ("T", "<f4")])
HIT_MISS, HIT_INSIDE, HIT_PIXEL_CENTRE = 0xFFFFFFFF, 0x80000000, 1


class RtDenoiseDesc(ctypes.Structure):  # rt_denoise_desc: one rt_denoise call, 88 B
    _fields_ = [("Size", c_uint32), ("Width", c_uint32), ("Height", c_uint32), ("Iterations", c_uint32),
                ("Flags", c_uint32), ("NormalPower", c_uint32), ("SigmaDepth", c_float), ("SigmaColor", c_float),
                ("Mean", c_void_p), ("Hit", c_void_p), ("Normal", c_void_p), ("Albedo", c_void_p), ("Out", c_void_p),
                ("Scratch", c_void_p), ("Rgba8", c_void_p)]


DENOISE_DEMODULATE, DENOISE_SRGB_POW, DENOISE_MAX_ITERATIONS = 1, 2, 8


class RtReprojectDesc(ctypes.Structure):  # rt_reproject_desc: one rt_reproject call, 112 B
    _fields_ = [("Size", c_uint32), ("Width", c_uint32), ("Height", c_uint32), ("Frames", c_uint32),
                ("MaxHistory", c_uint32), ("Flags", c_uint32), ("DepthTolerance", c_float),
                ("Camera", POINTER(RtCameraInfo)), ("PreviousCamera", POINTER(RtCameraInfo)), ("Mean", c_void_p),
                ("Hit", c_void_p), ("History", c_void_p), ("HistoryHit", c_void_p), ("HistoryCount", c_void_p),
                ("Out", c_void_p), ("OutCount", c_void_p), ("Rgba8", c_void_p)]


REPROJECT_SRGB_POW = 2


class RtReprojectClipDesc(ctypes.Structure):  # rt_reproject_clip_desc: one rt_reproject_clip call, 128 B
    _fields_ = [("Size", c_uint32), ("Radius", c_uint32), ("Gamma", c_float), ("Reproject", RtReprojectDesc)]


OPTION_FIELDS = ("Cull", "Prefilter", "PrefilterRelative", "Clusters", "ClusterCount", "SubClusterSpheres",
                 "SecondaryThreshold", "LanesPerPixel", "PixelsPerLane", "OneWaveGroups", "SphereSourceLds",
                 "SceneInHbm", "TablesInLds", "WalkAny", "Interleave", "MergeRounds", "TileOrder", "WaveOrder",
                 "PixelSort", "PixelSegment", "XcdGroup", "SplitFirstLaunch", "HeadSamples", "SplitParts",
                 "SplitGrowth", "OrderLaunches", "EncodePass", "DirectionTable")
RT_OPT_DEFAULT, RT_OPT_ON, RT_OPT_OFF = 0, 1, -1


class RtDeviceOptions(ctypes.Structure):  # rt_device_options: kernel / schedule choices, 0 = default
    _fields_ = [("Size", c_uint32)] + [(n, ctypes.c_int32) for n in OPTION_FIELDS]


def device_options(options: Optional[dict]) -> Optional[RtDeviceOptions]:
    """rt_device_options from {"Cull": RT_OPT_OFF, "LanesPerPixel": 16, ...} (None: the defaults).
    Switches also take True / False for RT_OPT_ON / RT_OPT_OFF."""
    if not options:
        return None
    o = RtDeviceOptions()
    o.Size = ctypes.sizeof(RtDeviceOptions)
    for k, v in options.items():
        if k not in OPTION_FIELDS:
            raise KeyError(f"unknown device option {k!r} (rt_device_options: {', '.join(OPTION_FIELDS)})")
        setattr(o, k, (RT_OPT_ON if v else RT_OPT_OFF) if isinstance(v, bool) else int(v))
    return o


def parse_options(items) -> dict:
    """["Cull=off", "LanesPerPixel=16", ...] (bench.py --opt) -> an options dict."""
    out = {}
    for it in items or ():
        k, _, v = it.partition("=")
        v = v.strip().lower()
        out[k.strip()] = {"on": RT_OPT_ON, "off": RT_OPT_OFF, "default": RT_OPT_DEFAULT}.get(v, None)
        if out[k.strip()] is None:
            out[k.strip()] = int(v)
    return out


class RtDirectionTableInfo(ctypes.Structure):  # rt_direction_table_info
    _fields_ = [(n, c_uint32) for n in ("CellsPerEdge", "MaskBits", "Rows", "CellsPerRow")]


class RtMultiInfo(ctypes.Structure):  # rt_multi_get_info
    _fields_ = [(n, c_uint32) for n in ("DeviceCount", "Transport", "BandRows", "MaxLocalRows")] + [
        ("SegmentsFolded", c_uint64)]


class RtOnRenderProfile(ctypes.Structure):  # rt_on_render_get_profile
    _fields_ = [(n, c_uint64) for n in ("Calls", "FramesLaunched", "FramesCopied")] + [
        (n, c_double) for n in ("CallMs", "HostCopyMs", "HostWaitMs", "GpuFrameMs")] + [
        ("FrameAllocations", c_uint64)]


RT_MULTI_AUTO, RT_MULTI_RCCL, RT_MULTI_PEER = 0, 1, 2
RT_MULTI_RESERVE_MEAN = 1
RT_COMM_ID_BYTES = 128

for _t, _n in ((RtV3, 16), (RtMaterial, 48), (RtScalarSphere, 80), (RtSphereGroup, 64), (RtArray, 16),
               (RtScene, 80), (RtImage, 24), (RtCameraInfo, 144), (RtRenderParams, 12)):
    assert ctypes.sizeof(_t) == _n, (_t.__name__, ctypes.sizeof(_t), _n)

# Every symbol include/rt_trace.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "rt_scene_builtin": (c_int, [c_uint32, POINTER(RtScene)]),
    "rt_scene_prefix": (c_int, [POINTER(RtScene), c_uint32, POINTER(RtScene)]),
    "rt_camera_setup": (c_int, [POINTER(RtScene), c_float, c_float, c_float, c_uint32, c_uint32,
                                POINTER(RtCameraInfo)]),
    "rt_pixel_seed": (c_uint64, [c_uint32, c_uint32, c_uint32, c_uint32, c_uint32]),
    "rt_device_create": (c_int, [c_int, POINTER(c_void_p)]),
    "rt_device_create_ex": (c_int, [c_int, POINTER(RtDeviceOptions), POINTER(c_void_p)]),
    "rt_device_get_options": (c_int, [c_void_p, POINTER(RtDeviceOptions)]),
    "rt_device_destroy": (c_int, [c_void_p]),
    "rt_set_rsqrt_table": (c_int, [c_void_p, c_void_p]),
    "rt_rsqrt_table_builtin": (c_int, [c_void_p]),
    "rt_rsqrt_table_capture_host": (c_int, [c_void_p]),
    "rt_scene_upload": (c_int, [c_void_p, POINTER(RtScene)]),
    "rt_band_local_rows": (c_uint32, [c_uint32, c_uint32, c_uint32, c_uint32]),
    "rt_trace": (c_int, [c_void_p, POINTER(RtCameraInfo), POINTER(RtTraceDesc), c_void_p, c_void_p]),
    "rt_tile_count": (c_uint32, [c_uint32, c_uint32, POINTER(c_uint32)]),
    "rt_trace_tiles": (c_int, [c_void_p, POINTER(RtCameraInfo), POINTER(RtTraceDesc), c_void_p, c_uint32, c_void_p,
                               c_void_p]),
    "rt_trace_tile_work": (c_int, [c_void_p, POINTER(RtCameraInfo), POINTER(RtTraceDesc), c_void_p, c_uint32,
                                   c_void_p, c_void_p]),
    "rt_trace_tile_work_delta": (c_int, [c_void_p, POINTER(RtCameraInfo), POINTER(RtTraceDesc), c_void_p, c_uint32,
                                         c_void_p, c_void_p, c_void_p]),
    "rt_tile_delta_rgba8": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p]),
    "rt_trace_tile_counts": (c_int, [c_void_p, POINTER(RtCameraInfo), POINTER(RtTraceDesc), c_void_p, c_uint32,
                                     c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]),
    "rt_tile_counts_step": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, POINTER(RtTileRule), c_void_p, c_void_p]),
    "rt_trace_first_hit": (c_int, [c_void_p, POINTER(RtCameraInfo), POINTER(RtTraceDesc), c_void_p, c_uint32, c_uint32,
                                   POINTER(RtFirstHitPlanes), c_void_p]),
    "rt_denoise": (c_int, [POINTER(RtDenoiseDesc), c_void_p]),
    "rt_denoise_defaults": (c_int, [POINTER(RtDenoiseDesc)]),
    "rt_reproject": (c_int, [POINTER(RtReprojectDesc), c_void_p]),
    "rt_reproject_defaults": (c_int, [POINTER(RtReprojectDesc)]),
    "rt_reproject_clip": (c_int, [POINTER(RtReprojectClipDesc), c_void_p]),
    "rt_reproject_clip_defaults": (c_int, [POINTER(RtReprojectClipDesc)]),
    "rt_assemble_bands": (c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_uint32,
                                  c_void_p]),
    "rt_trace_last_info": (c_int, [c_void_p, POINTER(RtTraceInfo)]),
    "rt_trace_last_tile_counts": (c_int, [c_void_p, POINTER(c_uint32)]),
    "rt_encode_rgba8": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p]),
    "rt_device_synchronize": (c_int, [c_void_p]),
    "rt_multi_create": (c_int, [POINTER(c_int), c_uint32, c_uint32, POINTER(c_void_p)]),
    "rt_multi_create_ex": (c_int, [POINTER(c_int), c_uint32, c_uint32, POINTER(RtDeviceOptions), POINTER(c_void_p)]),
    "rt_multi_resident_frames": (c_int, [c_void_p, POINTER(c_uint64)]),
    "rt_multi_destroy": (c_int, [c_void_p]),
    "rt_multi_set_rsqrt_table": (c_int, [c_void_p, c_void_p]),
    "rt_multi_scene_upload": (c_int, [c_void_p, POINTER(RtScene)]),
    "rt_multi_trace": (c_int, [c_void_p, POINTER(RtCameraInfo), POINTER(RtTraceDesc), c_void_p, c_void_p]),
    "rt_multi_synchronize": (c_int, [c_void_p]),
    "rt_multi_get_info": (c_int, [c_void_p, POINTER(RtMultiInfo)]),
    "rt_multi_last_trace_ms": (c_int, [c_void_p, c_void_p, c_uint32]),
    "rt_multi_last_gather_ms": (c_int, [c_void_p, POINTER(c_float)]),
    "rt_multi_shard_info": (c_int, [c_void_p, c_uint32, POINTER(RtTraceInfo)]),
    "rt_multi_reserve": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_uint32]),
    "rt_device_reserve": (c_int, [c_void_p, c_uint32, c_uint32]),
    "rt_comm_unique_id": (c_int, [c_void_p]),
    "rt_comm_create": (c_int, [c_int, c_void_p, c_uint32, c_uint32, POINTER(c_void_p)]),
    "rt_comm_destroy": (c_int, [c_void_p]),
    "rt_comm_gather_bands": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_uint32,
                                     c_void_p]),
    "rt_debug_stats": (c_int, [c_void_p, c_void_p, c_int]),
    "rt_debug_wave_times": (ctypes.c_int64, [c_void_p, c_void_p, c_uint64]),
    "rt_debug_masks": (ctypes.c_int64, [c_void_p, c_void_p, c_uint64]),
    "rt_scene_prefilter": (c_int, [POINTER(RtScene), c_uint32, c_void_p, c_void_p, c_uint32, POINTER(c_uint32),
                                   POINTER(c_uint32)]),
    "rt_scene_own_sphere": (c_int, [POINTER(RtScene), c_uint32, c_void_p, c_uint32, POINTER(c_uint32)]),
    "rt_scene_clusters": (c_int, [POINTER(RtScene), c_uint32, c_void_p, c_uint32, POINTER(c_uint32),
                                  POINTER(c_uint32)]),
    "rt_scene_groups": (c_int, [POINTER(RtScene), c_uint32, c_void_p, c_uint32, POINTER(c_uint32), c_void_p]),
    "rt_scene_clusters_expanded": (c_int, [POINTER(RtScene), c_uint32, c_void_p, c_uint32, POINTER(c_uint32),
                                           POINTER(ctypes.c_float), POINTER(c_uint32)]),
    "rt_scene_cluster_layout": (c_int, [POINTER(RtScene), c_uint32, POINTER(c_uint32), POINTER(c_uint32)]),
    "rt_scene_direction_table": (c_int, [POINTER(RtScene), c_uint32, c_void_p, c_uint64, POINTER(c_uint64),
                                         POINTER(RtDirectionTableInfo)]),
    "rt_scene_direction_members": (c_int, [POINTER(RtScene), c_uint32, c_void_p, c_uint32, POINTER(c_uint32)]),
    "rt_direction_cell": (c_uint32, [c_float, c_float, c_float]),
    "rt_direction_union": (c_int, [c_void_p, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_void_p]),
    "rt_trace_last_direction_table": (c_int, [c_void_p, POINTER(c_uint32)]),
    "rt_last_error": (c_char_p, []),
    "rt_on_init": (c_int, [POINTER(RtInitParams)]),
    "rt_on_init_devices": (c_int, [POINTER(RtInitParams), POINTER(c_int), c_uint32]),
    "rt_on_render": (c_int, [POINTER(RtImage), RtRenderParams, c_uint32, POINTER(c_uint64), POINTER(c_double)]),
    "rt_on_render_wait": (c_int, []),
    "rt_on_render_register_image": (c_int, [c_void_p, c_uint64]),
    "rt_on_render_unregister_image": (c_int, []),
    "rt_on_shutdown": (c_int, []),
    "rt_on_render_get_profile": (c_int, [POINTER(RtOnRenderProfile), c_int]),
    "rt_on_render_reserve": (c_int, [c_uint32, c_uint32]),
    "rt_image_write_ppm": (c_int, [POINTER(RtImage), c_char_p, c_uint32]),
    "rt_image_write_png": (c_int, [POINTER(RtImage), c_char_p, c_uint32]),
    "rt_frame_hash": (c_uint64, [c_void_p, c_uint64]),
}

_LIB: Optional[ctypes.CDLL] = None


class RtError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Loads librt_trace.so (built by __graft_entry__.build()); raises if absent."""
    global _LIB
    if _LIB is None:
        if not LIB_PATH.exists():
            raise RtError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        try:  # share torch's HIP runtime when torch is present: its libamdhip64 carries the
            import torch  # noqa: F401  same soname, so loading it first keeps ONE runtime per process
        except ImportError:
            pass
        L = ctypes.CDLL(str(LIB_PATH))
        ab_build = "RT_TRACE_LIB" in os.environ  # an older A/B build may lack newer inspection hooks
        for name, (res, args) in SIGNATURES.items():
            if ab_build and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _check(rc: int, what: str) -> None:
    if rc < 0:
        msg = lib().rt_last_error()
        raise RtError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


# ------------------------------------------------------- host-side inputs
def scene_builtin(index: int) -> RtScene:
    s = RtScene()
    _check(lib().rt_scene_builtin(index, ctypes.byref(s)), "rt_scene_builtin")
    return s


def scene_prefix(scene: RtScene, n_spheres: int) -> RtScene:
    out = RtScene()
    _check(lib().rt_scene_prefix(ctypes.byref(scene), n_spheres, ctypes.byref(out)), "rt_scene_prefix")
    out._keep = getattr(scene, "_keep", None)
    return out


def scene_from_spheres(spheres: np.ndarray, look_at=(0.0, 0.0, 0.0), use_sky: bool = False,
                       distance: float = 1.0, x_angle: float = 0.0, y_height: float = 0.0) -> RtScene:
    """Scene from an (N, 20) f32 array of scalar_sphere records (main.cpp:17-21),
    converted to SIMD groups as ConvertScalarSpheresToSIMDSpheres does (main.cpp:73-91)."""
    sp = np.ascontiguousarray(spheres, dtype=np.float32).reshape(-1, 20)
    n = sp.shape[0]
    ng = (n + 3) // 4
    groups = np.zeros((ng, 16), np.float32)
    mats = np.zeros((n + 1, 12), np.float32)
    for i in range(n):
        g, l = divmod(i, 4)
        groups[g, l], groups[g, 4 + l], groups[g, 8 + l], groups[g, 12 + l] = sp[i, 0], sp[i, 1], sp[i, 2], sp[i, 4]
        mats[i] = sp[i, 8:20]
    s = RtScene()
    s.LookAt = RtV3(*look_at, 0.0)
    s.UseSkyColor = bool(use_sky)
    s.DefaultDistanceFromLookAt = distance
    s.DefaultXAngle = x_angle
    s.DefaultYHeight = y_height
    s.ScalarSpheres = RtArray(sp.ctypes.data, n)
    s.SIMDSpheres = RtArray(groups.ctypes.data, ng)
    s.Materials = RtArray(mats.ctypes.data, n + 1)
    s._keep = (sp, groups, mats)
    return s


def scene_arrays(scene: RtScene):
    """(spheres (N,20), groups (G,16), materials (M,12)) f32 copies of a scene."""
    def arr(a: RtArray, width: int):
        buf = (ctypes.c_float * (a.Count * width)).from_address(a.Data)
        return np.frombuffer(buf, dtype=np.float32).reshape(a.Count, width).copy()
    return arr(scene.ScalarSpheres, 20), arr(scene.SIMDSpheres, 16), arr(scene.Materials, 12)


def camera_setup(scene: RtScene, width: int, height: int, distance: Optional[float] = None,
                 x_angle: Optional[float] = None, y_height: Optional[float] = None) -> RtCameraInfo:
    cam = RtCameraInfo()
    d = scene.DefaultDistanceFromLookAt if distance is None else distance
    a = scene.DefaultXAngle if x_angle is None else x_angle
    h = scene.DefaultYHeight if y_height is None else y_height
    _check(lib().rt_camera_setup(ctypes.byref(scene), d, a, h, width, height, ctypes.byref(cam)), "rt_camera_setup")
    return cam


def camera_floats(cam: RtCameraInfo) -> np.ndarray:
    """The 24-float camera record the oracle consumes (position, Z, X, Y, film centre, W, H, tiles)."""
    raw = np.frombuffer(ctypes.string_at(ctypes.addressof(cam), 96), dtype=np.float32).copy()
    return raw


def pixel_seed(x: int, y: int, frame: int, width: int, height: int) -> int:
    return int(lib().rt_pixel_seed(x, y, frame, width, height))


def band_local_rows(height: int, band_rows: int, band_count: int, band_index: int) -> int:
    return int(lib().rt_band_local_rows(height, band_rows, band_count, band_index))


RT_TILE_SIZE = 32  # the reference's TileSize (main.cpp:9)


def tile_count(width: int, height: int) -> int:
    """TilesX * TilesY of a width x height image as OnRender forms its 32 x 32 tiles
    (rt_tile_count; TilesX = ceil(width / 32)); 0 for an empty or oversized image."""
    return int(lib().rt_tile_count(width, height, None))


def tiles_of_rect(width: int, height: int, x0: int, y0: int, x1: int, y1: int) -> list:
    """The tiles (Tile = TileY * TilesX + TileX, ascending) of a width x height image that the pixel
    rectangle [x0, x1) x [y0, y1) touches, clipped to the image; [] when it covers no pixel.
    Pure Python (no library call)."""
    x0, y0, x1, y1 = max(0, int(x0)), max(0, int(y0)), min(int(width), int(x1)), min(int(height), int(y1))
    if x0 >= x1 or y0 >= y1:
        return []
    tiles_x = (width + RT_TILE_SIZE - 1) // RT_TILE_SIZE
    return [ty * tiles_x + tx
            for ty in range(y0 // RT_TILE_SIZE, (y1 - 1) // RT_TILE_SIZE + 1)
            for tx in range(x0 // RT_TILE_SIZE, (x1 - 1) // RT_TILE_SIZE + 1)]


def tile_work_array(work) -> np.ndarray:
    """(n, 3) uint32 array of rt_tile_work records {Tile, PreviousRayCount, Frames} from a sequence
    of (tile, prev_count, frames) triples or an (n, 3) integer array; ValueError for anything else
    (another shape, non-integers, values outside u32).  Pure Python (no library call)."""
    w = np.asarray(list(work) if not isinstance(work, np.ndarray) else work)
    if w.size == 0:
        return np.zeros((0, 3), np.uint32)
    if w.ndim != 2 or w.shape[1] != 3 or w.dtype.kind not in "iu":
        raise ValueError("work: (tile, prev_count, frames) triples of integers, or an (n, 3) integer array")
    if int(w.min()) < 0 or int(w.max()) > 0xFFFFFFFF:
        raise ValueError("work: tile indices and counts are u32 values")
    return np.ascontiguousarray(w.astype(np.uint32))


def scene_prefilter(scene: RtScene, simd: bool = True):
    """(r2, r2p, flags) per sphere slot 4*group+lane as rt_scene_upload packs
    them: the exact test's r^2, the secondary-ray prefilter threshold, and
    flags bit 0 = prefilter on by default, bit 1 = short candidate sqrt."""
    n, fl = c_uint32(), c_uint32()
    _check(lib().rt_scene_prefilter(ctypes.byref(scene), int(simd), None, None, 0, ctypes.byref(n), ctypes.byref(fl)),
           "rt_scene_prefilter")
    r2 = np.zeros(n.value, np.float32)
    r2p = np.zeros(n.value, np.float32)
    _check(lib().rt_scene_prefilter(ctypes.byref(scene), int(simd), r2.ctypes.data, r2p.ctypes.data, n.value,
                                    ctypes.byref(n), ctypes.byref(fl)), "rt_scene_prefilter")
    return r2, r2p, int(fl.value)


def scene_own_sphere(scene: RtScene, simd: bool = True) -> np.ndarray:
    """rho per sphere slot 4*group+lane (rt_scene_own_sphere): r^2 where the own-sphere rule of the
    cluster walk applies to the sphere, +inf where it is off."""
    n = c_uint32()
    _check(lib().rt_scene_own_sphere(ctypes.byref(scene), int(simd), None, 0, ctypes.byref(n)), "rt_scene_own_sphere")
    rho = np.zeros(n.value, np.float32)
    _check(lib().rt_scene_own_sphere(ctypes.byref(scene), int(simd), rho.ctypes.data, n.value, ctypes.byref(n)),
           "rt_scene_own_sphere")
    return rho


def scene_groups(scene: RtScene, simd: bool = True):
    """The packed group records rt_scene_upload builds (rt_scene_groups): (records
    (n_groups, rows, 4) f32, layout dict of the row indices rt_kernel.h names)."""
    nf4 = c_uint32()
    rows = np.zeros(6, np.uint32)
    _check(lib().rt_scene_groups(ctypes.byref(scene), int(simd), None, 0, ctypes.byref(nf4), rows.ctypes.data),
           "rt_scene_groups")
    tab = np.zeros((nf4.value, 4), np.float32)
    if nf4.value:
        _check(lib().rt_scene_groups(ctypes.byref(scene), int(simd), tab.ctypes.data, nf4.value, ctypes.byref(nf4),
                                     None), "rt_scene_groups")
    layout = dict(zip(("kGroupF4", "kRowX", "kRowY", "kRowZ", "kRowR2", "kRowR2P"), (int(v) for v in rows)))
    return tab.reshape(-1, layout["kGroupF4"], 4), layout


def scene_clusters(scene: RtScene, simd: bool = True):
    """The clustered prefilter table rt_scene_upload builds: (table (n, rows, 4)
    f32, n_cpairs) with rows = 4 for a one-word pair mask (<= 32 groups), else
    3 + words (rt_kernel.h cl_entry_f4); n_cpairs == 0 means the per-group loop
    is used."""
    nf4, ncp = c_uint32(), c_uint32()
    _check(lib().rt_scene_clusters(ctypes.byref(scene), int(simd), None, 0, ctypes.byref(nf4), ctypes.byref(ncp)),
           "rt_scene_clusters")
    tab = np.zeros((nf4.value, 4), np.float32)
    if nf4.value:
        _check(lib().rt_scene_clusters(ctypes.byref(scene), int(simd), tab.ctypes.data, nf4.value, ctypes.byref(nf4),
                                       ctypes.byref(ncp)), "rt_scene_clusters")
    # the pair-mask words follow the rule set's group count (rt_pack.cpp cluster_table):
    # SIMDSpheres groups for the SIMD rules, ceil(ScalarSpheres / 4) for the scalar ones;
    # per-lane ("relative") tables carry a fifth row at one word (the height slab)
    groups = scene.SIMDSpheres.Count if simd else (scene.ScalarSpheres.Count + 3) // 4
    words = 1 if groups <= 32 else 2 if groups <= 64 else 4
    relative = bool(scene_prefilter(scene, simd)[2] & 4)
    rows = (5 if relative else 4) if words == 1 else 3 + words
    return tab.reshape(-1, rows, 4), int(ncp.value)


def scene_clusters_expanded(scene: RtScene, simd: bool = True):
    """The expanded form of a scene-wide cluster table (rt_scene_clusters_expanded): (table shaped as
    scene_clusters' -- empty without one --, c0 (3,) f32, in_use)."""
    nf4, use = c_uint32(), c_uint32()
    c0 = (ctypes.c_float * 3)()
    _check(lib().rt_scene_clusters_expanded(ctypes.byref(scene), int(simd), None, 0, ctypes.byref(nf4), c0,
                                            ctypes.byref(use)), "rt_scene_clusters_expanded")
    tab = np.zeros((nf4.value, 4), np.float32)
    if nf4.value:
        _check(lib().rt_scene_clusters_expanded(ctypes.byref(scene), int(simd), tab.ctypes.data, nf4.value,
                                                ctypes.byref(nf4), c0, ctypes.byref(use)), "rt_scene_clusters_expanded")
    rows = scene_clusters(scene, simd)[0].shape[1]
    return tab.reshape(-1, rows, 4), np.array(list(c0), np.float32), bool(use.value)


def scene_cluster_layout(scene: RtScene, simd: bool = True):
    """(levels, sub_pairs) of the clustered prefilter table (rt_scene_cluster_layout):
    levels 2 means the first n_cpairs entries index sub_pairs sub-cluster pair
    entries, which index the member entries."""
    lv, sp = c_uint32(), c_uint32()
    _check(lib().rt_scene_cluster_layout(ctypes.byref(scene), int(simd), ctypes.byref(lv), ctypes.byref(sp)),
           "rt_scene_cluster_layout")
    return int(lv.value), int(sp.value)


def scene_direction_table(scene: RtScene, simd: bool = True):
    """The direction table of a one-word scene-wide table (rt_scene_direction_table): (masks shaped
    (Rows, CellsPerRow), uint32 or uint64 -- None where the scene has no table --, cells per face edge)."""
    nbytes, info = c_uint64(), RtDirectionTableInfo()
    _check(lib().rt_scene_direction_table(ctypes.byref(scene), int(simd), None, 0, ctypes.byref(nbytes),
                                          ctypes.byref(info)), "rt_scene_direction_table")
    if not nbytes.value:
        return None, 0
    tab = np.zeros((info.Rows, info.CellsPerRow), np.uint64 if info.MaskBits == 64 else np.uint32)
    assert tab.nbytes == nbytes.value
    _check(lib().rt_scene_direction_table(ctypes.byref(scene), int(simd), tab.ctypes.data, tab.nbytes,
                                          ctypes.byref(nbytes), ctypes.byref(info)), "rt_scene_direction_table")
    return tab, int(info.CellsPerEdge)


def scene_direction_members(scene: RtScene, simd: bool = True) -> np.ndarray:
    """The direction walk's member entries in pair order (rt_scene_direction_members): (pairs, 4, 4) f32."""
    nf4 = c_uint32()
    _check(lib().rt_scene_direction_members(ctypes.byref(scene), int(simd), None, 0, ctypes.byref(nf4)),
           "rt_scene_direction_members")
    tab = np.zeros((nf4.value, 4), np.float32)
    if nf4.value:
        _check(lib().rt_scene_direction_members(ctypes.byref(scene), int(simd), tab.ctypes.data, nf4.value,
                                                ctypes.byref(nf4)), "rt_scene_direction_members")
    return tab.reshape(-1, 4, 4)


def direction_cell(dx, dy, dz) -> int:
    """rt_direction_cell: the kernel's own cell function."""
    return int(lib().rt_direction_cell(float(dx), float(dy), float(dz)))


def rsqrt_table_builtin() -> np.ndarray:
    t = np.zeros(2048, np.float32)
    _check(lib().rt_rsqrt_table_builtin(t.ctypes.data), "rt_rsqrt_table_builtin")
    return t


# ---------------------------------------------------------------- device
class Device:
    """One GPU: rsqrt table, uploaded scene, trace launches (rt_device)."""

    def __init__(self, ordinal: int = 0, rsqrt_table: Optional[np.ndarray] = None, options: Optional[dict] = None):
        h = c_void_p()
        o = device_options(options)
        _check(lib().rt_device_create_ex(ordinal, ctypes.byref(o) if o is not None else None, ctypes.byref(h)),
               "rt_device_create")
        self.handle = h
        table = rsqrt_table_builtin() if rsqrt_table is None else np.ascontiguousarray(rsqrt_table, np.float32)
        _check(lib().rt_set_rsqrt_table(self.handle, table.ctypes.data), "rt_set_rsqrt_table")
        self._scene = None

    def upload_scene(self, scene: RtScene) -> None:
        _check(lib().rt_scene_upload(self.handle, ctypes.byref(scene)), "rt_scene_upload")
        self._scene = scene

    def options(self) -> dict:
        """The non-default rt_device_options the device was created with."""
        o = RtDeviceOptions()
        _check(lib().rt_device_get_options(self.handle, ctypes.byref(o)), "rt_device_get_options")
        return {n: int(getattr(o, n)) for n in OPTION_FIELDS if getattr(o, n)}

    def trace(self, cam: RtCameraInfo, *, width: int, height: int, prev_ptr: int, cur_ptr: int, rays_ptr: int,
              prev_count: int = 0, frames: int = 1, max_bounce: int = 5, simd: bool = True,
              band_rows: int = 32, band_count: int = 1, band_index: int = 0, accum_zero: bool = False,
              srgb_pow: bool = False, stream: Optional[int] = None) -> None:
        """Traces `frames` progressive frames into device images (raw device pointers)
        on the HIP stream handle `stream` (None/0 = the null stream)."""
        c = RtCameraInfo()
        ctypes.pointer(c)[0] = cam
        c.CurrentImage = RtImage(cur_ptr, width, height, RT_FORMAT_R8G8B8A8_U32)
        c.PreviousImage = RtImage(prev_ptr, width, height, RT_FORMAT_R32B32G32A32_F32)
        d = RtTraceDesc(width, height, prev_count, frames, max_bounce, 1 if simd else 0, RT_SEED_PIXEL,
                        band_rows, band_count, band_index,
                        (RT_FLAG_ACCUM_ZERO if accum_zero else 0) | (RT_FLAG_SRGB_POW if srgb_pow else 0))
        _check(lib().rt_trace(self.handle, ctypes.byref(c), ctypes.byref(d), c_void_p(rays_ptr),
                              c_void_p(stream or 0)), "rt_trace")

    def trace_tiles(self, cam: RtCameraInfo, *, tiles, width: int, height: int, prev_ptr: int, cur_ptr: int,
                    rays_ptr: int, prev_count: int = 0, frames: int = 1, max_bounce: int = 5, simd: bool = True,
                    band_rows: int = 32, accum_zero: bool = False, srgb_pow: bool = False,
                    stream: Optional[int] = None) -> None:
        """trace() over the listed 32 x 32 tiles only (rt_trace_tiles): `tiles` is any sequence of
        integers Tile = TileY * TilesX + TileX (tiles_of_rect lists those of a pixel rectangle); the
        images are the full width x height ones and no pixel outside the listed tiles is written.
        The list is consumed before the call returns."""
        t = np.ascontiguousarray(np.asarray(list(tiles) if not isinstance(tiles, np.ndarray) else tiles).reshape(-1))
        if t.size and (t.dtype.kind not in "iu" or int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
            raise ValueError("tiles: a sequence of tile indices (non-negative integers)")
        t = t.astype(np.uint32)
        c = RtCameraInfo()
        ctypes.pointer(c)[0] = cam
        c.CurrentImage = RtImage(cur_ptr, width, height, RT_FORMAT_R8G8B8A8_U32)
        c.PreviousImage = RtImage(prev_ptr, width, height, RT_FORMAT_R32B32G32A32_F32)
        d = RtTraceDesc(width, height, prev_count, frames, max_bounce, 1 if simd else 0, RT_SEED_PIXEL,
                        band_rows, 1, 0,
                        (RT_FLAG_ACCUM_ZERO if accum_zero else 0) | (RT_FLAG_SRGB_POW if srgb_pow else 0))
        _check(lib().rt_trace_tiles(self.handle, ctypes.byref(c), ctypes.byref(d),
                                    c_void_p(t.ctypes.data if t.size else None), int(t.size), c_void_p(rays_ptr),
                                    c_void_p(stream or 0)), "rt_trace_tiles")

    def trace_tile_work(self, cam: RtCameraInfo, *, work, width: int, height: int, prev_ptr: int, cur_ptr: int,
                        rays_ptr: int, max_bounce: int = 5, simd: bool = True, band_rows: int = 32,
                        accum_zero: bool = False, srgb_pow: bool = False, stream: Optional[int] = None,
                        delta_ptr: int = 0) -> None:
        """trace_tiles() with each tile's own counts in one launch (rt_trace_tile_work): `work` is a
        sequence of (tile, prev_count, frames) triples or an (n, 3) integer array; every listed tile
        folds `frames` frames from its own `prev_count`, an entry with frames == 0 is dropped, and no
        pixel outside the listed tiles is written.  The counts are no part of the launch key: the same
        tiles with other counts reuse the cull masks and the learned order.  The array is consumed
        before the call returns.  A non-zero `delta_ptr` (rt_trace_tile_work_delta) is a device array of
        tile_count(width, height) rt_tile_delta entries, 16-byte aligned: the entry of every listed tile
        with frames > 0 receives how far the call moved the tile's RGBA8 pixels (tile_delta_dtype)."""
        w = tile_work_array(work)
        c = RtCameraInfo()
        ctypes.pointer(c)[0] = cam
        c.CurrentImage = RtImage(cur_ptr, width, height, RT_FORMAT_R8G8B8A8_U32)
        c.PreviousImage = RtImage(prev_ptr, width, height, RT_FORMAT_R32B32G32A32_F32)
        d = RtTraceDesc(width, height, 0, 0, max_bounce, 1 if simd else 0, RT_SEED_PIXEL, band_rows, 1, 0,
                        (RT_FLAG_ACCUM_ZERO if accum_zero else 0) | (RT_FLAG_SRGB_POW if srgb_pow else 0))
        if delta_ptr:
            _check(lib().rt_trace_tile_work_delta(self.handle, ctypes.byref(c), ctypes.byref(d),
                                                  c_void_p(w.ctypes.data if w.size else None), int(w.shape[0]),
                                                  c_void_p(delta_ptr), c_void_p(rays_ptr), c_void_p(stream or 0)),
                   "rt_trace_tile_work_delta")
            return
        _check(lib().rt_trace_tile_work(self.handle, ctypes.byref(c), ctypes.byref(d),
                                        c_void_p(w.ctypes.data if w.size else None), int(w.shape[0]),
                                        c_void_p(rays_ptr), c_void_p(stream or 0)), "rt_trace_tile_work")

    def trace_tile_counts(self, cam: RtCameraInfo, *, tiles, counts_ptr: int, max_frames: int, width: int, height: int,
                          prev_ptr: int, cur_ptr: int, rays_ptr: int, delta_ptr: int = 0, max_bounce: int = 5,
                          simd: bool = True, band_rows: int = 32, accum_zero: bool = False, srgb_pow: bool = False,
                          stream: Optional[int] = None) -> None:
        """trace_tile_work() whose pairs live on the device (rt_trace_tile_counts): `tiles` lists the tiles
        that may be traced (the launch key, as trace_tiles), `counts_ptr` is a device table of
        tile_count(width, height) rt_tile_counts entries (tile_counts_dtype) read when the launch runs in
        stream order -- a listed tile folds min(Frames, max_frames) frames from its PreviousRayCount, and
        rests, untouched, at 0 -- and a non-zero `delta_ptr` receives the statistics of the tiles that
        folded a frame.  The host reads nothing back: a loop of this call and tile_counts_step() is
        enqueued without a host wait."""
        t = np.ascontiguousarray(np.asarray(list(tiles) if not isinstance(tiles, np.ndarray) else tiles).reshape(-1))
        if t.size and (t.dtype.kind not in "iu" or int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
            raise ValueError("tiles: a sequence of tile indices (non-negative integers)")
        if not 0 <= int(max_frames) <= 0xFFFFFFFF:
            raise ValueError("max_frames: a u32")
        t = t.astype(np.uint32)
        c = RtCameraInfo()
        ctypes.pointer(c)[0] = cam
        c.CurrentImage = RtImage(cur_ptr, width, height, RT_FORMAT_R8G8B8A8_U32)
        c.PreviousImage = RtImage(prev_ptr, width, height, RT_FORMAT_R32B32G32A32_F32)
        d = RtTraceDesc(width, height, 0, 0, max_bounce, 1 if simd else 0, RT_SEED_PIXEL, band_rows, 1, 0,
                        (RT_FLAG_ACCUM_ZERO if accum_zero else 0) | (RT_FLAG_SRGB_POW if srgb_pow else 0))
        _check(lib().rt_trace_tile_counts(self.handle, ctypes.byref(c), ctypes.byref(d),
                                          c_void_p(t.ctypes.data if t.size else None), int(t.size),
                                          c_void_p(counts_ptr or None), int(max_frames), c_void_p(delta_ptr or None),
                                          c_void_p(rays_ptr), c_void_p(stream or 0)), "rt_trace_tile_counts")

    def trace_first_hit(self, cam: RtCameraInfo, *, width: int, height: int, frame: int = 0, simd: bool = True,
                        centre: bool = False, tiles=None, hit_ptr: int = 0, normal_ptr: int = 0, albedo_ptr: int = 0,
                        stream: Optional[int] = 0) -> None:
        """What every pixel sees (rt_trace_first_hit): the first segment of frame `frame`'s primary ray --
        the ray trace() starts at prev_count == frame, or with `centre` the ray through the pixel centre --
        under the rule set `simd`.  `hit_ptr` (width * height first_hit_dtype entries: the sphere index,
        HIT_INSIDE in bit 31, or HIT_MISS; the distance), `normal_ptr` and `albedo_ptr` (width * height v4
        f32 each) are device pointers, each optional but not all.  `tiles` (None: every tile) lists the
        32 x 32 tiles to write, as trace_tiles; no other pixel is written.  Asynchronous on `stream`;
        nothing of the device's trace state changes."""
        t = None
        if tiles is not None:
            t = np.ascontiguousarray(np.asarray(list(tiles) if not isinstance(tiles, np.ndarray) else tiles).reshape(-1))
            if t.size and (t.dtype.kind not in "iu" or int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
                raise ValueError("tiles: a sequence of tile indices (non-negative integers)")
            t = t.astype(np.uint32)
        d = RtTraceDesc(width, height, frame, 0, 0, 1 if simd else 0, RT_SEED_PIXEL, 0, 1, 0, 0)
        planes = RtFirstHitPlanes(ctypes.sizeof(RtFirstHitPlanes), hit_ptr or None, normal_ptr or None, albedo_ptr or None)
        # (an empty list stays a list: a non-NULL pointer with n_tiles == 0 is "nothing to do", not "every tile")
        empty = np.zeros(1, np.uint32)
        ptr = None if t is None else (t.ctypes.data if t.size else empty.ctypes.data)
        _check(lib().rt_trace_first_hit(self.handle, ctypes.byref(cam), ctypes.byref(d), c_void_p(ptr),
                                        0 if t is None else int(t.size), HIT_PIXEL_CENTRE if centre else 0,
                                        ctypes.byref(planes), c_void_p(stream or 0)), "rt_trace_first_hit")

    def last_info(self) -> dict:
        """What the last trace launched (rt_trace_last_info): segments counted
        but folded analytically (dead tiles), P, tiles traced / total, whether
        the cull pass ran; plus "TileCounts" (rt_trace_last_tile_counts): 1 when the launch took
        per-tile counts, and "DirectionTable" (rt_trace_last_direction_table): 1 when its kernel chose
        the member entries by the direction table."""
        info = RtTraceInfo()
        _check(lib().rt_trace_last_info(self.handle, ctypes.byref(info)), "rt_trace_last_info")
        out = {n: int(getattr(info, n)) for n, _ in RtTraceInfo._fields_}
        tc = c_uint32(0)
        if hasattr(lib(), "rt_trace_last_tile_counts"):  # (an older A/B build, RT_TRACE_LIB, has no such launches)
            _check(lib().rt_trace_last_tile_counts(self.handle, ctypes.byref(tc)), "rt_trace_last_tile_counts")
        out["TileCounts"] = int(tc.value)
        dt = c_uint32(0)
        if hasattr(lib(), "rt_trace_last_direction_table"):  # (as above)
            _check(lib().rt_trace_last_direction_table(self.handle, ctypes.byref(dt)), "rt_trace_last_direction_table")
        out["DirectionTable"] = int(dt.value)
        return out

    def direction_union(self, words: np.ndarray, lanes: int, canary: np.ndarray):
        """rt_direction_union: the direction walk's union of 64 lane words (uint32 or uint64) with only the
        lanes of the bit mask `lanes` enabled -> (the union, the 64 canaries read back)."""
        words = np.ascontiguousarray(words)
        assert words.shape == (64,) and words.dtype in (np.uint32, np.uint64), (words.shape, words.dtype)
        canary = np.ascontiguousarray(canary, np.uint32)
        assert canary.shape == (64,)
        u = np.zeros(2, np.uint32)
        back = np.zeros(64, np.uint32)
        _check(lib().rt_direction_union(self.handle, words.ctypes.data, 8 * words.dtype.itemsize, int(lanes),
                                        canary.ctypes.data, u.ctypes.data, back.ctypes.data), "rt_direction_union")
        return int(u[0]) | (int(u[1]) << 32), back

    def reserve(self, width: int, local_rows: int) -> None:
        """rt_device_reserve: pre-size the launch buffers for bands up to width x local_rows."""
        _check(lib().rt_device_reserve(self.handle, width, local_rows), "rt_device_reserve")

    def debug_stats(self, reset: bool = True):
        """RT_STATS=1 scheduling counters (see rt_debug_stats), or None when disabled."""
        out = np.zeros(32, np.uint64)
        rc = lib().rt_debug_stats(self.handle, out.ctypes.data, int(reset))
        _check(rc, "rt_debug_stats")
        if rc == 0:
            return None
        keys = ["pri_iters", "pri_lanes", "sec_iters", "sec_lanes", "pri_groups", "sec_hit_groups",
                "sec_sparse_iters", "sec_sparse_lanes", "sec_tail_iters", "pri_cycles", "sec_cycles",
                "fold_cycles", "init_cycles", "cull_cycles", "sync_cycles", "post_cycles", "pf_iters", "pf_groups",
                "cl_tested", "pf_pairs", "cl_top_entered", "pf_lane_pairs", "pri_blocked", "pri_waitsec",
                "pri_done", "sec_done", "sec_waitpri", "done_trips", "done_lane_trips",
                "sec_exact", "sec_badlanes", "sec_zerodir"]
        return {k: int(v) for k, v in zip(keys, out) if not k.startswith("_")}

    def debug_wave_times(self, max_waves: int = 1 << 22):
        """RT_WAVETIMES=1: (n, 2) array of per-wave {start, end} (100 MHz ticks), or None."""
        out = np.zeros(2 * max_waves, np.uint64)
        n = int(lib().rt_debug_wave_times(self.handle, out.ctypes.data, max_waves))
        _check(n, "rt_debug_wave_times")
        return out[: 2 * n].reshape(-1, 2) if n else None

    def debug_masks(self, max_words: int = 1 << 24):
        """Primary group masks of the last cull pass (see rt_debug_masks), or None."""
        out = np.zeros(max_words, np.uint64)
        n = int(lib().rt_debug_masks(self.handle, out.ctypes.data, max_words))
        _check(n, "rt_debug_masks")
        return out[:n].copy() if n else None

    def synchronize(self) -> None:
        _check(lib().rt_device_synchronize(self.handle), "rt_device_synchronize")

    def close(self) -> None:
        if self.handle:
            lib().rt_device_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


class Multi:
    """Several GPUs from one process (rt_multi): interleaved row bands, one
    device each, gathered to devices[0] over RCCL or peer copies."""

    def __init__(self, devices, transport: int = RT_MULTI_AUTO, rsqrt_table: Optional[np.ndarray] = None,
                 options: Optional[dict] = None):
        devs = (c_int * len(devices))(*devices)
        h = c_void_p()
        o = device_options(options)
        _check(lib().rt_multi_create_ex(devs, len(devices), transport, ctypes.byref(o) if o is not None else None,
                                        ctypes.byref(h)), "rt_multi_create")
        self.handle = h
        table = rsqrt_table_builtin() if rsqrt_table is None else np.ascontiguousarray(rsqrt_table, np.float32)
        _check(lib().rt_multi_set_rsqrt_table(self.handle, table.ctypes.data), "rt_multi_set_rsqrt_table")

    def upload_scene(self, scene: RtScene) -> None:
        _check(lib().rt_multi_scene_upload(self.handle, ctypes.byref(scene)), "rt_multi_scene_upload")

    def trace(self, cam: RtCameraInfo, *, width: int, height: int, cur_ptr: int, rays_ptr: int, prev_ptr: int = 0,
              prev_count: int = 0, frames: int = 1, max_bounce: int = 5, simd: bool = True, band_rows: int = 8,
              accum_zero: bool = False, srgb_pow: bool = False, stream: Optional[int] = None) -> None:
        """Full-frame RGBA8 (and, with prev_ptr, the gathered running mean) on devices[0]."""
        c = RtCameraInfo()
        ctypes.pointer(c)[0] = cam
        c.CurrentImage = RtImage(cur_ptr, width, height, RT_FORMAT_R8G8B8A8_U32)
        c.PreviousImage = RtImage(prev_ptr or None, width, height, RT_FORMAT_R32B32G32A32_F32)
        d = RtTraceDesc(width, height, prev_count, frames, max_bounce, 1 if simd else 0, RT_SEED_PIXEL, band_rows, 0, 0,
                        (RT_FLAG_ACCUM_ZERO if accum_zero else 0) | (RT_FLAG_SRGB_POW if srgb_pow else 0))
        _check(lib().rt_multi_trace(self.handle, ctypes.byref(c), ctypes.byref(d), c_void_p(rays_ptr),
                                    c_void_p(stream or 0)), "rt_multi_trace")

    def last_trace_ms(self, n_devices: int) -> list:
        """Each device's trace time (ms) of the last trace call (waits for them)."""
        out = (c_float * n_devices)()
        _check(lib().rt_multi_last_trace_ms(self.handle, out, n_devices), "rt_multi_last_trace_ms")
        return [float(v) for v in out]

    def last_gather_ms(self) -> float:
        """The last call's gather (transfer + scatter) time on devices[0] (waits for it)."""
        ms = c_float(0.0)
        _check(lib().rt_multi_last_gather_ms(self.handle, ctypes.byref(ms)), "rt_multi_last_gather_ms")
        return float(ms.value)

    def shard_info(self, index: int) -> dict:
        """rt_trace_last_info of devices[index] for the last call."""
        info = RtTraceInfo()
        _check(lib().rt_multi_shard_info(self.handle, index, ctypes.byref(info)), "rt_multi_shard_info")
        return {n: int(getattr(info, n)) for n, _ in RtTraceInfo._fields_}

    def reserve(self, width: int, height: int, band_rows: int = 8, mean: bool = False) -> None:
        """rt_multi_reserve: pre-size every buffer a call of this geometry needs."""
        _check(lib().rt_multi_reserve(self.handle, width, height, band_rows, RT_MULTI_RESERVE_MEAN if mean else 0),
               "rt_multi_reserve")

    def resident_frames(self) -> int:
        """Frames folded into the devices' resident means (0: none resident, rt_multi_resident_frames)."""
        n = c_uint64(0)
        _check(lib().rt_multi_resident_frames(self.handle, ctypes.byref(n)), "rt_multi_resident_frames")
        return int(n.value)

    def info(self) -> dict:
        i = RtMultiInfo()
        _check(lib().rt_multi_get_info(self.handle, ctypes.byref(i)), "rt_multi_get_info")
        return {n: int(getattr(i, n)) for n, _ in RtMultiInfo._fields_}

    def synchronize(self) -> None:
        _check(lib().rt_multi_synchronize(self.handle), "rt_multi_synchronize")

    def close(self) -> None:
        if self.handle:
            lib().rt_multi_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(RT_COMM_ID_BYTES)
    _check(lib().rt_comm_unique_id(buf), "rt_comm_unique_id")
    return buf.raw


class Comm:
    """The RCCL band gather of a one-process-per-GPU launch (rt_comm)."""

    def __init__(self, device: int, uid: bytes, nranks: int, rank: int):
        assert len(uid) == RT_COMM_ID_BYTES
        h = c_void_p()
        buf = ctypes.create_string_buffer(uid, RT_COMM_ID_BYTES)
        _check(lib().rt_comm_create(device, buf, nranks, rank, ctypes.byref(h)), "rt_comm_create")
        self.handle = h

    def gather_bands(self, local_ptr: int, full_ptr: int, width: int, height: int, elem_bytes: int, band_rows: int,
                     stream: Optional[int] = None) -> None:
        _check(lib().rt_comm_gather_bands(self.handle, c_void_p(local_ptr or None), c_void_p(full_ptr or None), width,
                                          height, elem_bytes, band_rows, c_void_p(stream or 0)),
               "rt_comm_gather_bands")

    def close(self) -> None:
        if self.handle:
            lib().rt_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


def assemble_bands(compact_ptr: int, rank_stride_bytes: int, dst_ptr: int, width: int, height: int,
                   elem_bytes: int, band_rows: int, band_count: int, stream: Optional[int] = None) -> None:
    _check(lib().rt_assemble_bands(c_void_p(compact_ptr), rank_stride_bytes, c_void_p(dst_ptr), width, height,
                                   elem_bytes, band_rows, band_count, c_void_p(stream or 0)),
           "rt_assemble_bands")


def encode_rgba8(accum_ptr: int, rgba8_ptr: int, n_pixels: int, srgb_pow: bool = False,
                 stream: Optional[int] = None) -> None:
    """ColorFromV4(LinearToSRGB(v)) over a device-resident running mean (main.cpp:312-346)."""
    _check(lib().rt_encode_rgba8(c_void_p(accum_ptr), c_void_p(rgba8_ptr), n_pixels,
                                 RT_FLAG_SRGB_POW if srgb_pow else 0, c_void_p(stream or 0)), "rt_encode_rgba8")


def tile_rule(max_round_frames: int, max_tile_frames: int, rest_max_delta: int = 0,
              rest_sum_squares: int = 0xFFFFFFFF) -> RtTileRule:
    """An rt_tile_rule with its Size set."""
    return RtTileRule(ctypes.sizeof(RtTileRule), max_round_frames, max_tile_frames, rest_max_delta, rest_sum_squares)


def tile_counts_step(counts_ptr: int, delta_ptr: int, width: int, height: int, rule: RtTileRule, summary_ptr: int = 0,
                     stream: Optional[int] = None) -> None:
    """rt_tile_counts_step: advances the device table `counts_ptr` (tile_count(width, height) rt_tile_counts
    entries) by the round Device.trace_tile_counts(max_frames=rule.MaxRoundFrames, delta_ptr=...) just
    traced and decides every tile's next one by `rule` (tile_rule()); a non-zero `summary_ptr` (16 B of
    device memory, tile_step_summary_dtype) receives the next round's frames, active tiles and the tiles
    put to rest.  Enqueued on `stream`; nothing is read back."""
    _check(lib().rt_tile_counts_step(c_void_p(counts_ptr or None), c_void_p(delta_ptr or None), width, height,
                                     ctypes.byref(rule), c_void_p(summary_ptr or None), c_void_p(stream or 0)),
           "rt_tile_counts_step")


def tile_delta_rgba8(old_ptr: int, new_ptr: int, width: int, height: int, delta_ptr: int,
                     stream: Optional[int] = None) -> None:
    """rt_tile_delta_rgba8: per-tile change statistics between two device RGBA8 images (width x height
    u32 each) into the device array `delta_ptr` (tile_count(width, height) rt_tile_delta entries,
    16-byte aligned; view a copy with tile_delta_dtype).  Traces nothing."""
    _check(lib().rt_tile_delta_rgba8(c_void_p(old_ptr), c_void_p(new_ptr), width, height, c_void_p(delta_ptr),
                                     c_void_p(stream or 0)), "rt_tile_delta_rgba8")


def denoise_defaults() -> dict:
    """rt_denoise_defaults: the library's Iterations, NormalPower, SigmaDepth and SigmaColor."""
    d = RtDenoiseDesc()
    _check(lib().rt_denoise_defaults(ctypes.byref(d)), "rt_denoise_defaults")
    assert d.Size == ctypes.sizeof(RtDenoiseDesc)
    return dict(iterations=d.Iterations, normal_power=d.NormalPower, sigma_depth=d.SigmaDepth, sigma_color=d.SigmaColor)


def denoise(width: int, height: int, mean_ptr: int, hit_ptr: int, out_ptr: int, scratch_ptr: int = 0,
            normal_ptr: int = 0, albedo_ptr: int = 0, rgba8_ptr: int = 0, iterations: Optional[int] = None,
            normal_power: Optional[int] = None, sigma_depth: Optional[float] = None,
            sigma_color: Optional[float] = None, demodulate: bool = False, srgb_pow: bool = False,
            stream: Optional[int] = None) -> None:
    """rt_denoise: the edge-avoiding a-trous filter of the device running mean `mean_ptr` (width * height v4 f32)
    guided by Device.trace_first_hit's planes of the same frame (`hit_ptr` always; `normal_ptr` when the normal
    stop is on; `albedo_ptr` with `demodulate`), into `out_ptr` and, when non-zero, its RGBA8 into `rgba8_ptr`.
    `scratch_ptr` (another width * height v4 f32) is needed from two iterations on.  iterations, normal_power,
    sigma_depth, sigma_color: None takes the library's default (denoise_defaults()); 0 turns a stop off.
    Enqueued on `stream`; needs no Device.  ValueError for a count or a width no call can take, RtError for
    what the library refuses."""
    dflt = denoise_defaults()
    it = dflt["iterations"] if iterations is None else iterations
    k = dflt["normal_power"] if normal_power is None else normal_power
    sd = dflt["sigma_depth"] if sigma_depth is None else sigma_depth
    sc = dflt["sigma_color"] if sigma_color is None else sigma_color
    for name, v, hi in (("iterations", it, DENOISE_MAX_ITERATIONS), ("normal_power", k, 8)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= hi:
            raise ValueError(f"denoise: {name} must be an integer of at most {hi}, got {v!r}")
    if int(it) < 1:
        raise ValueError("denoise: iterations must be at least 1")
    for name, v in (("sigma_depth", sd), ("sigma_color", sc)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) < float("inf"):
            raise ValueError(f"denoise: {name} must be a finite number >= 0, got {v!r}")
        if float(v) > float(np.finfo(np.float32).max):
            raise ValueError(f"denoise: {name} {v!r} is not a finite f32")
    flags = (DENOISE_DEMODULATE if demodulate else 0) | (DENOISE_SRGB_POW if srgb_pow else 0)
    d = RtDenoiseDesc(ctypes.sizeof(RtDenoiseDesc), width, height, int(it), flags, int(k), float(sd), float(sc),
                      mean_ptr or None, hit_ptr or None, normal_ptr or None, albedo_ptr or None, out_ptr or None,
                      scratch_ptr or None, rgba8_ptr or None)
    _check(lib().rt_denoise(ctypes.byref(d), c_void_p(stream or 0)), "rt_denoise")


def reproject_defaults() -> dict:
    """rt_reproject_defaults: the library's Frames, MaxHistory and DepthTolerance."""
    d = RtReprojectDesc()
    _check(lib().rt_reproject_defaults(ctypes.byref(d)), "rt_reproject_defaults")
    assert d.Size == ctypes.sizeof(RtReprojectDesc)
    return dict(frames=d.Frames, max_history=d.MaxHistory, depth_tolerance=d.DepthTolerance)


def reproject(width: int, height: int, camera: RtCameraInfo, previous_camera: RtCameraInfo, mean_ptr: int, hit_ptr: int,
              out_ptr: int, out_count_ptr: int, history_ptr: int = 0, history_hit_ptr: int = 0,
              history_count_ptr: int = 0, rgba8_ptr: int = 0, frames: int = 1, max_history: Optional[int] = None,
              depth_tolerance: Optional[float] = None, srgb_pow: bool = False, stream: Optional[int] = None) -> None:
    """rt_reproject: carries the accumulated frame `history_ptr` (width * height v4 f32, with its first-hit plane
    `history_hit_ptr` and its per-pixel frame counts `history_count_ptr`, all seen from `previous_camera`) to
    `camera` and folds the fresh mean `mean_ptr` of `frames` frames into it, guided by Device.trace_first_hit's
    centre=True plane `hit_ptr` at `camera`: the result into `out_ptr`, its frame counts into `out_count_ptr` (u32)
    and, when non-zero, its RGBA8 into `rgba8_ptr`.  The three history pointers are 0 together on a loop's first
    frame.  max_history, depth_tolerance: None takes the library's default (reproject_defaults()); a
    depth_tolerance of 0 turns the depth test off.  Enqueued on `stream`; needs no Device.  ValueError for a count
    or a tolerance no call can take, RtError for what the library refuses."""
    d = _reproject_desc("reproject", width, height, camera, previous_camera, mean_ptr, hit_ptr, out_ptr, out_count_ptr,
                        history_ptr, history_hit_ptr, history_count_ptr, rgba8_ptr, frames, max_history,
                        depth_tolerance, srgb_pow)
    _check(lib().rt_reproject(ctypes.byref(d), c_void_p(stream or 0)), "rt_reproject")


def _reproject_desc(who, width, height, camera, previous_camera, mean_ptr, hit_ptr, out_ptr, out_count_ptr, history_ptr,
                    history_hit_ptr, history_count_ptr, rgba8_ptr, frames, max_history, depth_tolerance, srgb_pow):
    """The rt_reproject_desc of reproject() and reproject_clip(), with the wrapper's own checks (`who` names the
    caller in their texts).  The desc points at `camera` and `previous_camera`: they must outlive it."""
    dflt = reproject_defaults()
    cap = dflt["max_history"] if max_history is None else max_history
    tol = dflt["depth_tolerance"] if depth_tolerance is None else depth_tolerance
    for name, v in (("frames", frames), ("max_history", cap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{who}: {name} must be an integer in 1..2^32-1, got {v!r}")
    if int(cap) < int(frames):
        raise ValueError(f"{who}: max_history {cap!r} is below frames {frames!r}")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not 0.0 <= float(tol) < float("inf"):
        raise ValueError(f"{who}: depth_tolerance must be a finite number >= 0, got {tol!r}")
    if float(tol) > float(np.finfo(np.float32).max):
        raise ValueError(f"{who}: depth_tolerance {tol!r} is not a finite f32")
    for name, c in (("camera", camera), ("previous_camera", previous_camera)):
        if not isinstance(c, RtCameraInfo):
            raise ValueError(f"{who}: {name} must be an RtCameraInfo (camera_setup), got {type(c).__name__}")
    d = RtReprojectDesc(ctypes.sizeof(RtReprojectDesc), width, height, int(frames), int(cap),
                        REPROJECT_SRGB_POW if srgb_pow else 0, float(tol), ctypes.pointer(camera),
                        ctypes.pointer(previous_camera), mean_ptr or None, hit_ptr or None, history_ptr or None,
                        history_hit_ptr or None, history_count_ptr or None, out_ptr or None, out_count_ptr or None,
                        rgba8_ptr or None)
    return d


def reproject_clip_defaults() -> dict:
    """rt_reproject_clip_defaults: the library's Radius and Gamma, and rt_reproject_defaults' values."""
    d = RtReprojectClipDesc()
    _check(lib().rt_reproject_clip_defaults(ctypes.byref(d)), "rt_reproject_clip_defaults")
    assert d.Size == ctypes.sizeof(RtReprojectClipDesc) and d.Reproject.Size == ctypes.sizeof(RtReprojectDesc)
    return dict(radius=d.Radius, gamma=d.Gamma, frames=d.Reproject.Frames, max_history=d.Reproject.MaxHistory,
                depth_tolerance=d.Reproject.DepthTolerance)


def reproject_clip(width: int, height: int, camera: RtCameraInfo, previous_camera: RtCameraInfo, mean_ptr: int,
                   hit_ptr: int, out_ptr: int, out_count_ptr: int, history_ptr: int = 0, history_hit_ptr: int = 0,
                   history_count_ptr: int = 0, rgba8_ptr: int = 0, frames: int = 1, max_history: Optional[int] = None,
                   depth_tolerance: Optional[float] = None, srgb_pow: bool = False, radius: Optional[int] = None,
                   gamma: Optional[float] = None, stream: Optional[int] = None) -> None:
    """rt_reproject_clip: reproject() with the gathered history clamped, per channel, to mean +- `gamma` standard
    deviations of the fresh frame's pixels of the same sphere in a (2 * radius + 1)^2 window, before the fold: what
    a mirror or glass showed from the previous camera is pulled towards what it shows now.  Every other argument is
    reproject()'s.  radius (1..3), gamma (finite, > 0): None takes the library's default
    (reproject_clip_defaults())."""
    dflt = reproject_clip_defaults()
    r = dflt["radius"] if radius is None else radius
    g = dflt["gamma"] if gamma is None else gamma
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= int(r) <= 3:
        raise ValueError(f"reproject_clip: radius must be an integer in 1..3, got {r!r}")
    if isinstance(g, bool) or not isinstance(g, (int, float, np.integer, np.floating)) or not 0.0 < float(g) < float("inf"):
        raise ValueError(f"reproject_clip: gamma must be a finite number > 0, got {g!r}")
    if float(g) > float(np.finfo(np.float32).max) or float(np.float32(min(float(g), 1.0))) == 0.0:
        raise ValueError(f"reproject_clip: gamma {g!r} is not a finite f32 above 0")
    inner = _reproject_desc("reproject_clip", width, height, camera, previous_camera, mean_ptr, hit_ptr, out_ptr,
                            out_count_ptr, history_ptr, history_hit_ptr, history_count_ptr, rgba8_ptr, frames,
                            max_history, depth_tolerance, srgb_pow)
    d = RtReprojectClipDesc(ctypes.sizeof(RtReprojectClipDesc), int(r), float(g), inner)
    _check(lib().rt_reproject_clip(ctypes.byref(d), c_void_p(stream or 0)), "rt_reproject_clip")


# ------------------------------------------------- OnInit / OnRender mirror
def on_init(devices=None) -> RtInitParams:
    """OnInit; `devices` (a list of HIP ordinals) drives several GPUs through rt_multi."""
    p = RtInitParams()
    if devices is None:
        _check(lib().rt_on_init(ctypes.byref(p)), "rt_on_init")
    else:
        devs = (c_int * len(devices))(*devices)
        _check(lib().rt_on_init_devices(ctypes.byref(p), devs, len(devices)), "rt_on_init_devices")
    return p


def on_render(image: np.ndarray, scene_index: int, enable_simd: bool = True, keys: int = 0):
    """OnRender(Image, RenderParams, &Rays, &Time): `image` is an (H, W) uint32
    RGBA8 host array.  Returns (completed, total_rays_cast, time_elapsed_ms)."""
    assert image.dtype == np.uint32 and image.ndim == 2 and image.flags.c_contiguous
    img = RtImage(image.ctypes.data, image.shape[1], image.shape[0], RT_FORMAT_R8G8B8A8_U32)
    rays = c_uint64(0)
    ms = c_double(0.0)
    rc = lib().rt_on_render(ctypes.byref(img), RtRenderParams(0, enable_simd, scene_index), keys,
                            ctypes.byref(rays), ctypes.byref(ms))
    _check(rc, "rt_on_render")
    return bool(rc), int(rays.value), float(ms.value)


def on_render_register_image(image: np.ndarray) -> None:
    """rt_on_render_register_image: page-lock `image` so frames handed to it
    arrive by one DMA; keep it alive until on_render_unregister_image()."""
    assert image.dtype == np.uint32 and image.flags.c_contiguous
    _check(lib().rt_on_render_register_image(c_void_p(image.ctypes.data), c_uint64(image.nbytes)),
           "rt_on_render_register_image")


def on_render_unregister_image() -> None:
    _check(lib().rt_on_render_unregister_image(), "rt_on_render_unregister_image")


def on_render_reserve(width: int, height: int) -> None:
    """rt_on_render_reserve: frames up to width x height need no allocation in the frame loop."""
    _check(lib().rt_on_render_reserve(width, height), "rt_on_render_reserve")


def on_render_wait() -> None:
    _check(lib().rt_on_render_wait(), "rt_on_render_wait")


def on_shutdown() -> None:
    _check(lib().rt_on_shutdown(), "rt_on_shutdown")


def on_render_profile(reset: bool = False) -> dict:
    """Where rt_on_render's time went (rt_on_render_get_profile): calls, frames
    launched / handed out, host ms in the call, its frame copies and waits,
    and the frames' GPU time."""
    p = RtOnRenderProfile()
    _check(lib().rt_on_render_get_profile(ctypes.byref(p), int(reset)), "rt_on_render_get_profile")
    return {n: (int(getattr(p, n)) if t is c_uint64 else float(getattr(p, n))) for n, t in RtOnRenderProfile._fields_}


# ------------------------------------------------------------ output path
RT_IMAGE_FLIP_Y = 1


def write_image(image: np.ndarray, path, flip_y: bool = True) -> None:
    """Writes an (H, W) uint32 RGBA8 host frame (rt_on_render / rt_trace's
    CurrentImage) as PPM or PNG by the path's suffix (rt_image_write_ppm /
    rt_image_write_png); flip_y: on-screen orientation (row H-1 first)."""
    assert image.dtype == np.uint32 and image.ndim == 2 and image.flags.c_contiguous
    img = RtImage(image.ctypes.data, image.shape[1], image.shape[0], RT_FORMAT_R8G8B8A8_U32)
    path = str(path)
    fn = lib().rt_image_write_png if path.lower().endswith(".png") else lib().rt_image_write_ppm
    name = "rt_image_write_png" if path.lower().endswith(".png") else "rt_image_write_ppm"
    _check(fn(ctypes.byref(img), path.encode(), RT_IMAGE_FLIP_Y if flip_y else 0), name)


def code_object_hash(path=None) -> str:
    """SHA-256 (first 16 hex digits) of the gfx950 code objects a library
    carries: the bytes of its ELF `.hip_fatbin` section (every kernel
    translation unit's offload bundle).  Host-only changes leave it alone; any
    kernel change moves it.  bench.py uses a committed PMC record only when
    the record's `binary_hash` equals the loaded library's.  Reads the file
    (no GPU, no load)."""
    import hashlib
    import struct
    data = pathlib.Path(path or LIB_PATH).read_bytes()
    if data[:4] != b"\x7fELF" or data[4] != 2:
        raise RtError(f"{path or LIB_PATH}: not an ELF64 file")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize) for i in range(shnum)]
    stroff = secs[shstrndx][4]
    for name, _, _, _, off, size in secs:
        end = data.index(b"\0", stroff + name)
        if data[stroff + name:end] == b".hip_fatbin":
            return hashlib.sha256(data[off:off + size]).hexdigest()[:16]
    raise RtError(f"{path or LIB_PATH}: no .hip_fatbin section")


def frame_hash(a) -> int:
    """FNV-1a 64 of a host array's bytes (rt_frame_hash): the golden fixtures' frame checksum."""
    a = np.ascontiguousarray(a)
    return int(lib().rt_frame_hash(c_void_p(a.ctypes.data), a.nbytes))
