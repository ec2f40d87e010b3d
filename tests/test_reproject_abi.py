"""CPU-side checks of rt_reproject's interface (no GPU needed): a C99 unit compiled against the header has
rt_reproject_desc's offsets and size and the flag; the ctypes mirror agrees with the C compiler; both symbols are in
SIGNATURES and the library exports them; rt_reproject_defaults fills what the header documents; the refusals, which
need no device, return RT_EINVAL through the library itself; and the Python wrapper checks its counts, tolerance
and cameras before it calls."""
import ctypes
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_trace.h"
EINVAL = -22
SIZE = 112
OFFSETS = [("Size", 0), ("Width", 4), ("Height", 8), ("Frames", 12), ("MaxHistory", 16), ("Flags", 20),
           ("DepthTolerance", 24), ("Camera", 32), ("PreviousCamera", 40), ("Mean", 48), ("Hit", 56), ("History", 64),
           ("HistoryHit", 72), ("HistoryCount", 80), ("Out", 88), ("OutCount", 96), ("Rgba8", 104)]
DEFAULTS = dict(frames=1, max_history=8, depth_tolerance=float(np.float32(0.1)))
POINTERS = ("Camera", "PreviousCamera", "Mean", "Hit", "History", "HistoryHit", "HistoryCount", "Out", "OutCount", "Rgba8")


def _cc():
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler (build() needs one too)"
    return cc


def _compile(tmp_path, body):
    src = tmp_path / "reproject_layout.c"
    src.write_text("#include <stddef.h>\n#include \"rt_trace.h\"\n" + body + "\n")
    return subprocess.run([_cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(HEADER.parent),
                           str(src)], capture_output=True, text=True)


# C99 has no _Static_assert: a negative array size is the failed assertion
def _assert(name, cond):
    return f"typedef char {name}[({cond}) ? 1 : -1];"


def test_c99_layout_and_constants(rt, tmp_path):
    lines = [_assert("size_desc", f"sizeof(rt_reproject_desc) == {SIZE}")]
    lines += [_assert("off_" + n.lower(), f"offsetof(rt_reproject_desc, {n}) == {o}") for n, o in OFFSETS]
    lines += [_assert("c_pow", "RT_REPROJECT_SRGB_POW == 2u"),
              _assert("c_pow_is_the_trace_flag", "RT_REPROJECT_SRGB_POW == RT_FLAG_SRGB_POW"),
              # the call as a C host writes it: a frame of a loop
              "int carry(const rt_camera_info *cam, const rt_camera_info *prev, const float *d_mean,",
              "          const rt_first_hit *d_hit, const float *d_history, const rt_first_hit *d_history_hit,",
              "          const uint32_t *d_history_count, float *d_out, uint32_t *d_out_count, uint32_t *d_rgba8) {",
              "    rt_reproject_desc d;",
              "    if (rt_reproject_defaults(&d) != RT_OK) return -1;",
              "    d.Width = 1920; d.Height = 1080; d.Camera = cam; d.PreviousCamera = prev;",
              "    d.Mean = d_mean; d.Hit = d_hit; d.History = d_history; d.HistoryHit = d_history_hit;",
              "    d.HistoryCount = d_history_count; d.Out = d_out; d.OutCount = d_out_count; d.Rgba8 = d_rgba8;",
              "    return rt_reproject(&d, NULL);",
              "}"]
    r = _compile(tmp_path, "\n".join(lines))
    assert r.returncode == 0, r.stderr
    # a wrong value is caught (the check above is not vacuous)
    assert _compile(tmp_path, _assert("wrong_on_purpose", "offsetof(rt_reproject_desc, Camera) == 28")).returncode != 0
    assert _compile(tmp_path, _assert("wrong_on_purpose", "RT_REPROJECT_SRGB_POW == 1u")).returncode != 0


def test_ctypes_mirror_agrees(rt):
    assert ctypes.sizeof(rt.RtReprojectDesc) == SIZE
    assert [(n, getattr(rt.RtReprojectDesc, n).offset) for n, _ in rt.RtReprojectDesc._fields_] == OFFSETS
    assert rt.REPROJECT_SRGB_POW == 2 == rt.RT_FLAG_SRGB_POW
    m = re.search(r"#define\s+RT_REPROJECT_SRGB_POW\s+(0x[0-9A-Fa-f]+|\d+)u", HEADER.read_text())
    assert m and int(m.group(1), 0) == 2


def test_header_and_library_carry_the_entry_points(rt):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ws = lambda s: re.sub(r"\s+", r"\\s*", re.escape(s).replace(r"\ ", " "))  # noqa: E731
    assert re.search(ws("int rt_reproject(const rt_reproject_desc *desc, void *stream)"), code)
    assert re.search(ws("int rt_reproject_defaults(rt_reproject_desc *out)"), code)
    # after the rt_denoise block, as the interface grew
    assert code.index("int rt_denoise_defaults(") < code.index("int rt_reproject(") < code.index("rt_trace_last_info(")
    for name, n_args in (("rt_reproject", 2), ("rt_reproject_defaults", 1)):
        assert name in rt.SIGNATURES and len(rt.SIGNATURES[name][1]) == n_args
        assert rt.SIGNATURES[name][0] is ctypes.c_int and hasattr(rt.lib(), name)
    # the definition is in the header, step by step
    text = HEADER.read_text()
    doc = text[text.index("typedef struct rt_reproject_desc"):text.index("int rt_reproject(const")]
    for word in ("dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z", "ff = dot3(fv, fv)", "qx = (u / d) * ff",
                 "x0 = floorf(sx)", "n = min(n, HistoryCount[q])", "Out.ch = H.ch + (Mean.ch - H.ch) * a",
                 "OutCount = min(n + Frames, MaxHistory)", "Out.w = Mean[p].w"):
        assert word in doc, word


def test_defaults(rt):
    L = rt.lib()
    d = rt.RtReprojectDesc()
    ctypes.memset(ctypes.byref(d), 0xA5, ctypes.sizeof(d))
    assert L.rt_reproject_defaults(ctypes.byref(d)) == 0
    assert d.Size == SIZE and (d.Width, d.Height, d.Flags) == (0, 0, 0)
    assert (d.Frames, d.MaxHistory, d.DepthTolerance) == tuple(DEFAULTS.values())
    assert not d.Camera and not d.PreviousCamera
    assert all(getattr(d, n) is None for n in POINTERS[2:])
    assert rt.reproject_defaults() == DEFAULTS
    assert L.rt_reproject_defaults(None) == EINVAL and b"rt_reproject_defaults: NULL argument" in L.rt_last_error()
    # the header documents them
    text = HEADER.read_text()
    doc = text[text.index("int rt_reproject(const"):text.index("int rt_reproject_defaults(")]
    for word in ("Frames = 1", "MaxHistory = 8", "DepthTolerance = 0.1f"):
        assert word in doc, word


def _desc(rt, base, cams, **kw):
    """A desc the library accepts up to the launch (never reached here: each case below is refused first)."""
    d = rt.RtReprojectDesc(SIZE, 64, 48, 1, 8, 0, 0.1, ctypes.pointer(cams[0]), ctypes.pointer(cams[1]), base, base + 64,
                           base + 128, base + 192, base + 256, base + 320, base + 384, base + 448)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_refusals_through_the_library(rt):
    """Every refusal comes before anything is enqueued, so it needs no device: the plane pointers are host
    addresses, compared and never followed."""
    L = rt.lib()
    buf = (ctypes.c_uint8 * 640)()
    base = (ctypes.addressof(buf) + 15) & ~15
    scene = rt.scene_builtin(0)
    cams = (rt.camera_setup(scene, 64, 48), rt.camera_setup(scene, 64, 48, x_angle=scene.DefaultXAngle + 1 / 16))
    nan, inf = float("nan"), float("inf")
    no_cam = ctypes.POINTER(rt.RtCameraInfo)()
    cases = [(dict(Size=104), b"Size 104"), (dict(Width=0), b"bad image size"), (dict(Height=65537), b"bad image size"),
             (dict(Frames=0), b"Frames is 0"), (dict(Frames=9), b"MaxHistory 8 is below Frames 9"),
             (dict(MaxHistory=0), b"MaxHistory 0 is below Frames 1"), (dict(Flags=1), b"unknown flags 0x1"),
             (dict(Flags=6), b"unknown flags 0x6"), (dict(DepthTolerance=-1.0), b"DepthTolerance"),
             (dict(DepthTolerance=nan), b"DepthTolerance"), (dict(DepthTolerance=inf), b"DepthTolerance"),
             (dict(Camera=no_cam), b"Camera is NULL"), (dict(PreviousCamera=no_cam), b"PreviousCamera is NULL"),
             (dict(Mean=None), b"Mean is NULL"), (dict(Hit=None), b"Hit is NULL"), (dict(Out=None), b"Out is NULL"),
             (dict(OutCount=None), b"OutCount is NULL"), (dict(History=None), b"all NULL or all given"),
             (dict(HistoryHit=None), b"all NULL or all given"), (dict(HistoryCount=None), b"all NULL or all given"),
             (dict(History=None, HistoryHit=None), b"all NULL or all given"),
             (dict(Mean=base + 8), b"Mean is not 16-byte"), (dict(Hit=base + 68), b"Hit is not 8-byte"),
             (dict(History=base + 136), b"History is not 16-byte"), (dict(HistoryHit=base + 196), b"HistoryHit is not 8-byte"),
             (dict(HistoryCount=base + 258), b"HistoryCount is not 4-byte"), (dict(Out=base + 328), b"Out is not 16-byte"),
             (dict(OutCount=base + 385), b"OutCount is not 4-byte"), (dict(Rgba8=base + 450), b"Rgba8 is not 4-byte"),
             (dict(Out=base), b"Out is Mean"), (dict(Out=base + 128), b"Out is History"),
             (dict(OutCount=base + 256), b"OutCount is HistoryCount")]
    for kw, text in cases:
        assert L.rt_reproject(ctypes.byref(_desc(rt, base, cams, **kw)), None) == EINVAL, kw
        assert text in L.rt_last_error(), (kw, L.rt_last_error())
    assert L.rt_reproject(None, None) == EINVAL and b"rt_reproject: NULL argument" in L.rt_last_error()


def test_wrapper_checks_its_arguments(rt):
    buf = (ctypes.c_uint8 * 640)()
    base = (ctypes.addressof(buf) + 15) & ~15
    scene = rt.scene_builtin(0)
    cam = rt.camera_setup(scene, 64, 48)
    ok = dict(width=64, height=48, camera=cam, previous_camera=cam, mean_ptr=base, hit_ptr=base + 64, out_ptr=base + 320,
              out_count_ptr=base + 384)
    for bad in (dict(frames=0), dict(frames=1.0), dict(frames=True), dict(frames="1"), dict(frames=2 ** 32),
                dict(max_history=0), dict(max_history=8.0), dict(max_history=-1), dict(frames=9), dict(frames=3, max_history=2),
                dict(depth_tolerance=-0.5), dict(depth_tolerance=float("nan")), dict(depth_tolerance=float("inf")),
                dict(depth_tolerance="0.1"), dict(depth_tolerance=1e39), dict(depth_tolerance=np.float64(-1e-9)),
                dict(depth_tolerance=False), dict(camera=None), dict(previous_camera=rt.camera_floats(cam))):
        with pytest.raises(ValueError, match="reproject: "):
            rt.reproject(**{**ok, **bad})
    # what the wrapper lets through, the library refuses
    with pytest.raises(rt.RtError, match="all NULL or all given"):
        rt.reproject(**ok, history_ptr=base + 128)
    with pytest.raises(rt.RtError, match="Out is Mean"):
        rt.reproject(**{**ok, "out_ptr": base}, frames=np.int64(2), max_history=np.uint32(4))
    with pytest.raises(rt.RtError, match="OutCount is HistoryCount"):
        rt.reproject(**ok, history_ptr=base + 128, history_hit_ptr=base + 192, history_count_ptr=base + 384)
    with pytest.raises(rt.RtError, match="bad image size"):
        rt.reproject(**{**ok, "width": 0})
