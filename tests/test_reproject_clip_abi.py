"""CPU-side checks of rt_reproject_clip's interface (no GPU needed): a C99 unit compiled against the header has
rt_reproject_clip_desc's offsets and size; the ctypes mirror agrees with the C compiler; the symbols are in SIGNATURES
and the library exports them; rt_reproject_clip_defaults fills what the header documents; every refusal returns
RT_EINVAL with its rt_last_error text through the library itself, before anything is enqueued (the plane pointers
are host addresses here: a call that got as far as a launch would not return RT_EINVAL, and no HIP device is opened
by a refused call); and the Python wrapper checks its radius and gamma before it calls."""
import ctypes
import re

import numpy as np
import pytest

from test_reproject_abi import EINVAL, HEADER, _assert, _compile
from test_reproject_abi import SIZE as INNER_SIZE

SIZE = 128
OFFSETS = [("Size", 0), ("Radius", 4), ("Gamma", 8), ("Reproject", 16)]
DEFAULTS = dict(radius=1, gamma=0.5, frames=1, max_history=8, depth_tolerance=float(np.float32(0.1)))


def test_c99_layout(rt, tmp_path):
    lines = [_assert("size_desc", f"sizeof(rt_reproject_clip_desc) == {SIZE}"),
             _assert("size_inner", f"sizeof(rt_reproject_desc) == {INNER_SIZE}")]
    lines += [_assert("off_" + n.lower(), f"offsetof(rt_reproject_clip_desc, {n}) == {o}") for n, o in OFFSETS]
    lines += [_assert("off_inner_size", "offsetof(rt_reproject_clip_desc, Reproject.Size) == 16"),
              _assert("off_inner_rgba8", "offsetof(rt_reproject_clip_desc, Reproject.Rgba8) == 120"),
              # the call as a C host writes it: rt_reproject's frame of a loop with the clamp
              "int carry(const rt_camera_info *cam, const rt_camera_info *prev, const float *d_mean,",
              "          const rt_first_hit *d_hit, const float *d_history, const rt_first_hit *d_history_hit,",
              "          const uint32_t *d_history_count, float *d_out, uint32_t *d_out_count) {",
              "    rt_reproject_clip_desc d;",
              "    if (rt_reproject_clip_defaults(&d) != RT_OK) return -1;",
              "    d.Radius = 2; d.Gamma = 1.0f;",
              "    d.Reproject.Width = 1920; d.Reproject.Height = 1080; d.Reproject.Camera = cam;",
              "    d.Reproject.PreviousCamera = prev; d.Reproject.Mean = d_mean; d.Reproject.Hit = d_hit;",
              "    d.Reproject.History = d_history; d.Reproject.HistoryHit = d_history_hit;",
              "    d.Reproject.HistoryCount = d_history_count; d.Reproject.Out = d_out; d.Reproject.OutCount = d_out_count;",
              "    return rt_reproject_clip(&d, NULL);",
              "}"]
    r = _compile(tmp_path, "\n".join(lines))
    assert r.returncode == 0, r.stderr
    # a wrong value is caught (the check above is not vacuous)
    assert _compile(tmp_path, _assert("wrong_on_purpose", "offsetof(rt_reproject_clip_desc, Reproject) == 12")).returncode != 0
    assert _compile(tmp_path, _assert("wrong_on_purpose", "sizeof(rt_reproject_clip_desc) == 124")).returncode != 0


def test_ctypes_mirror_agrees(rt):
    assert ctypes.sizeof(rt.RtReprojectClipDesc) == SIZE
    assert [(n, getattr(rt.RtReprojectClipDesc, n).offset) for n, _ in rt.RtReprojectClipDesc._fields_] == OFFSETS
    assert dict(rt.RtReprojectClipDesc._fields_)["Reproject"] is rt.RtReprojectDesc


def test_header_and_library_carry_the_entry_points(rt):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ws = lambda s: re.sub(r"\s+", r"\\s*", re.escape(s).replace(r"\ ", " "))  # noqa: E731
    assert re.search(ws("int rt_reproject_clip(const rt_reproject_clip_desc *desc, void *stream)"), code)
    assert re.search(ws("int rt_reproject_clip_defaults(rt_reproject_clip_desc *out)"), code)
    # after the rt_reproject block, as the interface grew
    assert code.index("int rt_reproject_defaults(") < code.index("int rt_reproject_clip(") < code.index("rt_trace_last_info(")
    for name, n_args in (("rt_reproject_clip", 2), ("rt_reproject_clip_defaults", 1)):
        assert name in rt.SIGNATURES and len(rt.SIGNATURES[name][1]) == n_args
        assert rt.SIGNATURES[name][0] is ctypes.c_int and hasattr(rt.lib(), name)
    # the definition is in the header, step by step, and says what an isolated pixel gets
    text = HEADER.read_text()
    doc = text[text.index("typedef struct rt_reproject_clip_desc"):text.index("int rt_reproject_clip(const")]
    for word in ("dy = -R..R (outer), dx = -R..R (inner)", "Hit[q].Key != kp", "s1.ch = s1.ch + c.ch",
                 "s2.ch = s2.ch + c.ch * c.ch", "nf = nf + 1.0f", "m.ch = s1.ch / nf", "v.ch = pos(s2.ch / nf - m.ch * m.ch)",
                 "sd.ch = sqrtf(v.ch)", "lo.ch = m.ch - Gamma * sd.ch", "hi.ch = m.ch + Gamma * sd.ch",
                 "if (H.ch < lo.ch) H.ch = lo.ch; if (H.ch > hi.ch) H.ch = hi.ch", "nf == 0: no clamp",
                 "its history becomes its fresh value", "OutCount does not\n * depend on the clamp"):
        assert word in doc, word


def test_defaults(rt):
    L = rt.lib()
    d = rt.RtReprojectClipDesc()
    ctypes.memset(ctypes.byref(d), 0xA5, ctypes.sizeof(d))
    assert L.rt_reproject_clip_defaults(ctypes.byref(d)) == 0
    assert d.Size == SIZE and (d.Radius, d.Gamma) == (DEFAULTS["radius"], DEFAULTS["gamma"])
    inner = rt.RtReprojectDesc()
    assert L.rt_reproject_defaults(ctypes.byref(inner)) == 0
    assert bytes(d.Reproject) == bytes(inner) and d.Reproject.Size == INNER_SIZE
    assert bytes(d)[12:16] == b"\0\0\0\0"  # (the padding too: the struct can be compared as bytes)
    assert rt.reproject_clip_defaults() == DEFAULTS
    assert L.rt_reproject_clip_defaults(None) == EINVAL and b"rt_reproject_clip_defaults: NULL argument" in L.rt_last_error()
    text = HEADER.read_text()
    doc = text[text.index("int rt_reproject_clip(const"):text.index("int rt_reproject_clip_defaults(")]
    for word in ("Radius = 1", "Gamma = 0.5f"):
        assert word in doc, word


def _desc(rt, base, cams, outer=None, **inner):
    """A desc the library accepts up to the launch (never reached here: each case below is refused first)."""
    r = rt.RtReprojectDesc(INNER_SIZE, 64, 48, 1, 8, 0, 0.1, ctypes.pointer(cams[0]), ctypes.pointer(cams[1]), base, base + 64,
                           base + 128, base + 192, base + 256, base + 320, base + 384, base + 448)
    for k, v in inner.items():
        setattr(r, k, v)
    d = rt.RtReprojectClipDesc(SIZE, 2, 1.0, r)
    for k, v in (outer or {}).items():
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
    outer = [(dict(Size=112), b"rt_reproject_clip_desc: Size 112, this library's is 128"), (dict(Size=0), b"Size 0"),
             (dict(Radius=0), b"rt_reproject_clip: Radius 0 is not in 1..3"), (dict(Radius=4), b"Radius 4 is not in 1..3"),
             (dict(Radius=0xFFFFFFFF), b"is not in 1..3"), (dict(Gamma=0.0), b"rt_reproject_clip: Gamma is not a finite number above 0"),
             (dict(Gamma=-0.0), b"Gamma is not"), (dict(Gamma=-1.0), b"Gamma is not"), (dict(Gamma=nan), b"Gamma is not"),
             (dict(Gamma=inf), b"Gamma is not"), (dict(Gamma=-inf), b"Gamma is not")]
    inner = [(dict(Size=128), b"rt_reproject_desc: Size 128, this library's is 112"), (dict(Width=0), b"bad image size"),
             (dict(Height=65537), b"bad image size"), (dict(Frames=0), b"Frames is 0"),
             (dict(Frames=9), b"MaxHistory 8 is below Frames 9"), (dict(MaxHistory=0), b"MaxHistory 0 is below Frames 1"),
             (dict(Flags=1), b"unknown flags 0x1"), (dict(DepthTolerance=-1.0), b"DepthTolerance"),
             (dict(DepthTolerance=nan), b"DepthTolerance"), (dict(DepthTolerance=inf), b"DepthTolerance"),
             (dict(Camera=no_cam), b"Camera is NULL"), (dict(PreviousCamera=no_cam), b"PreviousCamera is NULL"),
             (dict(Mean=None), b"Mean is NULL"), (dict(Hit=None), b"Hit is NULL"), (dict(Out=None), b"Out is NULL"),
             (dict(OutCount=None), b"OutCount is NULL"), (dict(History=None), b"all NULL or all given"),
             (dict(HistoryHit=None), b"all NULL or all given"), (dict(HistoryCount=None), b"all NULL or all given"),
             (dict(Mean=base + 8), b"Mean is not 16-byte"), (dict(Hit=base + 68), b"Hit is not 8-byte"),
             (dict(History=base + 136), b"History is not 16-byte"), (dict(HistoryHit=base + 196), b"HistoryHit is not 8-byte"),
             (dict(HistoryCount=base + 258), b"HistoryCount is not 4-byte"), (dict(Out=base + 328), b"Out is not 16-byte"),
             (dict(OutCount=base + 385), b"OutCount is not 4-byte"), (dict(Rgba8=base + 450), b"Rgba8 is not 4-byte"),
             (dict(Out=base), b"Out is Mean"), (dict(Out=base + 128), b"Out is History"),
             (dict(OutCount=base + 256), b"OutCount is HistoryCount")]
    cases = [(o, {}, text) for o, text in outer] + [(None, i, text) for i, text in inner]
    # the outer desc is judged first: a bad Radius with a bad inner desc is the Radius's refusal
    cases.append((dict(Radius=7), dict(Width=0), b"Radius 7 is not in 1..3"))
    for o, i, text in cases:
        L.rt_reproject_defaults(None)  # (leaves another text behind: the one checked below is this call's)
        assert L.rt_reproject_clip(ctypes.byref(_desc(rt, base, cams, o, **i)), None) == EINVAL, (o, i)
        assert text in L.rt_last_error(), (o, i, L.rt_last_error())
    assert L.rt_reproject_clip(None, None) == EINVAL and b"rt_reproject_clip: NULL argument" in L.rt_last_error()


def test_wrapper_checks_its_arguments(rt):
    buf = (ctypes.c_uint8 * 640)()
    base = (ctypes.addressof(buf) + 15) & ~15
    scene = rt.scene_builtin(0)
    cam = rt.camera_setup(scene, 64, 48)
    ok = dict(width=64, height=48, camera=cam, previous_camera=cam, mean_ptr=base, hit_ptr=base + 64, out_ptr=base + 320,
              out_count_ptr=base + 384)
    for bad in (dict(radius=0), dict(radius=4), dict(radius=1.0), dict(radius=True), dict(radius="2"), dict(gamma=0),
                dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma="1"), dict(gamma=True),
                dict(gamma=1e39), dict(gamma=1e-60), dict(frames=0), dict(frames=9), dict(depth_tolerance=-0.5),
                dict(camera=None)):
        with pytest.raises(ValueError, match="reproject_clip: "):
            rt.reproject_clip(**{**ok, **bad})
    # what the wrapper lets through, the library refuses (before any launch: these are host addresses)
    with pytest.raises(rt.RtError, match="Out is Mean"):
        rt.reproject_clip(**{**ok, "out_ptr": base}, radius=np.int64(3), gamma=np.float32(2.0))
    with pytest.raises(rt.RtError, match="all NULL or all given"):
        rt.reproject_clip(**ok, history_ptr=base + 128)
    with pytest.raises(rt.RtError, match="bad image size"):
        rt.reproject_clip(**{**ok, "width": 0})
