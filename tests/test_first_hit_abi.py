"""CPU-side checks of rt_trace_first_hit's interface (no GPU needed): a C99 unit compiled against the header
has sizeof(rt_first_hit) == 8, rt_first_hit_planes' offsets and size, and the three constants; the ctypes
mirrors and the numpy dtype agree with the C compiler; the symbol is in SIGNATURES with 8 arguments and the
library exports it; and the refusal that needs no device handle returns RT_EINVAL."""
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


def _cc():
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler (build() needs one too)"
    return cc


def _compile(tmp_path, body):
    src = tmp_path / "first_hit_layout.c"
    src.write_text("#include <stddef.h>\n#include \"rt_trace.h\"\n" + body + "\n")
    return subprocess.run([_cc(), "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", str(HEADER.parent),
                           str(src)], capture_output=True, text=True)


# C99 has no _Static_assert: a negative array size is the failed assertion
def _assert(name, cond):
    return f"typedef char {name}[({cond}) ? 1 : -1];"


def test_c99_layout_and_constants(rt, tmp_path):
    lines = [_assert("size_hit", "sizeof(rt_first_hit) == 8"),
             _assert("off_key", "offsetof(rt_first_hit, Key) == 0"),
             _assert("off_t", "offsetof(rt_first_hit, T) == 4"),
             _assert("size_planes", "sizeof(rt_first_hit_planes) == 32"),
             _assert("off_size", "offsetof(rt_first_hit_planes, Size) == 0"),
             _assert("off_hit", "offsetof(rt_first_hit_planes, Hit) == 8"),
             _assert("off_normal", "offsetof(rt_first_hit_planes, Normal) == 16"),
             _assert("off_albedo", "offsetof(rt_first_hit_planes, Albedo) == 24"),
             _assert("c_miss", "RT_HIT_MISS == 0xFFFFFFFFu"),
             _assert("c_inside", "RT_HIT_INSIDE == 0x80000000u"),
             _assert("c_centre", "RT_HIT_PIXEL_CENTRE == 1u"),
             # the call as a C host writes it
             "int pick(rt_device *dev, const rt_camera_info *cam, const rt_trace_desc *desc, rt_first_hit *d_hit) {",
             "    const uint32_t tile = 7;",
             "    rt_first_hit_planes out;",
             "    out.Size = sizeof(out); out.Hit = d_hit; out.Normal = NULL; out.Albedo = NULL;",
             "    return rt_trace_first_hit(dev, cam, desc, &tile, 1, RT_HIT_PIXEL_CENTRE, &out, NULL);",
             "}"]
    r = _compile(tmp_path, "\n".join(lines))
    assert r.returncode == 0, r.stderr
    # a wrong value is caught (the check above is not vacuous)
    assert _compile(tmp_path, _assert("wrong_on_purpose", "offsetof(rt_first_hit_planes, Normal) == 12")).returncode != 0
    assert _compile(tmp_path, _assert("wrong_on_purpose", "RT_HIT_INSIDE == 0x40000000u")).returncode != 0


def test_ctypes_mirrors_agree(rt):
    assert ctypes.sizeof(rt.RtFirstHit) == 8 and ctypes.sizeof(rt.RtFirstHitPlanes) == 32
    assert [(n, getattr(rt.RtFirstHit, n).offset) for n, _ in rt.RtFirstHit._fields_] == [("Key", 0), ("T", 4)]
    assert [(n, getattr(rt.RtFirstHitPlanes, n).offset) for n, _ in rt.RtFirstHitPlanes._fields_] == [
        ("Size", 0), ("Hit", 8), ("Normal", 16), ("Albedo", 24)]
    dt = rt.first_hit_dtype
    assert dt == np.dtype([("Key", "<u4"), ("T", "<f4")]) and dt.itemsize == 8
    assert [dt.fields[n][1] for n in dt.names] == [0, 4]
    assert (rt.HIT_MISS, rt.HIT_INSIDE, rt.HIT_PIXEL_CENTRE) == (0xFFFFFFFF, 0x80000000, 1)
    # the header's own values
    code = HEADER.read_text()
    for name, value in (("RT_HIT_MISS", rt.HIT_MISS), ("RT_HIT_INSIDE", rt.HIT_INSIDE),
                        ("RT_HIT_PIXEL_CENTRE", rt.HIT_PIXEL_CENTRE)):
        m = re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u" % name, code)
        assert m and int(m.group(1), 0) == value, name


def test_header_and_library_carry_the_entry_point(rt):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ws = lambda s: re.sub(r"\s+", r"\\s*", re.escape(s).replace(r"\ ", " "))  # noqa: E731
    assert re.search(ws("int rt_trace_first_hit(rt_device *dev, const rt_camera_info *cam, const rt_trace_desc *desc, "
                        "const uint32_t *tiles, uint32_t n_tiles, uint32_t flags, const rt_first_hit_planes *out, "
                        "void *stream)"), code)
    # behind rt_tile_counts_step, as the interface grew
    assert code.index("int rt_tile_counts_step(") < code.index("int rt_trace_first_hit(") < code.index("rt_trace_last_info(")
    assert "rt_trace_first_hit" in rt.SIGNATURES and len(rt.SIGNATURES["rt_trace_first_hit"][1]) == 8
    assert rt.SIGNATURES["rt_trace_first_hit"][0] is ctypes.c_int
    assert hasattr(rt.lib(), "rt_trace_first_hit")


def test_refusals_without_a_device_handle(rt):
    L = rt.lib()
    cam, d = rt.RtCameraInfo(), rt.RtTraceDesc(64, 64, 0, 0, 0, 1, 1, 0, 1, 0, 0)
    buf = (ctypes.c_uint8 * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    planes = rt.RtFirstHitPlanes(32, base, None, None)  # (compared, never followed, on the host)
    assert L.rt_trace_first_hit(None, ctypes.byref(cam), ctypes.byref(d), None, 0, 0, ctypes.byref(planes), None) == EINVAL
    assert b"rt_trace_first_hit: NULL argument" in L.rt_last_error()
    # every other refusal sits behind the device handle: tests/first_hit_check drives them on the device-free
    # plan, tests/test_gpu_first_hit.py through a real device
    dev = rt.Device.__new__(rt.Device)
    dev.handle = None
    for bad in ([1.5], [-1], [1 << 32], np.zeros(2, np.float32)):
        with pytest.raises(ValueError):
            dev.trace_first_hit(cam, width=64, height=64, tiles=bad, hit_ptr=base)
    with pytest.raises(rt.RtError):
        dev.trace_first_hit(cam, width=64, height=64, hit_ptr=base)
