"""CPU-side checks of the per-tile work entry point (no GPU needed): the header declares
rt_tile_work / rt_trace_tile_work and the library exports the function, the ctypes mirrors have the C
compiler's own sizes and offsets, rt_trace_info keeps its layout (the per-tile flag is a query of its
own, rt_trace_last_tile_counts), and the Python wrapper
validates its `work` argument before anything reaches the library."""
import ctypes
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_trace.h"


def _c_asserts(rt):
    """_Static_assert lines stating the ctypes mirrors' sizes and offsets."""
    lines = []
    for c_name, mirror in (("rt_tile_work", rt.RtTileWork), ("rt_trace_info", rt.RtTraceInfo)):
        lines.append(f"_Static_assert(sizeof({c_name}) == {ctypes.sizeof(mirror)}, \"sizeof {c_name}\");")
        for name, _ in mirror._fields_:
            off = getattr(mirror, name).offset
            lines.append(f"_Static_assert(offsetof({c_name}, {name}) == {off}, \"{c_name}.{name}\");")
    return lines


def test_mirrors_have_the_c_compilers_layout(rt, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler (build() needs one too)"
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"rt_trace.h\"\n" + "\n".join(_c_asserts(rt)) + "\n")
    r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", str(HEADER.parent), str(src)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(rt.RtTileWork) == 12
    assert [n for n, _ in rt.RtTileWork._fields_] == ["Tile", "PreviousRayCount", "Frames"]
    # a wrong offset is caught (the check above is not vacuous)
    src.write_text("#include <stddef.h>\n#include \"rt_trace.h\"\n"
                   "_Static_assert(offsetof(rt_tile_work, Frames) == 4, \"wrong on purpose\");\n")
    assert subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", str(HEADER.parent), str(src)],
                          capture_output=True).returncode != 0


def test_header_and_library_carry_the_entry_point(rt):
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+rt_trace_tile_work\s*\(\s*rt_device\s*\*\s*dev,\s*const\s+rt_camera_info\s*\*\s*cam,\s*"
                     r"const\s+rt_trace_desc\s*\*\s*desc,\s*const\s+rt_tile_work\s*\*\s*work,\s*uint32_t\s+n_work,\s*"
                     r"uint64_t\s*\*\s*d_rays,\s*void\s*\*\s*stream\s*\)", code)
    for name in ("rt_trace_tile_work", "rt_trace_last_tile_counts"):
        assert name in rt.SIGNATURES and hasattr(rt.lib(), name), name
    assert len(rt.SIGNATURES["rt_trace_tile_work"][1]) == 7
    body = re.search(r"typedef struct rt_trace_info \{(.*?)\} rt_trace_info;", code, flags=re.S).group(1)
    fields = re.findall(r"^\s*uint(?:32|64)_t\s+(\w+);", body, flags=re.M)
    # rt_trace_info is what it was: the flag is not a field of it (its size and last field are ABI)
    assert fields[-1] == "TilesSelected" and fields == [n for n, _ in rt.RtTraceInfo._fields_]
    assert ctypes.sizeof(rt.RtTraceInfo) == 64


def test_null_arguments_are_refused(rt):
    L = rt.lib()
    cam, d = rt.RtCameraInfo(), rt.RtTraceDesc()
    work = (rt.RtTileWork * 1)(rt.RtTileWork(0, 0, 1))
    assert L.rt_trace_tile_work(None, ctypes.byref(cam), ctypes.byref(d), work, 1, None, None) == -22
    assert b"NULL argument" in L.rt_last_error()
    assert L.rt_trace_tile_work(None, None, None, None, 0, None, None) == -22
    out = ctypes.c_uint32(7)
    assert L.rt_trace_last_tile_counts(None, ctypes.byref(out)) == -22 and out.value == 7


def test_work_argument_validation(rt):
    w = rt.tile_work_array([(3, 0, 8), (7, 4, 2)])
    assert w.dtype == np.uint32 and w.shape == (2, 3) and w.flags.c_contiguous
    assert w.tolist() == [[3, 0, 8], [7, 4, 2]]
    # the array is the C struct's memory: rt_tile_work records back to back
    rec = (rt.RtTileWork * 2).from_buffer_copy(w.tobytes())
    assert (rec[1].Tile, rec[1].PreviousRayCount, rec[1].Frames) == (7, 4, 2)
    assert rt.tile_work_array(np.array([[1, 2, 3]], np.int64)).tolist() == [[1, 2, 3]]
    assert rt.tile_work_array([(0, 0xFFFFFFFE, 1)]).tolist() == [[0, 0xFFFFFFFE, 1]]
    for empty in ([], (), np.zeros((0, 3), np.uint32)):
        assert rt.tile_work_array(empty).shape == (0, 3)
    for bad in ([(1, 2)], [1, 2, 3], [(1, 2, 3, 4)], [(1.5, 0, 1)], np.zeros((2, 3), np.float32), [(-1, 0, 1)],
                [(0, 1 << 32, 1)], [(0, 0, -3)], np.zeros((1, 2, 3), np.uint32)):
        with pytest.raises(ValueError):
            rt.tile_work_array(bad)


def test_trace_tile_work_validates_before_the_library(rt):
    """The wrapper refuses a malformed `work` with ValueError without touching its device handle."""
    dev = rt.Device.__new__(rt.Device)  # no device: validation must come first
    dev.handle = None
    with pytest.raises(ValueError):
        dev.trace_tile_work(rt.RtCameraInfo(), work=[(1, 2)], width=64, height=64, prev_ptr=0, cur_ptr=0, rays_ptr=0)
    with pytest.raises(ValueError):
        dev.trace_tile_work(rt.RtCameraInfo(), work=[(0, 0, -1)], width=64, height=64, prev_ptr=0, cur_ptr=0,
                            rays_ptr=0)
