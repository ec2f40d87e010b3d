"""CPU-side checks of the per-tile RGBA8 change statistics (no GPU needed): the header declares
rt_tile_delta, rt_trace_tile_work_delta and rt_tile_delta_rgba8 and the library exports both functions,
the ctypes mirror and the numpy dtype have the C compiler's own size and offsets, both entry points
refuse NULL and misaligned arguments before they touch a device, the Python wrapper validates `work`
before the library, rt_trace_info keeps its layout, and the numpy restatement of the four statistics
that the GPU tests compare against gives the values the header's bounds state."""
import ctypes
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_trace.h"


def tile_delta_ref(old, new, w, h):
    """(n_tiles, 4) u32 {Changed, MaxDelta, SumDelta, SumSquares} per 32 x 32 tile (clipped) between two
    (h * w,) u32 RGBA8 images; alpha is not looked at."""
    o = old.reshape(h, w).astype(np.uint32)
    n = new.reshape(h, w).astype(np.uint32)
    d = np.stack([np.abs(((o >> s) & 255).astype(np.int64) - ((n >> s) & 255).astype(np.int64)) for s in (0, 8, 16)], -1)
    tx, ty = (w + 31) // 32, (h + 31) // 32
    out = np.zeros((tx * ty, 4), np.uint32)
    for t in range(tx * ty):
        b = d[(t // tx) * 32:(t // tx) * 32 + 32, (t % tx) * 32:(t % tx) * 32 + 32]
        out[t] = (int((b.max(-1) > 0).sum()), int(b.max()), int(b.sum()), int((b * b).sum()))
    return out


def _c_asserts(rt):
    lines = []
    for c_name, mirror in (("rt_tile_delta", rt.RtTileDelta), ("rt_trace_info", rt.RtTraceInfo)):
        lines.append(f"_Static_assert(sizeof({c_name}) == {ctypes.sizeof(mirror)}, \"sizeof {c_name}\");")
        for name, _ in mirror._fields_:
            off = getattr(mirror, name).offset
            lines.append(f"_Static_assert(offsetof({c_name}, {name}) == {off}, \"{c_name}.{name}\");")
    return lines


def test_mirror_has_the_c_compilers_layout(rt, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler (build() needs one too)"
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"rt_trace.h\"\n" + "\n".join(_c_asserts(rt)) + "\n")
    r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", str(HEADER.parent), str(src)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    assert ctypes.sizeof(rt.RtTileDelta) == 16
    names = ["Changed", "MaxDelta", "SumDelta", "SumSquares"]
    assert [n for n, _ in rt.RtTileDelta._fields_] == names
    # the numpy view of a copied-back array is the same record
    assert rt.tile_delta_dtype.itemsize == 16 and list(rt.tile_delta_dtype.names) == names
    assert [rt.tile_delta_dtype.fields[n][1] for n in names] == [getattr(rt.RtTileDelta, n).offset for n in names]
    assert all(rt.tile_delta_dtype.fields[n][0] == np.dtype("<u4") for n in names)
    # a wrong offset is caught (the check above is not vacuous)
    src.write_text("#include <stddef.h>\n#include \"rt_trace.h\"\n"
                   "_Static_assert(offsetof(rt_tile_delta, SumDelta) == 4, \"wrong on purpose\");\n")
    assert subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", str(HEADER.parent), str(src)],
                          capture_output=True).returncode != 0


def test_header_and_library_carry_the_entry_points(rt):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+rt_tile_delta\s*\{\s*uint32_t\s+Changed;\s*uint32_t\s+MaxDelta;\s*"
                     r"uint32_t\s+SumDelta;\s*uint32_t\s+SumSquares;\s*\}\s*rt_tile_delta;", code)
    assert re.search(r"int\s+rt_trace_tile_work_delta\s*\(\s*rt_device\s*\*\s*dev,\s*const\s+rt_camera_info\s*\*\s*cam,\s*"
                     r"const\s+rt_trace_desc\s*\*\s*desc,\s*const\s+rt_tile_work\s*\*\s*work,\s*uint32_t\s+n_work,\s*"
                     r"rt_tile_delta\s*\*\s*d_delta,\s*uint64_t\s*\*\s*d_rays,\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"int\s+rt_tile_delta_rgba8\s*\(\s*const\s+uint32_t\s*\*\s*d_old,\s*const\s+uint32_t\s*\*\s*d_new,\s*"
                     r"uint32_t\s+width,\s*uint32_t\s+height,\s*rt_tile_delta\s*\*\s*d_delta,\s*void\s*\*\s*stream\s*\)",
                     code)
    for name, n_args in (("rt_trace_tile_work_delta", 8), ("rt_tile_delta_rgba8", 6)):
        assert name in rt.SIGNATURES and hasattr(rt.lib(), name), name
        assert len(rt.SIGNATURES[name][1]) == n_args
    # rt_trace_info is what it was: 64 B, TilesSelected last
    body = re.search(r"typedef struct rt_trace_info \{(.*?)\} rt_trace_info;", code, flags=re.S).group(1)
    fields = re.findall(r"^\s*uint(?:32|64)_t\s+(\w+);", body, flags=re.M)
    assert fields[-1] == "TilesSelected" and fields == [n for n, _ in rt.RtTraceInfo._fields_]
    assert ctypes.sizeof(rt.RtTraceInfo) == 64


def test_null_and_misaligned_arguments_are_refused(rt):
    L = rt.lib()
    cam, d = rt.RtCameraInfo(), rt.RtTraceDesc()
    work = (rt.RtTileWork * 1)(rt.RtTileWork(0, 0, 1))
    buf = (ctypes.c_uint8 * 96)()
    base = (ctypes.addressof(buf) + 15) & ~15  # 16 k
    vp = ctypes.c_void_p
    # rt_trace_tile_work_delta: d_delta is looked at before anything else but desc
    assert L.rt_trace_tile_work_delta(None, ctypes.byref(cam), ctypes.byref(d), work, 1, None, None, None) == -22
    assert b"d_delta is NULL" in L.rt_last_error()
    assert L.rt_trace_tile_work_delta(None, ctypes.byref(cam), ctypes.byref(d), work, 1, vp(base + 4), None, None) == -22
    assert b"not 16-byte aligned" in L.rt_last_error()
    assert L.rt_trace_tile_work_delta(None, ctypes.byref(cam), ctypes.byref(d), work, 1, vp(base), None, None) == -22
    assert b"NULL argument" in L.rt_last_error()
    assert L.rt_trace_tile_work_delta(None, None, None, None, 0, None, None, None) == -22
    # rt_tile_delta_rgba8 (the image pointers are never dereferenced on the host)
    img = vp(base + 32)
    assert L.rt_tile_delta_rgba8(None, img, 64, 64, vp(base), None) == -22
    assert L.rt_tile_delta_rgba8(img, None, 64, 64, vp(base), None) == -22
    assert L.rt_tile_delta_rgba8(img, img, 64, 64, None, None) == -22
    assert b"NULL" in L.rt_last_error()
    assert L.rt_tile_delta_rgba8(img, img, 64, 64, vp(base + 4), None) == -22
    assert b"not 16-byte aligned" in L.rt_last_error()
    for w, h in ((0, 64), (64, 0), (65537, 8), (8, 65537)):
        assert rt.tile_count(w, h) == 0
        assert L.rt_tile_delta_rgba8(img, img, w, h, vp(base), None) == -22, (w, h)
        assert b"bad image size" in L.rt_last_error()
    with pytest.raises(rt.RtError):
        rt.tile_delta_rgba8(0, 0, 64, 64, 0)


def test_trace_tile_work_validates_before_the_library(rt):
    """With a delta_ptr too, a malformed `work` is a ValueError without touching the device handle."""
    dev = rt.Device.__new__(rt.Device)  # no device: validation must come first
    dev.handle = None
    for bad in ([(1, 2)], [(0, 0, -1)], [(1.5, 0, 1)]):
        with pytest.raises(ValueError):
            dev.trace_tile_work(rt.RtCameraInfo(), work=bad, width=64, height=64, prev_ptr=0, cur_ptr=0, rays_ptr=0,
                                delta_ptr=4096)


def test_the_numpy_restatement_on_known_images():
    """The reference the GPU tests use, on images whose statistics are known by hand (the header's bounds)."""
    w = h = 64
    zero, white = np.zeros(w * h, np.uint32), np.full(w * h, 0x00FFFFFF, np.uint32)
    assert (tile_delta_ref(zero, white, w, h) == [1024, 255, 783360, 199756800]).all()
    assert (tile_delta_ref(zero, np.full(w * h, 0xFF000000, np.uint32), w, h) == 0).all()
    one = zero.copy()
    one[31 * w + 63] = 0x00000100  # G + 1 at the last pixel of tile 1's last row
    assert tile_delta_ref(zero, one, w, h).tolist() == [[0] * 4, [1] * 4, [0] * 4, [0] * 4]
    # 67 x 33: three columns and two rows of tiles, the last 3 px wide and 1 px tall
    rng = np.random.default_rng(5)
    a, b = (rng.integers(0, 1 << 32, 67 * 33, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    r = tile_delta_ref(a, b, 67, 33)
    assert r.shape == (6, 4) and (r[:, 0] <= [1024, 1024, 96, 32, 32, 3]).all() and (r[:, 1] <= 255).all()
    assert int(r[:, 2].sum()) == sum(int(np.abs(((a >> s) & 255).astype(np.int64) - ((b >> s) & 255)).sum())
                                     for s in (0, 8, 16))
