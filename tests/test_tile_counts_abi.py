"""CPU-side checks of the device-table entry points (no GPU needed): the header declares rt_tile_counts,
rt_tile_rule, rt_tile_step_summary, rt_trace_tile_counts and rt_tile_counts_step and the library exports
both functions; the ctypes mirrors and numpy dtypes have the C compiler's own sizes (8, 20 and 16 B) and
offsets; every refusal that is decided before a device is touched returns RT_EINVAL; the Python wrappers
validate before the library; and the plan's device-free part (rt_plan.cpp plan_tile_counts,
check_tile_step, rt_kernel.h rtk_effective_frames) passes its standalone check, tests/tile_counts_check."""
import collections
import ctypes
import os
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_trace.h"
CSRC = ROOT / "simd-ray-tracer_amd" / "csrc"
EINVAL = -22


def _mirrors(rt):
    return (("rt_tile_counts", rt.RtTileCounts, 8), ("rt_tile_rule", rt.RtTileRule, 20),
            ("rt_tile_step_summary", rt.RtTileStepSummary, 16))


def test_mirrors_have_the_c_compilers_layout(rt, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler (build() needs one too)"
    lines = []
    for c_name, mirror, size in _mirrors(rt):
        assert ctypes.sizeof(mirror) == size, c_name
        lines.append(f"_Static_assert(sizeof({c_name}) == {size}, \"sizeof {c_name}\");")
        for name, _ in mirror._fields_:
            lines.append(f"_Static_assert(offsetof({c_name}, {name}) == {getattr(mirror, name).offset}, \"{c_name}.{name}\");")
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include \"rt_trace.h\"\n" + "\n".join(lines) + "\n")
    r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", str(HEADER.parent), str(src)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    assert [n for n, _ in rt.RtTileCounts._fields_] == ["PreviousRayCount", "Frames"]
    assert [n for n, _ in rt.RtTileRule._fields_] == ["Size", "MaxRoundFrames", "MaxTileFrames", "RestMaxDelta",
                                                      "RestSumSquares"]
    assert [n for n, _ in rt.RtTileStepSummary._fields_] == ["NextFrames", "ActiveTiles", "RestedNow"]
    # the numpy views of a table and a copied-back summary are the same records
    for dt, mirror in ((rt.tile_counts_dtype, rt.RtTileCounts), (rt.tile_step_summary_dtype, rt.RtTileStepSummary)):
        assert dt.itemsize == ctypes.sizeof(mirror) and list(dt.names) == [n for n, _ in mirror._fields_]
        assert [dt.fields[n][1] for n in dt.names] == [getattr(mirror, n).offset for n in dt.names]
    assert rt.tile_step_summary_dtype.fields["NextFrames"][0] == np.dtype("<u8")
    assert rt.tile_rule(16, 32).Size == 20 and rt.tile_rule(16, 32).RestSumSquares == 0xFFFFFFFF
    # a wrong offset is caught (the check above is not vacuous)
    src.write_text("#include <stddef.h>\n#include \"rt_trace.h\"\n"
                   "_Static_assert(offsetof(rt_tile_step_summary, ActiveTiles) == 4, \"wrong on purpose\");\n")
    assert subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", str(HEADER.parent), str(src)],
                          capture_output=True).returncode != 0


def test_header_and_library_carry_the_entry_points(rt):
    code = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ws = lambda s: re.sub(r"\s+", r"\\s*", re.escape(s).replace(r"\ ", " "))  # noqa: E731
    assert re.search(ws("int rt_trace_tile_counts(rt_device *dev, const rt_camera_info *cam, const rt_trace_desc *desc, "
                        "const uint32_t *tiles, uint32_t n_tiles, const rt_tile_counts *d_counts, uint32_t max_frames, "
                        "rt_tile_delta *d_delta, uint64_t *d_rays, void *stream)"), code)
    assert re.search(ws("int rt_tile_counts_step(rt_tile_counts *d_counts, const rt_tile_delta *d_delta, uint32_t width, "
                        "uint32_t height, const rt_tile_rule *rule, rt_tile_step_summary *d_summary, void *stream)"), code)
    for struct, fields in (("rt_tile_counts", "PreviousRayCount Frames"),
                           ("rt_tile_rule", "Size MaxRoundFrames MaxTileFrames RestMaxDelta RestSumSquares"),
                           ("rt_tile_step_summary", "NextFrames ActiveTiles RestedNow")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
        assert re.findall(r"uint(?:32|64)_t\s+(\w+);", body) == fields.split(), struct
    for name, n_args in (("rt_trace_tile_counts", 10), ("rt_tile_counts_step", 7)):
        assert name in rt.SIGNATURES and hasattr(rt.lib(), name), name
        assert len(rt.SIGNATURES[name][1]) == n_args
    assert ctypes.sizeof(rt.RtTraceInfo) == 64  # (rt_trace_info is what it was)


def test_trace_tile_counts_refusals_before_a_device(rt):
    L = rt.lib()
    cam, d = rt.RtCameraInfo(), rt.RtTraceDesc()
    tiles = (ctypes.c_uint32 * 2)(0, 1)
    buf = (ctypes.c_uint8 * 96)()
    base = (ctypes.addressof(buf) + 15) & ~15
    vp = ctypes.c_void_p
    table, delta, rays = vp(base + 32), vp(base), vp(base + 64)  # (compared, never followed, on the host)
    call = lambda *a: L.rt_trace_tile_counts(*a)  # noqa: E731
    # no device: refused whatever else is given
    assert call(None, ctypes.byref(cam), ctypes.byref(d), tiles, 2, table, 4, delta, rays, None) == EINVAL
    assert b"NULL argument" in L.rt_last_error()
    assert call(None, None, None, None, 0, None, 0, None, None, None) == EINVAL
    # with a device handle the order is desc, d_counts, max_frames, d_delta, then rt_trace_tiles' own checks; a handle
    # cannot exist here, so the same order is checked on the device-free plan (tests/tile_counts_check) and, with a
    # real device, by tests/test_gpu_tile_counts.py
    dev = rt.Device.__new__(rt.Device)
    dev.handle = None
    for bad in ([1.5], [-1], [1 << 32], np.zeros(2, np.float32)):
        with pytest.raises(ValueError):
            dev.trace_tile_counts(cam, tiles=bad, counts_ptr=4096, max_frames=4, width=64, height=64, prev_ptr=0,
                                  cur_ptr=0, rays_ptr=0)
    with pytest.raises(ValueError):
        dev.trace_tile_counts(cam, tiles=[0], counts_ptr=4096, max_frames=1 << 32, width=64, height=64, prev_ptr=0,
                              cur_ptr=0, rays_ptr=0)
    with pytest.raises(rt.RtError):
        dev.trace_tile_counts(cam, tiles=[0], counts_ptr=4096, max_frames=4, width=64, height=64, prev_ptr=0,
                              cur_ptr=0, rays_ptr=0)


def test_tile_counts_step_refusals(rt):
    L = rt.lib()
    buf = (ctypes.c_uint8 * 96)()
    base = (ctypes.addressof(buf) + 15) & ~15
    vp = ctypes.c_void_p
    table, delta, summary = vp(base + 32), vp(base), vp(base + 64)
    good = rt.tile_rule(16, 32, 1)
    step = lambda t, dl, w, h, r, s=summary: L.rt_tile_counts_step(t, dl, w, h, r, s, None)  # noqa: E731
    assert step(None, delta, 64, 64, ctypes.byref(good)) == EINVAL and b"NULL" in L.rt_last_error()
    assert step(table, None, 64, 64, ctypes.byref(good)) == EINVAL and b"NULL" in L.rt_last_error()
    assert step(table, delta, 64, 64, None) == EINVAL and b"NULL" in L.rt_last_error()
    for size in (0, 16, 24):
        r = rt.RtTileRule(size, 16, 32, 1, 0xFFFFFFFF)
        assert step(table, delta, 64, 64, ctypes.byref(r)) == EINVAL and b"Size" in L.rt_last_error(), size
    for mr, mt in ((0, 32), (16, 0), (0, 0)):
        r = rt.tile_rule(mr, mt)
        assert step(table, delta, 64, 64, ctypes.byref(r)) == EINVAL and b"MaxRoundFrames" in L.rt_last_error()
    assert step(table, vp(base + 4), 64, 64, ctypes.byref(good)) == EINVAL
    assert b"not 16-byte aligned" in L.rt_last_error()
    for w, h in ((0, 64), (64, 0), (65537, 8), (8, 65537)):
        assert step(table, delta, w, h, ctypes.byref(good)) == EINVAL, (w, h)
        assert b"bad image size" in L.rt_last_error()
    with pytest.raises(rt.RtError):
        rt.tile_counts_step(0, 0, 64, 64, good)


def test_the_device_free_plan_standalone(tmp_path):
    """tests/tile_counts_check: rt_plan.cpp's part of both calls and the shared clamp as a plain host program,
    built as tests/plan_check is (no HIP library on the link line, host sanitizers inside the executable)."""
    from test_pack_standalone import host_compiler
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_include = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        pytest.skip("no ROCm headers")
    exe = tmp_path / "tile_counts_check"
    static_rt = ["-static-libasan", "-static-libubsan"] if pathlib.Path(cxx).name == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt,
                    "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", str(CSRC), "-I", str(rocm_include),
                    str(ROOT / "tests" / "tile_counts_check" / "tile_counts_check.cpp"), str(CSRC / "rt_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.splitlines()
    by_case = dict(l.split(" : ", 1) for l in lines)
    assert len(by_case) == len(lines), "a case is listed twice"
    # cases per section of tile_counts_check.cpp (a case is one printed line), and the closing line
    per_section = collections.Counter(n.split("/")[0] for n in by_case)
    assert dict(per_section) == {"clamp": 9, "refuse": 25, "key": 4, "step": 10, "tile_counts_check": 1}
    assert by_case["tile_counts_check"] == "ok"
    assert by_case["refuse/text_twice"] == "rt_trace_tile_counts: tiles[2] = 1 is listed twice"
    assert by_case["key/same_as_rt_trace_tiles"] == "1" and by_case["key/counts_launch_same_key"] == "1"
