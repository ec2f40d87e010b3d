"""The launch decisions (csrc/rt_plan.cpp) as a plain host program under a host sanitizer.

tests/plan_check/plan_check.cpp links csrc/rt_plan.cpp and nothing else of the library, and no HIP
library is on the link line: a HIP runtime call finding its way into the plan fails this link.  The
unit includes rt_kernel.h and rtk_shape.h (TraceArgs, the routing functions, rtk::Shape), so the ROCm
headers are on the include path, and nothing more of ROCm is used.  Built with AddressSanitizer and
UndefinedBehaviorSanitizer, the program runs its matrix -- lanes per pixel, pixels per lane, the
secondary threshold, the tables and the LDS image, the routing rows of rt_kernel.h, the split schedule,
the selection and the key -- and compares every value with the literal its case states.  A plain
executable: nothing is preloaded, no device is touched."""
import collections
import os
import pathlib
import subprocess

import pytest

from conftest import ROOT
from test_pack_standalone import host_compiler

CSRC = ROOT / "simd-ray-tracer_amd" / "csrc"
# cases per section of plan_check.cpp (a case is one printed line)
SECTIONS = {
    "shape": 7 * 3,            # the seven shape codes against rtk::Shape
    "lanes": 4 + 6 + 3,        # by pixels, by frames, a tile list and a forced value
    "ppl": 11,
    "sec": 8,
    "merge": 4,
    "table": 10,
    "lds": 15,
    "route": 5 + 3 * 7 + 2 + 3 * 4 + 3 + 9,  # walk 0 and 1, words x thresholds, unproven, shapes, no cull, counts
    "geometry": 16,
    "split": 6 * 2 + 3,
    "selection": 4 * (5 + 7) + 5 + 7 + 4 + 4,
    "work": 6 + 7 + 4 + 2,
    "key": 2 + 15 + 14 + 2 + 5 + 1,
    "options": 4 + 5 + 6,
}


def test_plan_links_without_hip_and_runs_clean_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_include = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        pytest.skip("no ROCm headers")
    exe = tmp_path / "plan_check"
    # (the sanitizer runtimes inside the executable, as clang links them by default: the program
    # then runs the same whatever else the environment loads in front of it)
    static_rt = ["-static-libasan", "-static-libubsan"] if pathlib.Path(cxx).name == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt,
                    "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", str(CSRC), "-I", str(rocm_include),
                    str(ROOT / "tests" / "plan_check" / "plan_check.cpp"), str(CSRC / "rt_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    names = [l.split(" : ")[0] for l in lines]
    assert len(set(names)) == len(names), "a case is listed twice"
    per_section = collections.Counter(n.split("/")[0] for n in names)
    assert dict(per_section) == SECTIONS
    assert len(lines) == sum(SECTIONS.values())
    # the matrix reaches what it is there for: every walk value, all three tables, both refusals
    by_case = dict(l.split(" : ", 1) for l in lines)
    walks = {v for k, v in by_case.items() if k.startswith("route/") and ("_scene_wide" == k[-11:] or "_per_lane" == k[-9:])}
    assert walks | {by_case["route/walk_any"], by_case["route/no_table"]} == {str(w) for w in range(8)}
    assert {by_case["table/no_cpairs"], by_case["table/one_cpair"], by_case["route/words1_scene_wide_table"]} == {"0", "1", "2"}
    assert by_case["split/frames256_parts8"] == "32,96,128"
    assert by_case["selection/text_twice"] == "rt_trace_tiles: tiles[3] = 0 is listed twice"
    assert by_case["work/past_text"] == "rt_trace_tile_work: work[1].Tile = 7, the image has 4 tiles"
