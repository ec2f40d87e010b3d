"""rt_trace_first_hit's device-free part (csrc/rt_plan.cpp plan_first_hit) as a plain host program under the
host sanitizers.

tests/first_hit_check/first_hit_check.cpp links csrc/rt_plan.cpp and nothing else of the library, with no HIP
library on the link line, as tests/plan_check does.  It drives plan_first_hit through every refusal of the
call (a NULL device, cam, desc or out; a wrong Size; all planes NULL; each plane misaligned; an unknown flag;
SeedMode; bands; the image size; no scene; tiles == NULL with a count, an index out of range, an index named
twice), the two "nothing to do" cases (every tile; a list of none), and compares the bitmap of a list with
build_selection's.  A plain executable built with AddressSanitizer and UndefinedBehaviorSanitizer: nothing is
preloaded, no device is touched."""
import collections
import os
import pathlib
import subprocess

import pytest

from conftest import ROOT
from test_pack_standalone import host_compiler

CSRC = ROOT / "simd-ray-tracer_amd" / "csrc"
# cases per section of first_hit_check.cpp (a case is one printed line), and the closing line
SECTIONS = {"accept": 4 + 3 + 1 + 1, "refuse": 2 + 3 + 3 + 1 + 2 + 6 + 3 + 1 + 2 + 4 + 2 + 2 + 2 + 2, "all": 5, "empty": 3,
            "bitmap": 4 * 6 + 3, "first_hit_check": 1}


def test_first_hit_plan_links_without_hip_and_runs_clean_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_include = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        pytest.skip("no ROCm headers")
    exe = tmp_path / "first_hit_check"
    static_rt = ["-static-libasan", "-static-libubsan"] if pathlib.Path(cxx).name == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt,
                    "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", str(CSRC), "-I", str(rocm_include),
                    str(ROOT / "tests" / "first_hit_check" / "first_hit_check.cpp"), str(CSRC / "rt_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.splitlines()
    by_case = dict(l.split(" : ", 1) for l in lines)
    assert len(by_case) == len(lines), "a case is listed twice"
    per_section = collections.Counter(n.split("/")[0] for n in by_case)
    assert dict(per_section) == SECTIONS
    assert by_case["first_hit_check"] == "ok"
    # every refusal is RT_EINVAL, every accepted call RT_OK
    assert {v for k, v in by_case.items() if k.startswith("refuse/") and not k.endswith("_text")} == {"-22"}
    assert {v for k, v in by_case.items() if k.startswith("accept/") and k != "accept/no_text"} == {"0"}
    assert by_case["refuse/twice_text"] == "rt_trace_first_hit: tiles[2] = 1 is listed twice"
    assert by_case["refuse/past_text"] == "rt_trace_first_hit: tiles[1] = 4, the image has 4 tiles"
    assert by_case["all/all"] == "1" and by_case["empty/nothing"] == "1"
    assert by_case["bitmap/clip_pixels"] == str(8 * 8 + 8 * 32 + 32 * 32)
