"""rt_reproject_clip's device-free part (csrc/rt_plan.cpp plan_reproject_clip) as a plain host program under the
host sanitizers.

tests/reproject_clip_check/reproject_clip_check.cpp links csrc/rt_plan.cpp and nothing else of the library, with no
HIP library on the link line, as tests/reproject_check does.  It drives plan_reproject_clip through the outer desc's
refusals, each with its text (a NULL desc; the outer Size wrong, the inner desc's size among the wrong values; the
inner Size wrong; Radius 0, 4 and 2^32 - 1; a Gamma of 0, -0, a negative, NaN and both infinities; a bad Radius
before a bad inner desc), through a sample of plan_reproject's refusals reached through it, each leaving the
arguments untouched, and through accepted descs (the full one, a first frame without history, each radius, the
smallest and the largest Gamma, a 1 x 1 image), whose arguments equal plan_reproject's of the inner desc byte for
byte, with the desc's radius and gamma.  A plain executable built with AddressSanitizer and
UndefinedBehaviorSanitizer: nothing is preloaded, no device is touched."""
import collections
import os
import pathlib
import subprocess

import pytest

from conftest import ROOT
from test_pack_standalone import host_compiler

CSRC = ROOT / "simd-ray-tracer_amd" / "csrc"
REFUSED = ("size112", "size0", "inner_size128", "radius0", "radius4", "radius_max", "gamma_zero", "gamma_minus_zero",
           "gamma_negative", "gamma_nan", "gamma_inf", "gamma_minus_inf", "radius_before_inner", "inner_image",
           "inner_max_history_below_frames", "inner_flags", "inner_depth_tolerance", "inner_no_camera", "inner_no_mean",
           "inner_history_partial", "inner_out_misaligned", "inner_out_is_history")
ACCEPTED = ("full", "minimal", "radius1", "radius2", "radius3", "gamma_denormal", "gamma_largest", "1x1")
# a case is one printed line
SECTIONS = {"refuse": 2 + 3 * len(REFUSED), "accept": 5 * len(ACCEPTED), "reproject_clip_check": 1}


def test_reproject_clip_plan_links_without_hip_and_runs_clean_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_include = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        pytest.skip("no ROCm headers")
    exe = tmp_path / "reproject_clip_check"
    static_rt = ["-static-libasan", "-static-libubsan"] if pathlib.Path(cxx).name == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt,
                    "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", str(CSRC), "-I", str(rocm_include),
                    str(ROOT / "tests" / "reproject_clip_check" / "reproject_clip_check.cpp"), str(CSRC / "rt_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.splitlines()
    by_case = dict(l.split(" : ", 1) for l in lines)
    assert len(by_case) == len(lines), "a case is listed twice"
    per_section = collections.Counter(n.split("/")[0] for n in by_case)
    assert dict(per_section) == SECTIONS
    assert by_case["reproject_clip_check"] == "ok"
    # every refusal is RT_EINVAL, has a text and leaves the arguments alone
    assert by_case["refuse/null_desc"] == "-22" and by_case["refuse/null_desc_text"] == "rt_reproject_clip: NULL argument"
    for name in REFUSED:
        assert by_case[f"refuse/{name}"] == "-22", name
        text = by_case[f"refuse/{name}_text"]
        own = "rt_reproject: " if name.startswith("inner_") and name != "inner_size128" else "rt_reproject"
        assert text.startswith(own) and len(text) > len("rt_reproject_clip: "), (name, text)
        assert by_case[f"refuse/{name}_args_untouched"] == "1", name
    assert by_case["refuse/size112_text"] == "rt_reproject_clip_desc: Size 112, this library's is 128"
    assert by_case["refuse/inner_size128_text"] == "rt_reproject_desc: Size 128, this library's is 112"
    assert by_case["refuse/radius_before_inner_text"] == "rt_reproject_clip: Radius 7 is not in 1..3"
    assert by_case["refuse/gamma_nan_text"] == "rt_reproject_clip: Gamma is not a finite number above 0"
    # every accepted call is RT_OK with plan_reproject's arguments and the desc's radius and gamma
    for name in ACCEPTED:
        assert by_case[f"accept/{name}"] == "0" and by_case[f"accept/{name}_inner"] == "0", name
        assert by_case[f"accept/{name}_rp"] == "1" and by_case[f"accept/{name}_gamma"] == "1", name
    assert [by_case[f"accept/radius{r}_radius"] for r in (1, 2, 3)] == ["1", "2", "3"]
