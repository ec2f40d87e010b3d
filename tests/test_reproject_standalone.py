"""rt_reproject's device-free part (csrc/rt_plan.cpp plan_reproject) as a plain host program under the host
sanitizers.

tests/reproject_check/reproject_check.cpp links csrc/rt_plan.cpp and nothing else of the library, with no HIP
library on the link line, as tests/denoise_check does.  It drives plan_reproject through every refusal of the call,
each with its text (a NULL desc; a wrong Size; an image rt_tile_count refuses; Frames 0; MaxHistory below Frames;
unknown flag bits; a negative, NaN or infinite DepthTolerance; each required pointer NULL; every way of giving one
or two of the three history planes; each plane misaligned; Out as Mean or History, OutCount as HistoryCount),
through accepted descs (the full one, a first frame without history, the smallest and largest image and counts, a
-0.0f tolerance, one camera twice), and through the launch's arguments: the planes and counts as given, both
cameras' fields, and the host's constants fv, ff, wf, hf, hw, hh bit for bit against the same f32 operations formed
at run time.  A plain executable built with AddressSanitizer and UndefinedBehaviorSanitizer: nothing is preloaded,
no device is touched."""
import collections
import os
import pathlib
import subprocess

import pytest

from conftest import ROOT
from test_pack_standalone import host_compiler

CSRC = ROOT / "simd-ray-tracer_amd" / "csrc"
# cases per section of reproject_check.cpp (a case is one printed line), and the closing line
REFUSALS = 2 + 3 + 2 + 4 + 2 + 3 * 2 + 3 + 2 + 5 * 2 + 6 * 2 + 6 * 2 + 8 * 2 + 3 * 2 + 1
SECTIONS = {"refuse": REFUSALS, "accept": 2 + 3 + 3 + 2 + 2 + 1, "args": 8 + 3 + 3 + 3 + 1 + 4 + 3 + 2, "reproject_check": 1}


def test_reproject_plan_links_without_hip_and_runs_clean_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_include = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"
    if not (rocm_include / "hip" / "hip_runtime.h").exists():
        pytest.skip("no ROCm headers")
    exe = tmp_path / "reproject_check"
    static_rt = ["-static-libasan", "-static-libubsan"] if pathlib.Path(cxx).name == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt,
                    "-D__HIP_PLATFORM_AMD__", "-I", str(ROOT / "include"), "-I", str(CSRC), "-I", str(rocm_include),
                    str(ROOT / "tests" / "reproject_check" / "reproject_check.cpp"), str(CSRC / "rt_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.splitlines()
    by_case = dict(l.split(" : ", 1) for l in lines)
    assert len(by_case) == len(lines), "a case is listed twice"
    per_section = collections.Counter(n.split("/")[0] for n in by_case)
    assert dict(per_section) == SECTIONS
    assert by_case["reproject_check"] == "ok"
    # every refusal is RT_EINVAL and has a text, every accepted call RT_OK
    refused = {k: v for k, v in by_case.items()
               if k.startswith("refuse/") and not k.endswith("_text") and k != "refuse/args_untouched"}
    assert set(refused.values()) == {"-22"}
    texts = {k: v for k, v in by_case.items() if k.startswith("refuse/") and k.endswith("_text")}
    assert all(v.startswith("rt_reproject") and len(v) > len("rt_reproject: ") for v in texts.values())
    for name in ("null_desc", "size111", "image", "frames0", "max_history_below_frames", "max_history0", "flags",
                 "depth_tolerance2", "depth_tolerance3", "no_camera", "no_previous_camera", "no_mean", "no_hit", "no_out",
                 "no_out_count", *(f"history_partial{m}" for m in range(1, 7)), "mean_misaligned", "hit_misaligned",
                 "history_misaligned", "history_hit_misaligned", "history_count_misaligned", "out_misaligned",
                 "out_count_misaligned", "rgba8_misaligned", "out_is_mean", "out_is_history", "out_count_is_history_count"):
        assert f"refuse/{name}" in refused and f"refuse/{name}_text" in texts, name
    assert by_case["refuse/args_untouched"] == "1"
    assert {v for k, v in by_case.items() if k.startswith("accept/") and k.endswith(
        ("full", "minimal", "1x1", "largest_image", "largest_counts", "tolerance", "as_history"))} == {"0"}
    assert by_case["refuse/size111_text"] == "rt_reproject_desc: Size 111, this library's is 112"
    assert by_case["refuse/max_history_below_frames_text"] == "rt_reproject: MaxHistory 32 is below Frames 33"
    assert by_case["refuse/out_is_history_text"] == "rt_reproject: Out is History (the pass does not run in place)"
    for name in ("fv_x", "fv_y", "fv_z", "ff", "wf", "hf", "hw", "hh", "odd_hw", "odd_hh"):
        assert by_case[f"args/{name}"] == "1", name
