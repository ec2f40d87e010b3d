"""The scene packer (csrc/rt_pack.cpp) as a plain host program under a host sanitizer.

tests/pack_check/pack_check.cpp links csrc/rt_pack.cpp and csrc/rt_scene.cpp and nothing else.  It is
built here with include/ and csrc/ as the only include paths -- no ROCm path, so a HIP include
finding its way back into the packer fails this build -- and with AddressSanitizer and
UndefinedBehaviorSanitizer, then run over its thinned case matrix: every scene at the default
options, and every override value once on a one-word, a two-word and a four-word scene.  The
packer is the code with the most index arithmetic in the project; every index it forms on these
scenes is checked.  A plain executable: nothing is preloaded, no device is touched."""
import os
import pathlib
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "simd-ray-tracer_amd" / "csrc"
SCENES = 14       # 3 built-in, 8 prefixes, translated, beyond kClMaxGroups, radius 0
VARIED = 3        # the one-, two- and four-word scenes the overrides are varied on
OVERRIDES = 8     # PrefilterRelative 0/1, ClusterCount 2/3/1000, SubClusterSpheres 1/2/5
CASES = 2 * (SCENES + VARIED * OVERRIDES)  # both rule sets


def host_compiler():
    rocm = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    for cxx in (shutil.which("g++"), shutil.which("clang++"), str(rocm / "llvm" / "bin" / "clang++")):
        if cxx and pathlib.Path(cxx).exists():
            return cxx
    return None


def test_packer_builds_without_hip_and_runs_clean_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "pack_check"
    # (the sanitizer runtimes inside the executable, as clang links them by default: the program
    # then runs the same whatever else the environment loads in front of it)
    static_rt = ["-static-libasan", "-static-libubsan"] if pathlib.Path(cxx).name == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt,
                    "-I", str(ROOT / "include"), "-I", str(CSRC),
                    str(ROOT / "tests" / "pack_check" / "pack_check.cpp"), str(CSRC / "rt_pack.cpp"),
                    str(CSRC / "rt_scene.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == CASES, (len(lines), CASES)
    keys = {l.split(" : ")[0] for l in lines}
    assert len(keys) == CASES, "a case is listed twice"
    for l in lines:
        case, scalars, hashes = l.split(" : ")
        assert len(hashes.split()) == 5 and all(len(h) == 16 for h in hashes.split()), l
    # the matrix reaches what it is there for: no table below 8 hittable spheres and beyond
    # kClMaxGroups groups, an expanded table that is built but not in use, all three mask widths
    by_case = {l.split(" : ")[0]: l.split(" : ")[1] for l in lines}
    assert "cpairs=0 " in by_case["scene1_first7 rs=1 pf_rel=-1 k=0 sub=0"]
    assert "cpairs=0 words=4 levels=0" in by_case["grid576 rs=0 pf_rel=-1 k=0 sub=0"]
    far = by_case["scene1_first64_x1e4 rs=0 pf_rel=-1 k=0 sub=0"]
    assert "x_ok=0" in far and "xf4=0" not in far
    assert {w for w in (1, 2, 4) if any(f" words={w} levels={1 if w == 1 else 2}" in s for s in by_case.values())} == {1, 2, 4}
