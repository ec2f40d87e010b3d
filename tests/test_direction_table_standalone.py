"""The direction table of the scene packer (csrc/rt_pack.cpp direction_table) as a plain host program
under a host sanitizer.

tests/dir_table_check/dir_table_check.cpp links csrc/rt_pack.cpp and csrc/rt_scene.cpp and nothing else.  It
is built here with include/ and csrc/ as the only include paths, with AddressSanitizer and
UndefinedBehaviorSanitizer, and run over Floating Spheres prefixes (4, below the table's minimum, 16, 33, 64, 128
spheres, and 129: two mask words, no table) and the adversarial scenes of tests/test_direction_table.py,
written to files as rt_scalar_sphere records.  Every index the packer forms for the table on these scenes
is checked.  A plain executable: nothing is preloaded, no device is touched."""
import pathlib
import subprocess

import numpy as np
import pytest

import random_scenes
from conftest import ROOT
from test_direction_table import ADVERSARIAL
from test_pack_standalone import host_compiler

CSRC = ROOT / "simd-ray-tracer_amd" / "csrc"
PREFIXES = (4, 16, 33, 64, 128, 129)


def test_direction_table_runs_clean_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "dir_table_check"
    static_rt = ["-static-libasan", "-static-libubsan"] if pathlib.Path(cxx).name == "g++" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt,
                    "-I", str(ROOT / "include"), "-I", str(CSRC),
                    str(ROOT / "tests" / "dir_table_check" / "dir_table_check.cpp"), str(CSRC / "rt_pack.cpp"),
                    str(CSRC / "rt_scene.cpp"), "-o", str(exe)], check=True)
    files = []
    for seed in ADVERSARIAL:
        sp = random_scenes.make(seed, n_max=300)["spheres"]
        assert sp.dtype == np.float32 and sp.shape[1] == 20  # rt_scalar_sphere, 80 bytes
        files.append(tmp_path / f"adversarial{seed}.bin")
        sp.tofile(files[-1])
    run = subprocess.run([str(exe), *map(str, files)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.splitlines()
    assert len(lines) == 2 * (len(PREFIXES) + len(ADVERSARIAL))
    by_case = {l.split(" : ")[0]: l.split(" : ")[1] for l in lines}
    for simd in (0, 1):
        assert by_case[f"floating4 simd={simd}"] == "none" and by_case[f"floating129 simd={simd}"] == "none"
        assert "bits=32 rows=16" in by_case[f"floating16 simd={simd}"]
        assert "bits=32 rows=36" in by_case[f"floating33 simd={simd}"]  # (18 pairs)
        assert "bits=32 rows=64" in by_case[f"floating64 simd={simd}"]
        assert "bits=64 rows=128" in by_case[f"floating128 simd={simd}"]
        for f in files:
            assert by_case[f"{f} simd={simd}"] != "none"
