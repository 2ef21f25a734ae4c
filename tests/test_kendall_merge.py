"""CPU: the partition arithmetic of the Kendall inversion count (correrender_amd/csrc/crf_kendall_merge.h: the run pairs of
a level, the chunk-to-diagonal split, the ragged last run, the carried odd run, the scalar merge with its count) driven by
a stand-alone program (tests/native/kendall_merge.cpp, g++) the way the kernels drive it: per level the chunks tile the
output exactly once, no index leaves its run, and the summed counts equal the O(n^2) count, over random and adversarial
sequences of 1, 2, 3, 5 and 65 runs.  Built plain and under AddressSanitizer + UBSan; each build runs as its own
executable (a few seconds)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

BUILDS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined"]}
REPORTS = ("ERROR: AddressSanitizer", "runtime error")


@pytest.mark.parametrize("build", list(BUILDS))
def test_kendall_merge(tmp_path, build):
    exe = tmp_path / f"kendall_merge_{build}"
    compiled = subprocess.run(["g++", "-std=c++17", *BUILDS[build], "-Wall", "-Werror",
                               f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "kendall_merge.cpp"),
                               "-o", str(exe)], capture_output=True, text=True)
    assert compiled.returncode == 0, compiled.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    for report in REPORTS:
        assert report not in out, out
    assert r.stdout.rstrip().endswith("OK kendall merge"), out
