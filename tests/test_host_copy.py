"""CPU: the host half of a host-output evaluation (correrender_amd/csrc/crf_host_copy.h: range partition, thread shares,
pre-faulting, the copier loop) and the thread pool under it (crf_pool.h), driven by a stand-alone program with a scripted
producer (tests/native/host_copy.cpp, built with g++): destination == source byte for byte and intact canaries over
release schedules, fault modes, thread counts, range counts, sizes and alignments.  A copier that finds a range landed
before it looks must not fault it in after the copy: touching would write zeros into the result.

Built plain and under ThreadSanitizer and AddressSanitizer + UBSan; each build runs as its own executable.  The plain
and the AddressSanitizer run take a few seconds; under ThreadSanitizer every hand-off of the spinning pool costs
milliseconds and every pass over an 8 MiB result tens of them, about 20 s in all on 8 cores (the program prints the
time of each part)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

BUILDS = {"plain": ["-O2"], "tsan": ["-O1", "-g", "-fsanitize=thread"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined"]}
REPORTS = ("WARNING: ThreadSanitizer", "ERROR: AddressSanitizer", "runtime error")


@pytest.mark.parametrize("build", list(BUILDS))
def test_host_copy(tmp_path, build):
    exe = tmp_path / f"host_copy_{build}"
    compiled = subprocess.run(["g++", "-std=c++17", *BUILDS[build], "-Wall", "-Werror", "-pthread",
                               f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "host_copy.cpp"),
                               "-o", str(exe)], capture_output=True, text=True)
    if compiled.returncode != 0 and build != "plain" and _runtime_missing(compiled.stderr):
        pytest.skip(f"g++ cannot link the sanitizer runtime: {compiled.stderr.strip()}")
    assert compiled.returncode == 0, compiled.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    for report in REPORTS:
        assert report not in out, out
    assert r.stdout.rstrip().endswith("OK host copy"), out


def _runtime_missing(stderr):
    """The link step did not find libtsan / libasan / libubsan (anything else, a compile error above all, fails the test)."""
    return any(f"cannot find {lib}" in stderr or f"cannot find -l{lib[3:]}" in stderr for lib in ("libtsan", "libasan", "libubsan"))
