"""CPU: the window arithmetic of a grid whose member volumes are 4 GiB or more (correrender_amd/csrc/crf_windows.h, no HIP
in it; api.cpp cuts such a grid into windows of 2^29 voxels, one launch each) and of the test switch CRF_WINDOW_VOXELS that
gives a small grid windows.  A stand-alone program (tests/native/windows.cpp, plain g++, no GPU) prints the header's answers
at sizes up to 2^32 + 5 voxels, which no GPU test can reach; this test states the rules on its own in Python integers, which
cannot overflow, and compares.  tests/test_gpu_windows.py runs every windowed route on a small grid through the switch.

Built plain and under AddressSanitizer + UBSan; each build runs as its own executable."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

BUILDS = {"plain": ["-O2"], "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined"]}
REPORTS = ("ERROR: AddressSanitizer", "runtime error")

DEFAULT_WINDOW = 2**29
GRANULE = 1024


def valid_rule(value):
    """CRF_WINDOW_VOXELS: 0 (the default rule) or a positive multiple of 1024 whose fp32 bytes a 32-bit offset below the
    kernels' out-of-range sentinel 0xFFFFFFF0 can address."""
    return value >= 0 and value % GRANULE == 0 and value * 4 < 0xFFFFFFF0


def parse_rule(text):
    """The variable as crf_set_grid takes it: unset or empty is 0; one decimal integer that valid_rule accepts is itself;
    anything else is -1 (refused).  No trailing text, no fraction, no exponent, no hexadecimal."""
    if text is None or text == "":
        return 0
    if not re.fullmatch(r"[+-]?[0-9]+", text):
        return -1
    return int(text) if valid_rule(int(text)) else -1


def windowed_rule(n, override):
    return n > override if override else n * 4 >= 0xFFFFFFF0


def grid_rule(n, override):
    """(windowed, count, last length, sum of lengths, every window but the last is full, largest end)."""
    if not windowed_rule(n, override):
        return (0, 1, n, n, 1, n)
    window = override or DEFAULT_WINDOW
    count = -(-n // window)
    bounds = [(w * window, min(window, n - w * window)) for w in range(count)] if count <= 64 else None
    if bounds is None:                              # millions of windows: the closed form
        last = n - (count - 1) * window
        return (1, count, last, n, 1, n)
    assert all(length == window for _, length in bounds[:-1]) and 1 <= bounds[-1][1] <= window
    return (1, count, bounds[-1][1], sum(length for _, length in bounds), 1, max(f + length for f, length in bounds))


@pytest.fixture(scope="module", params=list(BUILDS))
def lines(request, tmp_path_factory):
    build = request.param
    exe = tmp_path_factory.mktemp("windows") / f"windows_{build}"
    compiled = subprocess.run(["g++", "-std=c++17", *BUILDS[build], "-Wall", "-Werror",
                               f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "windows.cpp"),
                               "-o", str(exe)], capture_output=True, text=True)
    if compiled.returncode != 0 and build != "plain" and any(
            f"cannot find {lib}" in compiled.stderr or f"cannot find -l{lib[3:]}" in compiled.stderr
            for lib in ("libasan", "libubsan")):
        pytest.skip(f"g++ cannot link the sanitizer runtime: {compiled.stderr.strip()}")
    assert compiled.returncode == 0, compiled.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    for report in REPORTS:
        assert report not in out, out
    assert r.stdout.rstrip().endswith("OK windows"), out
    return r.stdout.split("\n")[:-2]


def _grids(lines):
    got = {}
    for line in lines:
        if line.startswith("grid "):
            n, override, *rest = (int(v) for v in line.split()[1:])
            got[(n, override)] = tuple(rest)
    return got


def test_every_printed_line_matches_the_rules(lines):
    seen = {"valid": 0, "grid": 0, "parse": 0}
    for line in lines:
        kind, *fields = line.split()
        seen[kind] += 1
        if kind == "valid":
            assert int(fields[1]) == int(valid_rule(int(fields[0]))), line
        elif kind == "parse":
            text = None if fields[0] == "null" else fields[0][1:-1]
            assert int(fields[1]) == parse_rule(text), line
        else:
            n, override, *rest = (int(v) for v in fields)
            assert tuple(rest) == grid_rule(n, override), line
    assert seen["valid"] >= 12 and seen["grid"] >= 60 and seen["parse"] >= 16


def test_default_rule_threshold_from_both_sides(lines):
    """n * sizeof(float) >= 0xFFFFFFF0 first holds at 2^30 - 4 voxels."""
    got = _grids(lines)
    assert (2**30 - 4) * 4 == 0xFFFFFFF0
    assert got[(2**30 - 5, 0)] == (0, 1, 2**30 - 5, 2**30 - 5, 1, 2**30 - 5)
    assert got[(2**30 - 4, 0)] == (1, 2, 2**29 - 4, 2**30 - 4, 1, 2**30 - 4)
    assert got[(216611, 0)][:2] == (0, 1) and got[(2**29 + 1, 0)][:2] == (0, 1)   # more than one window, yet ordinary


@pytest.mark.parametrize("n,count,last", [(2**30, 2, 2**29), (2**30 + 1, 3, 1), (3 * 2**29 - 1, 3, 2**29 - 1),
                                          (3 * 2**29, 3, 2**29), (2**32 + 5, 9, 5)])
def test_default_rule_counts_and_last_window(lines, n, count, last):
    windowed, got_count, got_last, total, full, max_end = _grids(lines)[(n, 0)]
    assert (windowed, got_count, got_last) == (1, count, last)
    assert total == n and max_end == n and full == 1        # lengths sum to n, no window passes n, all but the last full


def test_override_rule(lines):
    got = _grids(lines)
    for window in (1024, 65536, 2**29, 2**30 - 1024):
        assert got[(window, window)] == (0, 1, window, window, 1, window)            # n == window: one launch, ordinary
        assert got[(window - 1, window)][:2] == (0, 1)
        assert got[(window + 1, window)] == (1, 2, 1, window + 1, 1, window + 1)     # two windows, the last of one voxel
        assert got[(2 * window, window)][:3] == (1, 2, window)
        assert got[(2 * window + 1, window)][:3] == (1, 3, 1)
    assert got[(216611, 65536)] == (1, 4, 20003, 216611, 1, 216611)                  # the grid of tests/test_gpu_windows.py
    assert got[(1025, 1024)] == (1, 2, 1, 1025, 1, 1025)
    assert got[(2**32 + 5, 1024)][:3] == (1, 2**22 + 1, 5)
    valid = {int(line.split()[1]): line.split()[2] == "1" for line in lines if line.startswith("valid ")}
    for rejected in (-1, 1000, 1025):
        assert valid[rejected] is False
    assert valid[0] and valid[1024] and valid[65536] and valid[2**29] and valid[2**30 - 1024]
    assert not valid[2**30]        # a window of 4 GiB is what windows exist to avoid
    parsed = {line.split()[1]: int(line.split()[2]) for line in lines if line.startswith("parse ")}
    assert parsed["null"] == parsed["[]"] == parsed["[0]"] == 0 and parsed["[1024]"] == 1024 and parsed["[65536]"] == 65536
    for rejected in ("-1", "1000", "1025", "1024abc", "abc", "1e5", "1073741824", "99999999999999999999"):
        assert parsed[f"[{rejected}]"] == -1, rejected


def test_window_count_binding_without_a_context():
    """crf_window_count is a compatible addition to ABI 5 and answers 0 without a context."""
    import ctypes
    import correrender_amd as ca
    from correrender_amd import _lib
    assert _lib.SYMBOLS["crf_window_count"] == (ctypes.c_int, [ctypes.c_void_p])
    lib = ca.load_library()
    assert lib.crf_abi_version() == 5 and lib.crf_window_count(None) == 0
    header = (ROOT / "include" / "corrfield.h").read_text()
    version = header[header.index("int crf_abi_version(void);"):]
    assert "crf_window_count" in version[:version.index("4: crf_group_")]
