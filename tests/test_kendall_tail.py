"""CPU: the host tail of crf_kendall_values_device / crf_field_kendall_similarity -- from the integers (n, n1, n2, S) to
the float (correrender_amd/csrc/crf_similarity_tail.h: similarity_kendall_from_counts, the reference's
computeKendall<int64_t> expression, Correlation.cpp:439-453) -- run by a small host program (tests/native/kendall_tail.cpp,
plain g++ with -ffp-contract=off as the library is built, no GPU) on quadruples that numpy builds, against numpy's float64
expression (kendall_similarity_reference.tail_int64), bit for bit.  There are no special cases in the tail, so the
degenerate quadruples must come out as IEEE gives them."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from kendall_similarity_reference import f32_bits, tail_int64

ROOT = Path(__file__).resolve().parent.parent
N_MAX = (1 << 31) - 1


def _n0(n):
    return n * (n - 1) // 2


def _ordinary():
    rng = np.random.default_rng(11)
    out = []
    for n in (3, 8, 65, 4097, 20435, 262144, 1 << 24, 1 << 28, N_MAX):
        n0 = _n0(n)
        for _ in range(8):
            n1, n2 = (int(rng.integers(0, n0 // 2 + 1)) for _ in range(2))
            out.append((n, n1, n2, int(rng.integers(0, (n0 - max(n1, n2)) // 2 + 1))))
    return out


CASES = {
    "ordinary": _ordinary(),
    "known answer": [(8, 4, 4, 0)],
    "no pair, one pair, two": [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (2, 0, 0, 1), (2, 1, 0, 0), (2, 1, 1, 0)],
    # a constant x: every pair is a tie of x; the numerator is then -n2 - 2 S
    "n0 == n1, numerator 0": [(65, _n0(65), 0, 0), (N_MAX, _n0(N_MAX), 0, 0)],
    "n0 == n1, numerator not 0": [(65, _n0(65), 7, 0), (65, _n0(65), 0, 3), (N_MAX, _n0(N_MAX), 1 << 40, 0)],
    "numerator 0": [(65, 40, 40, (_n0(65) - 80) // 2), (4097, 0, 0, _n0(4097) // 2), (N_MAX, 1, 0, (_n0(N_MAX) - 1) // 2)],
    # n = 2^31 - 1: n0 = 2^61 - 3 * 2^30 + 1; doubles there are 512 apart
    "near 2^61": [(N_MAX, 0, 0, 0), (N_MAX, 0, 0, _n0(N_MAX)), (N_MAX, 1, 3, 5), (N_MAX, 255, 257, _n0(N_MAX) - 300),
                  (N_MAX, _n0(N_MAX) - 1, _n0(N_MAX) - 2, 0), (N_MAX, (1 << 60) + 1, (1 << 59) + 513, (1 << 58) + 129),
                  (N_MAX - 1, 12345, 0, _n0(N_MAX - 1) // 3)],
}


@pytest.fixture(scope="module")
def tail(tmp_path_factory):
    """{quadruple: (bits, n0, n1, n2, S)} from ONE run of the host program over every case."""
    exe = tmp_path_factory.mktemp("kendall_tail") / "kendall_tail"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror",
                    f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "kendall_tail.cpp"), "-o",
                    str(exe)], check=True)
    quads = [q for group in CASES.values() for q in group]
    r = subprocess.run([str(exe)], input=np.array(quads, np.int64).tobytes(), capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(quads)
    return {q: (int(line.split()[0], 16), *map(int, line.split()[1:])) for q, line in zip(quads, lines)}


@pytest.mark.parametrize("group", list(CASES))
def test_tail_matches_the_float64_expression(tail, group):
    for n, n1, n2, s in CASES[group]:
        bits, *counts = tail[(n, n1, n2, s)]
        assert counts == [_n0(n), n1, n2, s], (n, n1, n2, s)
        assert bits == f32_bits(tail_int64(_n0(n), n1, n2, s)), (n, n1, n2, s)


def test_what_the_degenerate_cases_are(tail):
    nan = lambda q: np.isnan(np.array([tail[q][0]], np.uint32).view(np.float32)[0])
    assert nan((0, 0, 0, 0)) and nan((1, 0, 0, 0)) and nan((65, _n0(65), 0, 0))
    assert tail[(65, _n0(65), 7, 0)][0] == f32_bits(-np.inf)
    assert tail[(2, 0, 0, 0)][0] == f32_bits(1.0) and tail[(2, 0, 0, 1)][0] == f32_bits(-1.0)
    assert tail[(8, 4, 4, 0)][0] == f32_bits(np.float32(20.0 / 24.0))
    assert tail[(4097, 0, 0, _n0(4097) // 2)][0] == f32_bits(0.0)
