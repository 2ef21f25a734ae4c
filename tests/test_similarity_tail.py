"""CPU: the host tail of crf_field_similarity's binned measures -- from the joint histogram's integer counts to the mutual
information (correrender_amd/csrc/crf_similarity_tail.h, no HIP in it) -- run by a small host program
(tests/native/similarity_tail.cpp, plain g++, no GPU) on counts that numpy builds.

  up to 46 340 samples   bit-identical to the reference's object code (ref_mi_binned of oracle/_ref/libref_mi.so; skipped
                         where oracle/_ref is absent), and so is the sequential restatement of similarity_reference.py
  beyond                 the reference's `es * es` overflows its int (NaN at 46 341 samples, the joint term lost at 65 536
                         and 262 144: shown below with the restatement's wrapped product); the library forms the product in
                         fp64 and must be bit-identical to the restatement that does the same
"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
from similarity_reference import f32_bits, joint_counts, mi_from_counts, mi_to_cc

ROOT = Path(__file__).resolve().parent.parent
SMALL_N = (0, 1, 2, 3, 480, 30720, 46340)      # the reference's defined range
LARGE_N = (46341, 65536, 262144)
BINS = (1, 2, 80, 128)
KINDS = ("unit", "outside", "infinite")


def _data(kind, n):
    """Normalised samples (x01, y01): random in [0, 1]; with values outside it and NaN on either side (pairs the
    reference counts in es and leaves out of the histogram); with +-inf."""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    x = rng.random(n, dtype=np.float32)
    y = (0.6 * x + 0.4 * rng.random(n, dtype=np.float32)).astype(np.float32)
    if kind == "outside":
        x, y = x * 2.0 - 0.5, y * 3.0 - 1.0
        x[5::97] = np.nan
        y[11::89] = np.nan
    if kind == "infinite":
        x[3::50] = np.inf
        x[7::61] = -np.inf
        y[2::40] = -np.inf
        y[9::73] = np.inf
    return x.astype(np.float32), y.astype(np.float32)


CASES = [(kind, n, bins) for kind in KINDS for n in SMALL_N + LARGE_N for bins in BINS]


@pytest.fixture(scope="module")
def tail(tmp_path_factory):
    """{case: (bits of the MI, bits of its correlation coefficient)} from ONE run of the host program over every case."""
    exe = tmp_path_factory.mktemp("similarity_tail") / "similarity_tail"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror",
                    f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "similarity_tail.cpp"), "-o",
                    str(exe)], check=True)
    blob = b""
    for kind, n, bins in CASES:
        counts, es = joint_counts(*_data(kind, n), bins)
        blob += np.array([bins, es], np.uint64).tobytes() + counts.tobytes()
    r = subprocess.run([str(exe)], input=blob, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().split()
    assert len(lines) == 2 * len(CASES)
    return {case: (int(lines[2 * i], 16), int(lines[2 * i + 1], 16)) for i, case in enumerate(CASES)}


@pytest.fixture(scope="module")
def ref():
    if not oracle_lib.reference_available():
        pytest.skip("oracle/_ref (the reference's object code) is not built here")
    return oracle_lib.load_reference()


@pytest.mark.parametrize("kind", KINDS)
def test_tail_and_restatement_match_the_object_code(tail, ref, kind):
    for n in SMALL_N:
        x01, y01 = _data(kind, n)
        for bins in BINS:
            want = f32_bits(ref.mi_binned(x01, y01, bins))
            counts, es = joint_counts(x01, y01, bins)
            assert es == n
            assert f32_bits(mi_from_counts(counts, es)) == want, f"restatement, {kind} N={n} bins={bins}"
            assert tail[(kind, n, bins)][0] == want, f"tail, {kind} N={n} bins={bins}"


@pytest.mark.parametrize("kind", KINDS)
def test_tail_matches_the_restatement_at_every_size(tail, kind):
    """Needs no reference: the defined range again, and the sizes at which only the fp64 product is defined."""
    for n in SMALL_N + LARGE_N:
        for bins in BINS:
            counts, es = joint_counts(*_data(kind, n), bins)
            want = mi_from_counts(counts, es)
            got_mi, got_cc = tail[(kind, n, bins)]
            assert got_mi == f32_bits(want), f"{kind} N={n} bins={bins}"
            assert got_cc == f32_bits(mi_to_cc(want)), f"correlation coefficient, {kind} N={n} bins={bins}"


def test_degenerate_counts(tail):
    assert tail[("unit", 0, 80)][0] == f32_bits(0.0)             # no sample: every probability is NaN and fails its test
    assert tail[("unit", 1, 80)][0] == f32_bits(0.0)             # one cell holds everything: 1 log 1 three times


def test_the_wrapped_product_is_what_the_object_code_does(ref):
    """The deviation, shown: with es * es wrapped to 32 bits the restatement reproduces the object code beyond 46 340
    samples -- NaN at 46 341 (a negative epsilon lets empty cells through: 0 log 0), H(x) + H(y) without the joint term
    at 65 536 (the product wraps to 0, the epsilon is infinite)."""
    for n in (46341, 65536):
        x01, y01 = _data("unit", n)
        counts, es = joint_counts(x01, y01, 80)
        want = ref.mi_binned(x01, y01, 80)
        assert f32_bits(mi_from_counts(counts, es, wrap_product=True)) == f32_bits(want)
        assert f32_bits(mi_from_counts(counts, es)) != f32_bits(want)
    assert np.isnan(ref.mi_binned(*_data("unit", 46341), 80))
