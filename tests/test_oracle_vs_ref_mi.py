"""CPU: the oracle's binned MI, Kraskov MI and DKL against the reference's own object code -- MutualInformation.cpp and
DKL.cpp compiled where they lie into oracle/_ref/libref_mi.so, with oracle/standins/ in place of boost, sgl and glm
(where oracle/_ref is absent: that object code's recorded answers, tests/golden/reference/mi_calls.npz).

What this pins is the arithmetic of those two files: bin indices and their int() conversion, summation order, epsilon
thresholds, the `<` of the range counts, how the noise is applied, the window descent of the DKL search.  The library
parts are stand-ins and are tested by themselves at the end of this file; the field / pair loops are driver code
(oracle/ref_mi_driver.cpp) and agree with the oracle's loops by construction of both after the same calculator code."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
from parity import assert_bit_exact
from test_oracle_vs_ref import FIELD_MEMBER_COUNTS
from test_pair_requests import PAIR_MEMBER_COUNTS, _case

ROOT = Path(__file__).resolve().parent.parent
BINS = (4, 80, 255)
NUM_VECTORS = 600


@pytest.fixture(scope="module")
def ref():
    return oracle_lib.load_reference_or_recorded()


@pytest.fixture(scope="module")
def standins():
    return oracle_lib.load_standins()


def _dkl(oracle, estimator, v, **kw):
    """The oracle's DKL estimators on one vector: a field of one voxel."""
    v = np.asarray(v, np.float32)
    return oracle.dkl(estimator, v.reshape(v.size, 1, 1, 1), **kw)[0]


def _vectors():
    """NUM_VECTORS pairs of 2 to 199 members, fixed seed: every third pair rounded to halves (ties), every seventh with
    a NaN (used by the binned calls only)."""
    rng = np.random.default_rng(20261018)
    for trial in range(NUM_VECTORS):
        n = int(rng.integers(2, 200))
        x = rng.standard_normal(n).astype(np.float32)
        y = (0.5 * x + rng.standard_normal(n)).astype(np.float32)
        if trial % 3 == 0:
            x, y = np.round(x * 2) / 2, np.round(y * 2) / 2
        nan_at = int(rng.integers(0, n)) if trial % 7 == 0 else None
        yield trial, n, x, y, nan_at


def test_primitives_bit_exact(oracle, ref):
    got, want, what = [], [], []

    def both(name, o, r):
        got.append(o)
        want.append(r)
        what.append(name)

    for trial, n, x, y, nan_at in _vectors():
        # binned MI takes normalised samples: most of N(0.5, 0.3) lies in [0, 1], the tails exercise the clamp
        x01, y01 = (0.3 * x + 0.5).astype(np.float32), (0.3 * y + 0.5).astype(np.float32)
        if nan_at is not None:
            y01[nan_at] = np.nan
        for bins in BINS:
            both(f"binned #{trial} n={n} bins={bins}", oracle.mi_binned(x01, y01, bins), ref.mi_binned(x01, y01, bins))
        for k in (1, 3, n + 2):
            for est in (1, 2):
                both(f"KSG-{est} #{trial} n={n} k={k}", oracle.mi_kraskov(x, y, k, est), ref.mi_kraskov(x, y, k, est))
        for bins in BINS:
            both(f"DKL binned #{trial} n={n} bins={bins}", _dkl(oracle, 0, y, num_bins=bins), ref.dkl_binned(y, bins))
        for k in sorted({1, 3, n - 1}):
            if k < n:          # the window of k + 1 sorted values must fit: the estimator's domain is 1 <= k < n
                both(f"DKL k-NN #{trial} n={n} k={k}", _dkl(oracle, 1, y, k=k), ref.dkl_knn(y, k))
    from parity import bit_identical
    same = bit_identical(np.array(got, np.float32), np.array(want, np.float32))
    bad = np.flatnonzero(~same)
    print(f"{same.size} primitive calls, {bad.size} mismatches")
    assert bad.size == 0, f"{bad.size}/{same.size} calls differ; first: {what[bad[0]]}: oracle {got[bad[0]]!r} " \
                          f"reference {want[bad[0]]!r}"


def test_kraskov_maximum(oracle, ref):
    """computeMaximumMutualInformationKraskov = float(psi(n) - psi(k)) in double."""
    for k, n in ((1, 2), (3, 64), (5, 100), (20, 1000)):
        assert np.float32(ref.kraskov_max(k, n)) == np.float32(oracle.digamma(n) - oracle.digamma(k))


# --- edge vectors ------------------------------------------------------------------------------------------------
def test_binned_constant_data_is_zero_not_nan(oracle, ref):
    ens = np.full((16, 1, 2, 4), 2.5, np.float32)
    kw = dict(num_bins=80, minmax_ref=(2.5, 2.5))
    want = ref.mi_field(oracle_lib.MI_BINNED, ens, ens[:, 0, 0, 0].copy(), **kw)
    assert (want == 0.0).all()
    assert_bit_exact(oracle.field(oracle_lib.MI_BINNED, ens, ens[:, 0, 0, 0].copy(), **kw), want, "constant data")
    nan = np.full(16, np.nan, np.float32)          # what the normalisation hands the estimator: every sample skipped
    assert ref.mi_binned(nan, nan, 80) == 0.0 and oracle.mi_binned(nan, nan, 80) == 0.0


def test_binned_infinite_samples_with_a_finite_range(oracle, ref):
    """+inf / -inf times numBins is outside the int range: the reference's compiled int() decides the bin."""
    rng = np.random.default_rng(5)
    x = rng.random(40).astype(np.float32)
    y = rng.random(40).astype(np.float32)
    x[3], y[3], y[7], x[11], y[11] = np.inf, 0.25, -np.inf, -np.inf, np.inf
    for bins in BINS:
        assert_bit_exact(oracle.mi_binned(x, y, bins), ref.mi_binned(x, y, bins), f"infinite samples bins={bins}")


@pytest.mark.parametrize("cs", [12, 64])
def test_binned_narrow_caller_range(oracle, ref, cs):
    """The inputs of test_gpu_mi.test_binned_positive_overflow_of_the_bin_index: value * numBins reaches 2^31."""
    rng = np.random.default_rng(40 + cs)
    ens = (rng.standard_normal((cs, 2, 6, 16)) * 100.0).astype(np.float32)
    ens[1, 0, 2, 3] = np.inf
    ens[2, 1, 4, 5] = -np.inf
    narrow = (0.0, 1e-8)
    for r in [(0, 0, 0), (3, 2, 0)]:
        refv = ens[:, r[2], r[1], r[0]].copy()
        kw = dict(num_bins=80, minmax_ref=narrow)
        assert_bit_exact(oracle.field(oracle_lib.MI_BINNED, ens, refv, **kw),
                         ref.mi_field(oracle_lib.MI_BINNED, ens, refv, **kw), f"narrow range cs={cs} ref={r}")


def test_binned_value_exactly_one(oracle, ref):
    x = np.array([0.0, 1.0, 1.0, 0.5, 0.999999940395, 1.0, 0.25, 0.0], np.float32)
    y = np.array([1.0, 0.0, 1.0, 0.5, 1.0, 0.75, 1.0, 0.0], np.float32)
    for bins in BINS:
        assert_bit_exact(oracle.mi_binned(x, y, bins), ref.mi_binned(x, y, bins), f"value 1.0 bins={bins}")


def test_dkl_knn_duplicate_values_give_nan(oracle, ref):
    """Two equal values: nearest-neighbour distance 0, log(0) = -inf, the estimate is inf and both sides answer NaN."""
    v = np.array([0.5, -1.0, 0.5, 2.0, 3.5, -0.25, 1.0, 1.0], np.float32)
    for k in (1, 2):
        want = ref.dkl_knn(v, k)
        assert_bit_exact(_dkl(oracle, 1, v, k=k), want, f"duplicates k={k}")
    assert np.isnan(ref.dkl_knn(v, 1))
    const = np.full(8, 4.0, np.float32)            # stdev 0
    assert_bit_exact(_dkl(oracle, 1, const, k=1), ref.dkl_knn(const, 1), "constant vector k-NN")
    assert_bit_exact(_dkl(oracle, 0, const, num_bins=10), ref.dkl_binned(const, 10), "constant vector binned")


def test_ksg2_marginal_count_of_one_evaluates_digamma_at_zero(oracle, ref):
    """KSG-2 counts the points with |x_j - x_e| < dx_e + 1e-15 and evaluates psi(count - 1).  The smallest input where a
    count reaches 1: two points, k = 1, x = (0, 2^40).  At 2^40 the 1e-10 noise and the 1e-15 slack are both below half
    an ulp, so for point 0 the interval's open upper end lands exactly on point 1, the count is 1 (the point itself)
    and psi(0) is a pole: the reference throws, the driver answers NaN, and so does the oracle."""
    x = np.array([0.0, 2.0 ** 40], np.float32)
    y = np.array([0.0, 1.0], np.float32)
    assert np.isnan(ref.mi_kraskov(x, y, 1, 2)) and np.isnan(oracle.mi_kraskov(x, y, 1, 2))
    assert np.isnan(ref.mi_kraskov(y, x, 1, 2)) and np.isnan(oracle.mi_kraskov(y, x, 1, 2))   # the y count
    # KSG-1 counts with the joint distance minus the slack and never reaches the pole
    assert_bit_exact(oracle.mi_kraskov(x, y, 1, 1), ref.mi_kraskov(x, y, 1, 1), "KSG-1 on the same input")
    assert np.isfinite(ref.mi_kraskov(x, y, 1, 1))


# --- fields (driver loops on both sides) ----------------------------------------------------------------------------
def _field_case(cs):
    """The ensemble of test_oracle_vs_ref.test_fields_bit_exact."""
    rng = np.random.default_rng(cs)
    ens = rng.standard_normal((cs, 3, 5, 7)).astype(np.float32)
    ens[:, 0, 0, 0] = np.round(ens[:, 0, 0, 0])
    ens[:, 0, 0, 1] = 0.25
    if cs > 2:
        ens[1, 1, 1, 1] = np.nan
    refv = ens[:, 2, 3, 4].copy()
    return ens, refv, np.round(refv * 2)


@pytest.mark.parametrize("cs", FIELD_MEMBER_COUNTS)
def test_fields_bit_exact(oracle, ref, cs):
    ens, refv, tied_ref = _field_case(cs)
    mm = oracle.minmax(ens)
    for rv, tag in ((refv, ""), (tied_ref, " tied ref")):
        for m in (oracle_lib.MI_BINNED, oracle_lib.BINNED_MI_CC):
            kw = dict(num_bins=80, minmax_ref=mm)
            assert_bit_exact(oracle.field(m, ens, rv, **kw), ref.mi_field(m, ens, rv, **kw), f"measure {m} cs={cs}{tag}")
        for m in (oracle_lib.MI_KRASKOV, oracle_lib.KMI_CC):
            for est in (1, 2):
                kw = dict(k=3, estimator=est)
                assert_bit_exact(oracle.field(m, ens, rv, **kw), ref.mi_field(m, ens, rv, **kw),
                                 f"measure {m} KSG-{est} cs={cs}{tag}")


@pytest.mark.parametrize("cs", FIELD_MEMBER_COUNTS)
def test_symmetric_fields_bit_exact(oracle, ref, cs):
    a, _, _ = _field_case(cs)
    rng = np.random.default_rng(1000 + cs)
    b = (0.6 * np.nan_to_num(a) + 0.8 * rng.standard_normal(a.shape) * 3.0).astype(np.float32)
    b[:, 0, 0, 2] = np.round(b[:, 0, 0, 2])
    if cs > 2:
        b[0, 2, 2, 2] = np.nan
    mm_a, mm_b = oracle.minmax(a), oracle.minmax(b)
    for m in (oracle_lib.MI_BINNED, oracle_lib.BINNED_MI_CC):
        kw = dict(num_bins=20, minmax_ref=mm_a, minmax_query=mm_b)
        assert_bit_exact(oracle.symmetric_field(m, a, b, **kw), ref.mi_symmetric_field(m, a, b, **kw),
                         f"symmetric {m} cs={cs}")
    for m in (oracle_lib.MI_KRASKOV, oracle_lib.KMI_CC):
        assert_bit_exact(oracle.symmetric_field(m, a, b, k=3), ref.mi_symmetric_field(m, a, b, k=3),
                         f"symmetric {m} cs={cs}")


@pytest.mark.parametrize("cs", PAIR_MEMBER_COUNTS)
def test_pair_requests_bit_exact(oracle, ref, cs):
    ens, _, ii, jj = _case(cs, 900 + cs)
    for m in (3, 4, 5, 6):
        kw = dict(k=3, num_bins=80)
        assert_bit_exact(oracle.pair_requests(m, ens, ii, jj, **kw), ref.mi_pair_requests(m, ens, ii, jj, **kw),
                         f"pairs measure {m} cs={cs}")


@pytest.mark.parametrize("cs", FIELD_MEMBER_COUNTS)
def test_dkl_fields_bit_exact(oracle, ref, cs):
    ens, _, _ = _field_case(cs)
    ens[:, 0, 1, 0] = np.random.default_rng(cs).exponential(2.0, cs)      # skewed
    assert_bit_exact(oracle.dkl(0, ens, num_bins=80), ref.dkl_field(0, ens, num_bins=80), f"DKL binned cs={cs}")
    for k in sorted({1, min(3, cs - 1)}):
        assert_bit_exact(oracle.dkl(1, ens, k=k), ref.dkl_field(1, ens, k=k), f"DKL k-NN cs={cs} k={k}")


# --- the stand-ins by themselves ----------------------------------------------------------------------------------
def test_standin_digamma_within_one_ulp_of_scipy(standins, oracle):
    from scipy.special import digamma
    n = np.arange(1, 4097)
    mine = np.array([standins.digamma(int(i)) for i in n])
    theirs = digamma(n.astype(np.float64))
    assert (np.abs(mine - theirs) <= np.spacing(np.abs(theirs))).all()
    assert np.isnan(standins.digamma(0)) and np.isnan(standins.digamma(-3))       # the pole: thrown, NaN at the C ABI
    assert all(standins.digamma(int(i)) == oracle.digamma(int(i)) for i in (1, 2, 3, 64, 65, 1000, 4096))


def test_standin_knn_is_an_exact_chebyshev_search(standins):
    rng = np.random.default_rng(3)
    for n, count in ((1, 1), (2, 2), (7, 3), (50, 4), (50, 60), (199, 200), (64, 1)):
        px, py = rng.standard_normal(n), np.round(rng.standard_normal(n) * 2) / 2      # ties in y
        for center in {0, n // 2, n - 1}:
            d, nx, ny = standins.knn(px, py, center, count)
            dist = np.maximum(np.abs(px - px[center]), np.abs(py - py[center]))
            order = np.argsort(dist, kind="stable")[:min(count, n)]
            np.testing.assert_array_equal(d, dist[order])                          # ascending, farthest last
            np.testing.assert_array_equal(nx, px[order])
            np.testing.assert_array_equal(ny, py[order])
            assert d[0] == 0.0 and (np.diff(d) >= 0).all()


def test_standin_knn_replaces_its_output_vectors(standins):
    """computeMutualInformationKraskov2 never clears its neighbour vector between queries and takes maxima over all of
    it: the query must replace the contents.  Five stale entries in the output vectors are gone after the call."""
    rng = np.random.default_rng(4)
    px, py = rng.standard_normal(20), rng.standard_normal(20)
    fresh = standins.knn(px, py, 5, 4, prefill=0)
    stale = standins.knn(px, py, 5, 4, prefill=5)
    assert len(stale[0]) == 4
    for a, b in zip(fresh, stale):
        np.testing.assert_array_equal(a, b)


def test_standin_generator_is_the_oracles_noise_stream(standins, oracle):
    for which in (0, 1):
        a, b = standins.noise01(which, 1000), oracle.noise01(which, 1000)
        assert a.tobytes() == b.tobytes()
        assert (a >= 0).all() and (a < 1).all()


def test_standins_selftest_under_sanitizers(tmp_path):
    """tests/native/standins_selftest.cpp: a host program with its own main, built with AddressSanitizer and UBSan (the
    runtimes linked into the program).  It runs the stand-ins, and -- where the reference tree is present -- the driver
    with the reference's two files."""
    reference = Path(os.environ.get("REFERENCE", "/root/reference")) / "src" / "Calculators"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", f"-I{ROOT / 'oracle' / 'standins'}",
           str(ROOT / "tests" / "native" / "standins_selftest.cpp")]
    with_driver = (reference / "MutualInformation.cpp").exists()
    if with_driver:
        cmd += ["-DWITH_REFERENCE", f"-I{reference}", str(ROOT / "oracle" / "ref_mi_driver.cpp"),
                str(reference / "MutualInformation.cpp"), str(reference / "DKL.cpp")]
    exe = tmp_path / "standins_selftest"
    subprocess.run(cmd + ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK stand-ins" + (" and driver" if with_driver else "")), r.stdout
