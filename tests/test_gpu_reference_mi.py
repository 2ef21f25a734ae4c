"""GPU parity DIRECTLY against the reference's object code for binned MI, Kraskov MI and DKL: every kernel family at
the smallest shapes that select it, compared with oracle/_ref/libref_mi.so (MutualInformation.cpp and DKL.cpp compiled
where they lie, over oracle/standins/) or, where that library is absent, with its recorded answers
(tests/golden/reference/mi_calls.npz).  The other GPU suites compare the kernels with the oracle; this one leaves the
oracle out, so a misreading shared by oracle and kernel does not pass.

Tolerance: parity.assert_close (1e-5 relative, 1e-6 absolute floor below 1e-3) plus the share of bit-identical voxels
the corresponding oracle suites require: 0.99; 0.98 for the box ensemble (exact ties) and for DKL; 0.95 with infinities.

Every case is a function of the reference alone (`_want_*`), so oracle/make_golden.py records exactly the calls made
here (record_reference_calls)."""
import numpy as np
import pytest

from correrender_amd import Measure, synth
from parity import assert_close, bit_identical
import oracle_lib
from test_gpu_dkl import _ensemble as _dkl_ensemble
from test_gpu_field_modes import _two_fields
from test_pair_requests import _case as _pair_case

GRID = (16, 6, 5)          # xs, ys, zs: 480 voxels, several waves, not a multiple of 64
SHARES = []                # (what, share of bit-identical voxels), printed per check


@pytest.fixture(scope="module")
def ref():
    return oracle_lib.load_reference_or_recorded()


def _minmax(ens):
    """Per-member extrema folded over members, NaN skipped (VolumeData's rule, = oracle.minmax)."""
    return float(np.nanmin(ens)), float(np.nanmax(ens))


def _compare(got, want, what, min_identical):
    got = np.asarray(got).reshape(-1)
    share = float(bit_identical(got, want).mean())
    SHARES.append((what, share))
    print(f"[reference parity] {what}: {share:.4%} bit-identical of {got.size}")
    assert_close(got, want, what)
    if min_identical is not None:
        assert share >= min_identical, f"{what}: only {share:.4%} of the voxels are bit-identical to the reference"


def _upload(engine, ens):
    cs, zs, ys, xs = ens.shape
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(ens)


# --- binned MI -----------------------------------------------------------------------------------------------------
BINNED = [(cs, bins) for cs in (17, 64, 128, 130) for bins in (10, 255)]
BINNED_REF = (5, 3, 2)


def _binned_inputs(cs):
    ens = synth.box_ensemble(*GRID, cs, seed=200 + cs)
    x, y, z = BINNED_REF
    return ens, ens[:, z, y, x].copy(), _minmax(ens)


def _want_binned(ref, cs, bins, measure=oracle_lib.MI_BINNED):
    ens, refv, mm = _binned_inputs(cs)
    return ref.mi_field(measure, ens, refv, num_bins=bins, minmax_ref=mm)


@pytest.mark.gpu
@pytest.mark.parametrize("cs,bins", BINNED)
def test_binned_kernels(engine, ref, cs, bins):
    """Up to 128 members: the register kernels; beyond: the histogram kernel, or the generic one where the bins do not
    fit its LDS rows."""
    ens, _, mm = _binned_inputs(cs)
    _upload(engine, ens)
    assert engine.member_minmax() == mm
    got = engine.compute(Measure.MUTUAL_INFORMATION_BINNED, BINNED_REF, num_bins=bins)
    assert engine.last_kernel_name() == ("mi_binned_kernel" if cs <= 128 else
                                         "mi_binned_hist_kernel" if bins == 10 else "generic_kernel")
    _compare(got, _want_binned(ref, cs, bins), f"binned cs={cs} bins={bins}", 0.99)


@pytest.mark.gpu
def test_binned_correlation_coefficient(engine, ref):
    ens, _, _ = _binned_inputs(64)
    _upload(engine, ens)
    got = engine.compute(Measure.BINNED_MI_CORRELATION_COEFFICIENT, BINNED_REF, num_bins=80)
    assert engine.last_kernel_name() == "mi_binned_kernel"
    _compare(got, _want_binned(ref, 64, 80, oracle_lib.BINNED_MI_CC), "binned MI-CC cs=64", 0.99)


BINNED_INF_REFS = [(0, 0, 0), (2, 1, 0)]       # reference vector without / with skipped samples


def _binned_inf_inputs():
    rng = np.random.default_rng(12)
    ens = rng.standard_normal((24, GRID[2], GRID[1], GRID[0])).astype(np.float32)
    ens[3, 0, 1, 2] = np.inf
    ens[5, 0, 1, 2] = np.inf
    ens[7, 1, 3, 9] = np.inf
    return ens, _minmax(ens)


def _want_binned_inf(ref, r):
    ens, mm = _binned_inf_inputs()
    return ref.mi_field(oracle_lib.MI_BINNED, ens, ens[:, r[2], r[1], r[0]].copy(), num_bins=20, minmax_ref=mm)


@pytest.mark.gpu
@pytest.mark.parametrize("r", BINNED_INF_REFS)
def test_binned_with_infinite_samples(engine, ref, r):
    """max = +inf: finite samples normalise to 0, inf / inf = NaN is skipped, the probabilities are c / total with
    total < cs."""
    ens, mm = _binned_inf_inputs()
    _upload(engine, ens)
    assert engine.member_minmax() == mm
    got = engine.compute(Measure.MUTUAL_INFORMATION_BINNED, r, num_bins=20)
    _compare(got, _want_binned_inf(ref, r), f"binned with infinities ref={r}", 0.95)


NARROW = (0.0, 1e-8)
NARROW_REFS = [(0, 0, 0), (3, 2, 0)]


def _narrow_inputs():
    """test_gpu_mi.test_binned_positive_overflow_of_the_bin_index at 64 members."""
    rng = np.random.default_rng(40 + 64)
    ens = (rng.standard_normal((64, 2, 6, 16)) * 100.0).astype(np.float32)
    ens[1, 0, 2, 3] = np.inf
    ens[2, 1, 4, 5] = -np.inf
    return ens


def _want_narrow(ref, r):
    ens = _narrow_inputs()
    return ref.mi_field(oracle_lib.MI_BINNED, ens, ens[:, r[2], r[1], r[0]].copy(), num_bins=80, minmax_ref=NARROW)


@pytest.mark.gpu
@pytest.mark.parametrize("r", NARROW_REFS)
def test_binned_bin_index_overflow(engine, ref, r):
    """Caller extrema far narrower than the data: value * numBins passes 2^31 and the reference's compiled int()
    decides the bin (bin 0 after the clamp, not the last bin)."""
    ens = _narrow_inputs()
    _upload(engine, ens)
    got = engine.compute(Measure.MUTUAL_INFORMATION_BINNED, r, num_bins=80, minmax_ref=NARROW, minmax_query=NARROW)
    _compare(got, _want_narrow(ref, r), f"binned bin-index overflow ref={r}", None)


# --- Kraskov -------------------------------------------------------------------------------------------------------
KRASKOV_REF = (2, 1, 0)
VARIANTS = {"CRF_KRASKOV_SORTED": "kraskov_sorted_kernel", "CRF_KRASKOV_DIRECT": "kraskov_direct_kernel",
            "CRF_KRASKOV_TILE": "mi_kraskov_kernel"}
VARIANT_CASES = [(cs, k, est) for cs in (33, 64) for k in (1, 4) for est in (1, 2)]
DEFAULT_DISPATCH = [(3, 40, "mi_kraskov_kernel"), (3, 41, "kraskov_direct_kernel"), (5, 20, "kraskov_direct_kernel"),
                    (3, 129, "kraskov_direct_kernel"), (8, 12, None)]            # (8, 12): k beyond the member count


def _kraskov_inputs(cs, k):
    ens = synth.normal_ensemble(*GRID, cs, seed=70 * cs + k)
    ens[3 % cs, 1, 2, 3] = np.nan
    x, y, z = KRASKOV_REF
    return ens, ens[:, z, y, x].copy()


def _want_kraskov(ref, cs, k, est):
    ens, refv = _kraskov_inputs(cs, k)
    return ref.mi_field(oracle_lib.MI_KRASKOV, ens, refv, k=k, estimator=est)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("cs", [33, 64])
def test_kraskov_kernels_forced(engine, ref, monkeypatch, variant, cs):
    """The sorted-column, tile-free and LDS-column kernels, forced one at a time (the launchers read the variable at
    every call): both estimators, k = 1 and 4, a NaN voxel."""
    monkeypatch.setenv(variant, "1")
    for k in (1, 4):
        ens, _ = _kraskov_inputs(cs, k)
        _upload(engine, ens)
        for est in (1, 2):
            got = engine.compute(Measure.MUTUAL_INFORMATION_KRASKOV, KRASKOV_REF, k=k, kraskov_estimator_index=est)
            assert engine.last_kernel_name() == VARIANTS[variant]
            _compare(got, _want_kraskov(ref, cs, k, est), f"{variant} KSG-{est} cs={cs} k={k}", 0.99)
            assert np.isnan(got[1, 2, 3])


@pytest.mark.gpu
@pytest.mark.parametrize("k,cs,expected", DEFAULT_DISPATCH)
def test_kraskov_default_dispatch(engine, ref, k, cs, expected):
    ens, _ = _kraskov_inputs(cs, k)
    _upload(engine, ens)
    for est in (1, 2):
        got = engine.compute(Measure.MUTUAL_INFORMATION_KRASKOV, KRASKOV_REF, k=k, kraskov_estimator_index=est)
        if expected is not None:
            assert engine.last_kernel_name() == expected
        _compare(got, _want_kraskov(ref, cs, k, est), f"default dispatch KSG-{est} cs={cs} k={k}", 0.99)


BOX_REF = (5, 2, 1)


def _box_inputs():
    ens = synth.box_ensemble(*GRID, 64, seed=21)
    x, y, z = BOX_REF
    return ens, ens[:, z, y, x].copy()


def _want_box(ref):
    ens, refv = _box_inputs()
    return ref.mi_field(oracle_lib.KMI_CC, ens, refv, k=3)


@pytest.mark.gpu
def test_kraskov_box_ensemble_with_exact_ties(engine, ref):
    """Plateaus of the box ensemble and the reference voxel itself are exact ties, resolved by the noise stream, which
    kernel, oracle and the stand-in generator share."""
    ens, _ = _box_inputs()
    _upload(engine, ens)
    got = engine.compute(Measure.KMI_CORRELATION_COEFFICIENT, BOX_REF, k=3)
    _compare(got, _want_box(ref), "KMI-CC box ensemble cs=64", 0.98)
    assert ((got >= 0) & (got <= 1)).all()


# --- DKL -----------------------------------------------------------------------------------------------------------
DKL_MEMBER_COUNTS = [16, 96, 97, 300]          # 96 / 97: the boundary of the register form
DKL_BINS, DKL_KS = (10, 80), (1, 3)


def _dkl_inputs(cs):
    return _dkl_ensemble(cs, 10 + cs, shape=(GRID[2], GRID[1], GRID[0]))


def _want_dkl(ref, cs, estimator, value):
    ens = _dkl_inputs(cs)
    return ref.dkl_field(0, ens, num_bins=value) if estimator == "binned" else ref.dkl_field(1, ens, k=value)


@pytest.mark.gpu
@pytest.mark.parametrize("cs", DKL_MEMBER_COUNTS)
def test_dkl_kernels(engine, ref, cs):
    _upload(engine, _dkl_inputs(cs))
    for bins in DKL_BINS:
        got = engine.dkl("binned", num_bins=bins)
        assert engine.last_kernel_name() == "dkl_kernel"
        _compare(got, _want_dkl(ref, cs, "binned", bins), f"DKL binned cs={cs} bins={bins}", 0.98)
    for k in DKL_KS:
        got = engine.dkl("knn", k=k)
        assert engine.last_kernel_name() == "dkl_kernel"
        _compare(got, _want_dkl(ref, cs, "knn", k), f"DKL k-NN cs={cs} k={k}", 0.98)
        assert np.isnan(got[0, 0, 3])                                  # a NaN member


# --- symmetric mode ------------------------------------------------------------------------------------------------
SYMMETRIC_MEMBER_COUNTS = [50, 100]


def _symmetric_inputs(cs):
    a, b = _two_fields(cs, shape=(GRID[2], GRID[1], GRID[0]), seed=100 + cs)
    b *= 3.0                                        # the two normalisations differ
    return a, b, _minmax(a), _minmax(b)


def _want_symmetric(ref, cs, measure):
    a, b, mm_a, mm_b = _symmetric_inputs(cs)
    return ref.mi_symmetric_field(measure, a, b, k=3, num_bins=20, minmax_ref=mm_a, minmax_query=mm_b)


@pytest.mark.gpu
@pytest.mark.parametrize("cs", SYMMETRIC_MEMBER_COUNTS)
def test_symmetric_mode(engine, ref, cs):
    a, b, mm_a, mm_b = _symmetric_inputs(cs)
    _upload(engine, a)
    engine.upload_secondary_members(b)
    assert engine.member_minmax() == mm_a and engine.secondary_member_minmax() == mm_b
    for measure, omeasure, kernel in ((Measure.MUTUAL_INFORMATION_BINNED, oracle_lib.MI_BINNED, "sorted_symmetric_kernel"),
                                      (Measure.MUTUAL_INFORMATION_KRASKOV, oracle_lib.MI_KRASKOV, "kraskov_direct_kernel")):
        got = engine.compute(measure, symmetric=True, k=3, num_bins=20)
        assert engine.last_kernel_name() == kernel
        _compare(got, _want_symmetric(ref, cs, omeasure), f"symmetric {measure.name} cs={cs}", 0.99)


# --- pair requests -------------------------------------------------------------------------------------------------
PAIR_MEMBER_COUNTS = [64, 300]                 # the sorted two-vector kernel / the any-member-count kernel


def _want_pairs(ref, cs, measure):
    ens, _, ii, jj = _pair_case(cs, 900 + cs)
    return ref.mi_pair_requests(measure, ens, ii, jj, k=3, num_bins=80)


@pytest.mark.gpu
@pytest.mark.parametrize("cs", PAIR_MEMBER_COUNTS)
def test_pair_requests(engine, ref, cs):
    ens, pairs, _, _ = _pair_case(cs, 900 + cs)
    _upload(engine, ens)
    got = engine.compute_requests(Measure.MUTUAL_INFORMATION_BINNED, pairs, num_bins=80)
    assert engine.last_kernel_name() == ("sorted_request_kernel" if cs <= 128 else "pair_request_kernel")
    _compare(got, _want_pairs(ref, cs, oracle_lib.MI_BINNED), f"pairs binned cs={cs}", None)
    got = engine.compute_requests(Measure.MUTUAL_INFORMATION_KRASKOV, pairs, k=3)
    _compare(got, _want_pairs(ref, cs, oracle_lib.MI_KRASKOV), f"pairs kraskov cs={cs}", None)


def record_reference_calls(ref):
    """Every call of the reference that the tests above make (oracle/make_golden.py, with a recording `ref`)."""
    for cs, bins in BINNED:
        _want_binned(ref, cs, bins)
    _want_binned(ref, 64, 80, oracle_lib.BINNED_MI_CC)
    for r in BINNED_INF_REFS:
        _want_binned_inf(ref, r)
    for r in NARROW_REFS:
        _want_narrow(ref, r)
    for cs, k, est in VARIANT_CASES:
        _want_kraskov(ref, cs, k, est)
    for k, cs, _ in DEFAULT_DISPATCH:
        for est in (1, 2):
            _want_kraskov(ref, cs, k, est)
    _want_box(ref)
    for cs in DKL_MEMBER_COUNTS:
        for bins in DKL_BINS:
            _want_dkl(ref, cs, "binned", bins)
        for k in DKL_KS:
            _want_dkl(ref, cs, "knn", k)
    for cs in SYMMETRIC_MEMBER_COUNTS:
        for m in (oracle_lib.MI_BINNED, oracle_lib.MI_KRASKOV):
            _want_symmetric(ref, cs, m)
    for cs in PAIR_MEMBER_COUNTS:
        for m in (oracle_lib.MI_BINNED, oracle_lib.MI_KRASKOV):
            _want_pairs(ref, cs, m)
