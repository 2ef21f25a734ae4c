"""GPU parity of the any-member-count kernels at the top of their range (1000 .. 2048 members, kMaxGenericMembers) and
on both sides of the LDS limits that choose their branches, vs the oracle.

The branches are chosen by member count, bin count and k, never by the grid, so the grid is 7 x 6 x 5 = 210 voxels: three
full 64-voxel tiles and a ragged tile of 18.  Member counts: 1001 (just above the reference's own 1000-member data set),
1024, 1706 / 1707 (the last count kraskov_direct_kernel accepts and the first it declines: kraskov_plan.h), 2047 / 2048
(the limit).  Every ensemble is built once per module and shared read-only."""
import functools

import numpy as np
import pytest

from correrender_amd import Measure, synth
from parity import assert_bit_exact, assert_close, bit_identical
import oracle_lib

pytestmark = pytest.mark.gpu

XS, YS, ZS = 7, 6, 5
REF = (3, 2, 2)                                   # (x, y, z): none of the planted voxels
FIELD_MEMBER_COUNTS = [1001, 1024, 1706, 1707, 2047, 2048]
KRASKOV_DIRECT_MAX_MEMBERS = 1706                 # 3 * cs * 8 + kDirectSumBytes (20480) <= 60 KiB: 61424 at 1706, 61448 at 1707

BINNED = ((Measure.MUTUAL_INFORMATION_BINNED, oracle_lib.MI_BINNED),
          (Measure.BINNED_MI_CORRELATION_COEFFICIENT, oracle_lib.BINNED_MI_CC))
EXACT = ((Measure.PEARSON, oracle_lib.PEARSON), (Measure.SPEARMAN, oracle_lib.SPEARMAN),
         (Measure.KENDALL, oracle_lib.KENDALL))


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays[0] if len(arrays) == 1 else arrays


def _ref_vector(ens):
    return ens[:, REF[2], REF[1], REF[0]].copy()


def _plant(ens, ties=True):
    """A voxel dependent on the reference, a NaN member and (ties) a voxel of rounded values and a constant voxel."""
    ens[:, 0, 0, 4] = 0.8 * _ref_vector(ens) + 0.2 * ens[:, 0, 0, 4]
    ens[3, 0, 0, 3] = np.nan
    if ties:
        ens[:, 0, 0, 1] = np.round(ens[:, 0, 0, 1] * 2)
        ens[:, 0, 0, 2] = 1.25
    return ens


@functools.lru_cache(maxsize=None)
def _box(cs):
    return _frozen(_plant(synth.box_ensemble(XS, YS, ZS, cs, seed=3000 + cs)))


@functools.lru_cache(maxsize=None)
def _normal(cs):
    return _frozen(_plant(synth.normal_ensemble(XS, YS, ZS, cs, seed=4000 + cs), ties=False))


def _upload(engine, ens):
    cs, zs, ys, xs = ens.shape
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(ens)


# ---- A. field mode ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", FIELD_MEMBER_COUNTS)
def test_rank_fields_bit_exact(engine, oracle, cs):
    """direct_rank_kernel: the doubled ranks reach 2 * cs - 1 = 4095 in a uint16_t column, Kendall's pair counts
    cs * (cs - 1) / 2 = 2.1e6; spearman_prep_kernel and kendall_prep_kernel (n_pad = cs) run as one block."""
    ens = _box(cs)
    _upload(engine, ens)
    for ref_values in (_ref_vector(ens), np.round(ens[:, 1, 1, 1] * 3)):            # without / with x ties
        for m, om in EXACT[1:]:
            got = engine.compute(m, reference_values=ref_values)
            assert engine.last_kernel_name() == "direct_rank_kernel"
            assert_bit_exact(got, oracle.field(om, ens, ref_values), f"upper {m.name} cs={cs}")
    for m, om in EXACT[1:]:                                                           # the gather fused into the preparation
        got = engine.compute(m, REF)
        assert engine.last_kernel_name() == "direct_rank_kernel"
        assert_bit_exact(got, oracle.field(om, ens, _ref_vector(ens)), f"upper {m.name} at {REF} cs={cs}")


@pytest.mark.parametrize("cs", [2048, 2049, 4096])
def test_pearson_field_bit_exact(engine, oracle, cs):
    ens = _box(cs)
    _upload(engine, ens)
    got = engine.compute(Measure.PEARSON, REF)
    assert engine.last_kernel_name() == "pearson_big_kernel"
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, ens, _ref_vector(ens)), f"upper PEARSON cs={cs}")


@pytest.mark.parametrize("cs", FIELD_MEMBER_COUNTS)
def test_binned_field_80_bins(engine, oracle, cs):
    """80 bins: rows = 80 * 384 = 30720 bytes, rows + 8 * cs <= 47104 at 2048 members: the difference table is in LDS."""
    ens = _box(cs)
    _upload(engine, ens)
    mm = engine.member_minmax()
    assert mm == oracle.minmax(ens)
    ref_values = _ref_vector(ens)
    for m, om in BINNED:
        got = engine.compute(m, REF, num_bins=80, minmax_ref=mm, minmax_query=mm)
        assert engine.last_kernel_name() == "mi_binned_hist_kernel"
        want = oracle.field(om, ens, ref_values, num_bins=80, minmax_ref=mm)
        assert_close(got, want, f"upper {m.name} cs={cs}")
        share = bit_identical(got, want).mean()
        print(f"{m.name} cs={cs}: {share:.4f} of the voxels bit-identical")
        assert share > 0.98


def _kraskov_kernel(cs, k):
    """kraskov_direct_plan: min(k, cs - 1) <= 128 and the three tables within LDS, else generic_kernel."""
    return "kraskov_direct_kernel" if min(k, cs - 1) <= 128 and cs <= KRASKOV_DIRECT_MAX_MEMBERS else "generic_kernel"


def _default_k(cs):
    return -(-3 * cs // 100)


@pytest.mark.parametrize("est", [1, 2])
@pytest.mark.parametrize("k", [3, "default", 64, 128, 129])
@pytest.mark.parametrize("cs", FIELD_MEMBER_COUNTS)
def test_kraskov_field(engine, oracle, cs, k, est):
    """Tie-free data.  K = 3 exactly, then the wide instantiations K = 32 (k = 31), K = 64 (k = 52, 64) and K = 128, which
    below this file only ran up to 160 members; k = 129, and every k from 1707 members: generic_kernel, its tile of
    cs * 64 * 6 bytes in the global workspace, the k-th neighbour by minimum passes (k = 3) and by pivots (k > 16)."""
    k = _default_k(cs) if k == "default" else k
    ens = _normal(cs)
    _upload(engine, ens)
    got = engine.compute(Measure.MUTUAL_INFORMATION_KRASKOV, REF, k=k, kraskov_estimator_index=est)
    assert engine.last_kernel_name() == _kraskov_kernel(cs, k)
    want = oracle.field(oracle_lib.MI_KRASKOV, ens, _ref_vector(ens), k=k, estimator=est)
    assert_close(got, want, f"upper KSG-{est} cs={cs} k={k}")


@pytest.mark.parametrize("k", [3, 64])
@pytest.mark.parametrize("cs", [1706, 1707])
def test_kmi_cc_field_on_tied_data(engine, oracle, cs, k):
    """The box ensemble with its rounded and constant voxels: exact ties, resolved by the noise stream that the kernels
    and the oracle share."""
    ens = _box(cs)
    _upload(engine, ens)
    got = engine.compute(Measure.KMI_CORRELATION_COEFFICIENT, REF, k=k)
    assert engine.last_kernel_name() == _kraskov_kernel(cs, k)
    assert_close(got, oracle.field(oracle_lib.KMI_CC, ens, _ref_vector(ens), k=k), f"upper KMI-CC cs={cs} k={k}")


# ---- B. mi_binned_hist_kernel: both placements of the difference table, and its O(cs^2) path -----------------------------
# rows = num_bins * 64 * 6 = num_bins * 384 bytes of LDS histogram rows (the kernel declines above 56 KiB: 150 bins);
# T[c + 1] - T[c] for c < cs lies behind them in LDS when rows + 8 * cs <= 60 KiB = 61440, else it is formed from the
# table in global memory.
HIST_CASES = [
    # cs, num_bins, table in LDS
    (528, 149, True),       # 57216 + 4224  = 61440
    (529, 149, False),      # 57216 + 4232  = 61448
    (1001, 149, False),     # 57216 + 8008  = 65224
    (2048, 117, True),      # 44928 + 16384 = 61312
    (2048, 118, False),     # 45312 + 16384 = 61696
]
INF_VOXEL = (1, 1, 1)                             # (x, y, z): two members are +inf here


@functools.lru_cache(maxsize=None)
def _box_with_infinities(cs):
    ens = _box(cs).copy()
    ens[5, 1, 1, 1] = ens[9, 1, 1, 1] = np.inf
    ens[7, 3, 4, 5] = np.inf
    return _frozen(ens)


def _hist_case_arithmetic(cs, num_bins, in_lds):
    rows = num_bins * 64 * 6
    assert rows <= 56 * 1024 and (rows + 8 * cs <= 60 * 1024) == in_lds


@pytest.mark.parametrize("cs,num_bins,in_lds", HIST_CASES)
def test_histogram_kernel_table_placements(engine, oracle, cs, num_bins, in_lds):
    _hist_case_arithmetic(cs, num_bins, in_lds)
    ens = _box(cs)
    _upload(engine, ens)
    mm = engine.member_minmax()
    assert mm == oracle.minmax(ens)
    for m, om in BINNED:
        got = engine.compute(m, REF, num_bins=num_bins, minmax_ref=mm, minmax_query=mm)
        assert engine.last_kernel_name() == "mi_binned_hist_kernel"
        assert_close(got, oracle.field(om, ens, _ref_vector(ens), num_bins=num_bins, minmax_ref=mm),
                     f"histogram {m.name} cs={cs} bins={num_bins} table in {'LDS' if in_lds else 'global memory'}")


@pytest.mark.parametrize("ref", [REF, INF_VOXEL], ids=["finite_reference", "reference_holds_inf"])
@pytest.mark.parametrize("cs,num_bins,in_lds", HIST_CASES)
def test_histogram_kernel_skipped_samples(engine, oracle, cs, num_bins, in_lds, ref):
    """max = +inf: every finite sample normalises to 0 and inf / inf is skipped.  At the voxels that hold an inf
    total != cs; with the reference point on one of them the reference vector has invalid bins (ref_all_valid is false)
    and every voxel takes the O(cs^2) path."""
    _hist_case_arithmetic(cs, num_bins, in_lds)
    ens = _box_with_infinities(cs)
    _upload(engine, ens)
    mm = engine.member_minmax()
    assert mm == oracle.minmax(ens) and mm[1] == np.inf
    ref_values = ens[:, ref[2], ref[1], ref[0]].copy()
    assert np.isinf(ref_values).any() == (ref == INF_VOXEL)
    for m, om in BINNED:
        got = engine.compute(m, ref, num_bins=num_bins, minmax_ref=mm, minmax_query=mm)
        assert engine.last_kernel_name() == "mi_binned_hist_kernel"
        assert_close(got, oracle.field(om, ens, ref_values, num_bins=num_bins, minmax_ref=mm),
                     f"histogram, skipped samples, {m.name} cs={cs} bins={num_bins} ref={ref}")


@pytest.mark.parametrize("cs,num_bins,in_lds", HIST_CASES)
def test_histogram_kernel_reference_with_invalid_samples(engine, oracle, cs, num_bins, in_lds):
    """With an infinite maximum every valid sample is in bin 0 and the O(cs^2) path can only answer 0.  A reference vector
    with NaN members and finite extrema takes the same path (ref_all_valid is false, total = cs - 3 at every voxel) over
    all the bins: the reference skips a sample whose normalised reference value is NaN and does not look for NaN in the
    reference vector."""
    _hist_case_arithmetic(cs, num_bins, in_lds)
    ens = _box(cs)
    _upload(engine, ens)
    mm = oracle.minmax(ens)
    ref_values = _ref_vector(ens)
    ref_values[[4, cs // 2, cs - 1]] = np.nan
    for m, om in BINNED:
        got = engine.compute(m, reference_values=ref_values, num_bins=num_bins, minmax_ref=mm, minmax_query=mm)
        assert engine.last_kernel_name() == "mi_binned_hist_kernel"
        want = oracle.field(om, ens, ref_values, num_bins=num_bins, minmax_ref=mm)
        assert np.nanmax(want) > 0.1
        assert_close(got, want, f"histogram, NaN in the reference vector, {m.name} cs={cs} bins={num_bins}")


# ---- C. symmetric mode --------------------------------------------------------------------------------------------------
SYMMETRIC_MEMBER_COUNTS = [1001, 1706, 1707, 2048]


@functools.lru_cache(maxsize=None)
def _two_fields(cs, rho=0.6):
    """As test_gpu_field_modes._two_fields, with its planted voxels, on the 7 x 6 x 5 grid."""
    rng = np.random.default_rng(5000 + cs)
    shape = (cs, ZS, YS, XS)
    a = rng.standard_normal(shape).astype(np.float32)
    b = (rho * a + np.sqrt(1 - rho * rho) * rng.standard_normal(shape)).astype(np.float32)
    b[:, 0, 0, :] = a[:, 0, 0, :]                   # identical vectors
    b[:, 0, 1, :] = -2.0 * a[:, 0, 1, :]            # exactly anti-correlated
    a[1, 2, 3, 4] = np.nan                          # NaN on the reference side
    b[0, 3, 1, 2] = np.nan                          # NaN on the query side
    b[:, 1, 1, 1] = 2.5                             # constant query vector
    a[:, 1, 2, 1] = np.round(a[:, 1, 2, 1])         # ties
    return _frozen(a, b)


def _upload_two(engine, a, b):
    _upload(engine, a)
    engine.upload_secondary_members(b)


@pytest.mark.parametrize("cs", SYMMETRIC_MEMBER_COUNTS)
def test_symmetric_exact_measures(engine, oracle, cs):
    a, b = _two_fields(cs)
    _upload_two(engine, a, b)
    for m, om in EXACT:
        got = engine.compute(m, symmetric=True)
        # Pearson beyond 128 members: the request kernel without a request list
        assert engine.last_kernel_name() == ("pair_request_kernel" if m == Measure.PEARSON else "direct_symmetric_kernel")
        assert_bit_exact(got, oracle.symmetric_field(om, a, b), f"upper symmetric {m.name} cs={cs}")
        g = got.reshape(a.shape[1:])
        assert np.isnan(g[2, 3, 4]) and np.isnan(g[3, 1, 2])


@pytest.mark.parametrize("num_bins", [20, 149])
@pytest.mark.parametrize("cs", SYMMETRIC_MEMBER_COUNTS)
def test_symmetric_binned(engine, oracle, cs, num_bins):
    a, b = _two_fields(cs)
    _upload_two(engine, a, b)
    mm_a, mm_b = engine.member_minmax(), engine.secondary_member_minmax()
    assert mm_a == oracle.minmax(a) and mm_b == oracle.minmax(b)
    got = engine.compute(Measure.MUTUAL_INFORMATION_BINNED, symmetric=True, num_bins=num_bins)
    assert engine.last_kernel_name() == "direct_symmetric_kernel"
    want = oracle.symmetric_field(oracle_lib.MI_BINNED, a, b, num_bins=num_bins, minmax_ref=mm_a, minmax_query=mm_b)
    assert_close(got, want, f"upper symmetric binned cs={cs} bins={num_bins}")


def _symmetric_kraskov_direct(cs, k):
    return k <= 64 and cs <= KRASKOV_DIRECT_MAX_MEMBERS


@pytest.mark.parametrize("k", [3, 64, 65])
@pytest.mark.parametrize("cs", SYMMETRIC_MEMBER_COUNTS)
def test_symmetric_kraskov(engine, oracle, cs, k):
    """kraskov_symmetric_plan: k <= 64 and the tables within LDS (up to 1706 members), else the request kernel without a
    request list, whose tile of cs * 64 * 12 bytes is in the global workspace."""
    a, b = _two_fields(cs)
    _upload_two(engine, a, b)
    got = engine.compute(Measure.MUTUAL_INFORMATION_KRASKOV, symmetric=True, k=k)
    direct = _symmetric_kraskov_direct(cs, k)
    assert engine.last_kernel_name() == ("kraskov_direct_kernel" if direct else "pair_request_kernel")
    assert_close(got, oracle.symmetric_field(oracle_lib.MI_KRASKOV, a, b, k=k), f"upper symmetric Kraskov cs={cs} k={k}")


# ---- D. pair requests ---------------------------------------------------------------------------------------------------

def _requests(seed, n, grid):
    xs, ys, zs = grid
    rng = np.random.default_rng(seed)
    pairs = np.stack([rng.integers(0, xs, n), rng.integers(0, ys, n), rng.integers(0, zs, n),
                      rng.integers(0, xs, n), rng.integers(0, ys, n), rng.integers(0, zs, n)], axis=1)
    pairs[0] = [1, 0, 0, 1, 0, 0]                          # a voxel with itself (ties)
    pairs[1] = [2, 0, 0, 5, 5, 3]                          # constant vs random -> 0/0
    pairs[2] = [3, 0, 0, 4, 4, 2]                          # NaN
    pairs[3] = [4, 4, 2, 4, 4, 2]                          # identical vectors
    idx = lambda p: (p[:, 2] * ys + p[:, 1]) * xs + p[:, 0]
    return pairs, idx(pairs[:, 0:3]), idx(pairs[:, 3:6])


@pytest.mark.parametrize("cs", [1000, 2048])
def test_pair_requests_exact_measures(engine, oracle, cs):
    """150 requests: two tiles and a ragged one of 22; pair_tile_bytes(cs) = cs * 768 is far beyond LDS."""
    ens = _box(cs)
    pairs, ii, jj = _requests(6000 + cs, 150, (XS, YS, ZS))
    _upload(engine, ens)
    for m, om in EXACT:
        for use_abs in (False, True):
            got = engine.compute_requests(m, pairs, absolute_value=use_abs)
            assert engine.last_kernel_name() == "pair_request_kernel"
            assert_bit_exact(got, oracle.pair_requests(om, ens, ii, jj, use_abs=use_abs),
                             f"upper pairs {m.name} abs={use_abs} cs={cs}")


@pytest.mark.parametrize("m,om,kw", [(Measure.MUTUAL_INFORMATION_BINNED, 3, dict(num_bins=80)),
                                     (Measure.BINNED_MI_CORRELATION_COEFFICIENT, 5, dict(num_bins=40)),
                                     (Measure.MUTUAL_INFORMATION_KRASKOV, 4, dict(k=3)),
                                     (Measure.KMI_CORRELATION_COEFFICIENT, 6, dict(k=3))],
                         ids=["binned", "binned_cc", "kraskov", "kmi_cc"])
@pytest.mark.parametrize("cs", [1000, 2048])
def test_pair_requests_mutual_information(engine, oracle, cs, m, om, kw):
    ens = _box(cs)
    pairs, ii, jj = _requests(6000 + cs, 150, (XS, YS, ZS))
    _upload(engine, ens)
    got = engine.compute_requests(m, pairs, **kw)
    assert engine.last_kernel_name() == "pair_request_kernel"
    assert_close(got, oracle.pair_requests(om, ens, ii, jj, **kw), f"upper pairs {m.name} cs={cs}")
    assert np.isnan(got[2]) and not np.isnan(got[0])


def test_two_field_pair_requests_2048_members(engine, oracle):
    """query_from_secondary: the j side reads the second field.  Expectation as test_gpu_two_field_pair_requests: the
    oracle on the two fields stacked along z."""
    cs = 2048
    ens = _box(cs)
    rng = np.random.default_rng(7)
    second = (0.5 * ens + rng.standard_normal(ens.shape)).astype(np.float32)
    second[:, 0, 0, 1] = np.round(second[:, 0, 0, 1])
    pairs, ii, jj = _requests(6100, 150, (XS, YS, ZS))
    stacked = np.concatenate([ens, second], axis=1)
    jj2 = jj + XS * YS * ZS
    _upload(engine, ens)
    engine.upload_secondary_members(second)
    for m, om in EXACT:
        got = engine.compute_requests(m, pairs, query_from_secondary=True)
        assert engine.last_kernel_name() == "pair_request_kernel"
        assert_bit_exact(got, oracle.pair_requests(om, stacked, ii, jj2), f"upper two-field pairs {m.name}")
    got = engine.compute_requests(Measure.MUTUAL_INFORMATION_BINNED, pairs, num_bins=60, query_from_secondary=True)
    assert engine.last_kernel_name() == "pair_request_kernel"
    assert_close(got, oracle.pair_requests(3, stacked, ii, jj2, num_bins=60), "upper two-field pairs binned")


# ---- E. DKL -------------------------------------------------------------------------------------------------------------
DKL_MEMBER_COUNTS = [1000, 2047, 2048]


@functools.lru_cache(maxsize=None)
def _dkl_ensemble(cs):
    """The planted voxels of test_gpu_dkl._ensemble."""
    rng = np.random.default_rng(8000 + cs)
    ens = rng.standard_normal((cs, ZS, YS, XS)).astype(np.float32)
    ens[:, 0, 0, 0] = rng.uniform(-3, 5, cs)                  # uniform: DKL > 0
    ens[:, 0, 0, 1] = rng.exponential(2.0, cs)                # skewed
    ens[:, 0, 0, 2] = 4.0                                     # constant: stdev 0 -> NaN
    ens[cs // 2, 0, 0, 3] = np.nan                            # NaN member -> NaN
    ens[:, 0, 0, 4] = np.round(ens[:, 0, 0, 4])               # duplicates: k-NN distance 0 -> log 0 -> NaN
    ens[:, 0, 0, 5] = ens[:, 0, 0, 5] * 1e-3 + 1e4            # large offset, small spread
    return _frozen(ens)


@pytest.mark.parametrize("num_bins", [10, 80, 300])
@pytest.mark.parametrize("cs", DKL_MEMBER_COUNTS)
def test_dkl_binned(engine, oracle, cs, num_bins):
    ens = _dkl_ensemble(cs)
    _upload(engine, ens)
    got = engine.dkl("binned", num_bins=num_bins)
    assert engine.last_kernel_name() == "dkl_kernel"
    want = oracle.dkl(0, ens, num_bins=num_bins)
    assert_close(got, want, f"upper DKL binned cs={cs} bins={num_bins}")
    assert np.array_equal(np.isnan(got).reshape(-1), np.isnan(want)) and np.isnan(got[0, 0, 3])


@pytest.mark.parametrize("k", [1, "default", 128])
@pytest.mark.parametrize("cs", DKL_MEMBER_COUNTS)
def test_dkl_knn(engine, oracle, cs, k):
    k = _default_k(cs) if k == "default" else k
    ens = _dkl_ensemble(cs)
    _upload(engine, ens)
    got = engine.dkl("knn", k=k)
    assert engine.last_kernel_name() == "dkl_kernel"
    want = oracle.dkl(1, ens, k=k)
    assert_close(got, want, f"upper DKL k-NN cs={cs} k={k}")
    assert np.array_equal(np.isnan(got).reshape(-1), np.isnan(want))
    assert np.isnan(got[0, 0, 2]) and np.isnan(got[0, 0, 3]) and np.isnan(got[0, 0, 4])


# ---- F. more tiles than persistent blocks, the tile in the global workspace ----------------------------------------------

@pytest.mark.parametrize("cs", [81, 129])
def test_pair_requests_walk_several_workspace_tiles(engine, oracle, cs):
    """pair_tile_bytes(cs) = cs * 768: 62208 bytes at 81 members, the first count above 60 KiB, so the tile is the block's
    slice of the workspace; 65 611 requests = 1025 full tiles and a ragged one of 11 on kGenericBlocks = 1024 blocks:
    blocks 0 and 1 walk a second tile.  Up to 128 members Kendall and binned MI requests run in sorted_request_kernel, which
    has no tile, and only the Kraskov measures reach pair_request_kernel; 129 members is the first count at which Kendall
    and binned MI walk workspace tiles."""
    grid, n = (12, 10, 6), 65611
    assert cs * 64 * 12 > 60 * 1024 and n > 1024 * 64 and n % 64
    ens = synth.box_ensemble(*grid, cs, seed=900 + cs)
    ens[:, 0, 0, 1] = np.round(ens[:, 0, 0, 1] * 2)
    ens[:, 0, 0, 2] = 0.5
    ens[1, 0, 0, 3] = np.nan
    pairs, ii, jj = _requests(982, n, grid)
    pairs[-1] = pairs[0]                                    # the last request of the ragged tile: known ties
    ii[-1], jj[-1] = ii[0], jj[0]
    _upload(engine, ens)
    expect = "pair_request_kernel" if cs > 128 else "sorted_request_kernel"
    got = engine.compute_requests(Measure.KENDALL, pairs)
    assert engine.last_kernel_name() == expect
    assert_bit_exact(got, oracle.pair_requests(oracle_lib.KENDALL, ens, ii, jj), f"cs={cs} pairs Kendall, 1026 tiles")
    got = engine.compute_requests(Measure.MUTUAL_INFORMATION_BINNED, pairs, num_bins=80)
    assert engine.last_kernel_name() == expect
    assert_close(got, oracle.pair_requests(oracle_lib.MI_BINNED, ens, ii, jj, num_bins=80),
                 f"cs={cs} pairs binned MI, 1026 tiles")
    if cs <= 128:
        got = engine.compute_requests(Measure.MUTUAL_INFORMATION_KRASKOV, pairs, k=3)
        assert engine.last_kernel_name() == "pair_request_kernel"
        assert_close(got, oracle.pair_requests(oracle_lib.MI_KRASKOV, ens, ii, jj, k=3),
                     f"cs={cs} pairs Kraskov, 1026 workspace tiles")


def test_dkl_binned_walks_several_workspace_tiles(engine, oracle):
    """200 members and 100 bins: the tile is 64000 bytes, above the 60 KiB LDS limit; 41 x 40 x 40 = 65 600 voxels = 1025
    tiles on kDklBlocks = 1024 blocks: block 0 walks a second tile."""
    cs, (xs, ys, zs) = 200, (41, 40, 40)
    assert xs * ys * zs == 65600 and xs * ys * zs > 1024 * 64
    rng = np.random.default_rng(983)
    ens = rng.standard_normal((cs, zs, ys, xs), dtype=np.float32)
    ens[:, 0, 0, 0] = rng.uniform(-3, 5, cs)
    ens[:, 0, 0, 2] = 4.0
    ens[cs // 2, 0, 0, 3] = np.nan
    ens[:, -1, -1, -1] = rng.exponential(2.0, cs)           # the last voxel, in the tile that block 0 walks second
    _upload(engine, ens)
    got = engine.dkl("binned", num_bins=100)
    assert engine.last_kernel_name() == "dkl_kernel"
    want = oracle.dkl(0, ens, num_bins=100)
    assert_close(got, want, "DKL binned, 1025 workspace tiles")
    assert np.array_equal(np.isnan(got).reshape(-1), np.isnan(want))
