"""GPU parity of the counting kernels (kernels_generic.hip) on the paths the other test files do not reach:
direct_symmetric_kernel at small member counts (CRF_SYMMETRIC_DIRECT=1) and for binned MI above 128 members,
pair_request_kernel without a request list (symmetric Kraskov with min(k, cs - 1) > 64) and at small member counts
(CRF_REQUESTS_GENERIC=1).  12x10x4 grid: 480 voxels, so the last 64-voxel tile is ragged."""
import numpy as np
import pytest

from correrender_amd import Measure
from parity import assert_bit_exact, assert_close
import oracle_lib
from test_gpu_field_modes import _setup, _two_fields
from test_pair_requests import _case

pytestmark = pytest.mark.gpu

SHAPE = (4, 10, 12)     # (zs, ys, xs)
BINNED = [(Measure.MUTUAL_INFORMATION_BINNED, oracle_lib.MI_BINNED),
          (Measure.BINNED_MI_CORRELATION_COEFFICIENT, oracle_lib.BINNED_MI_CC)]


def _fields(cs, seed):
    a, b = _two_fields(cs, shape=SHAPE, seed=seed)
    a[:, 1, 2, 1] = np.round(a[:, 1, 2, 1])         # ties
    b[:, 1, 2, 2] = np.round(b[:, 1, 2, 2] * 2)
    b[:, 1, 1, 1] = 2.5                             # constant vector
    a[cs // 2, 2, 3, 4] = np.nan                    # NaN on each side
    b[0, 3, 1, 2] = np.nan
    return a, b


def _check_binned(engine, oracle, a, b, num_bins, what):
    mm_a, mm_b = oracle.minmax(a), oracle.minmax(b)
    for m, om in BINNED:
        got = engine.compute(m, symmetric=True, num_bins=num_bins)
        assert engine.last_kernel_name() == "direct_symmetric_kernel"
        want = oracle.symmetric_field(om, a, b, num_bins=num_bins, minmax_ref=mm_a, minmax_query=mm_b)
        assert_close(got, want, f"{what} {m.name}")
        g = got.reshape(SHAPE)
        assert np.isnan(g[2, 3, 4]) and np.isnan(g[3, 1, 2])


@pytest.mark.parametrize("cs", [2, 15, 16, 17, 33])
def test_direct_symmetric_small_member_counts(engine, oracle, monkeypatch, cs):
    """One, two and three 16-row sweeps and both sides of a full sweep."""
    monkeypatch.setenv("CRF_SYMMETRIC_DIRECT", "1")
    a, b = _fields(cs, 2000 + cs)
    _setup(engine, a, b)
    for m, om in ((Measure.SPEARMAN, oracle_lib.SPEARMAN), (Measure.KENDALL, oracle_lib.KENDALL)):
        got = engine.compute(m, symmetric=True)
        assert engine.last_kernel_name() == "direct_symmetric_kernel"
        assert_bit_exact(got, oracle.symmetric_field(om, a, b), f"direct symmetric {m.name} cs={cs}")
    _check_binned(engine, oracle, a, b, 20, f"direct symmetric cs={cs}")
    # max_y = inf: finite samples normalise to 0 and inf/inf is skipped, so that voxel takes the division form
    b[cs - 1, 1, 4, 5] = np.inf
    engine.upload_secondary_members(b)
    _check_binned(engine, oracle, a, b, 20, f"direct symmetric (skipped samples) cs={cs}")


@pytest.mark.parametrize("num_bins", [20, 255])
@pytest.mark.parametrize("cs", [129, 150])
def test_direct_symmetric_binned_above_128_members(engine, oracle, cs, num_bins):
    a, b = _fields(cs, 2200 + cs)
    b *= 3.0                                        # different value ranges: the two normalisations differ
    _setup(engine, a, b)
    _check_binned(engine, oracle, a, b, num_bins, f"direct symmetric cs={cs} bins={num_bins}")


@pytest.mark.parametrize("cs,k", [(70, 65), (130, 70)])
def test_symmetric_kraskov_without_request_list(engine, oracle, cs, k):
    """min(k, cs - 1) > 64: the symmetric Kraskov kernel declines and pair_request_kernel evaluates voxel pair (v, v);
    its tile is in LDS at 70 members and in the workspace at 130."""
    a, b = _fields(cs, 2400 + cs)
    _setup(engine, a, b)
    for m, om in ((Measure.MUTUAL_INFORMATION_KRASKOV, oracle_lib.MI_KRASKOV),
                  (Measure.KMI_CORRELATION_COEFFICIENT, oracle_lib.KMI_CC)):
        got = engine.compute(m, symmetric=True, k=k)
        assert engine.last_kernel_name() == "pair_request_kernel"
        assert_close(got, oracle.symmetric_field(om, a, b, k=k), f"symmetric {m.name} cs={cs} k={k}")
        g = got.reshape(SHAPE)
        assert np.isnan(g[2, 3, 4]) and np.isnan(g[3, 1, 2])


@pytest.mark.parametrize("cs", [2, 16, 17])
def test_pair_requests_counting_kernel_small_member_counts(engine, oracle, monkeypatch, cs):
    monkeypatch.setenv("CRF_REQUESTS_GENERIC", "1")
    ens, pairs, ii, jj = _case(cs, 2600 + cs, n=400 + cs % 7)     # request counts that are not a multiple of 64
    _, zs, ys, xs = ens.shape
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(ens)
    k = min(3, cs - 1)
    for m, om, kw in ((Measure.PEARSON, 0, {}), (Measure.SPEARMAN, 1, {}), (Measure.KENDALL, 2, {}),
                      (Measure.MUTUAL_INFORMATION_BINNED, 3, dict(num_bins=80)),
                      (Measure.MUTUAL_INFORMATION_KRASKOV, 4, dict(k=k)),
                      (Measure.BINNED_MI_CORRELATION_COEFFICIENT, 5, dict(num_bins=40)),
                      (Measure.KMI_CORRELATION_COEFFICIENT, 6, dict(k=k))):
        check = assert_bit_exact if om <= 2 else assert_close
        for use_abs in (False, True):
            got = engine.compute_requests(m, pairs, absolute_value=use_abs, **kw)
            assert engine.last_kernel_name() == "pair_request_kernel"
            check(got, oracle.pair_requests(om, ens, ii, jj, use_abs=use_abs, **kw),
                  f"counting-kernel pairs {'|' if use_abs else ''}{m.name} cs={cs}")
