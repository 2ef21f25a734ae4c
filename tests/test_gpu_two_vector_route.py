"""GPU: the two-vector route table (correrender_amd/csrc/two_vector_route.h) against what actually runs.  At the boundaries of
the table -- 1, 2, 16, 17, 128 and 129 members, Kraskov with k either side of the direct kernel's 64 neighbours, binned
with the largest bin count -- the kernel the library reports is the one two_vector_rule (tests/test_two_vector_route.py,
the documented rules; the CPU test pins the C++ table to it) names, in the symmetric field mode and in request mode, and
the values are the oracle's, so a wrong route that still reports the right name cannot pass.  The grid has 480 voxels and
the request list 333 entries: the last wave and the last 256-lane block are ragged in both modes."""
import numpy as np
import pytest

from correrender_amd import CorrFieldError, Measure
from parity import assert_bit_exact, assert_close
from test_two_vector_route import two_vector_rule

pytestmark = pytest.mark.gpu

XS, YS, ZS = 12, 10, 4
NUM_REQUESTS = 333
MEASURES = [(Measure.PEARSON, 0), (Measure.SPEARMAN, 1), (Measure.KENDALL, 2), (Measure.MUTUAL_INFORMATION_BINNED, 3),
            (Measure.MUTUAL_INFORMATION_KRASKOV, 4), (Measure.BINNED_MI_CORRELATION_COEFFICIENT, 5),
            (Measure.KMI_CORRELATION_COEFFICIENT, 6)]


def _setup(engine, cs, seed):
    """Two correlated fields without ties or NaN (the neighbouring suites cover those), and a request list."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((cs, ZS, YS, XS)).astype(np.float32)
    b = (0.6 * a + 0.8 * rng.standard_normal(a.shape)).astype(np.float32)
    pairs = np.stack([rng.integers(0, XS, NUM_REQUESTS), rng.integers(0, YS, NUM_REQUESTS), rng.integers(0, ZS, NUM_REQUESTS),
                      rng.integers(0, XS, NUM_REQUESTS), rng.integers(0, YS, NUM_REQUESTS), rng.integers(0, ZS, NUM_REQUESTS)],
                     axis=1)
    pairs[0] = [3, 2, 1, 3, 2, 1]                   # a voxel with itself
    idx = lambda p: (p[:, 2] * YS + p[:, 1]) * XS + p[:, 0]
    engine.set_grid(XS, YS, ZS, cs)
    engine.upload_members(a)
    engine.upload_secondary_members(b)
    return a, b, pairs, idx(pairs[:, 0:3]), idx(pairs[:, 3:6])


def _check(got, want, omeasure, what):
    if omeasure <= 2:
        assert_bit_exact(got, want, what)
    else:
        assert_close(got, want, what)


def _both_modes(engine, oracle, data, measure, omeasure, k, num_bins):
    a, b, pairs, ii, jj = data
    cs = a.shape[0]
    got = engine.compute(measure, symmetric=True, k=k, num_bins=num_bins)
    assert engine.last_kernel_name() == two_vector_rule(False, omeasure, cs, k, num_bins)[1], f"symmetric {measure.name} cs={cs}"
    want = oracle.symmetric_field(omeasure, a, b, k=k, num_bins=num_bins, minmax_ref=oracle.minmax(a),
                                  minmax_query=oracle.minmax(b))
    _check(got, want, omeasure, f"symmetric {measure.name} cs={cs} k={k} bins={num_bins}")
    got = engine.compute_requests(measure, pairs, k=k, num_bins=num_bins)
    assert engine.last_kernel_name() == two_vector_rule(True, omeasure, cs, k, num_bins)[1], f"requests {measure.name} cs={cs}"
    want = oracle.pair_requests(omeasure, a, ii, jj, k=k, num_bins=num_bins)
    _check(got, want, omeasure, f"requests {measure.name} cs={cs} k={k} bins={num_bins}")


@pytest.mark.parametrize("cs", [1, 2, 16, 17, 128, 129])
def test_reported_kernel_is_the_routed_one(engine, oracle, cs):
    data = _setup(engine, cs, 4100 + cs)
    for measure, omeasure in MEASURES:
        _both_modes(engine, oracle, data, measure, omeasure, k=min(3, max(cs - 1, 1)), num_bins=80)


@pytest.mark.parametrize("k", [64, 65])
def test_kraskov_either_side_of_the_direct_kernels_limit(engine, oracle, k):
    """70 members: the symmetric direct kernel keeps at most 64 neighbours, one more goes to pair_request_kernel."""
    data = _setup(engine, 70, 4200)
    assert two_vector_rule(False, 4, 70, k)[0] == ("KraskovDirect" if k == 64 else "PairRequest")
    for measure, omeasure in (MEASURES[4], MEASURES[6]):
        _both_modes(engine, oracle, data, measure, omeasure, k=k, num_bins=80)


@pytest.mark.parametrize("cs", [16, 129])
def test_binned_at_the_largest_bin_count(engine, oracle, cs):
    """255 bins is the last count whose bin codes fit a byte; 256 is turned away before any route is taken."""
    data = _setup(engine, cs, 4300 + cs)
    for measure, omeasure in (MEASURES[3], MEASURES[5]):
        _both_modes(engine, oracle, data, measure, omeasure, k=3, num_bins=255)
        with pytest.raises(CorrFieldError, match="num_bins"):
            engine.compute(measure, symmetric=True, num_bins=256)
        with pytest.raises(CorrFieldError, match="num_bins"):
            engine.compute_requests(measure, data[2], num_bins=256)
