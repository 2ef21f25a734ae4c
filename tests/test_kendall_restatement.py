"""kendall_similarity_reference.kendall_restated -- what the GPU Kendall tests compare against -- checked four ways, none
of which needs a GPU: its level-by-level inversion count against the O(n^2) count of the reference's definition; its
integers, put through the <int32_t> tail, against the reference's own object code (ref_kendall, or its recorded answers
in tests/golden/reference/field_kendall_similarity_calls.npz), bit for bit; its value against scipy.stats.kendalltau on
tie-free data, where tau-b is tau-a and the reference's missing joint ties do not matter; and the survey's known answer.
The <int64_t> tail is restated, not pinned (see kendall_similarity_reference.py)."""
import numpy as np
import pytest

from kendall_similarity_reference import (KendallAnswers, f32_bits, inversions_slow, kendall_restated, pin_pair, tail_int32,
                                          tail_int64)
from rank_similarity_reference import PIN_KINDS, PIN_SIZES


@pytest.fixture(scope="module")
def ans():
    return KendallAnswers()


def _quantised(n, seed):
    rng = np.random.default_rng(seed)
    x = np.round(rng.standard_normal(n) * 2.0).astype(np.float32)
    y = np.round(0.5 * x + rng.standard_normal(n) * 2.0).astype(np.float32)
    return x, y


def _with_nans_and_zeros(n, seed):
    rng = np.random.default_rng(seed)
    x, y = _quantised(n, seed + 1)
    x[rng.random(n) < 0.2] = np.float32(-0.0)
    y[rng.random(n) < 0.2] = np.float32(0.0)
    x[rng.random(n) < 0.1] = np.float32(np.nan)
    y[rng.random(n) < 0.1] = np.float32(np.nan)
    return x, y


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 64, 65, 255, 1000, 2000])
def test_inversions_against_the_quadratic_count(n):
    rng = np.random.default_rng(n)
    cases = [(rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)), _quantised(n, n),
             _with_nans_and_zeros(n, n), (np.arange(n, dtype=np.float32), -np.arange(n, dtype=np.float32)),
             (np.zeros(n, np.float32), rng.standard_normal(n).astype(np.float32))]
    for i, (x, y) in enumerate(cases):
        kept, n0, n1, n2, s, _ = kendall_restated(x, y)
        assert kept == int((~(np.isnan(x) | np.isnan(y))).sum()) and n0 == kept * (kept - 1) // 2
        assert s == inversions_slow(x, y), f"case {i} n={n}"
    assert kendall_restated(*cases[3])[4] == n * (n - 1) // 2               # y descending: every pair is an inversion
    assert kendall_restated(*cases[4])[2:5] == (n * (n - 1) // 2, 0, 0)     # constant x: all ties, sorted by y


@pytest.mark.parametrize("n", PIN_SIZES)
@pytest.mark.parametrize("kind", PIN_KINDS)
def test_integers_are_the_references_bit_for_bit(ans, kind, n):
    """The <int32_t> object code is a function of (n0, n1, n2, S) alone: equal bits on continuous, tied, -0/+0 and +-inf
    data pin the integers' definitions (at these sizes they fit an int32: n0 <= 8 390 656)."""
    x, y = pin_pair(kind, n)
    _, n0, n1, n2, s, _ = kendall_restated(x, y)
    assert f32_bits(tail_int32(n0, n1, n2, s)) == f32_bits(ans.kendall_int32(x, y)), f"{kind} n={n}: {(n0, n1, n2, s)}"


@pytest.mark.parametrize("n", [2, 3, 65, 4097, 20435])
def test_tie_free_against_scipy(n):
    from scipy.stats import kendalltau
    rng = np.random.default_rng(50 + n)
    x = rng.permutation(n).astype(np.float32)
    y = (0.3 * x + rng.permutation(n)).astype(np.float64)
    y = np.argsort(np.argsort(y)).astype(np.float32)                        # tie-free and exact in float32
    _, n0, n1, n2, s, _ = kendall_restated(x, y)
    assert n1 == 0 and n2 == 0
    want = kendalltau(x, y).statistic
    assert abs(float(n0 - 2 * s) / float(n0) - want) <= 1e-12


def test_known_answer():
    x = [1, 1, 2, 2, 3, 3, 4, 4]
    y = [1, 2, 2, 3, 3, 3, 5, 4]
    n, n0, n1, n2, s, bits = kendall_restated(x, y)
    assert (n, n0, n1, n2, s) == (8, 28, 4, 4, 0)
    assert bits == f32_bits(np.float32(20.0 / 24.0))
    assert f32_bits(tail_int32(n0, n1, n2, s)) == f32_bits(np.float32(0.833333254))


def test_degenerate_values():
    assert np.isnan(tail_int64(0, 0, 0, 0)) and np.isnan(tail_int64(1, 1, 0, 0))
    assert np.isinf(tail_int64(3, 3, 1, 0))
    for x, y in (([], []), ([1.0], [2.0]), ([np.nan, 1.0], [1.0, np.nan])):
        assert np.isnan(np.array([kendall_restated(x, y)[5]], np.uint32).view(np.float32)[0])


def test_two_to_the_eighteen():
    """The size of the largest GPU case (seconds here, not minutes): y descending in x gives S = n0; a shuffle of tied
    data gives the same integers as the data in order."""
    n = 1 << 18
    x = np.arange(n, dtype=np.float32)
    assert kendall_restated(x, -x)[1:5] == (n * (n - 1) // 2, 0, 0, n * (n - 1) // 2)
    qx, qy = _quantised(n, 3)
    order = np.random.default_rng(4).permutation(n)
    first = kendall_restated(qx, qy)
    assert 0 < first[4] < first[1] and kendall_restated(qx[order], qy[order]) == first
