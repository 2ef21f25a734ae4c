"""rank_similarity_reference.ranks_restated -- what the GPU rank tests compare against -- pinned to ref_ranks of the
reference's own object code (computeRanks, Correlation.cpp:277-303): bit-identical on continuous, heavily tied, -0/+0 and
+-inf data.  The small cases run everywhere (their rank arrays are recorded in
tests/golden/reference/field_rank_similarity_calls.npz); the 2^24 cases need oracle/_ref."""
import numpy as np
import pytest

import oracle_lib
from rank_similarity_reference import PIN_KINDS, PIN_SIZES, RankAnswers, pin_data, ranks_restated

LIVE = pytest.mark.skipif(not oracle_lib.reference_available(),
                          reason="needs the reference's object code (oracle/_ref), present on the build machine only")


@pytest.fixture(scope="module")
def ans():
    return RankAnswers()


def _identical(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert differ.size == 0, f"{what}: {differ.size} of {got.size} ranks differ, first at {differ[0]}: " \
                             f"{got[differ[0]]!r} against {want[differ[0]]!r}"


@pytest.mark.parametrize("n", PIN_SIZES)
@pytest.mark.parametrize("kind", PIN_KINDS)
def test_restatement_is_the_reference_bit_for_bit(ans, kind, n):
    v = pin_data(kind, n)
    _identical(ranks_restated(v), ans.ranks(v), f"{kind} n={n}")


def test_restatement_on_plain_cases():
    """Independent of any reference: the definition on inputs small enough to rank by hand."""
    _identical(ranks_restated([3.0, 1.0, 2.0]), [3.0, 1.0, 2.0], "distinct")
    _identical(ranks_restated([5.0, 5.0, 5.0, 5.0]), [2.5] * 4, "constant")
    _identical(ranks_restated([0.0, -0.0, 1.0, -np.inf, np.inf]), [2.5, 2.5, 4.0, 1.0, 5.0], "zeros and infinities")
    _identical(ranks_restated([2.0, np.nan, 1.0, 2.0]), [2.5, np.nan, 1.0, 2.5], "a NaN is not ranked")


@LIVE
def test_tie_free_at_2_to_24(ans):
    v = np.random.default_rng(24).permutation(1 << 24).astype(np.float32)          # every integer below 2^24 is a float
    _identical(ranks_restated(v), ans.ranks(v), "2^24 tie-free")


@LIVE
def test_tied_pairs_at_2_to_24(ans):
    """Half ranks above 2^23 are rounded, in the reference as in the restatement."""
    v = (np.random.default_rng(25).permutation(1 << 24) >> 1).astype(np.float32)
    _identical(ranks_restated(v), ans.ranks(v), "2^24 in tied pairs")


@LIVE
def test_the_deviation_beyond_2_to_24(ans):
    """The reference's fp32 running sum stops counting runs of one at 2^24: from there its ranks stay at 2^24, while the
    restatement (and the library) keeps the exact start, rounded once."""
    n = (1 << 24) + 4096
    v = (np.arange(n, dtype=np.int64) - (1 << 23)).astype(np.float32)              # sorted, exact and tie-free: |v| < 2^24
    ours, theirs = ranks_restated(v), ans.ranks(v)
    _identical(ours[:1 << 24], theirs[:1 << 24], "the first 2^24 ranks")
    exact = np.arange(1, n + 1, dtype=np.int64).astype(np.float32)
    _identical(ours, exact, "restatement against the exact ranks, rounded once")
    assert (theirs[1 << 24:] == np.float32(1 << 24)).all() and (ours[(1 << 24) + 1:] > np.float32(1 << 24)).all()


def record_reference_calls(ans):
    for kind in PIN_KINDS:
        for n in PIN_SIZES:
            ans.ranks(pin_data(kind, n))
