"""What the Kendall tests (test_kendall_restatement.py, test_gpu_kendall_values.py, test_gpu_field_kendall_similarity.py)
compare against.

  kendall_restated  the reference's computeKendall<int64_t> (Correlation.cpp:423-455) with numpy: the pairs without a NaN,
                    n0 = n (n - 1) / 2, the tie sums n1 (x) and n2 (y) over the runs of equal values (joint ties stay 0, as
                    in the reference, which is why the value is not SciPy's tau-b on tied data), S = the strict inversions
                    of y in the order of std::sort on pair<float, float> (x ascending, y ascending among equal x), counted
                    level by level, and float(double(n0 - n1 - n2 - 2 S) / (sqrt(double(n0 - n1)) * sqrt(double(n0 - n2)))).
                    Returns (n, n0, n1, n2, S, bits of the float).
  inversions_slow   the O(n^2) count of the same S, for n <= 2000
  tail_int64        the <int64_t> tail of the four integers, in float64; tail_int32: the <int32_t> tail, in float32
  KendallAnswers    the reference's own object code where it was built (oracle/_ref/libref_corr.so: ref_kendall, the
                    <int32_t> instantiation, which runs the same S, M and computeTiesB templates), else its recorded answers
                    (tests/golden/reference/field_kendall_similarity_calls.npz, written by
                    `python tests/kendall_similarity_reference.py record` where the reference is present) for pin_data.

The <int64_t> tail itself -- three double operations and a cast -- is RESTATED here, not pinned to object code: the
symbol the reference exports for it takes std::vector scratch by reference, which the oracle's C drivers do not reach.
What is pinned is everything before it: the integers, through the <int32_t> instantiation on data whose integers fit.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

import oracle_lib
from rank_similarity_reference import PIN_KINDS, PIN_SIZES, pin_data
from similarity_reference import KEY_BYTES

ROOT = Path(__file__).resolve().parent.parent
RECORDED = ROOT / "tests" / "golden" / "reference" / "field_kendall_similarity_calls.npz"


def _kept(x, y):
    x = np.asarray(x, np.float32).reshape(-1)
    y = np.asarray(y, np.float32).reshape(-1)
    keep = ~(np.isnan(x) | np.isnan(y))
    return x[keep] + np.float32(0.0), y[keep] + np.float32(0.0)            # -0 becomes +0: they compare equal


def _ties(v) -> int:
    _, counts = np.unique(v, return_counts=True)
    return sum(int(m) * (int(m) - 1) // 2 for m in counts)


def _y_in_sort_order(x, y) -> np.ndarray:
    """y as dense integer ranks (equal y, equal rank) in the order of std::sort on the pairs."""
    _, dense = np.unique(y, return_inverse=True)
    return dense.reshape(-1)[np.lexsort((y, x))].astype(np.int64)


def inversions_levels(seq) -> int:
    """Pairs i < j with seq[j] < seq[i], bottom up: per level every row is two sorted halves; one searchsorted with a
    per-row offset counts, for every right value, the left values above it."""
    seq = np.asarray(seq, np.int64)
    n = seq.size
    if n < 2:
        return 0
    size = 1 << int(n - 1).bit_length()
    top = int(seq.max()) + 1                                              # the padding: last and largest, never inverted
    rows = np.full(size, top, np.int64)
    rows[:n] = seq
    total, width = 0, 1
    while width < size:
        rows = rows.reshape(-1, 2 * width)
        left, right = np.sort(rows[:, :width], axis=1), np.sort(rows[:, width:], axis=1)
        offset = (np.arange(rows.shape[0], dtype=np.int64) * (top + 1))[:, None]
        at_or_below = np.searchsorted((left + offset).reshape(-1), (right + offset).reshape(-1), side="right")
        at_or_below = at_or_below.reshape(right.shape) - (np.arange(rows.shape[0], dtype=np.int64) * width)[:, None]
        total += int((width - at_or_below).sum())
        rows = np.concatenate([left, right], axis=1)
        width *= 2
    return total


def inversions_slow(x, y) -> int:
    x, y = _kept(x, y)
    assert x.size <= 2000
    seq = _y_in_sort_order(x, y)
    return int(np.triu(seq[None, :] < seq[:, None], 1).sum())


def tail_int64(n0, n1, n2, s) -> np.float32:
    with np.errstate(all="ignore"):
        den = np.sqrt(np.float64(n0 - n1)) * np.sqrt(np.float64(n0 - n2))
        return np.float32(np.float64(n0 - n1 - n2 - 2 * s) / den)


def tail_int32(n0, n1, n2, s) -> np.float32:
    with np.errstate(all="ignore"):
        den = np.sqrt(np.float32(n0 - n1)) * np.sqrt(np.float32(n0 - n2))
        return np.float32(n0 - n1 - n2 - 2 * s) / den


def f32_bits(v) -> int:
    return int(np.float32(v).view(np.uint32))


def kendall_restated(x, y):
    x, y = _kept(x, y)
    n = int(x.size)
    n0, n1, n2 = n * (n - 1) // 2, _ties(x), _ties(y)
    s = inversions_levels(_y_in_sort_order(x, y))
    return n, n0, n1, n2, s, f32_bits(tail_int64(n0, n1, n2, s))


def pin_pair(kind, n):
    """x and y of one pinned case: two independent draws of the kind; the continuous y also takes half of x, so that one
    kind is correlated."""
    x, y = pin_data(kind, n), pin_data(kind, n, seed=7)
    if kind == "continuous":
        y = (np.float32(0.5) * x + y).astype(np.float32)
    return x, y


class KendallAnswers:
    def __init__(self, record=False):
        self.live = oracle_lib.load_reference() if oracle_lib.reference_available() else None
        self.scalars = {}
        if record and self.live is None:
            raise RuntimeError("recording needs oracle/_ref (python __graft_entry__.py build where the reference is present)")
        self.record = record
        if self.live is None and RECORDED.exists():
            d = np.load(RECORDED, allow_pickle=False)
            self.scalars = {bytes(k).hex(): v for k, v in zip(d["keys"], d["values"])}

    def kendall_int32(self, x, y) -> np.float32:
        """ref_kendall: computeKendall<int32_t>; recorded for pin_pair only."""
        x, y = oracle_lib._f32(x), oracle_lib._f32(y)
        key = oracle_lib._call_key("kendall_int32", x, y)[:2 * KEY_BYTES]
        if self.live is not None:
            v = np.float32(self.live.kendall(x, y))
            if self.record:
                self.scalars[key] = v
            return v
        if key not in self.scalars:
            raise KeyError(f"kendall_int32: no recorded answer of the reference for these inputs ({RECORDED.name})")
        return np.float32(self.scalars[key])

    def save(self):
        keys = sorted(self.scalars)
        raw = np.frombuffer(bytes.fromhex("".join(keys)), np.uint8).reshape(len(keys), KEY_BYTES)
        np.savez_compressed(RECORDED, keys=raw, values=np.array([self.scalars[k] for k in keys], np.float32))


def record_reference_calls(ans):
    for kind in PIN_KINDS:
        for n in PIN_SIZES:
            ans.kendall_int32(*pin_pair(kind, n))


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    answers = KendallAnswers(record=True)
    record_reference_calls(answers)
    answers.save()
    print(f"recorded {len(answers.scalars)} Kendall values of the reference in {RECORDED}")
