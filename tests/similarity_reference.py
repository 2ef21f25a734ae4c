"""What the field-similarity tests (test_similarity_tail.py, test_gpu_field_similarity.py) compare against.

  bins_x86 / joint_counts   the bin of a normalised value as the reference's x86-64 build converts it
                            (MutualInformation.cpp:64-67) and the joint histogram as integer counts, with numpy
  mi_from_counts            a SEQUENTIAL restatement of the arithmetic behind the counts (MutualInformation.cpp:71-142):
                            fp64, the reference's loop order, math.log (the host libm's log), and the product es * es
                            formed in fp64 -- or, with wrap_product=True, in a wrapping 32-bit int as the reference's object
                            code forms it (which reproduces its NaN at 46 341 samples and its lost joint term beyond)
  Answers                   the reference's own object code (oracle/_ref: ref_mi_binned of libref_mi.so,
                            computePearsonParallel<double> of libref_corr.so) where it was built, else its recorded answers
                            to exactly the calls of test_gpu_field_similarity.py (tests/golden/reference/field_similarity_calls.npz,
                            written by `python tests/similarity_reference.py record` where the reference is present)
"""
from __future__ import annotations

import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np

import oracle_lib

ROOT = Path(__file__).resolve().parent.parent
RECORDED = ROOT / "tests" / "golden" / "reference" / "field_similarity_calls.npz"
PEARSON_PARALLEL_DOUBLE = "_Z22computePearsonParallelIdEfPKfS1_i"   # float computePearsonParallel<double>(const float*, const float*, int)
KEY_BYTES = 12


def f32_bits(v) -> int:
    return int(np.float32(v).view(np.uint32))


def normalise(v, lo, hi):
    """(v - lo) / (hi - lo) in IEEE fp32, as the library forms it."""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        return ((v - np.float32(lo)) / (np.float32(hi) - np.float32(lo))).astype(np.float32)


def bins_x86(v01, num_bins):
    """clamp(int(double(v01) * num_bins), 0, num_bins - 1) with cvttsd2si's INT_MIN for NaN and out-of-range products."""
    with np.errstate(all="ignore"):
        t = np.asarray(v01, np.float32).astype(np.float64) * float(num_bins)
        inside = (t > -2147483649.0) & (t < 2147483648.0)
        b = np.where(inside, np.trunc(np.where(inside, t, 0.0)), -2147483648.0).astype(np.int64)
    return np.clip(b, 0, num_bins - 1)


def joint_counts(x01, y01, num_bins):
    """(counts[num_bins, num_bins] as uint64, es): es counts every pair handed over, the histogram leaves out the pairs
    with a NaN (MutualInformation.cpp:61-69)."""
    x01, y01 = np.asarray(x01, np.float32).reshape(-1), np.asarray(y01, np.float32).reshape(-1)
    keep = ~(np.isnan(x01) | np.isnan(y01))
    cell = bins_x86(x01[keep], num_bins) * num_bins + bins_x86(y01[keep], num_bins)
    counts = np.bincount(cell, minlength=num_bins * num_bins).astype(np.uint64)
    return counts.reshape(num_bins, num_bins), int(x01.size)


def mi_from_counts(counts, es, wrap_product=False) -> np.float32:
    counts = np.asarray(counts, np.uint64)
    nb = counts.shape[0]
    with np.errstate(all="ignore"):
        h2d = counts.astype(np.float64)
        total = np.cumsum(h2d.reshape(-1))[-1]                      # cumsum adds sequentially, in index order
        h2d = h2d / total
        h0 = np.cumsum(h2d, axis=1)[:, -1]                          # over b1 for every b0, in order
        h1 = np.cumsum(h2d, axis=0)[-1, :]                          # over b0 for every b1, in order
        eps1 = np.float64(0.5) / np.float64(es)
        if wrap_product:
            p32 = (es * es) & 0xFFFFFFFF
            p32 = p32 - (1 << 32) if p32 >= (1 << 31) else p32
            eps2 = np.float64(0.5) / np.float64(p32)
        else:
            eps2 = np.float64(0.5) / (np.float64(es) * np.float64(es))
    mi = 0.0
    for b in range(nb):
        px, py = float(h0[b]), float(h1[b])
        if px > eps1:
            mi -= px * math.log(px)
        if py > eps1:
            mi -= py * math.log(py)
    flat = h2d.reshape(-1)
    # an empty cell is 0 (or NaN without samples) and fails `p > eps2` -- unless the wrapped product made eps2 negative
    cells = range(flat.size) if wrap_product else np.flatnonzero(counts.reshape(-1))
    for i in cells:
        p = float(flat[i])
        if p > eps2:
            mi += p * (math.log(p) if p != 0.0 else -math.inf)
    return np.float32(mi)


_LIBM = C.CDLL("libm.so.6")
_LIBM.expf.restype = C.c_float
_LIBM.expf.argtypes = [C.c_float]


def mi_to_cc(mi) -> np.float32:
    """sqrt(1 - exp(-2 MI)) in fp32 with the host libm's expf (Similarity.cpp:165-167)."""
    with np.errstate(all="ignore"):
        return np.sqrt(np.float32(1.0) - np.float32(_LIBM.expf(float(np.float32(-2.0) * np.float32(mi)))))


def pearson_tolerance(ref, n) -> float:
    """|got - ref| <= ulp32(ref) + 8 N 2^-53: either side accumulates N terms whose absolute values sum to at most 1
    after normalisation (Cauchy-Schwarz), so it errs by about N 2^-53 per pass in any order; the cast adds one ulp."""
    return float(np.spacing(np.float32(abs(ref)))) + 8.0 * n * 2.0 ** -53


class Answers:
    def __init__(self, record=False):
        self.live = oracle_lib.load_reference() if oracle_lib.reference_available() else None
        self.recorded, self.made = {}, {}
        if record and self.live is None:
            raise RuntimeError("recording needs oracle/_ref (python __graft_entry__.py build where the reference is present)")
        if self.live is not None:
            fn = getattr(self.live.lib, PEARSON_PARALLEL_DOUBLE)
            fn.restype = C.c_float
            fn.argtypes = [oracle_lib.FP, oracle_lib.FP, C.c_int]
            self._pearson = fn
        elif RECORDED.exists():
            d = np.load(RECORDED, allow_pickle=False)
            self.recorded = {bytes(k).hex(): v for k, v in zip(d["keys"], d["values"])}

    def _answer(self, compute, *parts):
        key = oracle_lib._call_key(*parts)[:2 * KEY_BYTES]
        if self.live is not None:
            v = np.float32(compute())
            self.made[key] = v
            return v
        if key not in self.recorded:
            raise KeyError(f"{parts[0]}: no recorded answer of the reference for these inputs ({RECORDED.name})")
        return np.float32(self.recorded[key])

    def mi_binned(self, x01, y01, num_bins) -> np.float32:
        x01, y01 = oracle_lib._f32(x01), oracle_lib._f32(y01)
        return self._answer(lambda: self.live.mi_binned(x01, y01, num_bins), "mi_binned", x01, y01, int(num_bins))

    def pearson_parallel(self, x, y) -> np.float32:
        x, y = oracle_lib._f32(x), oracle_lib._f32(y)
        return self._answer(lambda: self._pearson(oracle_lib._fp(x), oracle_lib._fp(y), x.size), "pearson_parallel", x, y)

    def save(self):
        keys = sorted(self.made)
        raw = np.frombuffer(bytes.fromhex("".join(keys)), np.uint8).reshape(len(keys), KEY_BYTES)
        np.savez_compressed(RECORDED, keys=raw, values=np.array([self.made[k] for k in keys], np.float32))


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    sys.path.insert(0, str(ROOT))
    import test_gpu_field_similarity
    answers = Answers(record=True)
    test_gpu_field_similarity.record_reference_calls(answers)
    answers.save()
    print(f"recorded {len(answers.made)} calls of the reference in {RECORDED}")
