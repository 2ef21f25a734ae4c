"""What the rank tests (test_rank_restatement.py, test_gpu_rank_values.py, test_gpu_field_rank_similarity.py) compare
against.

  ranks_restated   the reference's computeRanks (Correlation.cpp:277-303) with numpy: a run of m equal values whose first
                   1-based position in sorted order is s gets fl32(float(s) + float(m - 1) * 0.5f), with s an exact integer
                   (the reference carries s as an fp32 running sum, which is the same up to 2^24 values and wrong beyond:
                   test_rank_restatement.py pins both).  NaN positions get NaN and are left out of the ranking.
  pin_data         the small inputs on which the restatement is pinned to the reference's object code
  RankAnswers      the reference's own object code (oracle/_ref/libref_corr.so: ref_ranks, and
                   computePearsonParallel<double> over two of its rank arrays for Spearman) where it was built, else its
                   recorded answers (tests/golden/reference/field_rank_similarity_calls.npz, written by
                   `python tests/rank_similarity_reference.py record` where the reference is present): one scalar per
                   Spearman call of test_gpu_field_rank_similarity.py and the rank arrays of pin_data.
"""
from __future__ import annotations

import ctypes as C
import sys
from pathlib import Path

import numpy as np

import oracle_lib
from similarity_reference import KEY_BYTES, PEARSON_PARALLEL_DOUBLE

ROOT = Path(__file__).resolve().parent.parent
RECORDED = ROOT / "tests" / "golden" / "reference" / "field_rank_similarity_calls.npz"
PIN_SIZES = (1, 2, 3, 65, 4097)
PIN_KINDS = ("continuous", "tied", "zeros", "infinite")


def ranks_restated(v) -> np.ndarray:
    v = np.asarray(v, np.float32).reshape(-1)
    out = np.full(v.size, np.nan, np.float32)
    keep = ~np.isnan(v)
    _, inverse, counts = np.unique(v[keep] + np.float32(0.0), return_inverse=True, return_counts=True)
    starts = 1 + np.cumsum(counts) - counts                            # exact integers
    ranks = starts.astype(np.float32) + (counts - 1).astype(np.float32) * np.float32(0.5)
    out[keep] = ranks[inverse.reshape(-1)]
    return out


def pin_data(kind, n, seed=0) -> np.ndarray:
    rng = np.random.default_rng(1000 * PIN_KINDS.index(kind) + n + seed)
    v = rng.standard_normal(n).astype(np.float32)
    if kind == "tied":
        v = np.round(v * 2.0).astype(np.float32) / np.float32(2.0)     # a handful of levels: long runs
    elif kind == "zeros":
        v[rng.random(n) < 0.3] = np.float32(0.0)
        v[rng.random(n) < 0.3] = np.float32(-0.0)
    elif kind == "infinite":
        v[rng.random(n) < 0.2] = np.float32(np.inf)
        v[rng.random(n) < 0.2] = np.float32(-np.inf)
    return v


class RankAnswers:
    def __init__(self, record=False):
        self.live = oracle_lib.load_reference() if oracle_lib.reference_available() else None
        self.scalars, self.arrays = {}, {}
        if record and self.live is None:
            raise RuntimeError("recording needs oracle/_ref (python __graft_entry__.py build where the reference is present)")
        self.record = record
        if self.live is not None:
            fn = getattr(self.live.lib, PEARSON_PARALLEL_DOUBLE)
            fn.restype = C.c_float
            fn.argtypes = [oracle_lib.FP, oracle_lib.FP, C.c_int]
            self._pearson = fn
        elif RECORDED.exists():
            d = np.load(RECORDED, allow_pickle=False)
            self.scalars = {bytes(k).hex(): v for k, v in zip(d["keys"], d["values"])}
            offsets = d["rank_offsets"]
            self.arrays = {bytes(k).hex(): d["rank_values"][offsets[i]:offsets[i + 1]] for i, k in enumerate(d["rank_keys"])}

    def _answer(self, store, compute, *parts):
        key = oracle_lib._call_key(*parts)[:2 * KEY_BYTES]
        if self.live is not None:
            v = compute()
            if self.record:
                store[key] = v
            return v
        if key not in store:
            raise KeyError(f"{parts[0]}: no recorded answer of the reference for these inputs ({RECORDED.name})")
        return store[key]

    def ranks(self, v) -> np.ndarray:
        """ref_ranks; recorded for pin_data only."""
        v = oracle_lib._f32(v)
        return self._answer(self.arrays, lambda: self.live.ranks(v), "ranks", v)

    def spearman(self, x, y) -> np.float32:
        """Similarity.cpp:134-143 in the <double> instantiation: computeRanks twice, computePearsonParallel<double>."""
        x, y = oracle_lib._f32(x), oracle_lib._f32(y)

        def compute():
            rx, ry = self.live.ranks(x), self.live.ranks(y)
            return np.float32(self._pearson(oracle_lib._fp(rx), oracle_lib._fp(ry), rx.size))
        return np.float32(self._answer(self.scalars, compute, "spearman", x, y))

    def save(self):
        keys = sorted(self.scalars)
        raw = np.frombuffer(bytes.fromhex("".join(keys)), np.uint8).reshape(len(keys), KEY_BYTES)
        rkeys = sorted(self.arrays)
        rraw = np.frombuffer(bytes.fromhex("".join(rkeys)), np.uint8).reshape(len(rkeys), KEY_BYTES)
        sizes = [self.arrays[k].size for k in rkeys]
        np.savez_compressed(RECORDED, keys=raw, values=np.array([self.scalars[k] for k in keys], np.float32),
                            rank_keys=rraw, rank_offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                            rank_values=np.concatenate([self.arrays[k] for k in rkeys]).astype(np.float32))


if __name__ == "__main__" and sys.argv[1:] == ["record"]:
    sys.path.insert(0, str(ROOT))
    import test_gpu_field_rank_similarity
    import test_rank_restatement
    answers = RankAnswers(record=True)
    test_rank_restatement.record_reference_calls(answers)
    test_gpu_field_rank_similarity.record_reference_calls(answers)
    answers.save()
    print(f"recorded {len(answers.scalars)} Spearman values and {len(answers.arrays)} rank arrays of the reference in {RECORDED}")
