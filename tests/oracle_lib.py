"""ctypes access to the CHECKER libraries (test infrastructure only):
   oracle/liboracle.so        this repo's CPU restatement (built on demand with g++; travels to the GPU box prebuilt)
   oracle/_ref/libref_corr.so the reference's own Correlation.cpp behind oracle/ref_driver.cpp (build container only)
   oracle/_ref/libref_mi.so   the reference's own MutualInformation.cpp and DKL.cpp behind oracle/ref_mi_driver.cpp, with
                              oracle/standins/ in place of boost, sgl and glm (build container only)
   tests/golden/reference/calls.npz, mi_calls.npz  that object code's answers to the calls of the tests that compare
                              against it, recorded by oracle/make_golden.py: what those tests compare against where
                              oracle/_ref is absent
Nothing under correrender_amd/ imports this module."""
from __future__ import annotations

import ctypes as C
import hashlib
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
ORACLE_DIR = ROOT / "oracle"
RECORDED_CALLS = ROOT / "tests" / "golden" / "reference" / "calls.npz"
RECORDED_MI_CALLS = ROOT / "tests" / "golden" / "reference" / "mi_calls.npz"
DP = C.POINTER(C.c_double)
FP = C.POINTER(C.c_float)

PEARSON, SPEARMAN, KENDALL, MI_BINNED, MI_KRASKOV, BINNED_MI_CC, KMI_CC = range(7)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(FP)


class Oracle:
    def __init__(self, lib: C.CDLL):
        self.lib = lib
        lib.oracle_pearson2.restype = C.c_float
        lib.oracle_pearson2.argtypes = [FP, FP, C.c_int]
        lib.oracle_ranks.restype = None
        lib.oracle_ranks.argtypes = [FP, FP, C.c_int]
        lib.oracle_spearman.restype = C.c_float
        lib.oracle_spearman.argtypes = [FP, FP, C.c_int]
        lib.oracle_kendall.restype = C.c_float
        lib.oracle_kendall.argtypes = [FP, FP, C.c_int]
        lib.oracle_mi_binned.restype = C.c_float
        lib.oracle_mi_binned.argtypes = [FP, FP, C.c_int, C.c_int]
        lib.oracle_mi_kraskov.restype = C.c_float
        lib.oracle_mi_kraskov.argtypes = [FP, FP, C.c_int, C.c_int, C.c_int]
        lib.oracle_digamma_int.restype = C.c_double
        lib.oracle_digamma_int.argtypes = [C.c_int]
        lib.oracle_set_kraskov_noise.restype = None
        lib.oracle_set_kraskov_noise.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
        lib.oracle_noise01.restype = None
        lib.oracle_noise01.argtypes = [C.c_int, C.c_int, FP]
        lib.oracle_minmax.restype = None
        lib.oracle_minmax.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_size_t, FP, FP]
        lib.oracle_correlation_field.restype = C.c_int
        lib.oracle_correlation_field.argtypes = [
            C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.c_size_t, FP, C.c_int, C.c_int, C.c_int,
            C.c_float, C.c_float, C.c_float, C.c_float, FP, C.c_int]
        lib.oracle_symmetric_field.restype = C.c_int
        lib.oracle_symmetric_field.argtypes = [
            C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
            C.c_float, C.c_float, C.c_float, C.c_float, FP]
        lib.oracle_set_predicate.restype = C.c_int
        lib.oracle_set_predicate.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int,
                                             C.c_size_t, FP]
        lib.oracle_tile_field.restype = None
        lib.oracle_tile_field.argtypes = [FP, C.c_int, C.c_int, C.c_int, FP]
        lib.oracle_dkl_field.restype = C.c_int
        lib.oracle_dkl_field.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.c_int, C.c_int, FP]
        lib.oracle_max_threads.restype = C.c_int
        lib.oracle_ensemble_stat.restype = C.c_int
        lib.oracle_ensemble_stat.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_size_t, FP]
        lib.oracle_pair_requests.restype = C.c_int
        lib.oracle_pair_requests.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_size_t),
                                             C.POINTER(C.c_size_t), C.c_size_t, C.c_int, C.c_int, C.c_int, FP]

    # -- primitives
    def pearson(self, x, y):
        x, y = _f32(x), _f32(y)
        return float(self.lib.oracle_pearson2(_fp(x), _fp(y), x.size))

    def ranks(self, v):
        v = _f32(v)
        out = np.empty_like(v)
        self.lib.oracle_ranks(_fp(v), _fp(out), v.size)
        return out

    def spearman(self, x, y):
        x, y = _f32(x), _f32(y)
        return float(self.lib.oracle_spearman(_fp(x), _fp(y), x.size))

    def kendall(self, x, y):
        x, y = _f32(x), _f32(y)
        return float(self.lib.oracle_kendall(_fp(x), _fp(y), x.size))

    def mi_binned(self, x01, y01, num_bins):
        x01, y01 = _f32(x01), _f32(y01)
        return float(self.lib.oracle_mi_binned(_fp(x01), _fp(y01), num_bins, x01.size))

    def mi_kraskov(self, x, y, k, estimator=1):
        x, y = _f32(x), _f32(y)
        return float(self.lib.oracle_mi_kraskov(_fp(x), _fp(y), k, x.size, estimator))

    def digamma(self, n):
        return float(self.lib.oracle_digamma_int(int(n)))

    def set_kraskov_noise(self, ref_noise=None, query_noise=None):
        """Per-member noise tables (already scaled by 1e-10) for the Kraskov estimators; None restores the default."""
        if ref_noise is None:
            self.lib.oracle_set_kraskov_noise(None, None, 0)
            return
        r = np.ascontiguousarray(ref_noise, np.float64)
        q = np.ascontiguousarray(query_noise, np.float64)
        assert r.size == q.size
        self.lib.oracle_set_kraskov_noise(r.ctypes.data_as(C.POINTER(C.c_double)), q.ctypes.data_as(C.POINTER(C.c_double)),
                                          r.size)

    def noise01(self, which, n):
        out = np.empty(n, np.float32)
        self.lib.oracle_noise01(which, n, _fp(out))
        return out

    def minmax(self, members):
        members = _members(members)
        ptrs = (C.c_void_p * len(members))(*[m.ctypes.data for m in members])
        mn, mx = C.c_float(), C.c_float()
        self.lib.oracle_minmax(ptrs, len(members), members[0].size, C.byref(mn), C.byref(mx))
        return mn.value, mx.value

    # -- the calculateCpu driver
    def field(self, measure, members, ref_values, *, k=3, estimator=1, num_bins=80, minmax_ref=(0.0, 1.0),
              minmax_query=None, voxel_range=None, threads=0):
        members = _members(members)
        cs = len(members)
        n = members[0].size
        lo, hi = voxel_range if voxel_range is not None else (0, n)
        ref_values = _f32(ref_values)
        assert ref_values.size == cs
        minmax_query = minmax_ref if minmax_query is None else minmax_query
        ptrs = (C.c_void_p * cs)(*[m.ctypes.data for m in members])
        out = np.empty(hi - lo, np.float32)
        rc = self.lib.oracle_correlation_field(
            int(measure), ptrs, cs, lo, hi, _fp(ref_values), int(k), int(estimator), int(num_bins),
            float(minmax_ref[0]), float(minmax_ref[1]), float(minmax_query[0]), float(minmax_query[1]), _fp(out),
            int(threads))
        assert rc == 0
        return out

    def symmetric_field(self, measure, members_ref, members_query, *, k=3, num_bins=80, minmax_ref=(0.0, 1.0),
                        minmax_query=(0.0, 1.0), voxel_range=None):
        """SEPARATE_SYMMETRIC: measure(members_ref[:, v], members_query[:, v]) at every voxel v."""
        mr, mq = _members(members_ref), _members(members_query)
        cs = len(mr)
        assert len(mq) == cs
        lo, hi = voxel_range if voxel_range is not None else (0, mr[0].size)
        pr = (C.c_void_p * cs)(*[m.ctypes.data for m in mr])
        pq = (C.c_void_p * cs)(*[m.ctypes.data for m in mq])
        out = np.empty(hi - lo, np.float32)
        rc = self.lib.oracle_symmetric_field(int(measure), pr, pq, cs, lo, hi, int(k), int(num_bins),
                                             float(minmax_ref[0]), float(minmax_ref[1]), float(minmax_query[0]),
                                             float(minmax_query[1]), _fp(out))
        assert rc == 0
        return out

    def set_predicate(self, op, comparison_value, count_lower, count_upper, members):
        members = _members(members)
        ptrs = (C.c_void_p * len(members))(*[m.ctypes.data for m in members])
        out = np.empty(members[0].size, np.float32)
        assert self.lib.oracle_set_predicate(int(op), float(comparison_value), int(count_lower), int(count_upper), ptrs,
                                             len(members), members[0].size, _fp(out)) == 0
        return out

    def tile_field(self, linear):
        zs, ys, xs = linear.shape
        lin = _f32(linear)
        out = np.empty(((xs + 7) // 8) * ((ys + 7) // 8) * ((zs + 3) // 4) * 256, np.float32)
        self.lib.oracle_tile_field(_fp(lin), xs, ys, zs, _fp(out))
        return out

    def dkl(self, estimator, members, *, num_bins=80, k=3):
        """DKLCalculator::calculateCpu: estimator 0 = binned, 1 = entropy k-NN."""
        members = _members(members)
        ptrs = (C.c_void_p * len(members))(*[m.ctypes.data for m in members])
        out = np.empty(members[0].size, np.float32)
        assert self.lib.oracle_dkl_field(int(estimator), ptrs, len(members), members[0].size, int(num_bins), int(k),
                                         _fp(out)) == 0
        return out

    def max_threads(self):
        return int(self.lib.oracle_max_threads())

    def first_touch_copy(self, members):
        """A copy of [cs, ...] float32 volumes whose pages were first touched by the OpenMP threads that will read them
        (same static partition over voxels as the field loops): NUMA placement for a bound cpu_baseline run."""
        members = np.ascontiguousarray(members, np.float32)
        cs = members.shape[0]
        n = members[0].size
        out = np.empty(members.shape, np.float32)          # untouched pages (large allocation: fresh mmap)
        src = (C.c_void_p * cs)(*[members[c].ctypes.data for c in range(cs)])
        dst = (C.c_void_p * cs)(*[out[c].ctypes.data for c in range(cs)])
        self.lib.oracle_first_touch_copy.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int64]
        assert self.lib.oracle_first_touch_copy(src, dst, cs, n) == 0
        return out

    def ensemble_stat(self, kind, members):
        members = _members(members)
        ptrs = (C.c_void_p * len(members))(*[m.ctypes.data for m in members])
        out = np.empty(members[0].size, np.float32)
        assert self.lib.oracle_ensemble_stat(int(kind), ptrs, len(members), members[0].size, _fp(out)) == 0
        return out

    def pair_requests(self, measure, members, idx_i, idx_j, *, k=3, num_bins=80, use_abs=False):
        members = _members(members)
        cs = len(members)
        ii = np.ascontiguousarray(idx_i, dtype=np.uint64)
        jj = np.ascontiguousarray(idx_j, dtype=np.uint64)
        ptrs = (C.c_void_p * cs)(*[m.ctypes.data for m in members])
        out = np.empty(ii.size, np.float32)
        rc = self.lib.oracle_pair_requests(int(measure), ptrs, cs, ii.ctypes.data_as(C.POINTER(C.c_size_t)),
                                           jj.ctypes.data_as(C.POINTER(C.c_size_t)), ii.size, int(k), int(num_bins),
                                           1 if use_abs else 0, _fp(out))
        assert rc == 0
        return out


class Reference:
    """The reference's own object code: Correlation.cpp (lib) and MutualInformation.cpp + DKL.cpp over the stand-ins
    (mi)."""

    def __init__(self, lib: C.CDLL, mi: C.CDLL):
        self.lib = lib
        self.mi = mi
        _declare_mi(mi)
        lib.ref_pearson2.restype = C.c_float
        lib.ref_pearson2.argtypes = [FP, FP, C.c_int]
        lib.ref_ranks.restype = None
        lib.ref_ranks.argtypes = [FP, FP, C.c_int]
        lib.ref_kendall.restype = C.c_float
        lib.ref_kendall.argtypes = [FP, FP, C.c_int]
        lib.ref_kendall_slow.restype = C.c_float
        lib.ref_kendall_slow.argtypes = [FP, FP, C.c_int]
        lib.ref_correlation_field.restype = C.c_int
        lib.ref_correlation_field.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_size_t, C.c_size_t, FP, FP]
        lib.ref_pair_requests.restype = C.c_int
        lib.ref_pair_requests.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_size_t), C.c_size_t, FP]

    def pearson(self, x, y):
        x, y = _f32(x), _f32(y)
        return float(self.lib.ref_pearson2(_fp(x), _fp(y), x.size))

    def ranks(self, v):
        v = _f32(v)
        out = np.empty_like(v)
        self.lib.ref_ranks(_fp(v), _fp(out), v.size)
        return out

    def kendall(self, x, y):
        x, y = _f32(x), _f32(y)
        return float(self.lib.ref_kendall(_fp(x), _fp(y), x.size))

    def kendall_slow(self, x, y):
        x, y = _f32(x), _f32(y)
        return float(self.lib.ref_kendall_slow(_fp(x), _fp(y), x.size))

    def field(self, measure, members, ref_values, voxel_range=None):
        members = _members(members)
        cs = len(members)
        n = members[0].size
        lo, hi = voxel_range if voxel_range is not None else (0, n)
        ref_values = _f32(ref_values)
        ptrs = (C.c_void_p * cs)(*[m.ctypes.data for m in members])
        out = np.empty(hi - lo, np.float32)
        rc = self.lib.ref_correlation_field(int(measure), ptrs, cs, lo, hi, _fp(ref_values), _fp(out))
        assert rc == 0
        return out


def _ref_pair_requests(self, measure, members, idx_i, idx_j):
    members = _members(members)
    cs = len(members)
    ii = np.ascontiguousarray(idx_i, dtype=np.uint64)
    jj = np.ascontiguousarray(idx_j, dtype=np.uint64)
    ptrs = (C.c_void_p * cs)(*[m.ctypes.data for m in members])
    out = np.empty(ii.size, np.float32)
    rc = self.lib.ref_pair_requests(int(measure), ptrs, cs, ii.ctypes.data_as(C.POINTER(C.c_size_t)),
                                    jj.ctypes.data_as(C.POINTER(C.c_size_t)), ii.size, _fp(out))
    assert rc == 0
    return out


Reference.pair_requests = _ref_pair_requests


def _declare_mi(mi: C.CDLL):
    VPP, SZP = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
    mi.ref_mi_binned.restype = C.c_float
    mi.ref_mi_binned.argtypes = [FP, FP, C.c_int, C.c_int]
    mi.ref_mi_kraskov.restype = C.c_float
    mi.ref_mi_kraskov.argtypes = [FP, FP, C.c_int, C.c_int, C.c_int]
    mi.ref_kraskov_max.restype = C.c_float
    mi.ref_kraskov_max.argtypes = [C.c_int, C.c_int]
    mi.ref_dkl_binned.restype = C.c_float
    mi.ref_dkl_binned.argtypes = [FP, C.c_int, C.c_int]
    mi.ref_dkl_knn.restype = C.c_float
    mi.ref_dkl_knn.argtypes = [FP, C.c_int, C.c_int]
    mi.ref_mi_field.restype = C.c_int
    mi.ref_mi_field.argtypes = [C.c_int, VPP, C.c_int, C.c_size_t, C.c_size_t, FP, C.c_int, C.c_int, C.c_int,
                                C.c_float, C.c_float, C.c_float, C.c_float, FP]
    mi.ref_mi_symmetric_field.restype = C.c_int
    mi.ref_mi_symmetric_field.argtypes = [C.c_int, VPP, VPP, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                          C.c_float, C.c_float, C.c_float, C.c_float, FP]
    mi.ref_mi_pair_requests.restype = C.c_int
    mi.ref_mi_pair_requests.argtypes = [C.c_int, VPP, C.c_int, SZP, SZP, C.c_size_t, C.c_int, C.c_int, C.c_int, FP]
    mi.ref_dkl_field.restype = C.c_int
    mi.ref_dkl_field.argtypes = [C.c_int, VPP, C.c_int, C.c_size_t, C.c_int, C.c_int, FP]


def _ptrs(members):
    return (C.c_void_p * len(members))(*[m.ctypes.data for m in members])


def _ref_mi_binned(self, x01, y01, num_bins):
    x01, y01 = _f32(x01), _f32(y01)
    return float(self.mi.ref_mi_binned(_fp(x01), _fp(y01), int(num_bins), x01.size))


def _ref_mi_kraskov(self, x, y, k, estimator=1):
    x, y = _f32(x), _f32(y)
    return float(self.mi.ref_mi_kraskov(_fp(x), _fp(y), int(k), x.size, int(estimator)))


def _ref_kraskov_max(self, k, n):
    return float(self.mi.ref_kraskov_max(int(k), int(n)))


def _ref_dkl_binned(self, values, num_bins):
    v = _f32(values)
    return float(self.mi.ref_dkl_binned(_fp(v), int(num_bins), v.size))


def _ref_dkl_knn(self, values, k):
    v = _f32(values)
    return float(self.mi.ref_dkl_knn(_fp(v), int(k), v.size))


def _ref_mi_field(self, measure, members, ref_values, *, k=3, estimator=1, num_bins=80, minmax_ref=(0.0, 1.0),
                  minmax_query=None, voxel_range=None):
    members, ref_values = _members(members), _f32(ref_values)
    cs = len(members)
    lo, hi = voxel_range if voxel_range is not None else (0, members[0].size)
    minmax_query = minmax_ref if minmax_query is None else minmax_query
    out = np.empty(hi - lo, np.float32)
    rc = self.mi.ref_mi_field(int(measure), _ptrs(members), cs, lo, hi, _fp(ref_values), int(k), int(estimator),
                              int(num_bins), float(minmax_ref[0]), float(minmax_ref[1]), float(minmax_query[0]),
                              float(minmax_query[1]), _fp(out))
    assert rc == 0
    return out


def _ref_mi_symmetric_field(self, measure, members_ref, members_query, *, k=3, num_bins=80, minmax_ref=(0.0, 1.0),
                            minmax_query=(0.0, 1.0)):
    mr, mq = _members(members_ref), _members(members_query)
    cs = len(mr)
    out = np.empty(mr[0].size, np.float32)
    rc = self.mi.ref_mi_symmetric_field(int(measure), _ptrs(mr), _ptrs(mq), cs, 0, mr[0].size, int(k), int(num_bins),
                                        float(minmax_ref[0]), float(minmax_ref[1]), float(minmax_query[0]),
                                        float(minmax_query[1]), _fp(out))
    assert rc == 0
    return out


def _ref_mi_pair_requests(self, measure, members, idx_i, idx_j, *, k=3, num_bins=80, use_abs=False):
    members = _members(members)
    ii = np.ascontiguousarray(idx_i, dtype=np.uint64)
    jj = np.ascontiguousarray(idx_j, dtype=np.uint64)
    out = np.empty(ii.size, np.float32)
    rc = self.mi.ref_mi_pair_requests(int(measure), _ptrs(members), len(members), ii.ctypes.data_as(C.POINTER(C.c_size_t)),
                                      jj.ctypes.data_as(C.POINTER(C.c_size_t)), ii.size, int(k), int(num_bins),
                                      1 if use_abs else 0, _fp(out))
    assert rc == 0
    return out


def _ref_dkl_field(self, estimator, members, *, num_bins=80, k=3):
    members = _members(members)
    out = np.empty(members[0].size, np.float32)
    assert self.mi.ref_dkl_field(int(estimator), _ptrs(members), len(members), members[0].size, int(num_bins), int(k),
                                 _fp(out)) == 0
    return out


Reference.mi_binned = _ref_mi_binned
Reference.mi_kraskov = _ref_mi_kraskov
Reference.kraskov_max = _ref_kraskov_max
Reference.dkl_binned = _ref_dkl_binned
Reference.dkl_knn = _ref_dkl_knn
Reference.mi_field = _ref_mi_field
Reference.mi_symmetric_field = _ref_mi_symmetric_field
Reference.mi_pair_requests = _ref_mi_pair_requests
Reference.dkl_field = _ref_dkl_field


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def _members(members):
    if isinstance(members, np.ndarray):
        members = [members[i] for i in range(members.shape[0])]
    return [np.ascontiguousarray(m, dtype=np.float32).reshape(-1) for m in members]


def build_oracle():
    """(Re)builds oracle/liboracle.so and, when /root/reference is present, oracle/_ref/."""
    subprocess.run(["make", "-s", "-C", str(ORACLE_DIR)], check=True)


def load_oracle() -> Oracle:
    so = ORACLE_DIR / "liboracle.so"
    if not so.exists() or so.stat().st_mtime < (ORACLE_DIR / "corr_oracle.cpp").stat().st_mtime:
        build_oracle()
    return Oracle(C.CDLL(str(so)))


class Standins:
    """oracle/standins/ by themselves (oracle/libstandins_probe.so: this repository's code only)."""

    def __init__(self, lib: C.CDLL):
        self.lib = lib
        lib.standin_digamma.restype = C.c_double
        lib.standin_digamma.argtypes = [C.c_int]
        lib.standin_noise01.restype = None
        lib.standin_noise01.argtypes = [C.c_int, C.c_int, FP]
        lib.standin_knn.restype = C.c_int
        lib.standin_knn.argtypes = [DP, DP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, DP, DP, DP]

    def digamma(self, n):
        return float(self.lib.standin_digamma(int(n)))

    def noise01(self, which, n):
        out = np.empty(n, np.float32)
        self.lib.standin_noise01(int(which), int(n), _fp(out))
        return out

    def knn(self, px, py, center, count, prefill=0):
        """(distances, neighbour x, neighbour y) as the 2-D search leaves its output vectors, which held `prefill` stale
        entries before the query."""
        px, py = np.ascontiguousarray(px, np.float64), np.ascontiguousarray(py, np.float64)
        cap = px.size + prefill + count
        d, nx, ny = (np.empty(cap, np.float64) for _ in range(3))
        as_dp = lambda a: a.ctypes.data_as(DP)
        n = self.lib.standin_knn(as_dp(px), as_dp(py), px.size, int(center), int(count), int(prefill), cap, as_dp(d),
                                 as_dp(nx), as_dp(ny))
        assert n >= 0, "the two findKNearestNeighbors overloads disagree"
        return d[:n], nx[:n], ny[:n]


def load_standins() -> Standins:
    so = ORACLE_DIR / "libstandins_probe.so"
    sources = [ORACLE_DIR / "standins_probe.cpp", *(ORACLE_DIR / "standins").rglob("*.hpp")]
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in sources):
        build_oracle()
    return Standins(C.CDLL(str(so)))


def reference_available() -> bool:
    return (ORACLE_DIR / "_ref" / "libref_corr.so").exists() and (ORACLE_DIR / "_ref" / "libref_mi.so").exists()


def load_reference() -> Reference:
    ref_dir = ORACLE_DIR / "_ref"
    return Reference(C.CDLL(str(ref_dir / "libref_corr.so")), C.CDLL(str(ref_dir / "libref_mi.so")))


def _call_key(*parts) -> str:
    """sha256 of a call: method name, integer arguments and the exact bytes / dtype / shape of every array argument."""
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, np.ndarray):
            h.update(f"a{p.dtype.str}{p.shape}".encode())
            h.update(np.ascontiguousarray(p).tobytes())
        else:
            h.update(f"v{p!r}".encode())
    return h.hexdigest()


class RecordedReference:
    """The Reference interface answered from recorded calls of the reference's object code.  With `live` set, every
    call is forwarded to it and recorded (oracle/make_golden.py); without, a call whose inputs were not recorded fails
    instead of answering."""

    # calls answered by libref_mi.so: recorded in mi_calls.npz, keyed by the first MI_KEY_BYTES bytes of the call's hash
    # (stored as bytes, not hex: the file holds thousands of scalar calls)
    MI_METHODS = frozenset(["mi_binned", "mi_kraskov", "kraskov_max", "dkl_binned", "dkl_knn", "mi_field",
                            "mi_symmetric_field", "mi_pair_requests", "dkl_field"])
    MI_KEY_BYTES = 12

    def __init__(self, calls=None, live: Reference | None = None, mi_calls=None):
        self.calls = dict(calls or {})
        self.mi_calls = dict(mi_calls or {})
        self.live = live

    @staticmethod
    def _unpack(d, keys):
        offsets, values, scalar = d["offsets"], d["values"], d["scalar"]
        calls = {}
        for i, k in enumerate(keys):
            v = values[offsets[i]:offsets[i + 1]]
            calls[k] = float(v[0]) if scalar[i] else v
        return calls

    @staticmethod
    def _pack(calls, keys):
        vals = [np.atleast_1d(np.asarray(calls[k], np.float32)) for k in keys]
        offsets = np.concatenate([[0], np.cumsum([v.size for v in vals])]).astype(np.int64)
        return dict(offsets=offsets, values=np.concatenate(vals),
                    scalar=np.array([not isinstance(calls[k], np.ndarray) for k in keys]))

    @classmethod
    def load(cls, path=RECORDED_CALLS, mi_path=RECORDED_MI_CALLS):
        d = np.load(path, allow_pickle=False)
        calls = cls._unpack(d, [str(k) for k in d["keys"]])
        m = np.load(mi_path, allow_pickle=False)
        mi_calls = cls._unpack(m, [bytes(k).hex() for k in m["keys"]])
        return cls(calls, mi_calls=mi_calls)

    def save(self, path=RECORDED_CALLS):
        keys = sorted(self.calls)
        np.savez_compressed(path, keys=np.array(keys), **self._pack(self.calls, keys))

    def save_mi(self, path=RECORDED_MI_CALLS):
        keys = sorted(self.mi_calls)
        raw = np.frombuffer(bytes.fromhex("".join(keys)), np.uint8).reshape(len(keys), self.MI_KEY_BYTES)
        np.savez_compressed(path, keys=raw, **self._pack(self.mi_calls, keys))

    def _answer(self, compute, *parts):
        key = _call_key(*parts)
        store, name = self.calls, RECORDED_CALLS.name
        if parts[0] in self.MI_METHODS:
            key, store, name = key[:2 * self.MI_KEY_BYTES], self.mi_calls, RECORDED_MI_CALLS.name
        if self.live is not None:
            v = compute(self.live)
            store[key] = np.float32(v) if isinstance(v, float) else np.array(v, np.float32)
            return v
        if key not in store:
            raise KeyError(f"{parts[0]}: no recorded answer of the reference for these inputs "
                           f"({name}; oracle/make_golden.py re-records it where the reference is present)")
        v = store[key]
        return float(v) if not isinstance(v, np.ndarray) else v.copy()

    def pearson(self, x, y):
        x, y = _f32(x), _f32(y)
        return self._answer(lambda r: r.pearson(x, y), "pearson", x, y)

    def ranks(self, v):
        v = _f32(v)
        return self._answer(lambda r: r.ranks(v), "ranks", v)

    def kendall(self, x, y):
        x, y = _f32(x), _f32(y)
        return self._answer(lambda r: r.kendall(x, y), "kendall", x, y)

    def kendall_slow(self, x, y):
        x, y = _f32(x), _f32(y)
        return self._answer(lambda r: r.kendall_slow(x, y), "kendall_slow", x, y)

    def field(self, measure, members, ref_values, voxel_range=None):
        members, ref_values = _members(members), _f32(ref_values)
        return self._answer(lambda r: r.field(measure, members, ref_values, voxel_range), "field", int(measure),
                            *members, ref_values, voxel_range)

    def pair_requests(self, measure, members, idx_i, idx_j):
        members = _members(members)
        ii = np.ascontiguousarray(idx_i, dtype=np.uint64)
        jj = np.ascontiguousarray(idx_j, dtype=np.uint64)
        return self._answer(lambda r: r.pair_requests(measure, members, ii, jj), "pair_requests", int(measure),
                            *members, ii, jj)

    # -- libref_mi.so: every scalar and every array of a call is part of its key
    def mi_binned(self, x01, y01, num_bins):
        x01, y01 = _f32(x01), _f32(y01)
        return self._answer(lambda r: r.mi_binned(x01, y01, num_bins), "mi_binned", x01, y01, int(num_bins))

    def mi_kraskov(self, x, y, k, estimator=1):
        x, y = _f32(x), _f32(y)
        return self._answer(lambda r: r.mi_kraskov(x, y, k, estimator), "mi_kraskov", x, y, int(k), int(estimator))

    def kraskov_max(self, k, n):
        return self._answer(lambda r: r.kraskov_max(k, n), "kraskov_max", int(k), int(n))

    def dkl_binned(self, values, num_bins):
        v = _f32(values)
        return self._answer(lambda r: r.dkl_binned(v, num_bins), "dkl_binned", v, int(num_bins))

    def dkl_knn(self, values, k):
        v = _f32(values)
        return self._answer(lambda r: r.dkl_knn(v, k), "dkl_knn", v, int(k))

    def mi_field(self, measure, members, ref_values, *, k=3, estimator=1, num_bins=80, minmax_ref=(0.0, 1.0),
                 minmax_query=None, voxel_range=None):
        members, ref_values = _members(members), _f32(ref_values)
        minmax_query = minmax_ref if minmax_query is None else minmax_query
        kw = dict(k=int(k), estimator=int(estimator), num_bins=int(num_bins), minmax_ref=_mm(minmax_ref),
                  minmax_query=_mm(minmax_query), voxel_range=voxel_range)
        return self._answer(lambda r: r.mi_field(measure, members, ref_values, **kw), "mi_field", int(measure), *members,
                            ref_values, *kw.values())

    def mi_symmetric_field(self, measure, members_ref, members_query, *, k=3, num_bins=80, minmax_ref=(0.0, 1.0),
                           minmax_query=(0.0, 1.0)):
        mr, mq = _members(members_ref), _members(members_query)
        kw = dict(k=int(k), num_bins=int(num_bins), minmax_ref=_mm(minmax_ref), minmax_query=_mm(minmax_query))
        return self._answer(lambda r: r.mi_symmetric_field(measure, mr, mq, **kw), "mi_symmetric_field", int(measure),
                            *mr, "|", *mq, *kw.values())

    def mi_pair_requests(self, measure, members, idx_i, idx_j, *, k=3, num_bins=80, use_abs=False):
        members = _members(members)
        ii = np.ascontiguousarray(idx_i, dtype=np.uint64)
        jj = np.ascontiguousarray(idx_j, dtype=np.uint64)
        kw = dict(k=int(k), num_bins=int(num_bins), use_abs=bool(use_abs))
        return self._answer(lambda r: r.mi_pair_requests(measure, members, ii, jj, **kw), "mi_pair_requests",
                            int(measure), *members, ii, jj, *kw.values())

    def dkl_field(self, estimator, members, *, num_bins=80, k=3):
        members = _members(members)
        return self._answer(lambda r: r.dkl_field(estimator, members, num_bins=num_bins, k=k), "dkl_field",
                            int(estimator), *members, int(num_bins), int(k))


def _mm(minmax):
    """An extrema pair as the C ABI receives it: two floats."""
    return (float(np.float32(minmax[0])), float(np.float32(minmax[1])))


def load_reference_or_recorded():
    """The reference's object code where oracle/_ref was built, else its recorded answers."""
    return load_reference() if reference_available() else RecordedReference.load()
