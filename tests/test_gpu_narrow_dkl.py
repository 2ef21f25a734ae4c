"""GPU: DKL (both estimators) on members in a narrow native format (uint8, uint16, float16), read as stored by
dkl_narrow_kernel.  Every case runs the call on float32 members holding the converted values (dkl_kernel) and on the narrow
members, and asserts that the narrow kernel ran, that no fp32 copy of the ensemble exists afterwards, that the two results
are bit-identical (NaNs in the same places) and that both are within parity.py's standing tolerance of the oracle on the
converted values.

The native route serves what the measurement of profiles/narrow_dkl_ab.md accepted: routed_native below mirrors
dkl_narrow_routed (crf_internal.h; tests/test_narrow_dkl_routing.py compares the two tables).  A case outside it asserts the
copy route instead (dkl_kernel, a copy held) with the same two comparisons.

The k-NN estimator returns NaN for a voxel with two equal values, so its cases build every voxel from distinct codes
(distinct_codes) and assert that the oracle's result is finite in at least 90 % of the voxels."""
import ctypes as C
import functools

import numpy as np
import pytest

from correrender_amd import CorrFieldError, Measure
from parity import assert_bit_exact, assert_close
from test_gpu_member_formats import FORMATS, box01, cast, convert, to_device, to_device_members, _every_code

pytestmark = pytest.mark.gpu

KERNEL = "dkl_narrow_kernel"
F32_KERNEL = "dkl_kernel"
FMT_OF = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}
FORMAT_IDS = {"u8": 1, "u16": 2, "f16": 3}
BINNED, KNN = 0, 1
GRID = (13, 11, 7)  # 1001 voxels: whole waves and a partial one


def routed_native(fmt, cs, estimator, k):
    """The routing table of native DKL (crf_internal.h: dkl_narrow_routed), from profiles/narrow_dkl_ab.md: binned -- u8 and
    u16 at 17..32 members, u8 and f16 from 97 members on (the counting-sort instantiation); k-NN -- u8 and u16 at 49..64
    members with k <= 2, every format from 129 members on."""
    if fmt not in ("u8", "u16", "f16"):
        return False
    n = (cs + 15) // 16 * 16
    if estimator == BINNED:
        return fmt != "u16" if cs >= 97 else (n == 32 and fmt != "f16")
    return cs >= 129 or (n == 64 and k <= 2 and fmt != "f16")


def default_k(cs):
    return max(-(-3 * cs // 100), 1)  # DKLCalculator.cpp:94-101


def knn_ks(cs):
    return sorted({1, min(2, cs - 1), default_k(cs), min(cs - 1, 7)})


# ---- data ---------------------------------------------------------------------------------------------------------------
def distinct_codes(fmt, cs, n, seed):
    """[cs, n] codes of `fmt`, the cs codes of every voxel distinct.  u8: a random draw of cs of the 256 codes per voxel.
    16-bit: code = lo + slot * stride + jitter with the voxel's slots a random permutation of 0..cs-1 and jitter < stride
    (u16: the whole code range; f16: the bit patterns of [0.125, 1), or of the normal numbers below 1 above 1024 members)."""
    rng = np.random.default_rng(seed)
    if fmt == "u8":
        assert cs <= 256
        codes = np.argsort(rng.random((n, 256)), axis=1)[:, :cs].T.astype(np.uint8)
    else:
        lo, hi = (0, 65536) if fmt == "u16" else ((0x3000, 0x3C00) if cs <= 1024 else (0x0400, 0x3C00))
        stride = (hi - lo) // cs
        assert stride >= 1
        slots = np.argsort(rng.random((n, cs)), axis=1).T
        codes = (lo + slots * stride + rng.integers(0, stride, (cs, n))).astype(np.uint16)
    ordered = np.sort(codes, axis=0)
    assert (ordered[1:] != ordered[:-1]).all()
    for v in (0, n // 2, n - 1):
        assert np.unique(codes[:, v]).size == cs
    return np.ascontiguousarray(codes) if fmt != "f16" else np.ascontiguousarray(codes).view(np.float16)


def plant(narrow):
    """Plants the special voxels into `narrow` ([cs, n], in place): 0 all members equal (stdev 0); 1 two equal codes (k-NN:
    NaN); 2 the codes 0 and the format's maximum; f16: 3 a NaN member, 4 a +inf, 5 a -inf member, 6 a subnormal; 16-bit: 7 a
    large offset with a tiny spread."""
    cs, n = narrow.shape
    if cs < 2 or n < 64:
        return narrow
    fmt = FMT_OF[narrow.dtype]
    bits = narrow.view(np.uint16) if fmt == "f16" else narrow
    top = {"u8": 0xFF, "u16": 0xFFFF, "f16": 0x7BFF}[fmt]
    bits[:, 0] = bits[0, 0]
    bits[1, 1] = bits[0, 1]
    bits[0, 2], bits[1, 2] = 0, top
    if fmt == "f16":
        bits[cs // 2, 3] = 0x7E00
        bits[cs // 2, 4] = 0x7C00
        bits[cs // 2, 5] = 0xFC00
        bits[cs // 2, 6] = 0x0001
    if fmt != "u8":
        base = 60000 if fmt == "u16" else 0x3B00  # 0.9155 + cs codes, 0.875 + cs ulps
        bits[:, 7] = base + np.random.default_rng(cs).permutation(cs)
    return narrow


@functools.lru_cache(maxsize=None)
def binned_data(fmt, cs, grid=GRID, seed=0):
    xs, ys, zs = grid
    narrow = cast(box01(xs, ys, zs, cs, seed=seed + cs), fmt).reshape(cs, -1)
    return plant(narrow).reshape(cs, zs, ys, xs)


@functools.lru_cache(maxsize=None)
def knn_data(fmt, cs, grid=GRID, seed=0):
    xs, ys, zs = grid
    return plant(distinct_codes(fmt, cs, xs * ys * zs, 100 + seed + cs)).reshape(cs, zs, ys, xs)


# ---- the check ----------------------------------------------------------------------------------------------------------
def dkl_device(eng, estimator, out=None, **kw):
    import torch
    if out is None:
        out = torch.empty(eng.num_voxels, dtype=torch.float32, device="cuda")
    eng.dkl_device(estimator, out, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def on_f32_members(eng, narrow, call):
    cs, zs, ys, xs = narrow.shape
    eng.set_grid(xs, ys, zs, cs)
    with np.errstate(all="ignore"):
        eng.upload_members(convert(narrow))
    got = call(eng)
    assert eng.last_kernel_name() == F32_KERNEL
    return got


def bind_narrow(eng, narrow, members=None):
    cs, zs, ys, xs = narrow.shape
    eng.set_grid(xs, ys, zs, cs)
    members = to_device_members(narrow.reshape(cs, -1)) if members is None else members
    eng.bind_members(members)
    assert eng.member_format() == FMT_OF[narrow.dtype]
    assert eng.wide_copy_bytes() == 0
    return members


def assert_route(eng, fmt, cs, estimator, k, what):
    """Native where the measured routing table says so, else the fp32 kernel on the copy."""
    if routed_native(fmt, cs, estimator, k):
        assert eng.last_kernel_name() == KERNEL, what
        assert eng.wide_copy_bytes() == 0, what
    else:
        assert eng.last_kernel_name() == F32_KERNEL, what
        assert eng.wide_copy_bytes() > 0, what


def check_native(eng, oracle, narrow, estimator, what, num_bins=80, k=3, members=None, out=None):
    """DKL of `narrow` ([cs, zs, ys, xs]) read as stored against dkl_kernel on fp32 members holding the converted values (bit
    for bit) and against the oracle on those values (tolerance)."""
    kw = dict(num_bins=num_bins, k=k)
    fmt, cs = FMT_OF[narrow.dtype], narrow.shape[0]
    with np.errstate(all="ignore"):
        want = oracle.dkl(estimator, convert(narrow), **kw)
    if estimator == KNN and cs <= 256:
        assert np.isfinite(want).mean() >= 0.9, what
    f32 = on_f32_members(eng, narrow, lambda e: dkl_device(e, estimator, **kw))
    assert_close(f32, want, f"{what}: fp32 members vs oracle")
    members = bind_narrow(eng, narrow, members)
    got = dkl_device(eng, estimator, out=out, **kw)
    assert_route(eng, fmt, cs, estimator, k, what)
    assert_bit_exact(got, f32, f"{what}: native vs fp32 members")
    assert_close(got, want, f"{what}: native vs oracle")
    return members, got


# ---- 1. member counts, binned -------------------------------------------------------------------------------------------
# 16 | 17: a network boundary; 96 | 97: the end of the register form; 128 | 129: the end of the networks; 200 | 201 with 80
# bins: the LDS limit (cs * 256 + bins * 128 <= 61440), so 201 and 300 run in the workspace, as does 97 with 300 bins
@pytest.mark.parametrize("cs", [1, 2, 3, 16, 17, 96, 97, 128, 129, 200, 201, 300])
@pytest.mark.parametrize("fmt", FORMATS)
def test_member_counts_binned(engine, oracle, fmt, cs):
    narrow = binned_data(fmt, cs)
    for bins in (10, 80, 300):
        _, got = check_native(engine, oracle, narrow, BINNED, f"binned {fmt} cs={cs} bins={bins}", num_bins=bins)
    if cs == 1:
        assert (got == 1.0).all()
    elif fmt == "f16":
        assert np.isnan(got[3])  # the NaN member


# ---- 2. member counts, k-NN ---------------------------------------------------------------------------------------------
# 3 | 4: the lower edge of the register descent; 96 | 97: its end; 129 and up: counting sort, both columns in the workspace
# (no 300 distinct uint8 codes: beyond 256 members the k-NN cases are uint16 / float16)
@pytest.mark.parametrize("fmt,cs", [(f, c) for f in FORMATS for c in [2, 3, 4, 5, 16, 17, 96, 97, 112, 128, 129, 300]
                                    if f != "u8" or c <= 256])
def test_member_counts_knn(engine, oracle, fmt, cs):
    narrow = knn_data(fmt, cs)
    for k in knn_ks(cs):
        _, got = check_native(engine, oracle, narrow, KNN, f"k-NN {fmt} cs={cs} k={k}", k=k)
        assert np.isnan(got[0])  # all members equal: no spread, or zero distances
        if fmt == "f16":
            assert np.isnan(got[3])  # the NaN member


# ---- 3. the upper limit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator", [BINNED, KNN])
@pytest.mark.parametrize("cs", [2047, 2048])
@pytest.mark.parametrize("fmt", ["u16", "f16"])
def test_upper_limit(engine, oracle, fmt, cs, estimator):
    grid = (16, 4, 1)
    if estimator == BINNED:
        check_native(engine, oracle, binned_data(fmt, cs, grid), BINNED, f"binned {fmt} cs={cs}")
    else:
        narrow = knn_data(fmt, cs, grid)
        for k in (1, default_k(cs)):
            check_native(engine, oracle, narrow, KNN, f"k-NN {fmt} cs={cs} k={k}", k=k)


# ---- 4. more workspace tiles than blocks --------------------------------------------------------------------------------
def test_workspace_tile_walk(engine, oracle):
    """201 members, 80 bins: the tile is above the LDS limit; 41 x 40 x 40 = 65 600 voxels = 1025 tiles on kDklBlocks = 1024
    blocks: block 0 walks a second workspace slice."""
    narrow = binned_data("u8", 201, (41, 40, 40))
    _, got = check_native(engine, oracle, narrow, BINNED, "binned u8 cs=201, 1025 workspace tiles")
    assert np.isfinite(got[-1])


# ---- 5. CRF_DKL_COUNTING_SORT -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator", [BINNED, KNN])
@pytest.mark.parametrize("fmt", FORMATS)
def test_counting_sort_switch(engine, oracle, monkeypatch, fmt, estimator):
    cs = 64
    narrow = binned_data(fmt, cs) if estimator == BINNED else knn_data(fmt, cs)
    k = default_k(cs)
    monkeypatch.setenv("CRF_DKL_COUNTING_SORT", "1")  # (restored when the test ends)
    check_native(engine, oracle, narrow, estimator, f"{fmt} est={estimator} CRF_DKL_COUNTING_SORT=1", k=k)


# ---- 6. every code ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["u16a", "u16b", "f16", "u8"])
def test_every_code(engine, oracle, which):
    narrow, count = _every_code(which)
    # the same codes as [cs, n] with a member count whose binned call is routed native: u8 and u16 at 32, f16 at 128
    cs = 128 if which == "f16" else 32
    narrow = np.ascontiguousarray(narrow.reshape(cs, -1))
    n = narrow.shape[1]
    assert routed_native(FMT_OF[narrow.dtype], cs, BINNED, 0)
    with np.errstate(all="ignore"):
        check_native(engine, oracle, narrow.reshape(cs, 1, 1, n), BINNED, f"every code {which}")


# ---- 7. borrowed members at element alignment -----------------------------------------------------------------------------
# (24 binned: native for u8 and u16; 100 binned: for u8 and f16; 56 k-NN with k = 1: for u8 and u16; 130 k-NN: for all)
@pytest.mark.parametrize("estimator,cs", [(BINNED, 24), (BINNED, 100), (KNN, 56), (KNN, 130)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_element_aligned_borrowed_members(engine, oracle, fmt, estimator, cs):
    grid = (7, 5, 3)
    n = 7 * 5 * 3
    narrow = binned_data(fmt, cs, grid) if estimator == BINNED else knn_data(fmt, cs, grid)
    rows = np.zeros((cs, n + 7), narrow.dtype)  # row stride 112 elements: whole dwords
    rows[:, 1:n + 1] = narrow.reshape(cs, n)
    buf = to_device(rows)
    members = [buf[c, 1:n + 1] for c in range(cs)]
    if fmt == "u8":
        assert all(m.data_ptr() % 2 == 1 for m in members)  # odd byte offsets
    else:
        assert all(m.data_ptr() % 4 == 2 for m in members)
    check_native(engine, oracle, narrow, estimator, f"{fmt} est={estimator} element-aligned rows", k=1, members=members)
    del members, buf


@pytest.mark.parametrize("fmt", ["u16", "f16"])
def test_16_bit_members_at_an_odd_byte_take_the_copy(engine, oracle, fmt):
    import torch
    cs, grid = 130, (7, 5, 3)  # k-NN from 129 members on: native in every format
    xs, ys, zs = grid
    n = xs * ys * zs
    narrow = knn_data(fmt, cs, grid)
    assert routed_native(fmt, cs, KNN, 1)
    _, aligned = check_native(engine, oracle, narrow, KNN, f"{fmt} at an even byte", k=1)
    raw = np.zeros((cs, 2 * n + 8), np.uint8)
    raw[:, 1:2 * n + 1] = narrow.reshape(cs, n).view(np.uint8)
    buf = torch.from_numpy(raw).cuda()
    # (no 16-bit torch tensor starts at an odd byte: the pointers go to the C entry point directly)
    odd = [buf[c, 1:].data_ptr() for c in range(cs)]
    assert all(p % 2 == 1 for p in odd)
    engine.set_grid(xs, ys, zs, cs)
    engine._check(engine._lib.crf_bind_members_device_format(engine._ctx, FORMAT_IDS[fmt], (C.c_void_p * cs)(*odd)))
    assert engine.member_format() == fmt and engine.wide_copy_bytes() == 0
    got = dkl_device(engine, KNN, k=1)
    assert engine.last_kernel_name() == F32_KERNEL and engine.wide_copy_bytes() > 0
    assert_bit_exact(got, aligned, f"{fmt} at an odd byte vs at an even byte")
    engine.set_grid(xs, ys, zs, cs)  # lets go of the borrowed pointers
    del buf


# ---- 8. ragged grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(3, 1, 1), (63, 1, 1), (64, 1, 1), (65, 1, 1), (257, 1, 1)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ragged_grids(engine, oracle, fmt, grid):
    check_native(engine, oracle, binned_data(fmt, 24, grid), BINNED, f"binned {fmt} grid={grid}")
    check_native(engine, oracle, knn_data(fmt, 24, grid), KNN, f"k-NN {fmt} grid={grid}", k=1)
    check_native(engine, oracle, knn_data(fmt, 130, grid), KNN, f"k-NN {fmt} cs=130 grid={grid}", k=4)  # native in every format


# ---- 9. output ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_output_aligned_to_four_bytes_only(engine, oracle, fmt):
    import torch
    grid = (7, 5, 3)
    out = torch.empty(7 * 5 * 3 + 1, dtype=torch.float32, device="cuda")[1:]
    assert out.data_ptr() % 8 == 4
    check_native(engine, oracle, binned_data(fmt, 24, grid), BINNED, f"binned {fmt} out + 4 B", out=out)
    check_native(engine, oracle, knn_data(fmt, 24, grid), KNN, f"k-NN {fmt} out + 4 B", k=1, out=out)
    check_native(engine, oracle, knn_data(fmt, 130, grid), KNN, f"k-NN {fmt} cs=130 out + 4 B", k=4, out=out)


@pytest.mark.parametrize("estimator", ["binned", "knn"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_and_device_output(engine, oracle, fmt, estimator):
    cs = 130  # native but for the binned estimator on u16
    narrow = binned_data(fmt, cs) if estimator == "binned" else knn_data(fmt, cs)
    members = bind_narrow(engine, narrow)
    engine.dkl(estimator, k=1)
    engine.set_profiling(True)
    try:
        engine.take_kernel_time()
        host = engine.dkl(estimator, k=1)
        assert_route(engine, fmt, cs, BINNED if estimator == "binned" else KNN, 1, f"{fmt} {estimator}")
        ms, launches = engine.take_kernel_time()
        assert launches == 1 and ms > 0
        device = dkl_device(engine, estimator, k=1)
        ms, launches = engine.take_kernel_time()
        assert launches == 1 and ms > 0
    finally:
        engine.set_profiling(False)
    assert_bit_exact(host.reshape(-1), device, f"{fmt} {estimator}: host vs device output")
    del members


# ---- 10. the life of the fp32 copy ----------------------------------------------------------------------------------------
def test_copy_lifetime(engine, oracle):
    import torch
    import oracle_lib
    cs, grid = 24, (16, 8, 4)
    xs, ys, zs = grid
    n = xs * ys * zs
    a, b = binned_data("u16", cs, grid, seed=1), binned_data("u16", cs, grid, seed=2)
    members, first = check_native(engine, oracle, a, BINNED, "first data")
    engine.ensemble_stat(0)
    engine.set_predicate(">", 0.5, 0, cs)
    assert engine.wide_copy_bytes() == 0  # native DKL, mean and predicate: no copy
    wide = convert(a)
    spearman = engine.compute(Measure.SPEARMAN, (5, 3, 2))  # 24 members: builds the copy
    assert engine.last_member_format() == "f32"
    assert engine.wide_copy_bytes() >= cs * n * 4
    assert_bit_exact(spearman, oracle.field(oracle_lib.SPEARMAN, wide, wide[:, 2, 3, 5].copy()), "spearman on the copy")
    held = engine.wide_copy_bytes()
    again = dkl_device(engine, BINNED)
    assert engine.last_kernel_name() == KERNEL  # still native, beside the copy
    assert engine.last_member_format() == "f32"  # DKL is no field evaluation: left alone
    assert engine.wide_copy_bytes() == held
    assert_bit_exact(again, first, "DKL next to the copy")
    engine.members_changed()
    assert engine.wide_copy_bytes() == 0
    members.view(torch.int16).copy_(to_device(b).view(torch.int16).reshape(cs, n))
    torch.cuda.synchronize()
    engine.members_changed()
    changed = dkl_device(engine, BINNED)
    assert engine.last_kernel_name() == KERNEL and engine.wide_copy_bytes() == 0
    with np.errstate(all="ignore"):
        assert_close(changed, oracle.dkl(BINNED, convert(b), num_bins=80), "new contents")
    assert not np.array_equal(changed, first)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(convert(b))  # rebound as fp32
    f32 = dkl_device(engine, BINNED)
    assert engine.last_kernel_name() == F32_KERNEL
    assert_bit_exact(f32, changed, "rebound as fp32")
    del members


# ---- 11. errors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_errors_unchanged(engine, fmt):
    cs, grid = 8, (4, 4, 2)
    members = bind_narrow(engine, binned_data(fmt, cs, grid))
    with pytest.raises(CorrFieldError, match="k=") as e:
        engine.dkl("knn", k=8)
    assert e.value.code == 1  # CRF_ERR_ARGUMENT
    with pytest.raises(CorrFieldError, match="num_bins") as e:
        engine.dkl("binned", num_bins=0)
    assert e.value.code == 1
    for est in (-1, 2):
        with pytest.raises(CorrFieldError, match=f"unknown DKL estimator {est}") as e:
            engine.dkl(est)
        assert e.value.code == 1
    lib = engine._lib
    assert lib.crf_compute_dkl(engine._ctx, 0, 20, 2, C.POINTER(C.c_float)()) == 1
    assert b"null output" in lib.crf_last_error(engine._ctx)
    assert lib.crf_compute_dkl_device(engine._ctx, 0, 20, 2, C.c_void_p(0), C.c_void_p(0)) == 1
    assert b"null output" in lib.crf_last_error(engine._ctx)
    assert engine.wide_copy_bytes() == 0
    del members
