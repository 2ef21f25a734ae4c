"""GPU: primary members in the narrow native formats (uint8, uint16, float16).  The definition of correct: every result
equals the result of the same call on float32 members that hold the converted values -- b / 255, s / 65535, float(h), the
reference's HostCacheEntry::data<float>() -- bit for bit.  The numpy conversions below are the same IEEE operations."""
import ctypes as C

import numpy as np
import pytest

from correrender_amd import CorrFieldError, Measure, synth
from parity import assert_bit_exact, assert_close
import oracle_lib

pytestmark = pytest.mark.gpu

FORMATS = ["u8", "u16", "f16"]
NATIVE_KERNEL = "pearson_narrow_kernel"


def convert(a: np.ndarray) -> np.ndarray:
    """The float32 values the calculators see of a narrow array."""
    if a.dtype == np.uint8:
        return a.astype(np.float32) / np.float32(255)
    if a.dtype == np.uint16:
        return a.astype(np.float32) / np.float32(65535)
    assert a.dtype == np.float16
    return a.astype(np.float32)


def cast(ens01: np.ndarray, fmt: str) -> np.ndarray:
    """A float32 ensemble in [0, 1] in format `fmt`."""
    if fmt == "u8":
        return np.rint(ens01 * np.float32(255)).astype(np.uint8)
    if fmt == "u16":
        return np.rint(ens01 * np.float32(65535)).astype(np.uint16)
    return ens01.astype(np.float16)


def box01(xs, ys, zs, cs, seed):
    ens = synth.box_ensemble(xs, ys, zs, cs, seed=seed)
    lo, hi = ens.min(), ens.max()
    return ((ens - lo) / (hi - lo)).astype(np.float32)


def to_device(a: np.ndarray):
    import torch
    if a.dtype == np.uint16:  # (torch.from_numpy takes no uint16 in every torch release)
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def to_device_members(narrow: np.ndarray):
    """`narrow` ([cs, ...]) on the device as a [cs, n] view whose rows all start on a 4-byte boundary, which the native
    path asks of borrowed members: a plain [cs, n] copy puts member 1 at byte n * itemsize, odd for most grids here."""
    cs, n = narrow.shape[0], narrow[0].size
    rows = np.zeros((cs, (n + 3) // 4 * 4), narrow.dtype)
    rows[:, :n] = narrow.reshape(cs, n)
    members = to_device(rows)[:, :n]
    assert all(members[c].data_ptr() % 4 == 0 for c in range(cs))
    return members


def pearson_device(eng, n, ref, out=None):
    import torch
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device="cuda")
    eng.compute_device(Measure.PEARSON, out, ref)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_native(eng, oracle, narrow, ref, what, out=None):
    """Binds `narrow` ([cs, zs, ys, xs]) and checks the native Pearson field against the oracle on the converted values."""
    cs, zs, ys, xs = narrow.shape
    eng.set_grid(xs, ys, zs, cs)
    members = to_device_members(narrow)
    eng.bind_members(members)
    fmt = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}[narrow.dtype]
    assert eng.member_format() == fmt
    got = pearson_device(eng, xs * ys * zs, ref, out)
    assert eng.last_member_format() == fmt, what
    assert eng.last_kernel_name() == NATIVE_KERNEL, what
    assert eng.last_member_layout() == "raw"
    wide = convert(narrow)
    x, y, z = ref
    want = oracle.field(oracle_lib.PEARSON, wide, wide[:, z, y, x].copy())
    assert_bit_exact(got, want, what)
    return members


# ---- 1. member counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [2, 7, 8, 9, 16, 17, 33, 64, 65, 100, 128])
@pytest.mark.parametrize("fmt", FORMATS)
def test_member_counts_native(engine, oracle, fmt, cs):
    # 13*11*7 = 1001 voxels, 1001 % 4 = 1: a ragged dword, whole blocks and a partial one
    narrow = cast(box01(13, 11, 7, cs, seed=cs), fmt)
    check_native(engine, oracle, narrow, (5, 6, 3), f"{fmt} cs={cs}")


# ---- 2. ragged ends -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(3, 1, 1), (2, 3, 1), (7, 5, 3), (255, 1, 1), (256, 1, 1), (257, 1, 1)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ragged_ends(engine, oracle, fmt, grid):
    xs, ys, zs = grid
    narrow = cast(box01(xs, ys, zs, 24, seed=xs), fmt)
    check_native(engine, oracle, narrow, (xs // 2, ys // 2, zs // 2), f"{fmt} grid={grid}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_output_aligned_to_four_bytes_only(engine, oracle, fmt):
    import torch
    n = 7 * 5 * 3
    out = torch.empty(n + 1, dtype=torch.float32, device="cuda")[1:]
    assert out.data_ptr() % 8 == 4
    check_native(engine, oracle, cast(box01(7, 5, 3, 24, seed=2), fmt), (1, 2, 1), f"{fmt} out + 4 B", out=out)


# ---- 3. borrowed views at odd byte offsets ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "u16"])
def test_unaligned_borrowed_members_take_the_widened_path(engine, oracle, fmt):
    cs, (xs, ys, zs) = 24, (7, 5, 3)
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=4), fmt)
    rows = np.zeros((cs, n + 7), narrow.dtype)  # row stride (n + 7) elements = 112 elements: whole dwords
    rows[:, 1:n + 1] = narrow.reshape(cs, n)
    buf = to_device(rows)
    members = [buf[c, 1:n + 1] for c in range(cs)]
    assert all(m.data_ptr() % 4 != 0 for m in members)
    engine.set_grid(xs, ys, zs, cs)
    engine.bind_members(members)
    assert engine.member_format() == fmt
    got = pearson_device(engine, n, (3, 2, 1))
    assert engine.last_member_format() == "f32"
    wide = convert(narrow)
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, wide, wide[:, 1, 2, 3].copy()), f"{fmt} offset 1")


# ---- 4. every code ------------------------------------------------------------------------------------------------------
def _every_code(which):
    if which == "u16a" or which == "u16b":
        codes = np.random.default_rng(1 if which == "u16a" else 2).permutation(65536).astype(np.uint16)
        return codes.reshape(64, 1024), 65536
    if which == "f16":
        bits = np.arange(65536, dtype=np.uint32)
        bits = bits[(bits & 0x7C00) != 0x7C00].astype(np.uint16)
        assert bits.size == 63488
        return np.random.default_rng(3).permutation(bits).view(np.float16).reshape(64, 992), 63488
    return np.tile(np.arange(256, dtype=np.uint8), 4).reshape(16, 64), 256


@pytest.mark.parametrize("which", ["u16a", "u16b", "f16", "u8"])
def test_every_code(engine, oracle, which):
    narrow, count = _every_code(which)
    assert np.unique(narrow.view(np.uint8 if narrow.dtype == np.uint8 else np.uint16)).size == count
    cs, n = narrow.shape
    wide = convert(narrow)
    assert np.unique(wide.view(np.uint32)).size >= count - 1  # (+0 and -0 of f16 are two codes and two floats)
    with np.errstate(all="ignore"):
        members = check_native(engine, oracle, narrow.reshape(cs, 1, 1, n), (n // 3, 0, 0), f"every code {which}")
    # the widened copy, value by value
    got = np.stack([engine.gather_reference(x, 0, 0) for x in range(n)], axis=1)
    assert (got.view(np.uint32) == wide.view(np.uint32)).all(), f"widened copy {which}"
    del members


# ---- 5. f16 special values ----------------------------------------------------------------------------------------------
def test_f16_special_values(engine, oracle):
    cs, n = 24, 300
    narrow = cast(box01(n, 1, 1, cs, seed=5), "f16").reshape(cs, n)
    narrow[3, 10] = np.float16(0.0)
    narrow[4, 10] = np.float16(-0.0)
    narrow[5, 11:14] = np.array([0x0001, 0x8001, 0x03FF], np.uint16).view(np.float16)  # denormals
    narrow[:, 20] = np.array([0x0001 + e for e in range(cs)], np.uint16).view(np.float16)  # a voxel of denormals only
    narrow[6, 30] = np.float16(np.inf)
    narrow[7, 31] = np.float16(-np.inf)
    narrow[8, 32] = np.float16(np.nan)
    narrow[9, 33] = np.float16(np.inf)
    narrow[10, 33] = np.float16(-np.inf)
    with np.errstate(all="ignore"):
        for ref in [(100, 0, 0), (10, 0, 0), (20, 0, 0), (30, 0, 0), (32, 0, 0)]:
            check_native(engine, oracle, narrow.reshape(cs, 1, 1, n), ref, f"f16 specials ref={ref}")


# ---- 6. the widened path ------------------------------------------------------------------------------------------------
def _widened_calls(eng, n, sec, pairs, mm):
    """Every entry point of the widened path on the members bound right now."""
    res = {}
    res["spearman"] = eng.compute(Measure.SPEARMAN, (5, 3, 2)).ravel()
    res["kendall"] = eng.compute(Measure.KENDALL, (5, 3, 2)).ravel()
    res["minmax"] = np.array(eng.member_minmax(), np.float32)
    res["mi_binned"] = eng.compute(Measure.MUTUAL_INFORMATION_BINNED, (5, 3, 2), minmax_ref=mm).ravel()
    res["kraskov"] = eng.compute(Measure.MUTUAL_INFORMATION_KRASKOV, (5, 3, 2), k=3).ravel()
    res["symmetric"] = eng.compute(Measure.PEARSON, symmetric=True).ravel()
    res["mean"] = eng.ensemble_stat(0).ravel()
    res["spread"] = eng.ensemble_stat(1).ravel()
    res["predicate"] = eng.set_predicate(">", 0.5, 2, 20).ravel()
    res["dkl"] = eng.dkl("binned").ravel()
    res["pairs"] = eng.compute_requests(Measure.PEARSON, pairs)
    return res


def test_widened_path(engine, oracle):
    cs, (xs, ys, zs) = 24, (16, 8, 4)
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=6), "u16")
    wide = convert(narrow)
    sec = synth.box_ensemble(xs, ys, zs, cs, seed=7)
    rng = np.random.default_rng(8)
    pairs = np.stack([rng.integers(0, xs, 200), rng.integers(0, ys, 200), rng.integers(0, zs, 200),
                      rng.integers(0, xs, 200), rng.integers(0, ys, 200), rng.integers(0, zs, 200)], axis=1)
    mm = (float(wide.min()), float(wide.max()))
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(wide)
    engine.upload_secondary_members(sec)
    want = _widened_calls(engine, n, sec, pairs, mm)
    engine.upload_members(narrow)
    assert engine.member_format() == "u16"
    got = _widened_calls(engine, n, sec, pairs, mm)
    assert engine.last_member_format() == "f32"
    for name in want:
        assert_bit_exact(got[name], want[name], f"u16 widened {name}")
    assert tuple(got["minmax"]) == mm
    ref = wide[:, 2, 3, 5].copy()
    assert_bit_exact(got["spearman"], oracle.field(oracle_lib.SPEARMAN, wide, ref), "spearman vs oracle")
    assert_bit_exact(got["kendall"], oracle.field(oracle_lib.KENDALL, wide, ref), "kendall vs oracle")
    assert_close(got["mi_binned"], oracle.field(oracle_lib.MI_BINNED, wide, ref, minmax_ref=mm), "binned vs oracle")
    assert_close(got["kraskov"], oracle.field(oracle_lib.MI_KRASKOV, wide, ref, k=3), "kraskov vs oracle")
    assert_bit_exact(got["symmetric"], oracle.symmetric_field(oracle_lib.PEARSON, wide, sec), "symmetric vs oracle")
    assert_bit_exact(got["mean"], oracle.ensemble_stat(0, wide), "mean vs oracle")
    assert_bit_exact(got["spread"], oracle.ensemble_stat(1, wide), "spread vs oracle")
    assert_bit_exact(got["predicate"], oracle.set_predicate(0, 0.5, 2, 20, wide), "predicate vs oracle")
    assert_close(got["dkl"], oracle.dkl(0, wide), "dkl vs oracle")
    flat = lambda p: (p[:, 2] * ys + p[:, 1]) * xs + p[:, 0]
    assert_bit_exact(got["pairs"], oracle.pair_requests(oracle_lib.PEARSON, wide, flat(pairs[:, :3]), flat(pairs[:, 3:])),
                     "pairs vs oracle")


def test_pearson_beyond_the_native_range(engine, oracle):
    cs, (xs, ys, zs) = 130, (16, 8, 4)
    narrow = cast(box01(xs, ys, zs, cs, seed=9), "u16")
    wide = convert(narrow)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    got = engine.compute(Measure.PEARSON, (5, 3, 2))
    assert engine.last_member_format() == "f32"
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, wide, wide[:, 2, 3, 5].copy()), "u16 cs=130")


# ---- 7. lifetime --------------------------------------------------------------------------------------------------------
def test_lifetime(engine, oracle):
    import torch
    cs, (xs, ys, zs) = 24, (16, 8, 4)
    n = xs * ys * zs
    a, b = cast(box01(xs, ys, zs, cs, seed=10), "u16"), cast(box01(xs, ys, zs, cs, seed=11), "u16")
    members = check_native(engine, oracle, a, (5, 3, 2), "first data")
    spearman_a = engine.compute(Measure.SPEARMAN, (5, 3, 2))  # builds the widened copy
    members.view(torch.int16).copy_(to_device(b).view(torch.int16).reshape(cs, n))  # (same bits; uint16 has few operators)
    torch.cuda.synchronize()
    engine.members_changed()
    wide = convert(b)
    ref = wide[:, 2, 3, 5].copy()
    assert_bit_exact(pearson_device(engine, n, (5, 3, 2)), oracle.field(oracle_lib.PEARSON, wide, ref), "native, new data")
    spearman_b = engine.compute(Measure.SPEARMAN, (5, 3, 2))
    assert_bit_exact(spearman_b, oracle.field(oracle_lib.SPEARMAN, wide, ref), "widened, new data")
    assert not np.array_equal(spearman_a, spearman_b)
    try:
        engine.set_member_layout("packed")
        assert_bit_exact(pearson_device(engine, n, (5, 3, 2)), oracle.field(oracle_lib.PEARSON, wide, ref), "layout packed")
        assert engine.last_member_layout() == "raw" and engine.last_member_format() == "u16"
    finally:
        engine.set_member_layout("auto")
    f32 = torch.from_numpy(wide).cuda()
    engine.bind_members(f32)
    assert engine.member_format() == "f32"
    assert_bit_exact(pearson_device(engine, n, (5, 3, 2)), oracle.field(oracle_lib.PEARSON, wide, ref), "rebound as f32")
    assert engine.last_member_format() == "f32" and engine.last_kernel_name() == "pearson_reg_kernel"


# ---- 8. prepared slots --------------------------------------------------------------------------------------------------
def test_prepared_slots(engine, oracle):
    import torch
    cs, (xs, ys, zs) = 24, (13, 11, 7)
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=12), "f16")
    points = [(1, 2, 3), (12, 10, 6), (6, 0, 4)]
    members = check_native(engine, oracle, narrow, points[0], "plain")
    plain = [pearson_device(engine, n, p) for p in points]
    rows = torch.empty((3, cs), dtype=torch.float32, device="cuda")
    engine.gather_reference_rows_device(points, rows)
    engine.prepare_rows_device(Measure.PEARSON, rows, 4, 3)
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in points]
    engine.compute_prepared_device(Measure.PEARSON, outs, 4)
    torch.cuda.synchronize()
    assert engine.last_member_format() == "f16" and engine.last_kernel_name() == NATIVE_KERNEL
    for p, o, want in zip(points, outs, plain):
        assert_bit_exact(o.cpu().numpy(), want, f"prepared {p}")
    del members


# ---- 9. host output through the range pipeline --------------------------------------------------------------------------
def test_host_output_range_pipeline(engine, oracle):
    cs, (xs, ys, zs) = 8, (160, 128, 103)  # 2 109 440 voxels: a result above 8 MiB, two streams
    narrow = cast(box01(xs, ys, zs, cs, seed=13), "u16")
    wide = convert(narrow)
    ref = wide[:, 50, 64, 80].copy()
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    got = engine.compute(Measure.PEARSON, (80, 64, 50))
    assert engine.last_member_format() == "u16" and engine.last_kernel_name() == NATIVE_KERNEL
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, wide, ref), "ranged native pearson")
    got = engine.compute(Measure.SPEARMAN, (80, 64, 50))
    assert engine.last_member_format() == "f32"
    assert_bit_exact(got, oracle.field(oracle_lib.SPEARMAN, wide, ref), "ranged widened spearman")
    got = engine.compute(Measure.PEARSON, (80, 64, 50))  # back to the native tables
    assert engine.last_member_format() == "u16"
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, wide, ref), "ranged native pearson again")


# ---- 10. errors ---------------------------------------------------------------------------------------------------------
def test_unknown_format_is_an_argument_error(engine):
    engine.set_grid(4, 4, 4, 3)
    ptrs = (C.c_void_p * 3)(1, 1, 1)
    assert engine._lib.crf_upload_members_format(engine._ctx, 7, ptrs) == 1       # CRF_ERR_ARGUMENT
    assert engine._lib.crf_bind_members_device_format(engine._ctx, -1, ptrs) == 1
    assert b"unknown member format" in engine._lib.crf_last_error(engine._ctx)


def test_unsupported_dtype_raises(engine):
    engine.set_grid(4, 4, 4, 3)
    import torch
    with pytest.raises(TypeError):
        engine.bind_members(torch.zeros((3, 64), dtype=torch.float64, device="cuda"))


def test_group_over_narrow_members_is_unsupported():
    import torch
    import correrender_amd as ca
    try:
        group = ca.CorrFieldGroup([0, 0])
    except CorrFieldError as e:
        pytest.skip(f"no device group on this machine: {e}")
    with group:
        cs, (xs, ys, zs) = 8, (8, 8, 4)
        group.set_grid(xs, ys, zs, cs)
        narrow = cast(box01(xs, ys, zs, cs, seed=14), "u16")
        group.upload_members(convert(narrow))
        lib = group._lib
        keep = []
        for slot in range(2):
            z0, zn = group.slab(slot)
            slab = to_device(np.ascontiguousarray(narrow[:, z0:z0 + zn]))
            keep.append(slab)
            ptrs = (C.c_void_p * cs)(*[slab[c].data_ptr() for c in range(cs)])
            assert lib.crf_bind_members_device_format(lib.crf_group_context(group._g, slot), 2, ptrs) == 0
        with pytest.raises(CorrFieldError) as err:
            group.compute(Measure.PEARSON, (1, 2, 3))
        assert err.value.code == 4  # CRF_ERR_UNSUPPORTED
        assert "fp32 members only" in err.value.message
