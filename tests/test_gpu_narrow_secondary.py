"""GPU: secondary members in the narrow native formats (uint8, uint16, float16), and the symmetric Pearson field that reads
two narrow fields as stored (pearson_symmetric_narrow_kernel).  The definition of correct, as for the primary members: every
result equals the result of the same call on float32 members that hold the converted values -- b / 255, s / 65535, float(h)
-- bit for bit, and the oracle's on those values."""
import ctypes as C

import numpy as np
import pytest

from correrender_amd import CorrFieldError, Measure, synth
from parity import assert_bit_exact
import oracle_lib

pytestmark = pytest.mark.gpu

FORMATS = ["u8", "u16", "f16"]
NATIVE_KERNEL = "pearson_symmetric_narrow_kernel"
FP32_KERNEL = "pearson_symmetric_kernel"
FORMAT_IDS = {"f32": 0, "u8": 1, "u16": 2, "f16": 3}
# mirror of symmetric_narrow_routed (csrc/symmetric_narrow_route.h): every format at 2..64 members; at 65..128 members the
# N = cs rounded up to 16 that profiles/narrow_symmetric_ab.md measured no slower than the copy route
ROUTED_ABOVE_64 = {"u8": {80, 96, 112, 128}, "u16": {80, 96, 112, 128}, "f16": {80, 96, 112, 128}}


def routed(fmt, cs):
    if fmt not in FORMATS or cs < 2 or cs > 128:
        return False
    return cs <= 64 or (cs + 15) // 16 * 16 in ROUTED_ABOVE_64[fmt]


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


def unaligned_device_members(narrow: np.ndarray):
    """`narrow` on the device as cs borrowed rows that start one element behind a 4-byte boundary."""
    cs, n = narrow.shape[0], narrow[0].size
    rows = np.zeros((cs, n + 7), narrow.dtype)
    rows[:, 1:n + 1] = narrow.reshape(cs, n)
    pad = (-rows.shape[1] * rows.itemsize) % 4 // rows.itemsize  # row stride in whole dwords
    rows = np.concatenate([rows, np.zeros((cs, pad), narrow.dtype)], axis=1)
    buf = to_device(rows)
    members = [buf[c, 1:n + 1] for c in range(cs)]
    assert all(m.data_ptr() % 4 != 0 for m in members)
    return buf, members


def fmt_of(a: np.ndarray) -> str:
    return {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16",
            np.dtype(np.float32): "f32"}[a.dtype]


def wide_of(a: np.ndarray) -> np.ndarray:
    return a if a.dtype == np.float32 else convert(a)


def symmetric_device(eng, n, measure=Measure.PEARSON, out=None, **kw):
    import torch
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device="cuda")
    eng.compute_device(measure, out, symmetric=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def upload_two(eng, a, b):
    cs, zs, ys, xs = a.shape
    eng.set_grid(xs, ys, zs, cs)
    eng.upload_members(a)
    eng.upload_secondary_members(b)
    assert eng.member_format() == fmt_of(a) and eng.secondary_member_format() == fmt_of(b)


def check_native(eng, oracle, a, b, what, out=None, expect_native=True):
    """Uploads two narrow fields ([cs, zs, ys, xs]) and checks the symmetric Pearson field against the oracle."""
    upload_two(eng, a, b)
    got = symmetric_device(eng, a[0].size, out=out)
    if expect_native:
        assert eng.last_kernel_name() == NATIVE_KERNEL, what
        assert eng.last_member_format() == fmt_of(a), what
        assert eng.wide_copy_bytes() == 0 and eng.secondary_wide_copy_bytes() == 0, what
    else:
        assert eng.last_kernel_name() == FP32_KERNEL, what
        assert eng.last_member_format() == "f32", what
    with np.errstate(all="ignore"):
        want = oracle.symmetric_field(oracle_lib.PEARSON, convert(a), convert(b))
    assert_bit_exact(got, want, what)
    return got


# ---- 1. member counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [2, 7, 8, 9, 16, 17, 33, 48, 64])
@pytest.mark.parametrize("fmt", FORMATS)
def test_member_counts_native(engine, oracle, fmt, cs):
    # 13*11*7 = 1001 voxels, 1001 % 4 = 1: whole blocks, a partial block, a ragged dword
    a, b = cast(box01(13, 11, 7, cs, seed=cs), fmt), cast(box01(13, 11, 7, cs, seed=1000 + cs), fmt)
    check_native(engine, oracle, a, b, f"{fmt} cs={cs}")


@pytest.mark.parametrize("cs", [65, 100, 112, 128])
@pytest.mark.parametrize("fmt", FORMATS)
def test_member_counts_above_64_follow_the_routing_table(engine, oracle, fmt, cs):
    a, b = cast(box01(13, 11, 7, cs, seed=cs), fmt), cast(box01(13, 11, 7, cs, seed=1000 + cs), fmt)
    check_native(engine, oracle, a, b, f"{fmt} cs={cs}", expect_native=routed(fmt, cs))


# ---- 2. ragged ends -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(3, 1, 1), (2, 3, 1), (7, 5, 3), (255, 1, 1), (256, 1, 1), (257, 1, 1)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ragged_ends(engine, oracle, fmt, grid):
    xs, ys, zs = grid
    a, b = cast(box01(xs, ys, zs, 24, seed=xs), fmt), cast(box01(xs, ys, zs, 24, seed=100 + xs), fmt)
    check_native(engine, oracle, a, b, f"{fmt} grid={grid}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_output_aligned_to_four_bytes_only(engine, oracle, fmt):
    import torch
    n = 7 * 5 * 3
    out = torch.empty(n + 1, dtype=torch.float32, device="cuda")[1:]
    assert out.data_ptr() % 8 == 4
    a, b = cast(box01(7, 5, 3, 24, seed=2), fmt), cast(box01(7, 5, 3, 24, seed=3), fmt)
    check_native(engine, oracle, a, b, f"{fmt} out + 4 B", out=out)


# ---- 3. division branches -----------------------------------------------------------------------------------------------
def test_division_branches(engine, oracle):
    """One lane owns 4 uint8 voxels, so a wave covers 256: voxels [0, 256) and [768, 1024) are ordinary (the exact_div
    branch), wave 1 holds ONE voxel that is constant in X among ordinary ones, wave 2 voxels constant in X, in Y and in
    both (sd = 0: the plain divisions give NaN or inf as the fp32 kernel does)."""
    cs, n = 24, 1024
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, (cs, 1, 1, n)).astype(np.uint8)
    b = rng.integers(0, 256, (cs, 1, 1, n)).astype(np.uint8)
    a[:, 0, 0, 300] = 17
    a[:, 0, 0, 520:530] = 200
    b[:, 0, 0, 540:550] = 3
    a[:, 0, 0, 560:563] = 0
    b[:, 0, 0, 560:563] = 255
    got = check_native(engine, oracle, a, b, "u8 division branches")
    assert np.isfinite(got[:256]).all() and np.isfinite(got[768:]).all()
    assert not np.isfinite(got[300]) and not np.isfinite(got[520:530]).any() and not np.isfinite(got[560:563]).any()
    assert np.isfinite(got[256:300]).all() and np.isfinite(got[301:512]).all()


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
    codes, count = _every_code(which)
    assert np.unique(codes.view(np.uint8 if codes.dtype == np.uint8 else np.uint16)).size == count
    cs, n = codes.shape
    primary = cast(box01(n, 1, 1, cs, seed=5), fmt_of(codes))
    check_native(engine, oracle, primary, codes.reshape(cs, 1, 1, n), f"every code {which}")


def _f16_specials(cs, n, seed):
    narrow = cast(box01(n, 1, 1, cs, seed=seed), "f16").reshape(cs, n)
    narrow[3, 10] = np.float16(0.0)
    narrow[4, 10] = np.float16(-0.0)
    narrow[5, 11:14] = np.array([0x0001, 0x8001, 0x03FF], np.uint16).view(np.float16)  # denormals
    narrow[:, 20] = np.array([0x0001 + e for e in range(cs)], np.uint16).view(np.float16)  # a voxel of denormals only
    narrow[6, 30] = np.float16(np.inf)
    narrow[7, 31] = np.float16(-np.inf)
    narrow[8, 32] = np.float16(np.nan)
    narrow[9, 33] = np.float16(np.inf)
    narrow[10, 33] = np.float16(-np.inf)
    return narrow.reshape(cs, 1, 1, n)


def test_f16_special_values_on_either_side(engine, oracle):
    cs, n = 24, 300
    special, plain = _f16_specials(cs, n, seed=5), cast(box01(n, 1, 1, cs, seed=6), "f16")
    check_native(engine, oracle, special, plain, "f16 specials in the primary field")
    check_native(engine, oracle, plain, special, "f16 specials in the secondary field")
    check_native(engine, oracle, special, _f16_specials(cs, n, seed=7), "f16 specials in both fields")


# ---- 5. fallbacks -------------------------------------------------------------------------------------------------------
def check_fallback(eng, oracle, a, b, what, measure=Measure.PEARSON, omeasure=oracle_lib.PEARSON, kernel=FP32_KERNEL, **kw):
    """Symmetric `measure` on fields a, b (already on the context) ran on fp32 views: the copies exist on the narrow sides
    only, and the result is that of the same call on fp32 members holding the converted values, and the oracle's."""
    n = a[0].size
    got = symmetric_device(eng, n, measure, **kw)
    assert eng.last_member_format() == "f32", what
    if kernel:
        assert eng.last_kernel_name() == kernel, what
    assert (eng.wide_copy_bytes() > 0) == (a.dtype != np.float32), what
    assert (eng.secondary_wide_copy_bytes() > 0) == (b.dtype != np.float32), what
    wa, wb = wide_of(a), wide_of(b)
    if omeasure is not None:
        assert_bit_exact(got, oracle.symmetric_field(omeasure, wa, wb), f"{what} vs oracle")
    upload_two(eng, wa, wb)
    assert_bit_exact(got, symmetric_device(eng, n, measure, **kw), f"{what} vs fp32 members")


def test_fallback_mixed_formats(engine, oracle):
    a, b = cast(box01(13, 11, 7, 24, seed=40), "u8"), cast(box01(13, 11, 7, 24, seed=41), "u16")
    upload_two(engine, a, b)
    check_fallback(engine, oracle, a, b, "u8 primary, u16 secondary")


@pytest.mark.parametrize("fmt", FORMATS)
def test_fallback_fp32_primary(engine, oracle, fmt):
    a, b = box01(13, 11, 7, 24, seed=42), cast(box01(13, 11, 7, 24, seed=43), fmt)
    upload_two(engine, a, b)
    check_fallback(engine, oracle, a, b, f"fp32 primary, {fmt} secondary")


@pytest.mark.parametrize("fmt", ["u8", "u16"])
def test_fallback_unaligned_borrowed_secondary(engine, oracle, fmt):
    cs, (xs, ys, zs) = 24, (7, 5, 3)
    a, b = cast(box01(xs, ys, zs, cs, seed=44), fmt), cast(box01(xs, ys, zs, cs, seed=45), fmt)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(a)
    buf, members = unaligned_device_members(b)
    engine.bind_secondary_members(members)
    assert engine.secondary_member_format() == fmt
    check_fallback(engine, oracle, a, b, f"{fmt} secondary one element behind a dword")
    del buf


def test_fallback_beyond_the_native_range(engine, oracle):
    a, b = cast(box01(16, 8, 4, 130, seed=46), "u16"), cast(box01(16, 8, 4, 130, seed=47), "u16")
    upload_two(engine, a, b)
    check_fallback(engine, oracle, a, b, "u16 cs=130", kernel="pair_request_kernel")


@pytest.mark.parametrize("measure,omeasure", [(Measure.SPEARMAN, oracle_lib.SPEARMAN), (Measure.KENDALL, oracle_lib.KENDALL),
                                              (Measure.MUTUAL_INFORMATION_BINNED, None)])
def test_fallback_other_measures(engine, oracle, measure, omeasure):
    a, b = cast(box01(13, 11, 7, 24, seed=48), "u16"), cast(box01(13, 11, 7, 24, seed=49), "u16")
    upload_two(engine, a, b)
    kw = dict(num_bins=20) if omeasure is None else {}
    check_fallback(engine, oracle, a, b, f"u16 symmetric {measure.name}", measure, omeasure, kernel="sorted_symmetric_kernel",
                   **kw)


@pytest.mark.parametrize("fmt", FORMATS)
def test_fallback_pair_requests_from_a_narrow_secondary(engine, oracle, fmt):
    cs, (xs, ys, zs) = 24, (16, 8, 4)
    a, b = cast(box01(xs, ys, zs, cs, seed=50), fmt), cast(box01(xs, ys, zs, cs, seed=51), fmt)
    rng = np.random.default_rng(52)
    pairs = np.stack([rng.integers(0, xs, 200), rng.integers(0, ys, 200), rng.integers(0, zs, 200),
                      rng.integers(0, xs, 200), rng.integers(0, ys, 200), rng.integers(0, zs, 200)], axis=1)
    upload_two(engine, a, b)
    got = engine.compute_requests(Measure.PEARSON, pairs, query_from_secondary=True)
    assert engine.wide_copy_bytes() > 0 and engine.secondary_wide_copy_bytes() > 0
    wa, wb = convert(a), convert(b)
    flat = lambda p: (p[:, 2] * ys + p[:, 1]) * xs + p[:, 0]
    i, j = flat(pairs[:, :3]), flat(pairs[:, 3:])
    want = np.array([oracle.pearson(wa.reshape(cs, -1)[:, p].copy(), wb.reshape(cs, -1)[:, q].copy()) for p, q in zip(i, j)],
                    np.float32)
    assert_bit_exact(got, want, f"{fmt} pair requests vs oracle")
    upload_two(engine, wa, wb)
    assert_bit_exact(got, engine.compute_requests(Measure.PEARSON, pairs, query_from_secondary=True),
                     f"{fmt} pair requests vs fp32 members")


def test_fallback_windowed_grid(engine, oracle, monkeypatch):
    cs, (xs, ys, zs) = 24, (13, 11, 17)  # 2431 voxels under a window of 1024: three windows
    a, b = cast(box01(xs, ys, zs, cs, seed=53), "u16"), cast(box01(xs, ys, zs, cs, seed=54), "u16")
    with monkeypatch.context() as m:
        m.setenv("CRF_WINDOW_VOXELS", "1024")
        engine.set_grid(xs, ys, zs, cs)
    try:
        assert engine.window_count() == 3
        engine.upload_members(a)
        engine.upload_secondary_members(b)
        got = symmetric_device(engine, xs * ys * zs)
        assert engine.last_member_format() == "f32" and engine.last_kernel_name() == FP32_KERNEL
        assert engine.wide_copy_bytes() > 0 and engine.secondary_wide_copy_bytes() > 0
        assert_bit_exact(got, oracle.symmetric_field(oracle_lib.PEARSON, convert(a), convert(b)), "windowed u16")
    finally:
        engine.set_grid(xs, ys, zs, cs)  # (the variable is back: an ordinary grid again)
    assert engine.window_count() == 1


# ---- 6. reference from a narrow secondary -------------------------------------------------------------------------------
def _separate_calls(eng):
    res = {}
    for measure in Measure:
        res[measure.name] = eng.compute(measure, (5, 3, 2), reference_from_secondary=True, k=3, num_bins=20).ravel()
    res["minmax"] = np.array(eng.secondary_member_minmax(), np.float32)
    return res


@pytest.mark.parametrize("primary", ["f32", "u16"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_reference_from_a_narrow_secondary(engine, oracle, fmt, primary):
    cs, (xs, ys, zs) = 24, (16, 8, 4)
    a01 = box01(xs, ys, zs, cs, seed=60)
    a = a01 if primary == "f32" else cast(a01, primary)
    b = cast(box01(xs, ys, zs, cs, seed=61), fmt)
    wb = convert(b)
    upload_two(engine, a, wb)
    want = _separate_calls(engine)
    engine.upload_secondary_members(b)
    assert engine.secondary_member_format() == fmt
    got = _separate_calls(engine)
    assert engine.secondary_wide_copy_bytes() == 0
    for name in want:
        assert_bit_exact(got[name], want[name], f"{fmt} secondary, {primary} primary: {name}")
    assert tuple(got["minmax"]) == (wb.min(), wb.max())
    wa = wide_of(a)
    assert_bit_exact(got["PEARSON"], oracle.field(oracle_lib.PEARSON, wa, wb[:, 2, 3, 5].copy()), "pearson vs oracle")
    assert_bit_exact(got["KENDALL"], oracle.field(oracle_lib.KENDALL, wa, wb[:, 2, 3, 5].copy()), "kendall vs oracle")
    if primary != "f32":  # the native routes of the narrow primary members keep serving such an evaluation
        engine.compute(Measure.PEARSON, (5, 3, 2), reference_from_secondary=True)
        assert engine.last_member_format() == primary and engine.last_kernel_name() == "pearson_narrow_kernel"


@pytest.mark.parametrize("fmt", ["u8", "u16"])
def test_reference_from_an_unaligned_narrow_secondary(engine, oracle, fmt):
    cs, (xs, ys, zs) = 24, (7, 5, 3)
    a, b = box01(xs, ys, zs, cs, seed=62), cast(box01(xs, ys, zs, cs, seed=63), fmt)
    wb = convert(b)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(a)
    buf, members = unaligned_device_members(b)
    engine.bind_secondary_members(members)
    got = engine.compute(Measure.PEARSON, (3, 2, 1), reference_from_secondary=True)
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, a, wb[:, 1, 2, 3].copy()), f"{fmt} offset 1")
    assert engine.secondary_member_minmax() == (wb.min(), wb.max())
    assert engine.secondary_wide_copy_bytes() == 0
    del buf


# ---- 7. lifetime --------------------------------------------------------------------------------------------------------
def test_lifetime(engine, oracle):
    import torch
    cs, (xs, ys, zs) = 24, (16, 8, 4)
    n = xs * ys * zs
    a = cast(box01(xs, ys, zs, cs, seed=70), "u16")
    b0, b1 = cast(box01(xs, ys, zs, cs, seed=71), "u16"), cast(box01(xs, ys, zs, cs, seed=72), "u16")
    wa = convert(a)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(a)
    members = to_device_members(b0)
    engine.bind_secondary_members(members)
    assert engine.secondary_member_format() == "u16"
    spearman_0 = symmetric_device(engine, n, Measure.SPEARMAN)  # builds both copies
    assert engine.secondary_wide_copy_bytes() >= 4 * cs * n
    assert_bit_exact(spearman_0, oracle.symmetric_field(oracle_lib.SPEARMAN, wa, convert(b0)), "widened, first data")
    members.view(torch.int16).copy_(to_device(b1).view(torch.int16).reshape(cs, n))  # (same bits; uint16 has few operators)
    torch.cuda.synchronize()
    engine.members_changed()
    assert engine.secondary_wide_copy_bytes() == 0 and engine.wide_copy_bytes() == 0
    wb = convert(b1)
    got = symmetric_device(engine, n)
    assert engine.last_kernel_name() == NATIVE_KERNEL and engine.secondary_wide_copy_bytes() == 0
    assert_bit_exact(got, oracle.symmetric_field(oracle_lib.PEARSON, wa, wb), "native, new data")
    spearman_1 = symmetric_device(engine, n, Measure.SPEARMAN)
    assert_bit_exact(spearman_1, oracle.symmetric_field(oracle_lib.SPEARMAN, wa, wb), "widened, new data")
    assert not np.array_equal(spearman_0, spearman_1)
    assert engine.secondary_wide_copy_bytes() > 0
    engine.upload_secondary_members(wb)
    assert engine.secondary_member_format() == "f32" and engine.secondary_wide_copy_bytes() == 0
    got = symmetric_device(engine, n)
    assert engine.last_kernel_name() == FP32_KERNEL and engine.last_member_format() == "f32"
    assert_bit_exact(got, oracle.symmetric_field(oracle_lib.PEARSON, wa, wb), "secondary uploaded again as fp32")
    engine.upload_secondary_members(b1)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(a)
    assert engine.secondary_member_format() == "f32" and engine.secondary_wide_copy_bytes() == 0
    with pytest.raises(CorrFieldError) as err:
        engine.compute(Measure.PEARSON, symmetric=True)
    assert err.value.code == 2  # CRF_ERR_STATE: the secondary members went with the grid
    with pytest.raises(CorrFieldError) as err:
        engine.secondary_member_minmax()
    assert err.value.code == 2


# ---- 8. errors ----------------------------------------------------------------------------------------------------------
def test_unknown_format_is_an_argument_error(engine):
    engine.set_grid(4, 4, 4, 3)
    ptrs = (C.c_void_p * 3)(1, 1, 1)
    assert engine._lib.crf_upload_secondary_members_format(engine._ctx, 7, ptrs) == 1       # CRF_ERR_ARGUMENT
    assert b"unknown member format" in engine._lib.crf_last_error(engine._ctx)
    assert engine._lib.crf_bind_secondary_members_device_format(engine._ctx, -1, ptrs) == 1
    assert b"unknown member format" in engine._lib.crf_last_error(engine._ctx)


def test_unsupported_dtype_raises(engine):
    engine.set_grid(4, 4, 4, 3)
    import torch
    with pytest.raises(TypeError):
        engine.bind_secondary_members(torch.zeros((3, 64), dtype=torch.float64, device="cuda"))


def test_group_over_narrow_secondary_members_is_unsupported():
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
        group.upload_secondary_members(convert(narrow))
        lib = group._lib
        keep = []
        for slot in range(2):
            z0, zn = group.slab(slot)
            slab = to_device(np.ascontiguousarray(narrow[:, z0:z0 + zn]))
            keep.append(slab)
            ptrs = (C.c_void_p * cs)(*[slab[c].data_ptr() for c in range(cs)])
            ctx = lib.crf_group_context(group._g, slot)
            assert lib.crf_bind_secondary_members_device_format(ctx, FORMAT_IDS["u16"], ptrs) == 0
            assert lib.crf_secondary_member_format(ctx) == FORMAT_IDS["u16"]
        with pytest.raises(CorrFieldError) as err:
            group.compute(Measure.PEARSON, (1, 2, 3), reference_from_secondary=True)
        assert err.value.code == 4  # CRF_ERR_UNSUPPORTED
        assert "fp32 members only" in err.value.message
