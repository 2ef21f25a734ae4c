"""GPU: the entry points that read members in a narrow native format (uint8, uint16, float16) as they are stored -- the
ensemble mean and spread, the set predicate, the extrema and the reference gathers.  The definition of correct is the one
of test_gpu_member_formats.py: every result equals the result of the same call on float32 members that hold the
converted values, bit for bit.  On top of that: the native kernels ran (last_kernel_name) and no fp32 copy of the
ensemble exists afterwards (wide_copy_bytes)."""
import numpy as np
import pytest

from correrender_amd import Measure
from parity import assert_bit_exact
import oracle_lib
from test_gpu_member_formats import (FORMATS, _every_code, box01, cast, convert, pearson_device, to_device,
                                     to_device_members)

pytestmark = pytest.mark.gpu

STAT_KERNEL = "ensemble_stat_narrow_kernel"
PREDICATE_KERNEL = "set_predicate_narrow_kernel"
FP32_STAT_KERNELS = ("ensemble_stat_stream_kernel", "ensemble_stat_reg_kernel")
OPERATORS = (">", ">=", "<", "<=", "==", "!=")


def between_two_codes(narrow):
    """A float32 strictly between the converted values of two neighbouring codes near the middle of the range."""
    if narrow.dtype == np.uint8:
        lo, hi = np.array([100, 101], np.uint8)
    elif narrow.dtype == np.uint16:
        lo, hi = np.array([30000, 30001], np.uint16)
    else:
        lo = np.float16(0.5)
        hi = np.nextafter(lo, np.float16(1))
    a, b = convert(np.array([lo, hi]))
    mid = np.float32((np.float64(a) + np.float64(b)) / 2)
    assert a < mid < b
    return float(mid)


def bits(value):
    return int(np.array([value], np.float32).view(np.uint32)[0])


def check_reductions(eng, oracle, narrow, what, counts=None):
    """The native mean, spread and set predicate of the members bound right now against the oracle on the converted
    values; after each call the narrow kernel has run and no fp32 copy exists."""
    cs = narrow.shape[0]
    wide = convert(narrow)

    def native(kernel):
        assert eng.last_kernel_name() == kernel, what
        assert eng.wide_copy_bytes() == 0, what

    with np.errstate(all="ignore"):
        assert_bit_exact(eng.ensemble_stat(0), oracle.ensemble_stat(0, wide), f"{what} mean")
        native(STAT_KERNEL)
        assert_bit_exact(eng.ensemble_stat(1), oracle.ensemble_stat(1, wide), f"{what} spread")
        native(STAT_KERNEL)
        occurring = float(wide.reshape(cs, -1)[cs // 2, wide[0].size // 3])  # the exact value of a code that occurs
        for lower, upper in counts or [(cs // 4, cs // 4 + max(1, cs // 2)), (cs // 2, cs // 2)]:
            for op, value in ((">", between_two_codes(narrow)), ("==", occurring)):
                got = eng.set_predicate(op, value, lower, upper)
                native(PREDICATE_KERNEL)
                want = oracle.set_predicate(OPERATORS.index(op), value, lower, upper, wide)
                assert_bit_exact(got, want, f"{what} predicate {op} {value!r} counts {lower}..{upper}")
                if op == "==":
                    assert (oracle.set_predicate(4, value, 0, 0, wide) > 0).any()  # the value does occur


def upload(eng, narrow):
    cs, zs, ys, xs = narrow.shape
    eng.set_grid(xs, ys, zs, cs)
    eng.upload_members(narrow)
    assert eng.wide_copy_bytes() == 0


# ---- 1. member counts x formats -----------------------------------------------------------------------------------------
# 16 | 17, 64 | 65: two 16-slot granules of the register-resident spread; 128 | 129: its end, the streaming spread beyond
@pytest.mark.parametrize("cs", [1, 2, 16, 17, 64, 65, 128, 129, 200])
@pytest.mark.parametrize("fmt", FORMATS)
def test_member_counts(engine, oracle, fmt, cs):
    # 13*11*7 = 1001 voxels, 1001 % 4 = 1: a ragged dword, whole blocks and a partial one
    narrow = cast(box01(13, 11, 7, max(cs, 2), seed=cs)[:cs], fmt)
    upload(engine, narrow)
    check_reductions(engine, oracle, narrow, f"{fmt} cs={cs}")


# ---- 2. ragged ends -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(3, 1, 1), (2, 3, 1), (7, 5, 3), (255, 1, 1), (256, 1, 1), (257, 1, 1), (1023, 1, 1),
                                  (1025, 1, 1)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ragged_ends(engine, oracle, fmt, grid):
    xs, ys, zs = grid
    narrow = cast(box01(xs, ys, zs, 24, seed=xs), fmt)
    upload(engine, narrow)
    check_reductions(engine, oracle, narrow, f"{fmt} grid={grid}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_output_aligned_to_four_bytes_only(engine, oracle, fmt):
    import torch
    narrow = cast(box01(7, 5, 3, 24, seed=2), fmt)
    wide = convert(narrow)
    upload(engine, narrow)
    n = 7 * 5 * 3
    out = torch.empty(n + 1, dtype=torch.float32, device="cuda")[1:]
    assert out.data_ptr() % 8 == 4
    for stat in (0, 1):
        engine.ensemble_stat_device(stat, out)
        torch.cuda.synchronize()
        assert engine.last_kernel_name() == STAT_KERNEL
        assert_bit_exact(out.cpu().numpy(), oracle.ensemble_stat(stat, wide), f"{fmt} stat {stat} out + 4 B")
    value = between_two_codes(narrow)
    engine.set_predicate_device(">", value, 2, 20, out)
    torch.cuda.synchronize()
    assert engine.last_kernel_name() == PREDICATE_KERNEL and engine.wide_copy_bytes() == 0
    assert_bit_exact(out.cpu().numpy(), oracle.set_predicate(0, value, 2, 20, wide), f"{fmt} predicate out + 4 B")


# ---- 3. f16 special values ----------------------------------------------------------------------------------------------
def _f16_specials():
    cs, n = 24, 300
    narrow = cast(box01(n, 1, 1, cs, seed=5), "f16").reshape(cs, n)
    nan, inf = np.float16(np.nan), np.float16(np.inf)
    narrow[[2, 8, 23], 40] = nan            # a NaN in some members of a voxel (first, middle and last dword slots)
    narrow[:, 41] = nan
    narrow[13, 41] = np.float16(0.375)      # exactly one valid member: mean = that value, spread NaN
    narrow[:, 42] = nan                     # no valid member: both NaN
    narrow[:, 43] = nan
    narrow[[0, 23], 43] = np.array([0.25, 0.75], np.float16)  # exactly two valid members
    narrow[6, 50] = inf
    narrow[7, 51] = -inf
    narrow[9, 52] = inf
    narrow[10, 52] = -inf                   # inf and -inf together
    narrow[5, 60:63] = np.array([0x0001, 0x8001, 0x03FF], np.uint16).view(np.float16)  # denormals
    narrow[:, 64] = np.array([0x0001 + e for e in range(cs)], np.uint16).view(np.float16)  # a voxel of denormals only
    narrow[:, 70] = np.float16(0.0)
    narrow[::2, 70] = np.float16(-0.0)      # +0 and -0 only
    narrow[3, 71] = np.float16(0.0)
    narrow[4, 71] = np.float16(-0.0)
    return narrow.reshape(cs, 1, 1, n)


def test_f16_special_values(engine, oracle):
    narrow = _f16_specials()
    wide = convert(narrow)
    upload(engine, narrow)
    check_reductions(engine, oracle, narrow, "f16 specials")
    with np.errstate(all="ignore"):
        mean, spread = engine.ensemble_stat(0).ravel(), engine.ensemble_stat(1).ravel()
        assert bits(mean[41]) == bits(0.375) and np.isnan(spread[41])
        assert np.isnan(mean[42]) and np.isnan(spread[42])
        assert np.isnan(mean[52]) and np.isinf(mean[50]) and np.isinf(mean[51])
        for value in (0.0, float("nan")):  # against the voxels that hold NaNs, infinities and both zeros
            for op in range(6):
                for lower, upper in ((2, 20), (12, 12)):
                    got = engine.set_predicate(op, value, lower, upper)
                    assert engine.last_kernel_name() == PREDICATE_KERNEL and engine.wide_copy_bytes() == 0
                    assert_bit_exact(got, oracle.set_predicate(op, value, lower, upper, wide),
                                     f"f16 specials {OPERATORS[op]} {value} counts {lower}..{upper}")


def _extrema_both_ways(eng, narrow):
    """member_minmax of `narrow` read natively, and of the converted values uploaded as fp32 to the same context."""
    upload(eng, narrow)
    native = eng.member_minmax()
    assert eng.wide_copy_bytes() == 0
    eng.upload_members(convert(narrow))
    assert eng.member_format() == "f32"
    return native, eng.member_minmax()


def test_f16_extrema_of_signed_zeros_and_nan_members(engine):
    cs, n = 8, 777
    narrow = cast(box01(n, 1, 1, cs, seed=6), "f16")
    narrow[narrow == 0] = np.float16(0.25)
    narrow[2, 0, 0, 500] = np.float16(0.0)
    narrow[5, 0, 0, 13] = np.float16(-0.0)   # the minimum is -0, with +0 present
    native, fp32 = _extrema_both_ways(engine, narrow)
    assert [bits(v) for v in native] == [bits(v) for v in fp32]
    assert bits(native[0]) == 0x80000000 and native[1] == float(convert(narrow).max())
    narrow[3] = np.float16(np.nan)           # a member of NaNs only
    narrow[6, 0, 0, 100:140] = np.float16(np.nan)
    native, fp32 = _extrema_both_ways(engine, narrow)
    assert [bits(v) for v in native] == [bits(v) for v in fp32]
    wide = convert(narrow)
    assert native[1] == float(np.nanmax(wide)) and native[0] == 0.0
    narrow[:] = np.float16(np.nan)           # nothing but NaNs: whatever the fp32 kernel leaves
    native, fp32 = _extrema_both_ways(engine, narrow)
    assert np.isnan(native).tolist() == np.isnan(fp32).tolist()


# ---- 4. every code ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["u16a", "u16b", "f16", "u8"])
def test_every_code(engine, oracle, which):
    narrow, count = _every_code(which)
    cs, n = narrow.shape
    wide = convert(narrow)
    upload(engine, narrow.reshape(cs, 1, 1, n))
    with np.errstate(all="ignore"):
        assert_bit_exact(engine.ensemble_stat(0), oracle.ensemble_stat(0, wide), f"every code {which} mean")
        assert engine.last_kernel_name() == STAT_KERNEL
        assert_bit_exact(engine.ensemble_stat(1), oracle.ensemble_stat(1, wide), f"every code {which} spread")
        assert engine.last_kernel_name() == STAT_KERNEL
    mn, mx = engine.member_minmax()
    assert (bits(mn), bits(mx)) == (bits(np.nanmin(wide)), bits(np.nanmax(wide))), f"every code {which} extrema"
    got = np.stack([engine.gather_reference(x, 0, 0) for x in range(n)], axis=1)
    assert (got.view(np.uint32) == wide.view(np.uint32)).all(), f"every code {which} gathers"
    assert engine.wide_copy_bytes() == 0


# ---- 5. gathers build nothing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_gathers_build_no_copy(engine, oracle, fmt):
    import torch
    cs, (xs, ys, zs) = 24, (13, 11, 7)
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=12), fmt)
    wide = convert(narrow)
    upload(engine, narrow)
    same = lambda got, want: (np.asarray(got, np.float32).view(np.uint32) == want.view(np.uint32)).all()
    points = [(1, 2, 3), (12, 10, 6), (6, 0, 4)]
    for x, y, z in points:
        assert same(engine.gather_reference(x, y, z), wide[:, z, y, x])
        one = torch.empty(cs, dtype=torch.float32, device="cuda")
        engine.gather_reference_device(x, y, z, one)
        torch.cuda.synchronize()
        assert same(one.cpu().numpy(), wide[:, z, y, x])
    rows = torch.full((3, cs), -1.0, dtype=torch.float32, device="cuda")
    engine.gather_reference_rows_device(points, rows)
    torch.cuda.synchronize()
    assert same(rows.cpu().numpy(), np.stack([wide[:, z, y, x] for x, y, z in points]))
    # the 32-row maximum; every third row belongs to somebody else (z < 0) and comes back as zeros
    rng = np.random.default_rng(7)
    many = [None if r % 3 == 1 else (int(rng.integers(xs)), int(rng.integers(ys)), int(rng.integers(zs))) for r in range(32)]
    rows32 = torch.full((32, cs), -1.0, dtype=torch.float32, device="cuda")
    engine.gather_reference_rows_device(many, rows32)
    torch.cuda.synchronize()
    want = np.stack([np.zeros(cs, np.float32) if p is None else wide[:, p[2], p[1], p[0]] for p in many])
    assert same(rows32.cpu().numpy(), want)
    assert engine.wide_copy_bytes() == 0
    # the flow of test_gpu_member_formats.py::test_prepared_slots: an all-native pipeline allocates no copy
    plain = [pearson_device(engine, n, p) for p in points]
    engine.gather_reference_rows_device(points, rows)
    engine.prepare_rows_device(Measure.PEARSON, rows, 4, 3)
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in points]
    engine.compute_prepared_device(Measure.PEARSON, outs, 4)
    torch.cuda.synchronize()
    assert engine.wide_copy_bytes() == 0 and engine.last_member_format() == fmt
    for p, o, w in zip(points, outs, plain):
        assert_bit_exact(o.cpu().numpy(), w, f"prepared {p}")
        assert_bit_exact(w, oracle.field(oracle_lib.PEARSON, wide, wide[:, p[2], p[1], p[0]].copy()), f"plain {p}")


# ---- 6. the copy still appears and disappears where it should -----------------------------------------------------------
def test_copy_lifetime(engine, oracle):
    import torch
    cs, (xs, ys, zs) = 24, (16, 8, 4)
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=10), "u16")
    wide = convert(narrow)
    members = to_device_members(narrow)
    engine.set_grid(xs, ys, zs, cs)
    engine.bind_members(members)
    check_reductions(engine, oracle, narrow, "before the copy")
    engine.member_minmax()
    engine.gather_reference(5, 3, 2)
    pearson_device(engine, n, (5, 3, 2))
    assert engine.wide_copy_bytes() == 0                              # after the native calls
    engine.compute(Measure.SPEARMAN, (5, 3, 2))
    assert engine.last_member_format() == "f32"
    assert engine.wide_copy_bytes() >= cs * n * 4                     # after a Spearman field
    assert_bit_exact(engine.ensemble_stat(0), oracle.ensemble_stat(0, wide), "mean beside the copy")
    assert engine.last_kernel_name() == STAT_KERNEL                   # the mean still reads the narrow members
    assert engine.last_member_format() == "f32"                       # ... and leaves the field's record alone
    assert engine.wide_copy_bytes() >= cs * n * 4
    engine.members_changed()
    assert engine.wide_copy_bytes() == 0                              # after members_changed()
    f32 = torch.from_numpy(wide).cuda()
    engine.bind_members(f32)
    assert_bit_exact(engine.ensemble_stat(0), oracle.ensemble_stat(0, wide), "rebound as f32")
    assert engine.last_kernel_name() in FP32_STAT_KERNELS and engine.wide_copy_bytes() == 0
    del members


# ---- 7. unaligned borrowed members --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "u16"])
def test_unaligned_borrowed_members(engine, oracle, fmt):
    cs, (xs, ys, zs) = 24, (7, 5, 3)
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=4), fmt)
    wide = convert(narrow)
    rows = np.zeros((cs, n + 7), narrow.dtype)  # the layout of test_unaligned_borrowed_members_take_the_widened_path
    rows[:, 1:n + 1] = narrow.reshape(cs, n)
    buf = to_device(rows)
    members = [buf[c, 1:n + 1] for c in range(cs)]
    assert all(m.data_ptr() % 4 != 0 for m in members)
    engine.set_grid(xs, ys, zs, cs)
    engine.bind_members(members)
    # the per-voxel reductions load dwords: the fp32 copy
    assert_bit_exact(engine.ensemble_stat(0), oracle.ensemble_stat(0, wide), f"{fmt} offset 1 mean")
    assert engine.last_kernel_name() in FP32_STAT_KERNELS and engine.wide_copy_bytes() > 0
    assert_bit_exact(engine.set_predicate(">", 0.5, 2, 20), oracle.set_predicate(0, 0.5, 2, 20, wide), f"{fmt} offset 1 predicate")
    assert engine.last_kernel_name() == "set_predicate_kernel"
    # the gathers and the extrema read element by element: a fresh binding stays without the copy
    engine.bind_members(members)
    assert engine.wide_copy_bytes() == 0
    for x, y, z in [(0, 0, 0), (3, 2, 1), (6, 4, 2)]:
        assert (engine.gather_reference(x, y, z).view(np.uint32) == wide[:, z, y, x].view(np.uint32)).all()
    mn, mx = engine.member_minmax()
    assert (bits(mn), bits(mx)) == (bits(wide.min()), bits(wide.max()))
    assert engine.wide_copy_bytes() == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_extrema_of_every_head_and_tail_length(engine, fmt):
    """The extrema kernel reads the elements before the first 16-byte boundary and behind the last whole 16 bytes one by
    one: members that start at every element offset of a 16-byte line, the extremes placed first and last."""
    cs, n = 3, 4099
    base = cast(box01(n + 16, 1, 1, cs, seed=3), fmt).reshape(cs, n + 16)
    lo, hi, below, above = {"u8": (40, 200, 3, 250), "u16": (4000, 60000, 300, 65000),
                            "f16": (np.float16(0.125), np.float16(0.875), np.float16(0.0625), np.float16(0.9375))}[fmt]
    base = np.clip(base, lo, hi).astype(base.dtype)
    for offset in range(16 // base.itemsize):
        view = base[:, offset:offset + n].copy()
        view[1, 0], view[2, n - 1] = below, above
        # (zeros around every member: an element read from outside it would become the minimum)
        dev = to_device(np.ascontiguousarray(np.pad(view, ((0, 0), (offset, 16 - offset)))))
        members = [dev[c, offset:offset + n] for c in range(cs)]
        engine.set_grid(n, 1, 1, cs)
        engine.bind_members(members)
        mn, mx = engine.member_minmax()
        wide = convert(view)
        assert (bits(mn), bits(mx)) == (bits(wide.min()), bits(wide.max())), f"{fmt} offset {offset}"
        assert engine.wide_copy_bytes() == 0


# ---- 8. host output and device output agree -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_and_device_output_agree_and_are_timed(engine, fmt):
    """With profiling on, every call queues ONE launch for take_kernel_time: the one-wave tail kernel (13*11*7 = 1001
    voxels leave a ragged dword) is bracketed by the same event pair as the main kernel."""
    import torch
    cs, (xs, ys, zs) = 24, (13, 11, 7)
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=8), fmt)
    upload(engine, narrow)
    value = between_two_codes(narrow)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    engine.set_profiling(True)
    try:
        engine.take_kernel_time()
        for stat in (0, 1):
            host = engine.ensemble_stat(stat)
            assert engine.take_kernel_time()[1] == 1
            engine.ensemble_stat_device(stat, out)
            torch.cuda.synchronize()
            ms, launches = engine.take_kernel_time()
            assert launches == 1 and ms > 0.0
            assert engine.last_kernel_name() == STAT_KERNEL
            assert_bit_exact(out.cpu().numpy(), host, f"{fmt} stat {stat} host vs device")
        host = engine.set_predicate(">", value, 2, 20)
        assert engine.take_kernel_time()[1] == 1
        engine.set_predicate_device(">", value, 2, 20, out)
        torch.cuda.synchronize()
        ms, launches = engine.take_kernel_time()
        assert launches == 1 and ms > 0.0
        assert engine.last_kernel_name() == PREDICATE_KERNEL
        assert_bit_exact(out.cpu().numpy(), host, f"{fmt} predicate host vs device")
    finally:
        engine.set_profiling(False)
    assert engine.wide_copy_bytes() == 0
