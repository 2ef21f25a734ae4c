"""GPU: the binned mutual-information field on members in a narrow native format (uint8, uint16, float16), read as stored
by mi_binned_narrow_kernel -- for uint8 through a 256-entry table of bins that each block fills once.  Every case runs
the call on float32 members holding the converted values (mi_binned_kernel) and on the narrow members, and asserts that the
narrow kernel ran, that it read the members' own format, that no fp32 copy of the ensemble exists afterwards, that the two
results are bit-identical (equal bins, the same code behind them) and that they are within parity.py's standing tolerance
of the oracle.  The extrema are always passed explicitly, so both runs get the same parameters.

The native route serves what the measurement of profiles/narrow_binned_ab.md accepted (routed_native below): uint8 at every
member count, uint16 at 17..32 and 49..64 members, float16 at 49..64.  A case outside that asserts the copy route instead
(mi_binned_kernel, format f32, a copy held) with the same two comparisons: in test_member_counts u16 at 2, 15, 16, 33, 48 and 65..128
members and f16 at all counts but 49 and 64; test_num_bins and test_correlation_coefficient_variant (f16, 100); the f16
cases of test_ragged_grids and test_element_aligned_borrowed_members; test_reference_side (u16, 65) and (f16, 100); the
100-member f16 cases."""
import numpy as np
import pytest

from correrender_amd import Measure, synth
from parity import assert_bit_exact, assert_close
import oracle_lib
from test_gpu_member_formats import FORMATS, box01, cast, convert, to_device, to_device_members, _every_code

pytestmark = pytest.mark.gpu

KERNEL = "mi_binned_narrow_kernel"
F32_KERNEL = "mi_binned_kernel"
FMT_OF = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}
MI = Measure.MUTUAL_INFORMATION_BINNED
UNIT = (0.0, 1.0)


def binned_device(eng, ref=None, measure=MI, **kw):
    import torch
    out = torch.empty(eng.num_voxels, dtype=torch.float32, device="cuda")
    eng.compute_device(measure, out, ref, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def routed_native(fmt, cs):
    """The routing table of the native binned-MI field (api.cpp: native_field; crf_internal.h: binned_narrow_routed), from profiles/narrow_binned_ab.md."""
    n = (cs + 15) // 16 * 16
    return fmt == "u8" or (fmt == "u16" and n in (32, 64)) or (fmt == "f16" and n == 64)


def assert_native(eng, fmt, what):
    assert eng.last_kernel_name() == KERNEL, what
    assert eng.last_member_format() == fmt, what
    assert eng.wide_copy_bytes() == 0, what


def assert_route(eng, fmt, cs, what):
    """Native where the measured routing table says so, else the fp32 kernel on the copy."""
    if routed_native(fmt, cs):
        assert_native(eng, fmt, what)
    else:
        assert eng.last_kernel_name() == F32_KERNEL, what
        assert eng.last_member_format() == "f32", what
        assert eng.wide_copy_bytes() > 0, what


def on_f32_members(eng, narrow, call, kernel=F32_KERNEL):
    """call(eng) on float32 members holding the converted values of `narrow` ([cs, zs, ys, xs])."""
    cs, zs, ys, xs = narrow.shape
    eng.set_grid(xs, ys, zs, cs)
    with np.errstate(all="ignore"):
        eng.upload_members(convert(narrow))
    got = call(eng)
    assert eng.last_member_format() == "f32"
    assert eng.last_kernel_name() == kernel
    return got


def bind_narrow(eng, narrow, members=None):
    cs, zs, ys, xs = narrow.shape
    eng.set_grid(xs, ys, zs, cs)
    members = to_device_members(narrow.reshape(cs, -1)) if members is None else members
    eng.bind_members(members)
    assert eng.member_format() == FMT_OF[narrow.dtype]
    assert eng.wide_copy_bytes() == 0
    return members


def check_native(eng, oracle, narrow, ref, what, num_bins=80, mm_ref=UNIT, mm_query=UNIT, members=None):
    """The native binned-MI field of `narrow` ([cs, zs, ys, xs]) at the reference point `ref` against mi_binned_kernel on
    fp32 members holding the converted values (bit for bit) and against the oracle on those values (tolerance)."""
    kw = dict(num_bins=num_bins, minmax_ref=mm_ref, minmax_query=mm_query)
    x, y, z = ref
    with np.errstate(all="ignore"):
        wide = convert(narrow)
        want = oracle.field(oracle_lib.MI_BINNED, wide, wide[:, z, y, x].copy(), **kw)
    f32 = on_f32_members(eng, narrow, lambda e: binned_device(e, ref, **kw))
    assert_close(f32, want, f"{what}: fp32 members vs oracle")
    members = bind_narrow(eng, narrow, members)
    got = binned_device(eng, ref, **kw)
    assert_route(eng, FMT_OF[narrow.dtype], narrow.shape[0], what)
    assert_bit_exact(got, f32, f"{what}: native vs fp32 members")
    assert_close(got, want, f"{what}: native vs oracle")
    return members, got


# ---- 1. member counts ---------------------------------------------------------------------------------------------------
# every multiple of 16 is an instantiation boundary (cs = N, N + 1); N - 15 .. N share one guarded instantiation
@pytest.mark.parametrize("cs", [2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 80, 96, 97, 112, 113, 127, 128])
@pytest.mark.parametrize("fmt", FORMATS)
def test_member_counts(engine, oracle, fmt, cs):
    # 13*11*7 = 1001 voxels: whole waves and a partial one
    narrow = cast(box01(13, 11, 7, cs, seed=cs), fmt)
    check_native(engine, oracle, narrow, (5, 6, 3), f"{fmt} cs={cs}")


# ---- 2. num_bins --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_bins", [1, 2, 7, 80, 254, 255])
@pytest.mark.parametrize("fmt,cs", [("u8", 64), ("u16", 24), ("f16", 100)])
def test_num_bins(engine, oracle, fmt, cs, num_bins):
    narrow = cast(box01(13, 11, 7, cs, seed=20 + cs), fmt)
    check_native(engine, oracle, narrow, (5, 6, 3), f"{fmt} cs={cs} bins={num_bins}", num_bins=num_bins)


# ---- 3. ragged grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(3, 1, 1), (63, 1, 1), (65, 1, 1), (257, 1, 1)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ragged_grids(engine, oracle, fmt, grid):
    xs, ys, zs = grid
    narrow = cast(box01(xs, ys, zs, 24, seed=xs), fmt)
    check_native(engine, oracle, narrow, (xs // 2, 0, 0), f"{fmt} grid={grid}")


# ---- 4. every code ------------------------------------------------------------------------------------------------------
# extrema (0, 1): for u8, b / 255 * 255 sits on the truncation boundary of the bin index for every code
@pytest.mark.parametrize("num_bins,mm", [(80, UNIT), (255, UNIT), (80, (0.25, 0.75))])
@pytest.mark.parametrize("which", ["u16a", "u16b", "f16", "u8"])
def test_every_code(engine, oracle, which, num_bins, mm):
    narrow, count = _every_code(which)
    cs, n = narrow.shape
    with np.errstate(all="ignore"):
        check_native(engine, oracle, narrow.reshape(cs, 1, 1, n), (n // 3, 0, 0), f"every code {which} bins={num_bins} {mm}",
                     num_bins=num_bins, mm_ref=mm, mm_query=mm)


# ---- 5. extrema ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["range_2^-70", "range_2^70", "overflow", "max_inf", "max_eq_min", "ref_max_eq_min"])
@pytest.mark.parametrize("fmt,cs", [("u8", 24), ("u8", 100), ("u16", 24), ("f16", 64)])  # all routed native
def test_extrema(engine, oracle, fmt, cs, case):
    narrow = cast(box01(13, 11, 7, cs, seed=40 + cs), fmt)
    ref = (5, 6, 3)
    mm_ref = UNIT
    if case == "range_2^-70":      # outside [2^-60, 2^60]: the division instantiation
        mm_query = (0.0, 2.0 ** -70)
    elif case == "range_2^70":
        mm_query = (0.0, 2.0 ** 70)
    elif case == "overflow":       # value * num_bins beyond the int range: bin 0, not the last bin
        mm_query = (0.0, 1e-8)
    elif case == "max_inf":
        mm_query = (0.0, float("inf"))
    elif case == "max_eq_min":     # (y - min) / 0: +-inf (bin 0) or, for y == min, NaN (skipped)
        v = float(convert(narrow)[3, 3, 6, 5])
        mm_query = (v, v)
    else:                          # the reference sample of member 0 is 0 / 0 = NaN: an invalid reference, every lane recounts
        v = float(convert(narrow)[0, 3, 6, 5])
        mm_ref, mm_query = (v, v), UNIT
    with np.errstate(all="ignore"):
        check_native(engine, oracle, narrow, ref, f"{fmt} cs={cs} {case}", mm_ref=mm_ref, mm_query=mm_query)
    assert routed_native(fmt, cs)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_sample_skipped_gives_zero(engine, oracle, fmt):
    # constant data with max == min == that value: every normalised sample is 0 / 0, skipped; the result is 0, not NaN
    cs = 64  # routed native in every format
    narrow = cast(np.full((cs, 2, 4, 40), 0.5, np.float32), fmt)
    v = float(convert(narrow)[0, 0, 0, 0])
    with np.errstate(all="ignore"):
        _, got = check_native(engine, oracle, narrow, (1, 1, 1), f"{fmt} constant", mm_ref=(v, v), mm_query=(v, v))
    assert (got == 0.0).all()


# ---- 6. f16 -------------------------------------------------------------------------------------------------------------
def _f16_values(cs, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((cs, n)) * 3).astype(np.float16)  # negative values too


F16_MM = (-8.0, 8.0)


@pytest.mark.parametrize("cs", [64, 100])  # 64: native, 100: the copy route
def test_f16_zeros_subnormals_and_infinities(engine, oracle, cs):
    n = 200
    narrow = _f16_values(cs, n, 50 + cs)
    rng = np.random.default_rng(60 + cs)
    zero = rng.integers(0, 8, (cs, n))
    narrow[zero == 0] = np.float16(0.0)
    narrow[zero == 1] = np.float16(-0.0)
    sub = rng.integers(0, 5, (cs, n)) == 0
    narrow[sub] = rng.integers(1, 0x0400, int(sub.sum())).astype(np.uint16).view(np.float16)       # +subnormals
    neg = rng.integers(0, 7, (cs, n)) == 0
    narrow[neg] = (0x8000 | rng.integers(1, 0x0400, int(neg.sum()))).astype(np.uint16).view(np.float16)  # -subnormals
    narrow[:, 10] = (1 + np.arange(cs)).astype(np.uint16).view(np.float16)  # a voxel of subnormals only
    narrow[1, 20:60] = np.float16(np.inf)   # +-inf under finite extrema: ordinary samples, bin 0 (bin-index overflow)
    narrow[2, 40:80] = np.float16(-np.inf)
    assert not np.isnan(narrow).any()
    with np.errstate(all="ignore"):
        for ref in [(100, 0, 0), (10, 0, 0), (55, 0, 0)]:
            _, got = check_native(engine, oracle, narrow.reshape(cs, 1, 1, n), ref, f"f16 cs={cs} specials ref={ref}",
                                  mm_ref=F16_MM, mm_query=F16_MM)
            assert not np.isnan(got).any()


@pytest.mark.parametrize("cs", [64, 100])
def test_f16_nan_in_one_member(engine, oracle, cs):
    n = 200
    narrow = _f16_values(cs, n, 70 + cs)
    bits = narrow.view(np.uint16)
    member = cs // 2
    bits[member, 30] = 0x7E00   # quiet NaN
    bits[member, 31] = 0xFE00   # its negative
    bits[member, 32] = 0x7C01   # the NaN pattern right above +inf
    bits[member, 33] = 0xFFFF   # the last pattern
    bits[member, 128] = 0x7FFF  # (second wave)
    has_nan = np.isnan(narrow).any(axis=0)
    assert has_nan.sum() == 5
    with np.errstate(all="ignore"):
        _, got = check_native(engine, oracle, narrow.reshape(cs, 1, 1, n), (100, 0, 0), f"f16 cs={cs} NaN member",
                              mm_ref=F16_MM, mm_query=F16_MM)
    assert (np.isnan(got) == has_nan).all()  # NaN exactly there
    clean = narrow.copy()
    clean[member, has_nan] = np.float16(1.0)
    _, got_clean = check_native(engine, oracle, clean.reshape(cs, 1, 1, n), (100, 0, 0), f"f16 cs={cs} no NaN",
                                mm_ref=F16_MM, mm_query=F16_MM)
    assert_bit_exact(got[~has_nan], got_clean[~has_nan], "the other voxels are unaffected")


# ---- 7. correlation-coefficient variant, absolute value -------------------------------------------------------------------
@pytest.mark.parametrize("absolute_value", [False, True])
@pytest.mark.parametrize("fmt,cs", [("u8", 64), ("u16", 24), ("f16", 100)])
def test_correlation_coefficient_variant(engine, oracle, fmt, cs, absolute_value):
    narrow = cast(box01(13, 11, 7, cs, seed=70 + cs), fmt)
    wide = convert(narrow)
    cc = Measure.BINNED_MI_CORRELATION_COEFFICIENT
    kw = dict(num_bins=80, minmax_ref=UNIT, minmax_query=UNIT)
    call = lambda e: binned_device(e, (5, 6, 3), measure=cc, absolute_value=absolute_value, **kw)
    what = f"{fmt} cs={cs} MI-CC abs={absolute_value}"
    f32 = on_f32_members(engine, narrow, call)
    members = bind_narrow(engine, narrow)
    got = call(engine)
    assert_route(engine, fmt, cs, what)
    assert_bit_exact(got, f32, f"{what}: native vs fp32 members")
    assert_close(got, oracle.field(oracle_lib.BINNED_MI_CC, wide, wide[:, 3, 6, 5].copy(), **kw), f"{what}: native vs oracle")
    assert ((got >= 0) & (got <= 1)).all()
    del members


# ---- 8. reference side --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["host", "device", "secondary"])
@pytest.mark.parametrize("fmt,cs", [("u8", 24), ("u16", 65), ("f16", 100)])
def test_reference_side(engine, oracle, fmt, cs, kind):
    import torch
    xs, ys, zs = 13, 11, 7
    narrow = cast(box01(xs, ys, zs, cs, seed=80 + cs), fmt)
    wide = convert(narrow)
    rng = np.random.default_rng(cs)
    sec = synth.box_ensemble(xs, ys, zs, cs, seed=81)
    # values no code of any format represents (irrational multiples, beyond the extrema on either side)
    vector = (rng.random(cs) * np.float32(np.pi / 2) - np.float32(0.2)).astype(np.float32)
    mm_ref = (0.0, 1.0) if kind != "secondary" else (float(sec.min()), float(sec.max()))
    kw = dict(num_bins=80, minmax_ref=mm_ref, minmax_query=UNIT)
    if kind == "secondary":
        ref_values = sec[:, 3, 6, 5].copy()
        ckw = dict(ref=(5, 6, 3), reference_from_secondary=True)
    elif kind == "host":
        ref_values = vector
        ckw = dict(reference_values=vector)
    else:
        ref_values = vector
        ckw = dict(device_reference=torch.from_numpy(vector).cuda())

    def call(eng):
        if kind == "secondary":
            eng.upload_secondary_members(sec)
        return binned_device(eng, **ckw, **kw)

    what = f"{fmt} cs={cs} reference {kind}"
    f32 = on_f32_members(engine, narrow, call)
    members = bind_narrow(engine, narrow)
    got = call(engine)
    assert_route(engine, fmt, cs, what)
    assert_bit_exact(got, f32, f"{what}: native vs fp32 members")
    assert_close(got, oracle.field(oracle_lib.MI_BINNED, wide, ref_values, **kw), f"{what}: native vs oracle")
    del members


# ---- 9. prepared slots --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,cs", [("f16", 64), ("u8", 65)])  # both routed native
def test_prepared_slots(engine, oracle, fmt, cs):
    import torch
    xs, ys, zs = 13, 11, 7
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=12), fmt)
    kw = dict(num_bins=80, minmax_ref=UNIT, minmax_query=UNIT)
    points = [(1, 2, 3), (12, 10, 6), (6, 0, 4)]
    members, _ = check_native(engine, oracle, narrow, points[0], "plain")
    plain = [binned_device(engine, p, **kw) for p in points]
    rows = torch.empty((3, cs), dtype=torch.float32, device="cuda")
    engine.gather_reference_rows_device(points, rows)
    engine.prepare_rows_device(MI, rows, 4, 3, **kw)
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in points]
    engine.compute_prepared_device(MI, outs, 4, **kw)
    torch.cuda.synchronize()
    assert_native(engine, fmt, "prepared")
    wide = convert(narrow)
    for p, o, want in zip(points, outs, plain):
        assert_bit_exact(o.cpu().numpy(), want, f"prepared {p}")
        assert_close(want, oracle.field(oracle_lib.MI_BINNED, wide, wide[:, p[2], p[1], p[0]].copy(), **kw), f"plain {p}")
    # one slot prepared from the reference point itself, evaluated later
    engine.prepare_device(MI, 9, points[1], **kw)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    engine.compute_device(MI, out, prepared_slot=9, **kw)
    torch.cuda.synchronize()
    assert_native(engine, fmt, "prepared from the point")
    assert_bit_exact(out.cpu().numpy(), plain[1], "prepared from the point")
    del members


# ---- 10. host output through the range pipeline -------------------------------------------------------------------------
def test_host_output_range_pipeline(engine, oracle):
    cs, (xs, ys, zs) = 8, (160, 128, 103)  # 2 109 440 voxels: a result above 8 MiB, two streams
    narrow = cast(box01(xs, ys, zs, cs, seed=13), "u8")
    wide = convert(narrow)
    ref = wide[:, 50, 64, 80].copy()
    kw = dict(num_bins=8, minmax_ref=UNIT, minmax_query=UNIT)  # (few bins: the oracle fills num_bins^2 cells per voxel)
    want = oracle.field(oracle_lib.MI_BINNED, wide, ref, **kw)
    f32 = on_f32_members(engine, narrow, lambda e: e.compute(MI, (80, 64, 50), **kw))
    assert_close(f32, want, "ranged binned on fp32 members")
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    got = engine.compute(MI, (80, 64, 50), **kw)
    assert_native(engine, "u8", "ranged native binned")
    assert_bit_exact(got, f32, "ranged native binned")
    got = engine.compute(Measure.PEARSON, (80, 64, 50))
    assert engine.last_member_format() == "u8" and engine.last_kernel_name() == "pearson_narrow_kernel"
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, wide, ref), "ranged native pearson")
    got = engine.compute(MI, (80, 64, 50), **kw)
    assert_native(engine, "u8", "ranged native binned again")
    assert_bit_exact(got, f32, "ranged native binned again")
    assert_close(got, want, "ranged native binned vs oracle")


# ---- 11. borrowed members that are only element-aligned ------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_element_aligned_borrowed_members(engine, oracle, fmt):
    # stay native where 24 members are routed native (u8, u16); f16 takes the copy route at this count
    cs, (xs, ys, zs) = 24, (7, 5, 3)
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=4), fmt)
    rows = np.zeros((cs, n + 7), narrow.dtype)  # row stride 112 elements: whole dwords
    rows[:, 1:n + 1] = narrow.reshape(cs, n)
    buf = to_device(rows)
    members = [buf[c, 1:n + 1] for c in range(cs)]
    if fmt == "u8":
        assert all(m.data_ptr() % 2 == 1 for m in members)  # odd byte offsets
    else:
        assert all(m.data_ptr() % 4 == 2 for m in members)
    check_native(engine, oracle, narrow, (3, 2, 1), f"{fmt} element-aligned rows", members=members)
    del members, buf


# ---- 12. coexistence with the fp32 copy ---------------------------------------------------------------------------------
def test_coexistence_with_the_fp32_copy(engine, oracle):
    import torch
    cs, (xs, ys, zs) = 24, (16, 8, 4)
    n = xs * ys * zs
    kw = dict(num_bins=80, minmax_ref=UNIT, minmax_query=UNIT)
    a, b = cast(box01(xs, ys, zs, cs, seed=10), "u16"), cast(box01(xs, ys, zs, cs, seed=11), "u16")
    members, first = check_native(engine, oracle, a, (5, 3, 2), "first data")
    wide = convert(a)
    spearman = engine.compute(Measure.SPEARMAN, (5, 3, 2))  # builds the copy
    assert engine.last_member_format() == "f32"
    assert engine.wide_copy_bytes() >= cs * n * 4
    assert_bit_exact(spearman, oracle.field(oracle_lib.SPEARMAN, wide, wide[:, 2, 3, 5].copy()), "spearman on the copy")
    again = binned_device(engine, (5, 3, 2), **kw)
    assert engine.last_kernel_name() == KERNEL and engine.last_member_format() == "u16"  # still native
    assert_bit_exact(again, first, "binned next to the copy")
    members.view(torch.int16).copy_(to_device(b).view(torch.int16).reshape(cs, n))
    torch.cuda.synchronize()
    engine.members_changed()
    wide = convert(b)
    changed = binned_device(engine, (5, 3, 2), **kw)
    assert engine.last_kernel_name() == KERNEL and engine.last_member_format() == "u16"
    assert_close(changed, oracle.field(oracle_lib.MI_BINNED, wide, wide[:, 2, 3, 5].copy(), **kw), "new contents")
    assert not np.array_equal(changed, first)
    del members


# ---- 13. not native -----------------------------------------------------------------------------------------------------
def _on_the_copy(engine, what):
    assert engine.last_member_format() == "f32" and engine.last_kernel_name() != KERNEL, what
    assert engine.wide_copy_bytes() > 0, what


def test_129_members_take_the_copy(engine, oracle):
    cs, (xs, ys, zs) = 129, (16, 8, 4)
    narrow = cast(box01(xs, ys, zs, cs, seed=9), "u16")
    wide = convert(narrow)
    kw = dict(num_bins=80, minmax_ref=UNIT, minmax_query=UNIT)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    got = engine.compute(MI, (5, 3, 2), **kw)
    _on_the_copy(engine, "129 members")
    assert_close(got, oracle.field(oracle_lib.MI_BINNED, wide, wide[:, 2, 3, 5].copy(), **kw), "u16 cs=129")


def test_symmetric_binned_takes_the_copy(engine, oracle):
    cs, (xs, ys, zs) = 24, (16, 8, 4)
    narrow = cast(box01(xs, ys, zs, cs, seed=15), "u8")
    wide = convert(narrow)
    sec = synth.box_ensemble(xs, ys, zs, cs, seed=16)
    kw = dict(num_bins=80, minmax_ref=UNIT, minmax_query=(float(sec.min()), float(sec.max())))
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    engine.upload_secondary_members(sec)
    got = engine.compute(MI, symmetric=True, **kw)
    _on_the_copy(engine, "symmetric")
    assert_close(got, oracle.symmetric_field(oracle_lib.MI_BINNED, wide, sec, **kw), "u8 symmetric binned")


def test_histogram_kernel_switch_takes_the_copy(engine, oracle, monkeypatch):
    cs, (xs, ys, zs) = 24, (16, 8, 4)
    narrow = cast(box01(xs, ys, zs, cs, seed=17), "f16")
    wide = convert(narrow)
    kw = dict(num_bins=80, minmax_ref=UNIT, minmax_query=UNIT)
    monkeypatch.setenv("CRF_BINNED_HIST", "1")
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    got = engine.compute(MI, (5, 3, 2), **kw)
    _on_the_copy(engine, "CRF_BINNED_HIST=1")
    assert engine.last_kernel_name() == "mi_binned_hist_kernel"
    assert_close(got, oracle.field(oracle_lib.MI_BINNED, wide, wide[:, 2, 3, 5].copy(), **kw), "f16 histogram kernel")
