"""GPU: the Spearman field on members in a narrow native format (uint8, uint16, float16), read as stored by
spearman_narrow_kernel at 33..128 members.  The definition of correct is the project's own: every result is bit-identical
to the oracle on the converted values AND to the same call on float32 members that hold those values.  On top of that each
native case asserts that the narrow kernel ran (last_kernel_name), that it read the members' own format
(last_member_format) and that no fp32 copy of the ensemble exists afterwards (wide_copy_bytes).

Every (format, member count) from 33 to 128 members is routed to the native kernel (profiles/narrow_spearman_ab.md), so no
case of this file asserts the copy route for a routed range; 2..32 members, 129 and more, and the symmetric mode stay on
the fp32 copy and section 11 asserts that."""
import numpy as np
import pytest

from correrender_amd import Measure, synth
from parity import assert_bit_exact
import oracle_lib
from test_gpu_member_formats import FORMATS, box01, cast, convert, to_device, to_device_members

pytestmark = pytest.mark.gpu

KERNEL = "spearman_narrow_kernel"
FMT_OF = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}


def spearman_device(eng, ref=None, **kw):
    import torch
    out = torch.empty(eng.num_voxels, dtype=torch.float32, device="cuda")
    eng.compute_device(Measure.SPEARMAN, out, ref, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_native(eng, fmt, what):
    assert eng.last_kernel_name() == KERNEL, what
    assert eng.last_member_format() == fmt, what
    assert eng.wide_copy_bytes() == 0, what


def on_f32_members(eng, narrow, call):
    """call(eng) on float32 members holding the converted values of `narrow` ([cs, zs, ys, xs])."""
    cs, zs, ys, xs = narrow.shape
    eng.set_grid(xs, ys, zs, cs)
    eng.upload_members(convert(narrow))
    got = call(eng)
    assert eng.last_member_format() == "f32"
    return got


def bind_narrow(eng, narrow, members=None):
    cs, zs, ys, xs = narrow.shape
    eng.set_grid(xs, ys, zs, cs)
    members = to_device_members(narrow.reshape(cs, -1)) if members is None else members
    eng.bind_members(members)
    assert eng.member_format() == FMT_OF[narrow.dtype]
    assert eng.wide_copy_bytes() == 0
    return members


def check_native(eng, oracle, narrow, ref, what, members=None):
    """The native Spearman field of `narrow` ([cs, zs, ys, xs]) at the reference point `ref` against the oracle on the
    converted values and against the fp32 kernels on fp32 members holding them."""
    wide = convert(narrow)
    x, y, z = ref
    with np.errstate(all="ignore"):
        want = oracle.field(oracle_lib.SPEARMAN, wide, wide[:, z, y, x].copy())
    f32 = on_f32_members(eng, narrow, lambda e: spearman_device(e, ref))
    assert_bit_exact(f32, want, f"{what}: fp32 members vs oracle")
    members = bind_narrow(eng, narrow, members)
    got = spearman_device(eng, ref)
    assert_native(eng, FMT_OF[narrow.dtype], what)
    assert_bit_exact(got, want, f"{what}: native vs oracle")
    assert_bit_exact(got, f32, f"{what}: native vs fp32 members")
    return members, got


def tied_voxels(narrow):
    """Per voxel: two members hold values that compare equal."""
    cs = narrow.shape[0]
    wide = convert(narrow).reshape(cs, -1)
    ordered = np.sort(wide, axis=0)
    return (ordered[1:] == ordered[:-1]).any(axis=0)


# ---- 1. member counts ---------------------------------------------------------------------------------------------------
# every multiple of 8 is an instantiation boundary (cs = N, N + 1); 33 and 128 are the first and the last routed count
@pytest.mark.parametrize("cs", [33, 39, 40, 41, 63, 64, 65, 96, 100, 127, 128])
@pytest.mark.parametrize("fmt", FORMATS)
def test_member_counts(engine, oracle, fmt, cs):
    # 13*11*7 = 1001 voxels: whole waves and a partial one
    narrow = cast(box01(13, 11, 7, cs, seed=cs), fmt)
    check_native(engine, oracle, narrow, (5, 6, 3), f"{fmt} cs={cs}")


# ---- 2. ragged grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(3, 1, 1), (63, 1, 1), (65, 1, 1), (257, 1, 1)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ragged_grids(engine, oracle, fmt, grid):
    xs, ys, zs = grid
    narrow = cast(box01(xs, ys, zs, 40, seed=xs), fmt)
    check_native(engine, oracle, narrow, (xs // 2, 0, 0), f"{fmt} grid={grid}")


# ---- 3. tie structure ---------------------------------------------------------------------------------------------------
def _tied(fmt, cs):
    """A 16x8x4 ensemble with a region where all members are equal (z = 0, y < 4) and one where the members take only
    two values (z = 1, y < 4); the rest is the box ensemble in `fmt`."""
    narrow = cast(box01(16, 8, 4, cs, seed=30 + cs), fmt)
    narrow[:, 0, :4, :] = narrow[0, 0, :4, :]
    two = narrow[:2, 1, :4, :].copy()
    two[1] = np.where(two[1] == two[0], narrow.max(), two[1])  # two distinct values at every voxel of the region
    pick = np.random.default_rng(cs).integers(0, 2, (cs, 4, 16))
    pick[0], pick[1] = 0, 1
    narrow[:, 1, :4, :] = np.where(pick == 0, two[0], two[1])
    return narrow


@pytest.mark.parametrize("where", ["all_equal", "two_values", "outside"])
@pytest.mark.parametrize("fmt,cs", [("u8", 64), ("u8", 128), ("u16", 40), ("f16", 40), ("u16", 100)])
def test_tie_structure(engine, oracle, fmt, cs, where):
    narrow = _tied(fmt, cs)
    ref = {"all_equal": (3, 2, 0), "two_values": (5, 1, 1), "outside": (9, 6, 3)}[where]
    x, y, z = ref
    distinct = np.unique(convert(narrow)[:, z, y, x]).size  # of the reference vector
    if where == "all_equal":
        assert distinct == 1
    elif where == "two_values":
        assert distinct == 2
    elif fmt == "u16":
        assert distinct == cs
    tied = tied_voxels(narrow)
    if fmt == "u8":
        assert tied.all()  # every voxel ties: on the fp32 kernels every voxel takes the list pass
    assert tied.any()
    # (what the all-equal voxels give is the oracle's business: bit-identity is all that is asked)
    check_native(engine, oracle, narrow, ref, f"{fmt} cs={cs} ref in {where}")


# ---- 4. extreme codes next to pads --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [33, 65, 121])
@pytest.mark.parametrize("fmt", ["u16", "u8"])
def test_extreme_codes_next_to_pads(engine, oracle, fmt, cs):
    # cs = N - 7: seven pads behind the real keys, the largest of which is the format's last code at most voxels
    rng = np.random.default_rng(cs)
    top = 65535 if fmt == "u16" else 255
    dtype = np.uint16 if fmt == "u16" else np.uint8
    narrow = rng.integers(0, top + 1, (cs, 3, 7, 13)).astype(dtype)
    extreme = rng.integers(0, 4, narrow.shape)
    narrow = np.where(extreme == 0, dtype(top), np.where(extreme == 1, dtype(0), narrow)).astype(dtype)
    assert (narrow == top).any(axis=0).mean() > 0.5 and (narrow == 0).any()
    for ref in [(6, 3, 1), (0, 0, 0)]:
        check_native(engine, oracle, narrow, ref, f"{fmt} cs={cs} extreme codes ref={ref}")


# ---- 5. f16 -------------------------------------------------------------------------------------------------------------
def _f16_values(cs, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((cs, n)) * 3).astype(np.float16)  # negative values too


@pytest.mark.parametrize("cs", [33, 64, 100])
def test_f16_zeros_of_both_signs(engine, oracle, cs):
    n = 200
    narrow = _f16_values(cs, n, cs)
    zero = np.random.default_rng(cs + 1).integers(0, 4, (cs, n))
    narrow[zero == 0] = np.float16(0.0)
    narrow[zero == 1] = np.float16(-0.0)
    voxel = np.arange(n)  # and one zero of each sign for certain, in two members that change from voxel to voxel
    narrow[voxel % cs, voxel] = np.float16(0.0)
    narrow[(voxel % cs + 1 + voxel // cs % (cs - 1)) % cs, voxel] = np.float16(-0.0)
    bits = narrow.view(np.uint16)
    assert ((bits == 0x8000).any(axis=0) & (bits == 0x0000).any(axis=0)).all()  # both zeros at every voxel: they tie
    check_native(engine, oracle, narrow.reshape(cs, 1, 1, n), (17, 0, 0), f"f16 cs={cs} +0 / -0")


@pytest.mark.parametrize("cs", [33, 64, 100])
def test_f16_subnormals_and_infinities(engine, oracle, cs):
    n = 200
    narrow = _f16_values(cs, n, 50 + cs)
    rng = np.random.default_rng(60 + cs)
    sub = rng.integers(0, 5, (cs, n)) == 0
    narrow[sub] = rng.integers(1, 0x0400, int(sub.sum())).astype(np.uint16).view(np.float16)       # +subnormals
    neg = rng.integers(0, 7, (cs, n)) == 0
    narrow[neg] = (0x8000 | rng.integers(1, 0x0400, int(neg.sum()))).astype(np.uint16).view(np.float16)  # -subnormals
    narrow[:, 10] = (1 + np.arange(cs)).astype(np.uint16).view(np.float16)  # a voxel of subnormals only
    narrow[1, 20:60] = np.float16(np.inf)
    narrow[2, 40:80] = np.float16(-np.inf)
    narrow[3, 50:70] = np.float16(np.inf)  # two +inf at one voxel: they tie
    assert not np.isnan(narrow).any()
    with np.errstate(all="ignore"):
        for ref in [(100, 0, 0), (10, 0, 0), (55, 0, 0)]:
            _, got = check_native(engine, oracle, narrow.reshape(cs, 1, 1, n), ref, f"f16 cs={cs} specials ref={ref}")
            assert not np.isnan(got).any()  # +-inf are ordinary values


@pytest.mark.parametrize("cs", [33, 64, 100])
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
    narrow[member - 1, 32] = np.float16(np.inf)
    narrow[member - 1, 33] = np.float16(-np.inf)
    has_nan = np.isnan(narrow).any(axis=0)
    assert has_nan.sum() == 5
    with np.errstate(all="ignore"):
        _, got = check_native(engine, oracle, narrow.reshape(cs, 1, 1, n), (100, 0, 0), f"f16 cs={cs} NaN member")
    assert (np.isnan(got) == has_nan).all()  # NaN exactly there
    clean = narrow.copy()
    clean[member, has_nan] = np.float16(1.0)
    with np.errstate(all="ignore"):
        _, got_clean = check_native(engine, oracle, clean.reshape(cs, 1, 1, n), (100, 0, 0), f"f16 cs={cs} no NaN")
    assert_bit_exact(got[~has_nan], got_clean[~has_nan], "the other voxels are unaffected")


# ---- 6. borrowed members that are only element-aligned ------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_element_aligned_borrowed_members_stay_native(engine, oracle, fmt):
    cs, (xs, ys, zs) = 40, (7, 5, 3)
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


# ---- 7. reference side --------------------------------------------------------------------------------------------------
def _reference_case(engine, oracle, fmt, cs, absolute_value, kind):
    import torch
    xs, ys, zs = 13, 11, 7
    narrow = cast(box01(xs, ys, zs, cs, seed=80 + cs), fmt)
    wide = convert(narrow)
    rng = np.random.default_rng(cs)
    sec = synth.box_ensemble(xs, ys, zs, cs, seed=81)
    # values no code of any format represents (irrational multiples, beyond [0, 1], negative), ties among them included
    vector = (rng.standard_normal(cs) * np.float32(np.pi)).astype(np.float32)
    vector[cs // 2] = vector[0]
    vector[cs - 1] = vector[1]
    vector[1] = vector[0]
    if kind == "secondary":
        ref_values = sec[:, 3, 6, 5].copy()
        kw = dict(ref=(5, 6, 3), reference_from_secondary=True)
    elif kind == "host":
        ref_values = vector
        kw = dict(reference_values=vector)
    else:
        ref_values = vector
        kw = dict(device_reference=torch.from_numpy(vector).cuda())

    def call(eng):
        if kind == "secondary":
            eng.upload_secondary_members(sec)
        return spearman_device(eng, absolute_value=absolute_value, **kw)

    want = oracle.field(oracle_lib.SPEARMAN, wide, ref_values)
    if absolute_value:
        want = np.abs(want)
        assert (oracle.field(oracle_lib.SPEARMAN, wide, ref_values) < 0).any()
    what = f"{fmt} cs={cs} reference {kind} abs={absolute_value}"
    f32 = on_f32_members(engine, narrow, call)
    assert_bit_exact(f32, want, f"{what}: fp32 members vs oracle")
    members = bind_narrow(engine, narrow)
    got = call(engine)
    assert_native(engine, fmt, what)
    assert_bit_exact(got, want, f"{what}: native vs oracle")
    assert_bit_exact(got, f32, f"{what}: native vs fp32 members")
    del members


@pytest.mark.parametrize("absolute_value", [False, True])
@pytest.mark.parametrize("kind", ["host", "device", "secondary"])
@pytest.mark.parametrize("fmt,cs", [("u8", 40), ("u16", 65), ("f16", 100)])
def test_reference_side(engine, oracle, fmt, cs, kind, absolute_value):
    _reference_case(engine, oracle, fmt, cs, absolute_value, kind)


# ---- 8. prepared slots --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,cs", [("f16", 40), ("u8", 65)])
def test_prepared_slots(engine, oracle, fmt, cs):
    import torch
    xs, ys, zs = 13, 11, 7
    n = xs * ys * zs
    narrow = cast(box01(xs, ys, zs, cs, seed=12), fmt)
    points = [(1, 2, 3), (12, 10, 6), (6, 0, 4)]
    members, _ = check_native(engine, oracle, narrow, points[0], "plain")
    plain = [spearman_device(engine, p) for p in points]
    rows = torch.empty((3, cs), dtype=torch.float32, device="cuda")
    engine.gather_reference_rows_device(points, rows)
    engine.prepare_rows_device(Measure.SPEARMAN, rows, 4, 3)
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in points]
    engine.compute_prepared_device(Measure.SPEARMAN, outs, 4)
    torch.cuda.synchronize()
    assert_native(engine, fmt, "prepared")
    wide = convert(narrow)
    for p, o, want in zip(points, outs, plain):
        assert_bit_exact(o.cpu().numpy(), want, f"prepared {p}")
        assert_bit_exact(want, oracle.field(oracle_lib.SPEARMAN, wide, wide[:, p[2], p[1], p[0]].copy()), f"plain {p}")
    # one slot prepared from the reference point itself, evaluated later
    engine.prepare_device(Measure.SPEARMAN, 9, points[1])
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    engine.compute_device(Measure.SPEARMAN, out, prepared_slot=9)
    torch.cuda.synchronize()
    assert_native(engine, fmt, "prepared from the point")
    assert_bit_exact(out.cpu().numpy(), plain[1], "prepared from the point")
    del members


# ---- 9. host output through the range pipeline --------------------------------------------------------------------------
def test_host_output_range_pipeline(engine, oracle):
    cs, (xs, ys, zs) = 33, (160, 128, 103)  # 2 109 440 voxels: a result above 8 MiB, two streams
    narrow = cast(box01(xs, ys, zs, cs, seed=13), "u8")
    wide = convert(narrow)
    ref = wide[:, 50, 64, 80].copy()
    want = oracle.field(oracle_lib.SPEARMAN, wide, ref)
    f32 = on_f32_members(engine, narrow, lambda e: e.compute(Measure.SPEARMAN, (80, 64, 50)))
    assert_bit_exact(f32, want, "ranged spearman on fp32 members")
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    got = engine.compute(Measure.SPEARMAN, (80, 64, 50))
    assert_native(engine, "u8", "ranged native spearman")
    assert_bit_exact(got, want, "ranged native spearman")
    assert_bit_exact(got, f32, "ranged native spearman vs fp32 members")
    got = engine.compute(Measure.PEARSON, (80, 64, 50))
    assert engine.last_member_format() == "u8" and engine.last_kernel_name() == "pearson_narrow_kernel"
    assert_bit_exact(got, oracle.field(oracle_lib.PEARSON, wide, ref), "ranged native pearson")
    got = engine.compute(Measure.SPEARMAN, (80, 64, 50))
    assert_native(engine, "u8", "ranged native spearman again")
    assert_bit_exact(got, want, "ranged native spearman again")


# ---- 10. coexistence with the fp32 copy ---------------------------------------------------------------------------------
def test_coexistence_with_the_fp32_copy(engine, oracle):
    import torch
    cs, (xs, ys, zs) = 40, (16, 8, 4)
    n = xs * ys * zs
    a, b = cast(box01(xs, ys, zs, cs, seed=10), "u16"), cast(box01(xs, ys, zs, cs, seed=11), "u16")
    members, first = check_native(engine, oracle, a, (5, 3, 2), "first data")
    wide = convert(a)
    sec = synth.box_ensemble(xs, ys, zs, cs, seed=16)
    engine.upload_secondary_members(sec)
    pearson = engine.compute(Measure.PEARSON, symmetric=True)  # stays widened: builds the copy
    assert engine.last_member_format() == "f32"
    assert engine.wide_copy_bytes() >= cs * n * 4
    assert_bit_exact(pearson, oracle.symmetric_field(oracle_lib.PEARSON, wide, sec), "symmetric pearson on the copy")
    again = spearman_device(engine, (5, 3, 2))
    assert engine.last_kernel_name() == KERNEL and engine.last_member_format() == "u16"  # still native
    assert_bit_exact(again, first, "spearman next to the copy")
    members.view(torch.int16).copy_(to_device(b).view(torch.int16).reshape(cs, n))
    torch.cuda.synchronize()
    engine.members_changed()
    wide = convert(b)
    changed = spearman_device(engine, (5, 3, 2))
    assert engine.last_kernel_name() == KERNEL and engine.last_member_format() == "u16"
    assert_bit_exact(changed, oracle.field(oracle_lib.SPEARMAN, wide, wide[:, 2, 3, 5].copy()), "new contents")
    assert not np.array_equal(changed, first)
    del members


# ---- 11. beyond the native range ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [32, 129])
def test_member_counts_outside_the_range_take_the_copy(engine, oracle, cs):
    xs, ys, zs = 16, 8, 4
    narrow = cast(box01(xs, ys, zs, cs, seed=9), "u16")
    wide = convert(narrow)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    got = engine.compute(Measure.SPEARMAN, (5, 3, 2))
    assert engine.last_member_format() == "f32" and engine.last_kernel_name() != KERNEL
    assert engine.wide_copy_bytes() > 0
    assert_bit_exact(got, oracle.field(oracle_lib.SPEARMAN, wide, wide[:, 2, 3, 5].copy()), f"u16 cs={cs}")


def test_symmetric_spearman_takes_the_copy(engine, oracle):
    cs, (xs, ys, zs) = 40, (16, 8, 4)
    narrow = cast(box01(xs, ys, zs, cs, seed=15), "u8")
    wide = convert(narrow)
    sec = synth.box_ensemble(xs, ys, zs, cs, seed=16)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    engine.upload_secondary_members(sec)
    got = engine.compute(Measure.SPEARMAN, symmetric=True)
    assert engine.last_member_format() == "f32" and engine.last_kernel_name() != KERNEL
    assert engine.wide_copy_bytes() > 0
    assert_bit_exact(got, oracle.symmetric_field(oracle_lib.SPEARMAN, wide, sec), "u8 symmetric spearman")


def test_rank_u32_switch_does_not_move_a_native_call(engine, oracle, monkeypatch):
    # CRF_RANK_U32 selects among the fp32 kernels (here: on the fp32 members of check_native); the narrow call stays native
    monkeypatch.setenv("CRF_RANK_U32", "0")
    narrow = cast(box01(13, 11, 7, 100, seed=21), "u8")
    check_native(engine, oracle, narrow, (5, 6, 3), "u8 cs=100 CRF_RANK_U32=0")
