"""GPU: the Kraskov (KSG) mutual-information field and its correlation-coefficient variant on members in a narrow native
format (uint8, uint16, float16), read as stored by mi_kraskov_narrow_kernel / kraskov_direct_narrow_kernel.

Every native case asserts four things: the result is bit-identical to the same call on float32 members that hold the
converted values (all voxels); it is within the project's parity tolerance of the oracle on the converted values; the
members were read in their own format and no fp32 copy of the ensemble exists (last_member_format, wide_copy_bytes); and
the kernel that ran is the narrow sibling of the family that kraskov_field_plan predicts (last_kernel_name).  A (format,
plan) that profiles/narrow_kraskov_ab.md does not route asserts the copy route instead of the third.  The plans come from
kraskov_plan.h itself, through the small program of tests/test_kraskov_narrow_plan.py.

The grid is 16 x 6 x 5 = 480 voxels unless stated otherwise: seven whole 64-voxel tiles and a ragged one, two groups of
four tiles for the tile-free kernel."""
import ctypes as C

import numpy as np
import pytest

from correrender_amd import Measure, synth
from parity import assert_bit_exact, assert_close, bit_identical
import oracle_lib
from test_gpu_member_formats import FORMATS, box01, cast, convert, to_device, to_device_members
from test_kraskov_narrow_plan import FORMATS as FORMAT_IDS, plans  # noqa: F401 (plans is a fixture)

pytestmark = pytest.mark.gpu

MI, CC = Measure.MUTUAL_INFORMATION_KRASKOV, Measure.KMI_CORRELATION_COEFFICIENT
ORACLE_OF = {MI: oracle_lib.MI_KRASKOV, CC: oracle_lib.KMI_CC}
FMT_OF = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}
FP32_KERNEL = {"Column": "mi_kraskov_kernel", "Direct": "kraskov_direct_kernel", "Sorted": "kraskov_sorted_kernel"}
NARROW_KERNEL = {"Column": "mi_kraskov_narrow_kernel", "Direct": "kraskov_direct_narrow_kernel"}
GRID = (16, 6, 5)
REF = (5, 3, 2)
SWITCHES = {"sorted": "CRF_KRASKOV_SORTED", "direct": "CRF_KRASKOV_DIRECT", "tile": "CRF_KRASKOV_TILE",
            "dxt": "CRF_KRASKOV_DXT", "ti4": "CRF_KRASKOV_TI4", "stage": "CRF_KRASKOV_STAGE"}


def kraskov_device(eng, measure=MI, ref=None, **kw):
    import torch
    out = torch.empty(eng.num_voxels, dtype=torch.float32, device="cuda")
    eng.compute_device(measure, out, ref, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def predict(plans, fmt, cs, k, sw=None):
    """(native, family) of a Kraskov field call at cs members of format fmt under the switches sw."""
    (narrow, field), = plans([(FORMAT_IDS[fmt], cs, k, sw or {})])
    return narrow != "no", field.split()[0]


def assert_route(eng, plans, fmt, cs, k, what, sw=None):
    """The native route where the plan routes the call, else the copy route; returns which."""
    native, family = predict(plans, fmt, cs, k, sw)
    if native:
        assert eng.last_member_format() == fmt, what
        assert eng.wide_copy_bytes() == 0, what
        assert eng.last_kernel_name() == NARROW_KERNEL[family], what
    else:
        assert eng.last_member_format() == "f32", what
        assert eng.wide_copy_bytes() > 0, what
        assert eng.last_kernel_name() == FP32_KERNEL[family], what
    return native


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


def oracle_field(oracle, narrow, ref, k, measure=MI, est=1):
    wide = convert(narrow)
    x, y, z = ref
    with np.errstate(all="ignore"):
        return oracle.field(ORACLE_OF[measure], wide, wide[:, z, y, x].copy(), k=k, estimator=est)


def check(eng, oracle, plans, narrow, ref, k, what, *, measure=MI, est=1, members=None, sw=None, want=None,
          against_oracle=True, **kw):
    """One Kraskov field of `narrow` ([cs, zs, ys, xs]) at the reference point `ref`: the four assertions of the module
    docstring.  Returns (members, result, whether the call was native)."""
    fmt, cs = FMT_OF[narrow.dtype], narrow.shape[0]
    call = lambda e: kraskov_device(e, measure, ref, k=k, kraskov_estimator_index=est, **kw)
    with np.errstate(all="ignore"):
        f32 = on_f32_members(eng, narrow, call)
    assert eng.last_kernel_name() == FP32_KERNEL[predict(plans, fmt, cs, k, sw)[1]], what
    members = bind_narrow(eng, narrow, members)
    got = call(eng)
    native = assert_route(eng, plans, fmt, cs, k, what, sw)
    assert_bit_exact(got, f32, f"{what}: narrow vs fp32 members")
    if against_oracle:
        if want is None:
            want = oracle_field(oracle, narrow, ref, k, measure, est)
            if kw.get("absolute_value"):
                want = np.abs(want)
        assert np.isfinite(want).all(), what
        assert_close(got, want, f"{what}: narrow vs oracle")
    return members, got, native


def ensemble(fmt, cs, grid=GRID, seed=None):
    xs, ys, zs = grid
    return cast(box01(xs, ys, zs, cs, seed=cs if seed is None else seed), fmt)


# ---- 1. member counts and k ---------------------------------------------------------------------------------------------
# both sides of every default dispatch change of kraskov_field_plan (k = 3: 40 | 41; k = 2: 44 | 45; k = 4: 28 | 29, 32 | 33,
# 36 | 37; column -> direct 80 | 81; staging 64 | 65; table 112 | 113), the ends, and counts that are no multiple of TI or of
# the 16-candidate batch
MEMBER_COUNTS = [2, 3, 9, 28, 29, 32, 33, 36, 37, 40, 41, 44, 45, 47, 57, 64, 65, 80, 81, 100, 112, 113, 127, 128]


@pytest.mark.parametrize("cs", MEMBER_COUNTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_member_counts(engine, oracle, plans, fmt, cs):
    narrow = ensemble(fmt, cs)
    for k in (1, 2, 3, 4):
        check(engine, oracle, plans, narrow, REF, k, f"{fmt} cs={cs} k={k}")


# k beyond 4 through every K class (8, 16, 32, 64, 128), and k >= cs
@pytest.mark.parametrize("cs,k", [(64, 5), (64, 8), (64, 9), (100, 17), (100, 33), (128, 65), (128, 127), (8, 12), (5, 20),
                                  (100, 12), (64, 70)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_k_beyond_four(engine, oracle, plans, fmt, cs, k):
    check(engine, oracle, plans, ensemble(fmt, cs), REF, k, f"{fmt} cs={cs} k={k}")


def test_the_feature_is_there(engine, oracle, plans):
    """At least the default measure of a uint8 ensemble at 64 members with the default k runs without the copy."""
    _, _, native = check(engine, oracle, plans, ensemble("u8", 64), REF, 2, "u8 cs=64 default k")
    assert native


# ---- 2. estimators and flags --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [40, 64])  # the LDS-column family (native for uint8), the tile-free family (native for all)
@pytest.mark.parametrize("fmt", FORMATS)
def test_estimators_and_flags(engine, oracle, plans, fmt, cs):
    narrow = ensemble(fmt, cs, seed=20 + cs)
    assert predict(plans, fmt, cs, 3) == (fmt == "u8" or cs == 64, "Column" if cs == 40 else "Direct")
    for measure, est, kw in [(MI, 1, {}), (MI, 2, {}), (CC, 1, {}), (CC, 2, {}), (MI, 1, dict(absolute_value=True)),
                             (CC, 1, dict(absolute_value=True))]:
        check(engine, oracle, plans, narrow, REF, 3, f"{fmt} cs={cs} {measure.name} KSG-{est} {kw}", measure=measure,
              est=est, **kw)


# ---- 3. forced plans ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", ["direct", "tile"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_forced_plans(engine, oracle, plans, monkeypatch, fmt, forced):
    for cs in (20, 33, 64):
        narrow = ensemble(fmt, cs, seed=40 + cs)
        for k in (2, 4):
            want = oracle_field(oracle, narrow, REF, k)
            for dxt in (0, 1):
                for ti4 in (0, 1):
                    for stage in (0, 1):
                        sw = {forced: 1, "dxt": dxt, "ti4": ti4, "stage": stage}
                        for name, value in sw.items():
                            monkeypatch.setenv(SWITCHES[name], str(value))
                        assert predict(plans, fmt, cs, k, sw)[1] == ("Direct" if forced == "direct" else "Column")
                        check(engine, oracle, plans, narrow, REF, k, f"{fmt} cs={cs} k={k} {sw}", sw=sw, want=want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_sorted_kernel_stays_on_the_copy(engine, oracle, plans, monkeypatch, fmt):
    monkeypatch.setenv("CRF_KRASKOV_SORTED", "1")
    sw = dict(sorted=1)
    assert predict(plans, fmt, 48, 3, sw) == (False, "Sorted")
    check(engine, oracle, plans, ensemble(fmt, 48), REF, 3, f"{fmt} cs=48 sorted", sw=sw)
    assert engine.last_kernel_name() == "kraskov_sorted_kernel" and engine.last_member_format() == "f32"


# ---- 4. ragged grids ----------------------------------------------------------------------------------------------------
# (257, 1, 1): one voxel into a second group of four tiles
@pytest.mark.parametrize("grid", [(3, 1, 1), (63, 1, 1), (65, 1, 1), (257, 1, 1)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ragged_grids(engine, oracle, plans, fmt, grid):
    for cs in (40, 64, 128):  # column family; tile-free family with a tile of floats, of codes
        narrow = ensemble(fmt, cs, grid=grid, seed=grid[0] + cs)
        check(engine, oracle, plans, narrow, (grid[0] // 2, 0, 0), 3, f"{fmt} cs={cs} grid={grid}")


# ---- 5. codes -----------------------------------------------------------------------------------------------------------
def _every_16bit_code(fmt):
    """[64, 1, 1, 1024]: every 16-bit code once.  f16: the NaN codes fill the first 32 voxels, so that the other 992 hold
    the infinities, the subnormals and both zeros without a NaN beside them."""
    rng = np.random.default_rng(5)
    codes = np.arange(65536, dtype=np.uint32)
    if fmt == "u16":
        return rng.permutation(codes).astype(np.uint16).reshape(64, 1, 1, 1024)
    is_nan = ((codes & 0x7C00) == 0x7C00) & ((codes & 0x03FF) != 0)
    nan, rest = rng.permutation(codes[is_nan]), rng.permutation(codes[~is_nan])
    assert nan.size == 2046
    grid = np.empty((64, 1024), np.uint32)
    head = np.concatenate([nan, rest[:2]])
    grid[:, :32] = head.reshape(64, 32)
    grid[:, 32:] = rest[2:].reshape(64, 992)
    return grid.astype(np.uint16).view(np.float16).reshape(64, 1, 1, 1024)


@pytest.mark.parametrize("k", [3, 2])  # 64 members: staged with the table and 4 points per sweep; 8 points, not staged
@pytest.mark.parametrize("fmt", ["u16", "f16"])
def test_every_16bit_code(engine, oracle, plans, fmt, k):
    narrow = _every_16bit_code(fmt)
    assert np.unique(narrow.view(np.uint16)).size == 65536
    with np.errstate(all="ignore"):
        _, got, _ = check(engine, oracle, plans, narrow, (500, 0, 0), k, f"every {fmt} code k={k}",
                          against_oracle=fmt == "u16")
    if fmt == "f16":
        has_nan = np.isnan(narrow.reshape(64, 1024)).any(axis=0)
        assert has_nan.sum() == 32 and np.isinf(narrow).sum() == 2
        assert (np.isnan(got) == has_nan).all()


@pytest.mark.parametrize("k", [3, 2])
def test_every_u8_code(engine, oracle, plans, k):
    narrow = np.random.default_rng(6).permutation(256).astype(np.uint8).reshape(64, 1, 1, 4)
    check(engine, oracle, plans, narrow, (1, 0, 0), k, f"every u8 code k={k}")


@pytest.mark.parametrize("cs", [24, 64, 128])  # column family (the copy); tile-free family: a tile of floats, of codes
def test_f16_nan_in_one_member_of_one_voxel(engine, oracle, plans, cs):
    narrow = ensemble("f16", cs, seed=50 + cs)
    flat = narrow.reshape(cs, -1)
    for member, voxel, bits in [(cs // 2, 70, 0x7E00), (cs - 1, 479, 0xFFFF), (0, 200, 0x7C01)]:
        flat.view(np.uint16)[member, voxel] = bits
    has_nan = np.isnan(flat).any(axis=0)
    assert has_nan.sum() == 3
    with np.errstate(all="ignore"):
        _, got, _ = check(engine, oracle, plans, narrow, REF, 3, f"f16 cs={cs} NaN", against_oracle=False)
    assert (np.isnan(got) == has_nan).all()  # NaN exactly there
    clean = narrow.copy()
    clean.reshape(cs, -1)[:, has_nan] = np.float16(0.5)
    _, got_clean, _ = check(engine, oracle, plans, clean, REF, 3, f"f16 cs={cs} no NaN")
    assert_bit_exact(got[~has_nan], got_clean[~has_nan], "the other voxels are unaffected")


@pytest.mark.parametrize("cs", [9, 65, 121])  # 7 padded candidate slots behind the last real member
@pytest.mark.parametrize("fmt", ["u8", "u16"])
def test_extreme_codes_next_to_padded_slots(engine, oracle, plans, fmt, cs):
    narrow = ensemble(fmt, cs, seed=60 + cs)
    top = np.iinfo(narrow.dtype).max
    last = narrow[cs - 1].reshape(-1)
    last[0::3] = 0
    last[1::3] = top
    narrow[cs - 2].reshape(-1)[0::2] = top
    for k in (1, 3, 4):
        check(engine, oracle, plans, narrow, REF, k, f"{fmt} cs={cs} k={k} extreme codes")


# ---- 6. alignment -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [40, 64, 128])
@pytest.mark.parametrize("fmt", FORMATS)
def test_element_aligned_borrowed_members_stay_native(engine, oracle, plans, fmt, cs):
    xs, ys, zs = GRID
    n = xs * ys * zs
    narrow = ensemble(fmt, cs, seed=4)
    rows = np.zeros((cs, n + 4), narrow.dtype)  # row stride 484 elements: whole dwords
    rows[:, 1:n + 1] = narrow.reshape(cs, n)
    buf = to_device(rows)
    members = [buf[c, 1:n + 1] for c in range(cs)]
    if fmt == "u8":
        assert all(m.data_ptr() % 2 == 1 for m in members)  # odd byte offsets
    else:
        assert all(m.data_ptr() % 4 == 2 for m in members)
    k = 4 if cs == 128 else 3  # (at 113..128 members k = 4 is routed for every format, k = 3 for float16 only)
    _, _, native = check(engine, oracle, plans, narrow, REF, k, f"{fmt} cs={cs} element-aligned rows", members=members)
    assert native == (fmt == "u8" or cs != 40)  # (no column cell of the 16-bit formats is routed)
    del members, buf


def test_u16_view_at_an_odd_byte_takes_the_copy(engine, oracle, plans):
    """64 members, k = 3: native for uint16 members aligned to their element -- the same bytes one byte further are not, and
    only the alignment sends that call to the copy."""
    import torch
    cs, (xs, ys, zs) = 64, GRID
    n = xs * ys * zs
    narrow = ensemble("u16", cs, seed=4)
    want = oracle_field(oracle, narrow, REF, 3)
    assert predict(plans, "u16", cs, 3) == (True, "Direct")
    raw = np.zeros((cs, 2 * n + 8), np.uint8)
    raw[:, 1:2 * n + 1] = narrow.reshape(cs, n).view(np.uint8)
    raw[:, 2 * n + 2:2 * n + 4] = 0xFF  # (behind the data: nothing reads it)
    buf = torch.from_numpy(raw).cuda()
    even = buf[:, 1:2 * n + 1].contiguous()  # the same bytes in rows that start on an even byte
    assert all(even[c].data_ptr() % 2 == 0 for c in range(cs))

    def bind(pointers):
        ptrs = (C.c_void_p * cs)(*pointers)
        engine.set_grid(xs, ys, zs, cs)
        engine._check(engine._lib.crf_bind_members_device_format(engine._ctx, FORMAT_IDS["u16"], ptrs))
        assert engine.member_format() == "u16" and engine.wide_copy_bytes() == 0

    bind([even[c].data_ptr() for c in range(cs)])
    aligned = kraskov_device(engine, MI, REF, k=3)
    assert engine.last_member_format() == "u16" and engine.wide_copy_bytes() == 0
    assert engine.last_kernel_name() == NARROW_KERNEL["Direct"]
    assert_close(aligned, want, "u16 at an even byte")
    # (no torch uint16 tensor starts at an odd byte: the pointers go to the C entry point directly)
    odd = [buf[c, 1:].data_ptr() for c in range(cs)]
    assert all(p % 2 == 1 for p in odd)
    bind(odd)
    got = kraskov_device(engine, MI, REF, k=3)
    assert engine.last_member_format() == "f32" and engine.wide_copy_bytes() > 0
    assert engine.last_kernel_name() == FP32_KERNEL["Direct"]
    assert_bit_exact(got, aligned, "u16 at an odd byte vs at an even byte")
    engine.set_grid(xs, ys, zs, cs)  # lets go of the borrowed pointers
    del buf, even


# ---- 7. reference side --------------------------------------------------------------------------------------------------
# 24, 65, 100 members, one format each (of these only uint8 at 65 is routed native), and one routed count per format
@pytest.mark.parametrize("fmt,cs", [("u16", 24), ("u8", 65), ("f16", 100), ("u8", 40), ("u16", 64), ("f16", 128)])
def test_reference_side(engine, oracle, plans, fmt, cs):
    import torch
    xs, ys, zs = GRID
    n = xs * ys * zs
    narrow = ensemble(fmt, cs, seed=80 + cs)
    wide = convert(narrow)
    sec = synth.box_ensemble(xs, ys, zs, cs, seed=81)
    k = 3
    members, plain, native = check(engine, oracle, plans, narrow, REF, k, f"{fmt} cs={cs} plain")
    assert native == ((fmt, cs) not in [("u16", 24), ("f16", 100)])
    x, y, z = REF
    vector = wide[:, z, y, x].copy()
    route = lambda what: assert_route(engine, plans, fmt, cs, k, f"{fmt} cs={cs} {what}")
    # the reference point's values as a host vector and as a device vector
    got = kraskov_device(engine, MI, None, k=k, reference_values=vector)
    route("host vector")
    assert_bit_exact(got, plain, "host vector")
    got = kraskov_device(engine, MI, None, k=k, device_reference=torch.from_numpy(vector).cuda())
    route("device vector")
    assert_bit_exact(got, plain, "device vector")
    # the reference point in secondary members that hold the converted values
    engine.upload_secondary_members(wide)
    got = kraskov_device(engine, MI, REF, k=k, reference_from_secondary=True)
    route("secondary")
    assert_bit_exact(got, plain, "reference from secondary")
    # ... and in other secondary members: against the oracle
    engine.upload_secondary_members(sec)
    got = kraskov_device(engine, MI, REF, k=k, reference_from_secondary=True)
    route("secondary")
    assert_close(got, oracle.field(oracle_lib.MI_KRASKOV, wide, sec[:, z, y, x].copy(), k=k), "other secondary members")
    # prepared slots
    points = [REF, (15, 5, 4), (0, 0, 0)]
    plains = [kraskov_device(engine, MI, p, k=k) for p in points]
    assert_bit_exact(plains[0], plain, "plain again")
    rows = torch.empty((3, cs), dtype=torch.float32, device="cuda")
    engine.gather_reference_rows_device(points, rows)
    engine.prepare_rows_device(MI, rows, 4, 3, k=k)
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in points]
    engine.compute_prepared_device(MI, outs, 4, k=k)
    torch.cuda.synchronize()
    route("prepared")
    for p, o, want in zip(points, outs, plains):
        assert_bit_exact(o.cpu().numpy(), want, f"prepared {p}")
    del members


# ---- 8. installed noise -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [40, 64])  # column family, tile-free family: both native for uint8
def test_installed_noise(engine, oracle, plans, cs):
    narrow = ensemble("u8", cs, seed=90 + cs)
    rng = np.random.default_rng(cs)
    r, q = rng.random(cs) * 1e-10, rng.random(cs) * 1e-10
    _, default, native = check(engine, oracle, plans, narrow, REF, 3, f"u8 cs={cs} default noise")
    assert native
    try:
        oracle.set_kraskov_noise(r, q)
        cs_, zs, ys, xs = narrow.shape
        engine.set_grid(xs, ys, zs, cs)  # drops installed tables
        engine.upload_members(convert(narrow))
        engine.set_kraskov_noise(r, q)
        f32 = kraskov_device(engine, MI, REF, k=3)
        assert engine.last_member_format() == "f32"
        members = bind_narrow(engine, narrow)  # set_grid again
        engine.set_kraskov_noise(r, q)
        got = kraskov_device(engine, MI, REF, k=3)
        assert assert_route(engine, plans, "u8", cs, 3, f"u8 cs={cs} installed noise") == native
        assert_bit_exact(got, f32, "installed noise: narrow vs fp32 members")
        assert_close(got, oracle_field(oracle, narrow, REF, 3), "installed noise: narrow vs oracle")
        assert not bit_identical(got, default).all()  # the ties of the u8 ensemble resolve differently
        del members
    finally:
        oracle.set_kraskov_noise(None)
        engine.set_kraskov_noise(None)


# ---- 9. host output through the range pipeline --------------------------------------------------------------------------
# 8 members of uint16 with k = 1 (a column plan: the copy route for a 16-bit format) and 40 members of uint8 with k = 2
# (native); 2 109 440 voxels: a result above 8 MiB, two streams.  The oracle checks the first 65 536 voxels of the larger case.
@pytest.mark.parametrize("fmt,cs,k,checked", [("u16", 8, 1, None), ("u8", 40, 2, 65536)])
def test_host_output_range_pipeline(engine, oracle, plans, fmt, cs, k, checked):
    xs, ys, zs = 160, 128, 103
    narrow = cast(box01(xs, ys, zs, cs, seed=13), fmt)
    wide = convert(narrow)
    ref = wide[:, 50, 64, 80].copy()
    checked = checked or xs * ys * zs
    want = oracle.field(oracle_lib.MI_KRASKOV, wide, ref, k=k, voxel_range=(0, checked))
    f32 = on_f32_members(engine, narrow, lambda e: e.compute(MI, (80, 64, 50), k=k))
    assert_close(f32.reshape(-1)[:checked], want, "ranged kraskov on fp32 members")
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    got = engine.compute(MI, (80, 64, 50), k=k)
    native = assert_route(engine, plans, fmt, cs, k, "ranged kraskov")
    assert native == (fmt == "u8")
    assert_bit_exact(got, f32, "ranged kraskov: narrow vs fp32 members")
    if cs <= 32:  # a Spearman call in between builds the copy (up to 32 members it has no native route)
        got = engine.compute(Measure.SPEARMAN, (80, 64, 50))
        assert_bit_exact(got, oracle.field(oracle_lib.SPEARMAN, wide, ref), "ranged spearman on the copy")
    else:         # (at 40 members Spearman is native too; Kraskov with k = 1 is not routed and builds it)
        engine.compute(MI, (80, 64, 50), k=1)
    assert engine.last_member_format() == "f32"
    assert engine.wide_copy_bytes() > 0
    got = engine.compute(MI, (80, 64, 50), k=k)
    assert engine.wide_copy_bytes() > 0  # the copy is still there
    if native:  # and the call does not use it
        assert engine.last_member_format() == fmt and engine.last_kernel_name() == NARROW_KERNEL["Column"]
    assert_bit_exact(got, f32, "ranged kraskov next to the copy")


# ---- 10. not native -----------------------------------------------------------------------------------------------------
def test_129_members_take_the_copy(engine, oracle):
    cs, (xs, ys, zs) = 129, GRID
    narrow = ensemble("u16", cs, seed=9)
    wide = convert(narrow)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    got = engine.compute(MI, REF, k=3)
    assert engine.last_member_format() == "f32" and engine.last_kernel_name() == "kraskov_direct_kernel"
    assert engine.wide_copy_bytes() > 0
    x, y, z = REF
    assert_close(got, oracle.field(oracle_lib.MI_KRASKOV, wide, wide[:, z, y, x].copy(), k=3), "u16 cs=129")


def test_symmetric_kraskov_takes_the_copy(engine, oracle):
    cs, (xs, ys, zs) = 24, GRID
    narrow = ensemble("u8", cs, seed=15)
    wide = convert(narrow)
    sec = synth.box_ensemble(xs, ys, zs, cs, seed=16)
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(narrow)
    engine.upload_secondary_members(sec)
    got = engine.compute(MI, symmetric=True, k=3)
    assert engine.last_member_format() == "f32" and engine.wide_copy_bytes() > 0
    assert "narrow" not in engine.last_kernel_name()
    assert_close(got, oracle.symmetric_field(oracle_lib.MI_KRASKOV, wide, sec, k=3), "u8 symmetric kraskov")
