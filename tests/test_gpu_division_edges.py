"""GPU: the kernels that replace the reference's per-sample division by a reciprocal and a two-fma correction, on inputs
that sit on the edges of that replacement (tests/division_edge_inputs.py; test_division_edge_inputs.py shows on the CPU
that these inputs fail a kernel whose quotient is one ulp off or that ignores its guard).

Binned MI and MI-CC (the UDIV instantiations, crf_binned_bins.h: query_bin_rcp): every sample of a bin-edge lattice is
within an ulp of a bin edge.  Expectation: the oracle, parity.assert_close; the share of bit-identical voxels is printed,
not asserted.  The extrema are always passed explicitly.  Ranges inside and outside the launchers' window [2^-60, 2^60]
and right at its ends; CRF_BINNED_PLAIN_DIV=1 must not change a bit.  The histogram, generic, counting and request
kernels divide per sample: they are the controls.

Pearson (crf_exact_div.h: exact_div behind exact_div_guard): whole grids whose standard deviation and mean sit just
inside the guard (every wave takes the exact branch), just outside, or inside except for one lane of every wave; and
voxels whose sd underflows to 0, where the reference's +inf would become NaN in a kernel that ignored the guard.
Expectation: the oracle, bit for bit.

Every test asserts engine.last_kernel_name()."""
import numpy as np
import pytest

from correrender_amd import Measure
import division_edge_inputs as dei
from parity import assert_bit_exact, assert_close, bit_identical
import oracle_lib
from test_gpu_member_formats import check_native as check_native_pearson
from test_gpu_packed_members import _check_layouts

pytestmark = pytest.mark.gpu

MI, MI_CC = Measure.MUTUAL_INFORMATION_BINNED, Measure.BINNED_MI_CORRELATION_COEFFICIENT
SHARES = []                # (what, share of bit-identical voxels)


def _compare(got, want, what):
    got = np.asarray(got).reshape(-1)
    share = float(bit_identical(got, want).mean())
    SHARES.append((what, share))
    print(f"[division edges] {what}: {share:.4%} bit-identical of {got.size}")
    assert_close(got, want, what)


def _upload(engine, ens, secondary=None):
    cs, zs, ys, xs = ens.shape
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(ens)
    if secondary is not None:
        engine.upload_secondary_members(secondary)


def _at(field, xyz):
    x, y, z = xyz
    return np.asarray(field).reshape(dei.GRID[2], dei.GRID[1], dei.GRID[0])[z, y, x]


# ---- binned MI, one reference vector ----------------------------------------------------------------------------------
def _field_kernel(cs, nb):
    if cs <= 128:
        return "mi_binned_kernel"
    return "mi_binned_hist_kernel" if nb * 64 * 6 <= 56 * 1024 else "generic_kernel"


def _binned_field(engine, oracle, cs, mm, nb, refs, measure=MI, what=""):
    ens = dei.lattice_case(cs, mm, nb, plants=True)
    _upload(engine, ens)
    omeasure = oracle_lib.MI_BINNED if measure == MI else oracle_lib.BINNED_MI_CC
    got = None
    for r in refs:
        got = engine.compute(measure, r, num_bins=nb, minmax_ref=mm, minmax_query=mm)
        assert engine.last_kernel_name() == _field_kernel(cs, nb)
        want = oracle.field(omeasure, ens, dei.voxel(ens, r), num_bins=nb, minmax_ref=mm, minmax_query=mm)
        _compare(got, want, f"{what}{measure.name} cs={cs} range={mm} bins={nb} ref={r}")
        assert np.isnan(_at(got, dei.PLANT_NAN))
    return got


# 16, 96, 128: exact instantiations; 17, 95: guarded; 130: the histogram kernel (10, 80 bins) and the generic one (255)
@pytest.mark.parametrize("cs", [16, 17, 95, 96, 128, 130])
def test_binned_field_ordinary_ranges(engine, oracle, monkeypatch, cs):
    refs = [dei.LATTICE_REF, dei.PLANT_POS_INF]
    for mm in dei.ORDINARY_RANGES:
        for nb in dei.NUM_BINS:
            _binned_field(engine, oracle, cs, mm, nb, refs)
    mm = dei.ORDINARY_RANGES[0]
    _binned_field(engine, oracle, cs, mm, 80, refs[:1], measure=MI_CC)
    default = _binned_field(engine, oracle, cs, mm, 80, refs[:1])
    monkeypatch.setenv("CRF_BINNED_PLAIN_DIV", "1")          # the launchers read it at every call
    plain = _binned_field(engine, oracle, cs, mm, 80, refs[:1], what="plain division: ")
    assert_bit_exact(plain, default, f"CRF_BINNED_PLAIN_DIV=1 vs the reciprocal form cs={cs}")


# one bin count per member count
@pytest.mark.parametrize("cs,nb", [(16, 10), (17, 255), (95, 80), (96, 255), (128, 10), (130, 10), (130, 255)])
def test_binned_field_window_boundaries(engine, oracle, cs, nb):
    for mm, _inside in dei.BOUNDARY_RANGES:
        _binned_field(engine, oracle, cs, mm, nb, [dei.LATTICE_REF, dei.PLANT_POS_INF, dei.PLANT_TINY])


# ---- binned MI, symmetric field mode ----------------------------------------------------------------------------------
def _binned_symmetric(engine, oracle, cs, mm_a, mm_b, nb, measure=MI, what=""):
    a, b = dei.lattice_case(cs, mm_a, nb, plants=True), dei.lattice_case(cs, mm_b, nb, side=1)
    _upload(engine, a, b)
    got = engine.compute(measure, symmetric=True, num_bins=nb, minmax_ref=mm_a, minmax_query=mm_b)
    assert engine.last_kernel_name() == ("sorted_symmetric_kernel" if cs <= 128 else "direct_symmetric_kernel")
    omeasure = oracle_lib.MI_BINNED if measure == MI else oracle_lib.BINNED_MI_CC
    want = oracle.symmetric_field(omeasure, a, b, num_bins=nb, minmax_ref=mm_a, minmax_query=mm_b)
    _compare(got, want, f"{what}symmetric {measure.name} cs={cs} ranges={mm_a},{mm_b} bins={nb}")
    assert np.isnan(_at(got, dei.PLANT_NAN))
    return got


@pytest.mark.parametrize("cs", [31, 64, 128, 130])
def test_binned_symmetric_ordinary_ranges(engine, oracle, monkeypatch, cs):
    ranges = dei.ORDINARY_RANGES
    for i, mm_a in enumerate(ranges):
        for nb in dei.NUM_BINS:
            _binned_symmetric(engine, oracle, cs, mm_a, ranges[(i + 1) % len(ranges)], nb)
    _binned_symmetric(engine, oracle, cs, ranges[0], ranges[1], 80, measure=MI_CC)
    default = _binned_symmetric(engine, oracle, cs, ranges[0], ranges[1], 80)
    monkeypatch.setenv("CRF_BINNED_PLAIN_DIV", "1")
    plain = _binned_symmetric(engine, oracle, cs, ranges[0], ranges[1], 80, what="plain division: ")
    assert_bit_exact(plain, default, f"CRF_BINNED_PLAIN_DIV=1 vs the reciprocal form, symmetric cs={cs}")


@pytest.mark.parametrize("cs,nb", [(31, 80), (64, 255), (128, 10), (130, 80)])
def test_binned_symmetric_window_boundaries(engine, oracle, cs, nb):
    """One side at the window's boundary, the other ordinary, in both orders: with a range outside the window (the first
    and the last of BOUNDARY_RANGES) the launcher takes the division form for BOTH sides."""
    inside = dei.ORDINARY_RANGES[0]
    for mm, _inside in dei.BOUNDARY_RANGES:
        _binned_symmetric(engine, oracle, cs, inside, mm, nb)
        _binned_symmetric(engine, oracle, cs, mm, inside, nb)


# ---- binned MI, pair requests (the pair's own extrema, per-sample division: controls) -----------------------------------
@pytest.mark.parametrize("cs", [64, 130])
def test_binned_requests(engine, oracle, cs):
    pairs, ii, jj = dei.request_pairs(dei.GRID, dei.REQUEST_COUNT, cs)
    for mm in dei.ORDINARY_RANGES:
        for nb in dei.NUM_BINS:
            ens = dei.lattice_case(cs, mm, nb)
            _upload(engine, ens)
            for measure, omeasure in ((MI, oracle_lib.MI_BINNED), (MI_CC, oracle_lib.BINNED_MI_CC)):
                got = engine.compute_requests(measure, pairs, num_bins=nb)
                assert engine.last_kernel_name() == ("sorted_request_kernel" if cs <= 128 else "pair_request_kernel")
                _compare(got, oracle.pair_requests(omeasure, ens, ii, jj, num_bins=nb),
                         f"requests {measure.name} cs={cs} range={mm} bins={nb}")


# ---- Pearson, the two-vector kernel -----------------------------------------------------------------------------------
# 2, 16: CS_PAD 16; 17: 32; 64; 81, 96: 96; 112; 128
TWO_VECTOR_MEMBER_COUNTS = [2, 16, 17, 64, 81, 96, 112, 128]


@pytest.mark.parametrize("cs", TWO_VECTOR_MEMBER_COUNTS)
def test_pearson_symmetric_every_family_pair(engine, oracle, cs):
    fields_x = {f: dei.guard_field(f, cs, seed=10 + cs) for f in dei.FAMILIES}
    fields_y = {f: dei.guard_field(f, cs, seed=20 + cs) for f in dei.FAMILIES}      # independent of X
    for fx in dei.FAMILIES:
        for fy in dei.FAMILIES:
            _upload(engine, fields_x[fx], fields_y[fy])
            got = engine.compute(Measure.PEARSON, symmetric=True)
            assert engine.last_kernel_name() == "pearson_symmetric_kernel"
            assert_bit_exact(got, oracle.symmetric_field(oracle_lib.PEARSON, fields_x[fx], fields_y[fy]),
                             f"symmetric pearson cs={cs} X={fx} Y={fy}")
    # Y = X times 2^-45 in every voxel / in one voxel of every 64: sd == 0 there, the reference gives +inf, exact_div NaN
    x = fields_x["low-in"]
    for one_lane in (False, True):
        y = dei.tiny_shadow(x.reshape(cs, -1), one_lane).reshape(x.shape)
        _upload(engine, x, y)
        got = engine.compute(Measure.PEARSON, symmetric=True)
        assert engine.last_kernel_name() == "pearson_symmetric_kernel"
        want = oracle.symmetric_field(oracle_lib.PEARSON, x, y)
        assert np.isposinf(want[dei.one_out_voxels(want.size)]).all()
        assert_bit_exact(got, want, f"symmetric pearson cs={cs} X=low-in Y=its tiny shadow, one lane only: {one_lane}")


@pytest.mark.parametrize("cs", TWO_VECTOR_MEMBER_COUNTS + [150])      # 150: pair_request_kernel, plain divisions
def test_pearson_requests_pairing_families(engine, oracle, cs):
    ens, pairs, ii, jj = dei.guard_request_case(cs, seed=30 + cs)
    _upload(engine, ens)
    for use_abs in (False, True):
        got = engine.compute_requests(Measure.PEARSON, pairs, absolute_value=use_abs)
        assert engine.last_kernel_name() == ("pearson_request_kernel" if cs <= 128 else "pair_request_kernel")
        want = oracle.pair_requests(oracle_lib.PEARSON, ens, ii, jj, use_abs=use_abs)
        assert np.isposinf(want[159]) and np.isposinf(want[256:320:2]).all()      # a voxel with its tiny shadow
        assert_bit_exact(got, want, f"pearson requests cs={cs} abs={use_abs}")


# ---- Pearson, one reference vector ------------------------------------------------------------------------------------
UNIT_VOXEL = (15, 7, 7)        # an O(1) voxel inside every family grid (the last one: no failing lane of one-out)
ONE_REFERENCE = [(16, "pearson_reg_kernel"), (64, "pearson_reg_kernel"), (200, "pearson_reg_kernel"),
                 (256, "pearson_reg_lds_kernel"), (340, "pearson_split_kernel"), (1000, "pearson_split_kernel"),
                 (1300, "pearson_big_kernel")]      # pearson_big_kernel divides per sample: the control


def _family_with_unit_voxel(name, cs):
    xs, ys, zs = dei.GUARD_GRID
    ens = dei.guard_family(name, cs, xs * ys * zs, seed=40 + cs)
    return dei.with_unit_voxel(ens, dei.linear_index(np.array([UNIT_VOXEL]), dei.GUARD_GRID)[0]).reshape(cs, zs, ys, xs)


@pytest.mark.parametrize("cs,kernel", ONE_REFERENCE)
def test_pearson_field_at_the_guard(engine, oracle, cs, kernel):
    for name in ("low-in", "high-in", "one-out"):
        ens = _family_with_unit_voxel(name, cs)
        _upload(engine, ens)
        for r in (dei.GUARD_REF, UNIT_VOXEL):      # the reference point inside the family / at the O(1) voxel
            got = engine.compute(Measure.PEARSON, r)
            assert engine.last_kernel_name() == kernel
            want = oracle.field(oracle_lib.PEARSON, ens, dei.voxel(ens, r))
            if name == "one-out" and r == dei.GUARD_REF:      # the sd == 0 voxels are tiny multiples of this reference
                assert np.isposinf(want[dei.one_out_voxels(want.size)[2::4]]).all()
            assert_bit_exact(got, want, f"pearson {name} cs={cs} ref={r}")


def test_pearson_packed_members_at_the_guard(engine, oracle):
    try:
        for name in ("low-in", "high-in", "one-out"):
            ens = _family_with_unit_voxel(name, 64)
            for r in (dei.GUARD_REF, UNIT_VOXEL):
                _check_layouts(engine, oracle, ens, r, f"{name} ref={r}")      # asserts pearson_reg_kernel on the packed copy
    finally:
        engine.set_member_layout("auto")


def test_pearson_narrow_f16_outside_and_inside_the_guard(engine, oracle):
    xs, ys, zs = dei.GUARD_GRID
    n = xs * ys * zs
    # every mean exactly 0: the guard is false in every lane; then f16 denormals only: inside the guard
    for what, narrow in (("antithetic", dei.antithetic_f16(64, n, 1)), ("denormals", dei.denormal_f16(64, n, 2))):
        members = check_native_pearson(engine, oracle, narrow.reshape(64, zs, ys, xs), dei.GUARD_REF, f"f16 {what}")
        assert engine.last_kernel_name() == "pearson_narrow_kernel"
        del members
