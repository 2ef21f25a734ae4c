"""GPU: crf_field_similarity / CorrField.field_similarity -- one value of Pearson or binned MI over every sample of two
resident fields (the reference's computeFieldSimilarity<double>, Similarity.cpp:36-180).

What the values are compared with (similarity_reference.py):
  binned, up to 46 340 samples   ref_mi_binned of the reference's object code on the gathered, NaN-filtered, normalised
                                 samples: bit-identical
  binned, beyond                 the sequential restatement with the fp64 product (the reference's int product overflows
                                 there; tests/test_similarity_tail.py pins the restatement to the object code below): bit-identical
  Pearson                        the reference's computePearsonParallel<double>: |got - ref| <= ulp32(ref) + 8 N 2^-53
                                 (similarity_reference.pearson_tolerance; the reference's own OpenMP summation order is
                                 unspecified, so bit identity is not defined)
Where oracle/_ref is absent the object code's answers come from tests/golden/reference/field_similarity_calls.npz, which
`python tests/similarity_reference.py record` writes from record_reference_calls below: every case is a function of its
data alone and runs without an engine for that purpose.

Sizes: the moments kernel works in chunks of 4096 voxels of one member, the histogram kernel in chunks of 8192; the ragged
grids stay below one chunk, 67 x 61 x 5 = 20 435 voxels has whole chunks and a ragged one for both, and
CRF_SIMILARITY_MAX_BLOCKS caps the persistent grid so that a small field takes several grid-stride rounds."""
import numpy as np
import pytest

from correrender_amd import CorrFieldError, Measure
from similarity_reference import (Answers, f32_bits, joint_counts, mi_from_counts, mi_to_cc, normalise, pearson_tolerance)

pytestmark = pytest.mark.gpu

PEARSON, BINNED, BINNED_CC = Measure.PEARSON, Measure.MUTUAL_INFORMATION_BINNED, Measure.BINNED_MI_CORRELATION_COEFFICIENT
RAGGED_GRIDS = [(3, 1, 1), (63, 1, 1), (65, 1, 1), (257, 1, 1), (16, 6, 5)]
MEMBER_COUNTS = [1, 2, 3, 8, 64]
LARGER = [(16, 16, 16, 16), (64, 64, 8, 8)]     # xs, ys, zs, members: 65 536 and 262 144 samples
CHUNKY = (67, 61, 5)                            # whole chunks and a ragged one in both kernels
BINS = (1, 2, 80, 128)
UNIT = (0.0, 1.0)
REFERENCE_LIMIT = 46340                         # the reference's es * es is defined up to here


@pytest.fixture(scope="module")
def ans():
    return Answers()


def _fields(grid, cs, seed):
    """Two correlated fields, values partly outside [0, 1]."""
    xs, ys, zs = grid
    rng = np.random.default_rng(seed)
    a = (1.5 * rng.random((cs, zs, ys, xs), dtype=np.float32) - 0.25).astype(np.float32)
    b = (0.5 * a + 0.8 * rng.random((cs, zs, ys, xs), dtype=np.float32) - 0.1).astype(np.float32)
    return a, b


def _samples(a, b, member):
    """The reference's gather (Similarity.cpp:59-127): member after member, pairs with a NaN left out."""
    x = (a if member is None else a[member:member + 1]).reshape(-1)
    y = (b if member is None else b[member:member + 1]).reshape(-1)
    keep = ~(np.isnan(x) | np.isnan(y))
    return x[keep], y[keep]


def _extrema(v):
    """min of the minima / max of the maxima over the members, NaN skipped (crf_member_minmax)."""
    with np.errstate(all="ignore"):
        return (float(np.nanmin(v)), float(np.nanmax(v))) if not np.isnan(v).all() else None


def _upload(engine, a, b):
    cs, zs, ys, xs = a.shape
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(a)
    engine.upload_secondary_members(b)


def _same(got, want, what):
    assert f32_bits(got) == f32_bits(want), f"{what}: got {got!r} ({f32_bits(got):08x}), want {want!r} ({f32_bits(want):08x})"


def _check(engine, ans, a, b, what, *, members=(None,), bins=BINS, ranges=("unit", "extrema"), pearson=True):
    """Every measure on fields a (primary) and b (secondary) against the reference.  engine None: only the calls of the
    reference are made (recording)."""
    if engine is not None:
        _upload(engine, a, b)
    for member in members:
        x, y = _samples(a, b, member)
        n = x.size
        tag = f"{what} member={member} N={n}"
        want_r = ans.pearson_parallel(x, y) if pearson else None
        if engine is not None and pearson:
            got, samples = engine.field_similarity(PEARSON, member=member, return_samples=True)
            assert engine.last_kernel_name() == "similarity_moments_kernel"
            assert samples == n, tag
            err = abs(float(got) - float(want_r))
            print(f"[field similarity] pearson {tag}: got {got!r} reference {float(want_r)!r} |diff| {err:.3e} "
                  f"bound {pearson_tolerance(want_r, n):.3e}")
            if np.isnan(want_r):
                assert np.isnan(got), tag
            else:
                assert err <= pearson_tolerance(want_r, n), tag
        for kind in ranges:
            if isinstance(kind, tuple):
                mm_x, mm_y = kind                           # ranges given by the case
            else:
                mm_x, mm_y = (UNIT, UNIT) if kind == "unit" else (_extrema(a), _extrema(b))
            if mm_x is None or mm_y is None:
                continue                                    # a field of NaN only has no extrema
            if engine is not None and kind == "extrema":
                assert engine.member_minmax() == mm_x and engine.secondary_member_minmax() == mm_y
            x01, y01 = normalise(x, *mm_x), normalise(y, *mm_y)
            for nb in bins:
                if n <= REFERENCE_LIMIT:
                    want = ans.mi_binned(x01, y01, nb)
                else:
                    want = mi_from_counts(*joint_counts(x01, y01, nb))
                if engine is None:
                    continue
                got, samples = engine.field_similarity(BINNED, member=member, num_bins=nb, minmax_x=mm_x, minmax_y=mm_y,
                                                       return_samples=True)
                assert engine.last_kernel_name() == "similarity_histogram_kernel"
                assert samples == n, tag
                _same(got, want, f"binned {tag} {kind} bins={nb}")
                if nb == 80:
                    cc = engine.field_similarity(BINNED_CC, member=member, num_bins=nb, minmax_x=mm_x, minmax_y=mm_y)
                    _same(cc, mi_to_cc(want), f"binned CC {tag} {kind}")


# ---- ragged grids ------------------------------------------------------------------------------------------------------
def _case_ragged(engine, ans, grid, cs):
    a, b = _fields(grid, cs, 7 * cs + grid[0])
    _check(engine, ans, a, b, f"ragged {grid}x{cs}", members=(None, cs // 2))


@pytest.mark.parametrize("cs", MEMBER_COUNTS)
@pytest.mark.parametrize("grid", RAGGED_GRIDS)
def test_ragged_grids(engine, ans, grid, cs):
    """Vector tails and the partial last block; 16 x 6 x 5 x 64 = 30 720 samples stays inside the reference's range."""
    _case_ragged(engine, ans, grid, cs)


# ---- larger grids ------------------------------------------------------------------------------------------------------
def _case_larger(engine, ans, shape):
    a, b = _fields(shape[:3], shape[3], 99 + shape[0])
    _check(engine, ans, a, b, f"larger {shape}", bins=(80, 128))


@pytest.mark.parametrize("shape", LARGER)
def test_larger_grids(engine, ans, shape):
    _case_larger(engine, ans, shape)


@pytest.mark.parametrize("cap", [1, 5])
def test_grid_stride_rounds_and_partial_records(engine, ans, monkeypatch, cap):
    """A capped persistent grid: 64 (moments) / 32 (histogram) chunks over 5 blocks, unevenly, or over one."""
    monkeypatch.setenv("CRF_SIMILARITY_MAX_BLOCKS", str(cap))
    _case_larger(engine, ans, LARGER[1])


def _case_chunky(engine, ans):
    a, b = _fields(CHUNKY, 3, 41)
    _check(engine, ans, a, b, f"chunky {CHUNKY}x3", members=(None, 2), bins=(80,))


def test_whole_chunks_and_a_ragged_one(engine, ans):
    _case_chunky(engine, ans)


# ---- NaN handling ------------------------------------------------------------------------------------------------------
def _nan_cases():
    a, b = _fields((16, 6, 5), 8, 5)
    a[1], b[6] = np.nan, np.nan                              # whole members of either field
    b[3, 2:4] = np.nan                                       # a voxel range in one field only
    a[0, 0, 0, 3] = np.nan
    yield "NaN members and ranges", a, b
    a, b = _fields(CHUNKY, 2, 6)
    a[1, 1:3] = np.nan
    b[0, :, 7:40] = np.nan
    yield "NaN ranges across chunks", a, b
    a, b = _fields((65, 1, 1), 3, 8)
    a[:] = np.nan
    yield "everything NaN", a, b


def _case_nan(engine, ans):
    for what, a, b in _nan_cases():
        _check(engine, ans, a, b, what, members=(None, 0), bins=(80,))


def test_nan_handling(engine, ans):
    _case_nan(engine, ans)
    what, a, b = list(_nan_cases())[-1]
    _upload(engine, a, b)
    for measure in (PEARSON, BINNED):
        value, samples = engine.field_similarity(measure, return_samples=True)
        assert samples == 0 and f32_bits(value) == f32_bits(0.0), what


# ---- degenerate data ---------------------------------------------------------------------------------------------------
def _degenerate_cases():
    grid, cs = (67, 61, 5), 2
    n = grid[0] * grid[1] * grid[2]
    a, b = _fields(grid, cs, 12)
    yield "constant field", np.full_like(a, 0.3), b
    yield "all samples in one cell", np.full_like(a, 0.3), np.full_like(b, 0.71)
    v = np.arange(n)
    for what, sel in (("two cells alternating lane by lane", (v // 4) % 2), ("two cells alternating voxel by voxel", v % 2)):
        x = np.where(sel == 0, np.float32(0.1), np.float32(0.9)).astype(np.float32).reshape(grid[::-1])
        yield what, np.stack([x, x]), np.stack([x, 1.0 - x]).astype(np.float32)
    yield "one sample", a[:1, :1, :1, :1].copy(), b[:1, :1, :1, :1].copy()
    a, b = _fields((16, 6, 5), 4, 13)
    a, b = a * 3.0 - 1.0, b * 3.0 - 1.0
    a[0, 0, 0, 1], a[1, 2, 3, 4], b[2, 1, 1, 1], b[3, 4, 5, 15] = np.inf, -np.inf, np.inf, -np.inf
    yield "outside [0, 1] and infinite", a.astype(np.float32), b.astype(np.float32)


def _case_degenerate(engine, ans):
    for what, a, b in _degenerate_cases():
        # +-inf has no finite extrema and one sample no range: the unit ranges only.  A constant side: the reference's own
        # mean of N equal values is not that value in general, so its Pearson value there is rounding noise; the library
        # gives NaN (asserted in the test), as the reference does wherever its mean is exact.
        unit_only = "infinite" in what or "one sample" in what
        constant = "constant" in what or "one cell" in what
        _check(engine, ans, a, b, what, bins=(2, 80), ranges=("unit",) if unit_only else ("unit", "extrema"),
               pearson=not constant)


def test_degenerate_data(engine, ans):
    _case_degenerate(engine, ans)
    cases = {what: (a, b) for what, a, b in _degenerate_cases()}
    a, b = cases["constant field"]
    _upload(engine, a, b)
    assert np.isnan(engine.field_similarity(PEARSON))
    a, b = cases["all samples in one cell"]
    _upload(engine, a, b)
    assert np.isnan(engine.field_similarity(PEARSON))
    _same(engine.field_similarity(BINNED), 0.0, "one cell")


# ---- ranges outside the reciprocal form of the normalisation ------------------------------------------------------------
INF = float("inf")
ODD_RANGES = [((0.0, INF), (0.0, 1.0)),          # an infinite range: finite samples normalise to 0, inf / inf is NaN
              ((-INF, 1.0), (0.25, INF)),        # an infinite minimum: every normalised x is NaN or +inf
              ((0.0, 1e-30), (0.0, 1.0)),        # a range below 2^-60: the products pass 2^31, the compiled int() decides
              ((0.5, 0.5), (0.0, 1.0))]          # an empty range: x / 0


def _case_odd_ranges(engine, ans):
    """The kernel normalises with a reciprocal where both ranges lie inside [2^-60, 2^60] and with the division
    elsewhere: these take the division.  Pairs whose normalised value is NaN count as samples and enter no cell."""
    a, b = _fields(CHUNKY, 2, 21)
    a[0, 1, 2, 3], a[1, 0, 0, 0], b[0, 4, 60, 66], b[1, 2, 30, 1] = np.inf, -np.inf, np.inf, np.nan
    _check(engine, ans, a, b, "odd ranges", bins=(2, 80), ranges=tuple(ODD_RANGES), pearson=False)


def test_ranges_that_take_the_division(engine, ans):
    _case_odd_ranges(engine, ans)


# ---- alignment, reproducibility ----------------------------------------------------------------------------------------
def _calls(engine):
    return [f32_bits(engine.field_similarity(PEARSON)), f32_bits(engine.field_similarity(PEARSON, member=1)),
            f32_bits(engine.field_similarity(BINNED, num_bins=80)),
            f32_bits(engine.field_similarity(BINNED, num_bins=128, minmax_x=(-0.25, 1.25), minmax_y=(-0.3, 1.4), member=2))]


def test_members_that_are_only_dword_aligned(engine):
    """Borrowed members offset by one float: 4-byte but not 16-byte aligned -- the dword-load form, same bits."""
    import torch
    a, b = _fields(CHUNKY, 3, 77)
    a[1, 2, 5, 9] = np.nan
    cs, n = a.shape[0], a[0].size
    stride = n + (-n) % 4                                      # rows a multiple of 16 bytes apart

    def rows(v, offset):
        store = torch.empty(cs * stride + 1, dtype=torch.float32, device="cuda")
        out = [store[offset + c * stride:offset + c * stride + n] for c in range(cs)]
        for c in range(cs):
            out[c].copy_(torch.from_numpy(v[c].reshape(-1)))
            assert out[c].data_ptr() % 16 == 4 * offset
        return out

    engine.set_grid(*CHUNKY, cs)
    engine.bind_members(rows(a, 0))
    engine.bind_secondary_members(rows(b, 0))
    want = _calls(engine)
    for off_a, off_b in ((1, 1), (1, 0), (0, 1)):
        engine.bind_members(rows(a, off_a))
        engine.bind_secondary_members(rows(b, off_b))
        assert _calls(engine) == want, (off_a, off_b)
    torch.cuda.synchronize()


def test_the_same_call_gives_the_same_bits(engine):
    a, b = _fields(LARGER[1][:3], LARGER[1][3], 3)
    _upload(engine, a, b)
    first = _calls(engine)
    assert _calls(engine) == first and _calls(engine) == first


# ---- narrow fields -----------------------------------------------------------------------------------------------------
def _narrow(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.float16:
        v = (rng.standard_normal(shape) * 0.4 + 0.5).astype(np.float16)
        return v, v.astype(np.float32)
    top = 255 if dtype == np.uint8 else 65535
    v = rng.integers(0, top + 1, shape).astype(dtype)
    return v, (v.astype(np.float32) / np.float32(top)).astype(np.float32)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float16])
@pytest.mark.parametrize("which", ["primary", "secondary", "both"])
def test_narrow_fields_read_through_their_fp32_copies(engine, dtype, which):
    shape = (3, CHUNKY[2], CHUNKY[1], CHUNKY[0])
    na, fa = _narrow(dtype, shape, 1)
    nb, fb = _narrow(dtype, shape, 2)
    _upload(engine, fa, fb)
    want = _calls(engine)
    _upload(engine, na if which != "secondary" else fa, nb if which != "primary" else fb)
    assert engine.wide_copy_bytes() == 0 and engine.secondary_wide_copy_bytes() == 0
    assert _calls(engine) == want
    assert (engine.wide_copy_bytes() != 0) == (which != "secondary")
    assert (engine.secondary_wide_copy_bytes() != 0) == (which != "primary")


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _refused(engine, code, fragment, **kw):
    with pytest.raises(CorrFieldError) as e:
        engine.field_similarity(kw.pop("measure", PEARSON), **kw)
    assert e.value.code == code and fragment in e.value.message, e.value.message


def _still_usable(engine, a):
    _upload(engine, a, a)
    out = engine.compute(PEARSON, (1, 1, 1))
    assert out.shape == a.shape[1:] and np.isfinite(out).all()
    assert isinstance(engine.field_similarity(PEARSON), float)


def test_refusals_leave_the_context_usable(engine, monkeypatch):
    import torch
    a, b = _fields((16, 6, 5), 4, 1)
    cs, zs, ys, xs = a.shape
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(a)
    _refused(engine, 2, "secondary")                                            # CRF_ERR_STATE
    _still_usable(engine, a)
    for member in (-2, cs):
        _refused(engine, 1, "member", member=member)                            # CRF_ERR_ARGUMENT
    for bins in (0, 129):
        _refused(engine, 1, "num_bins", measure=BINNED, num_bins=bins)
    _still_usable(engine, a)
    for measure, word in ((Measure.SPEARMAN, "sort"), (Measure.KENDALL, "sort"),
                          (Measure.MUTUAL_INFORMATION_KRASKOV, "neighbour"), (Measure.KMI_CORRELATION_COEFFICIENT, "neighbour")):
        _refused(engine, 4, word, measure=measure)                              # CRF_ERR_UNSUPPORTED
    _still_usable(engine, a)
    # a windowed context, set up as tests/test_gpu_windows.py does it
    with monkeypatch.context() as m:
        m.setenv("CRF_WINDOW_VOXELS", "1024")
        engine.set_grid(67, 61, 5, 2)
    assert engine.window_count() > 1
    wa, wb = _fields((67, 61, 5), 2, 2)
    engine.upload_members(wa)
    engine.upload_secondary_members(wb)
    _refused(engine, 4, "windowed")
    _still_usable(engine, a)
    # more samples than the reference's int holds: 2048 members x 128 x 128 x 65 voxels, every member the same volume
    engine.set_grid(128, 128, 65, 2048)
    volume = torch.zeros(128 * 128 * 65, dtype=torch.float32, device="cuda")
    engine.bind_members([volume] * 2048)
    engine.bind_secondary_members([volume] * 2048)
    _refused(engine, 4, "samples")
    _refused(engine, 4, "samples", measure=BINNED)
    assert isinstance(engine.field_similarity(PEARSON, member=2047), float)     # one member of it is fine
    _still_usable(engine, a)


def test_profiling_covers_the_call(engine):
    a, b = _fields(CHUNKY, 2, 4)
    _upload(engine, a, b)
    engine.set_profiling(True)
    try:
        engine.take_kernel_time()
        for measure in (PEARSON, BINNED):
            engine.field_similarity(measure)
            ms, launches = engine.take_kernel_time()
            assert launches == 1 and ms > 0.0
    finally:
        engine.set_profiling(False)


def record_reference_calls(ans):
    """Every call of the reference that the tests above make (similarity_reference.py record)."""
    for grid in RAGGED_GRIDS:
        for cs in MEMBER_COUNTS:
            _case_ragged(None, ans, grid, cs)
    for shape in LARGER:
        _case_larger(None, ans, shape)
    _case_chunky(None, ans)
    _case_nan(None, ans)
    _case_degenerate(None, ans)
    _case_odd_ranges(None, ans)
