"""GPU: crf_field_rank_similarity / CorrField.field_rank_similarity -- Spearman over every sample of two resident fields
(the reference's computeFieldSimilarity<double> with a rank measure, Similarity.cpp:134-143): ranks over ALL samples by
the device-wide radix sort of kernels_rank_similarity.hip, then the moments path of crf_field_similarity.

What the value is compared with (rank_similarity_reference.RankAnswers): the reference's own computeRanks of the kept x
and of the kept y, then its computePearsonParallel<double> over the two rank arrays; |got - ref| <=
similarity_reference.pearson_tolerance(ref, N), the bound of the Pearson field similarity (the reference's OpenMP
summation order is unspecified, so bit identity is not defined).  Where oracle/_ref is absent the answers come from
tests/golden/reference/field_rank_similarity_calls.npz, which `python tests/rank_similarity_reference.py record` writes
from record_reference_calls below: every case is a function of its data alone.

The ranks themselves are checked bit for bit in test_gpu_rank_values.py."""
import numpy as np
import pytest

from correrender_amd import CorrFieldError, Measure
from rank_similarity_reference import RankAnswers
from similarity_reference import f32_bits, pearson_tolerance

pytestmark = pytest.mark.gpu

SPEARMAN, PEARSON = Measure.SPEARMAN, Measure.PEARSON
RAGGED_GRIDS = [(3, 1, 1), (63, 1, 1), (65, 1, 1), (257, 1, 1), (16, 6, 5)]
MEMBER_COUNTS = [1, 2, 3, 8, 64]
CHUNKY = (67, 61, 5)                            # 20 435 voxels: whole chunks and a ragged one, five tiles of the sort
LARGER = (64, 64, 8, 8)                         # xs, ys, zs, members: 262 144 samples


@pytest.fixture(scope="module")
def ans():
    return RankAnswers()


def _fields(grid, cs, seed):
    """Two correlated fields (as tests/test_gpu_field_similarity.py makes them)."""
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


def _upload(engine, a, b):
    cs, zs, ys, xs = a.shape
    engine.set_grid(xs, ys, zs, cs)
    engine.upload_members(a)
    engine.upload_secondary_members(b)


def _check(engine, ans, a, b, what, members=(None,)):
    """Spearman of fields a (primary) and b (secondary) against the reference.  engine None: only the calls of the
    reference are made (recording)."""
    if engine is not None:
        _upload(engine, a, b)
    for member in members:
        x, y = _samples(a, b, member)
        n = x.size
        tag = f"{what} member={member} N={n}"
        want = ans.spearman(x, y)
        if engine is None:
            continue
        got, samples = engine.field_rank_similarity(SPEARMAN, member=member, return_samples=True)
        assert engine.last_kernel_name() == "similarity_rank_sort_kernel"
        assert samples == n, tag
        err = abs(float(got) - float(want))
        print(f"[field rank similarity] spearman {tag}: got {got!r} reference {float(want)!r} |diff| {err:.3e} "
              f"bound {pearson_tolerance(want, n):.3e}")
        if np.isnan(want):
            assert np.isnan(got), tag
        else:
            assert err <= pearson_tolerance(want, n), tag


# ---- grids -------------------------------------------------------------------------------------------------------------
def _case_ragged(engine, ans, grid, cs):
    a, b = _fields(grid, cs, 7 * cs + grid[0])
    _check(engine, ans, a, b, f"ragged {grid}x{cs}", members=(None, cs // 2))


@pytest.mark.parametrize("cs", MEMBER_COUNTS)
@pytest.mark.parametrize("grid", RAGGED_GRIDS)
def test_ragged_grids(engine, ans, grid, cs):
    _case_ragged(engine, ans, grid, cs)


def _case_chunky(engine, ans):
    a, b = _fields(CHUNKY, 3, 41)
    _check(engine, ans, a, b, f"chunky {CHUNKY}x3", members=(None, 2))


def test_whole_chunks_and_a_ragged_one(engine, ans):
    _case_chunky(engine, ans)


def _case_larger(engine, ans):
    a, b = _fields(LARGER[:3], LARGER[3], 163)
    _check(engine, ans, a, b, f"larger {LARGER}")


@pytest.mark.parametrize("cap", [1, 5])
def test_capped_grids(engine, ans, monkeypatch, cap):
    """64 tiles of the sort and 64 chunks of the streaming kernels over five blocks, unevenly, or over one."""
    monkeypatch.setenv("CRF_SIMILARITY_MAX_BLOCKS", str(cap))
    _case_larger(engine, ans)


def _case_quantised(engine, ans):
    a, b = _fields(CHUNKY, 3, 43)
    _check(engine, ans, np.round(a * 8.0).astype(np.float32), np.round(b * 5.0).astype(np.float32), "quantised", members=(None, 1))


def test_ties_on_both_sides(engine, ans, monkeypatch):
    """A dozen levels on either side: runs of thousands, which cross the 64-key tiles many times over."""
    monkeypatch.setenv("CRF_RANK_TILE_KEYS", "64")
    _case_quantised(engine, ans)


# ---- NaN handling, degenerate data -------------------------------------------------------------------------------------
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


def _case_nan(engine, ans):
    for what, a, b in _nan_cases():
        _check(engine, ans, a, b, what, members=(None, 0))


def test_nan_handling(engine, ans):
    """The kept count is numpy's (asserted in _check)."""
    _case_nan(engine, ans)


def test_everything_nan(engine):
    a, b = _fields((65, 1, 1), 3, 8)
    a[:] = np.nan
    _upload(engine, a, b)
    value, samples = engine.field_rank_similarity(SPEARMAN, return_samples=True)
    assert samples == 0 and f32_bits(value) == f32_bits(0.0)


def test_a_constant_side_and_one_sample(engine):
    a, b = _fields(CHUNKY, 2, 12)
    _upload(engine, np.full_like(a, 0.3), b)
    value, samples = engine.field_rank_similarity(SPEARMAN, return_samples=True)
    assert np.isnan(value) and samples == a.size
    _upload(engine, a[:1, :1, :1, :1].copy(), b[:1, :1, :1, :1].copy())
    value, samples = engine.field_rank_similarity(SPEARMAN, return_samples=True)
    assert np.isnan(value) and samples == 1


# ---- checks without a reference ----------------------------------------------------------------------------------------
def test_monotone_maps(engine):
    """(a, a) gives 1 and (a, -a) gives -1 within the bound; doubling is exact and strictly monotone, so (a, 2a) has the
    ranks of (a, a) and gives the same bits."""
    a, _ = _fields(CHUNKY, 3, 51)
    a = (a - 0.5).astype(np.float32)                          # both signs
    n = a.size
    _upload(engine, a, a)
    same = engine.field_rank_similarity(SPEARMAN)
    assert abs(same - 1.0) <= pearson_tolerance(1.0, n)
    _upload(engine, a, -a)
    assert abs(engine.field_rank_similarity(SPEARMAN) + 1.0) <= pearson_tolerance(1.0, n)
    _upload(engine, a, (2.0 * a).astype(np.float32))
    assert f32_bits(engine.field_rank_similarity(SPEARMAN)) == f32_bits(same)


# ---- alignment, reproducibility ----------------------------------------------------------------------------------------
def _calls(engine):
    return [f32_bits(engine.field_rank_similarity(SPEARMAN)), f32_bits(engine.field_rank_similarity(SPEARMAN, member=1))]


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
    torch.cuda.synchronize()
    want = _calls(engine)
    for off_a, off_b in ((1, 1), (1, 0), (0, 1)):
        engine.bind_members(rows(a, off_a))
        engine.bind_secondary_members(rows(b, off_b))
        torch.cuda.synchronize()
        assert _calls(engine) == want, (off_a, off_b)
    torch.cuda.synchronize()


def test_the_same_call_gives_the_same_bits(engine):
    a, b = _fields(LARGER[:3], LARGER[3], 3)
    _upload(engine, a, b)
    first = _calls(engine)
    assert _calls(engine) == first and _calls(engine) == first


# ---- refusals, instrumentation -----------------------------------------------------------------------------------------
def _refused(engine, code, fragment, measure=SPEARMAN, **kw):
    with pytest.raises(CorrFieldError) as e:
        engine.field_rank_similarity(measure, **kw)
    assert e.value.code == code and fragment in e.value.message, e.value.message


def _still_usable(engine, a):
    _upload(engine, a, a)
    out = engine.compute(PEARSON, (1, 1, 1))
    assert out.shape == a.shape[1:] and np.isfinite(out).all()
    assert isinstance(engine.field_rank_similarity(SPEARMAN), float)


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
    _refused(engine, 4, "inversion count", measure=Measure.KENDALL)             # CRF_ERR_UNSUPPORTED
    for measure in (PEARSON, Measure.MUTUAL_INFORMATION_BINNED, Measure.MUTUAL_INFORMATION_KRASKOV):
        _refused(engine, 1, "crf_field_similarity", measure=measure)
    _still_usable(engine, a)
    with monkeypatch.context() as m:                                            # a windowed context
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
    _still_usable(engine, a)


def test_field_similarity_still_refuses_spearman(engine):
    """The split is deliberate: crf_field_similarity keeps its pinned refusal, the rank measure has its own entry point."""
    a, b = _fields((16, 6, 5), 2, 9)
    _upload(engine, a, b)
    with pytest.raises(CorrFieldError) as e:
        engine.field_similarity(SPEARMAN)
    assert e.value.code == 4 and "sort" in e.value.message
    assert isinstance(engine.field_rank_similarity(SPEARMAN), float)


def test_profiling_covers_the_call(engine):
    a, b = _fields(CHUNKY, 2, 4)
    _upload(engine, a, b)
    engine.set_profiling(True)
    try:
        engine.take_kernel_time()
        engine.field_rank_similarity(SPEARMAN)
        ms, launches = engine.take_kernel_time()
        assert launches == 1 and ms > 0.0
    finally:
        engine.set_profiling(False)


def test_scratch_is_held_and_released(engine):
    a, b = _fields((16, 6, 5), 2, 10)
    _upload(engine, a, b)
    assert engine.rank_scratch_bytes() == 0                                     # a fresh grid
    engine.field_rank_similarity(SPEARMAN)
    held = engine.rank_scratch_bytes()
    assert held >= 24 * a.size
    engine.field_rank_similarity(SPEARMAN, member=0)                            # fewer samples: no growth
    assert engine.rank_scratch_bytes() == held
    engine.set_grid(16, 6, 5, 2)
    assert engine.rank_scratch_bytes() == 0


def record_reference_calls(ans):
    """Every call of the reference that the tests above make (rank_similarity_reference.py record)."""
    for grid in RAGGED_GRIDS:
        for cs in MEMBER_COUNTS:
            _case_ragged(None, ans, grid, cs)
    _case_chunky(None, ans)
    _case_larger(None, ans)
    _case_quantised(None, ans)
    _case_nan(None, ans)
