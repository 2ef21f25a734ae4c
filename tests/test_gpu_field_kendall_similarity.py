"""GPU: crf_field_kendall_similarity / CorrField.field_kendall_similarity -- Kendall's tau-b over every sample of two
resident fields (the reference's computeFieldSimilarity<double> with Kendall, Similarity.cpp:134-143, which calls
computeKendall<int64_t>): the pairs masked as the Spearman path masks them, then the sorts and the inversion count of
kernels_kendall_similarity.hip.

Exact throughout: samples, n0, n1, n2 and S equal those of kendall_similarity_reference.kendall_restated over the
reference's gather of the two fields, and the value has the bits of the restated <int64_t> tail.  The grids, member
choices, NaN cases, borrowed members and capped grids are those of test_gpu_field_rank_similarity.py (imported, not
copied).  The arrays themselves are covered size by size in test_gpu_kendall_values.py."""
import numpy as np
import pytest

from correrender_amd import CorrFieldError, Measure
from kendall_similarity_reference import f32_bits, kendall_restated
from test_gpu_field_rank_similarity import CHUNKY, LARGER, MEMBER_COUNTS, RAGGED_GRIDS, _fields, _nan_cases, _samples, _upload

pytestmark = pytest.mark.gpu

NAME = "similarity_kendall_merge_kernel"


def _check(engine, a, b, what, members=(None,)):
    _upload(engine, a, b)
    for member in members:
        x, y = _samples(a, b, member)
        want = kendall_restated(x, y)
        value, samples, counts = engine.field_kendall_similarity(member=member, return_samples=True, return_counts=True)
        assert engine.last_kernel_name() == NAME
        tag = f"{what} member={member} N={x.size}"
        print(f"[field kendall similarity] {tag}: samples {samples} counts {counts} value {value!r}; restated {want}")
        assert samples == x.size == want[0], tag
        assert counts == want[1:5], tag
        assert f32_bits(value) == want[5], tag


@pytest.mark.parametrize("cs", MEMBER_COUNTS)
@pytest.mark.parametrize("grid", RAGGED_GRIDS)
def test_ragged_grids(engine, grid, cs):
    a, b = _fields(grid, cs, 7 * cs + grid[0])
    _check(engine, a, b, f"ragged {grid}x{cs}", members=(None, cs // 2))


def test_whole_chunks_and_a_ragged_one(engine):
    a, b = _fields(CHUNKY, 3, 41)
    _check(engine, a, b, f"chunky {CHUNKY}x3", members=(None, 2))


@pytest.fixture(scope="module")
def larger():
    """262 144 samples and what the restatement makes of them, once for both capped grids."""
    a, b = _fields(LARGER[:3], LARGER[3], 163)
    return a, b, kendall_restated(*_samples(a, b, None))


@pytest.mark.parametrize("cap", [1, 5])
def test_capped_grids(engine, larger, monkeypatch, cap):
    """1024 tiles and ten merge levels of 128 to 512 chunks over five blocks, unevenly, or over one."""
    monkeypatch.setenv("CRF_SIMILARITY_MAX_BLOCKS", str(cap))
    a, b, want = larger
    _upload(engine, a, b)
    value, samples, counts = engine.field_kendall_similarity(return_samples=True, return_counts=True)
    assert (samples, *counts, f32_bits(value)) == want


def test_ties_on_both_sides(engine, monkeypatch):
    """A dozen levels on either side: runs of thousands in both sorts, equal s by the thousand in the merges."""
    monkeypatch.setenv("CRF_RANK_TILE_KEYS", "64")
    monkeypatch.setenv("CRF_KENDALL_TILE_KEYS", "64")
    a, b = _fields(CHUNKY, 3, 43)
    _check(engine, np.round(a * 8.0).astype(np.float32), np.round(b * 5.0).astype(np.float32), "quantised", members=(None, 1))


def test_nan_handling(engine):
    """The kept count is numpy's (asserted in _check)."""
    for what, a, b in _nan_cases():
        _check(engine, a, b, what, members=(None, 0))


def test_everything_nan(engine):
    a, b = _fields((65, 1, 1), 3, 8)
    a[:] = np.nan
    _upload(engine, a, b)
    value, samples, counts = engine.field_kendall_similarity(return_samples=True, return_counts=True)
    assert np.isnan(value) and samples == 0 and counts == (0, 0, 0, 0)


def test_a_constant_side_and_one_sample(engine):
    a, b = _fields(CHUNKY, 2, 12)
    _check(engine, np.full_like(a, 0.3), b, "constant x")
    assert not np.isfinite(engine.field_kendall_similarity())                   # 0 / 0, or -n2 / 0 where y has ties
    _check(engine, a[:1, :1, :1, :1].copy(), b[:1, :1, :1, :1].copy(), "one sample")
    assert np.isnan(engine.field_kendall_similarity())


def _calls(engine):
    return [engine.field_kendall_similarity(return_samples=True, return_counts=True)[1:],
            f32_bits(engine.field_kendall_similarity()), f32_bits(engine.field_kendall_similarity(member=1))]


def test_members_that_are_only_dword_aligned(engine):
    """Borrowed members offset by one float: 4-byte but not 16-byte aligned -- the dword-load form, same integers."""
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

    want = kendall_restated(*_samples(a, b, None))
    engine.set_grid(*CHUNKY, cs)
    for off_a, off_b in ((0, 0), (1, 1), (1, 0), (0, 1)):
        engine.bind_members(rows(a, off_a))
        engine.bind_secondary_members(rows(b, off_b))
        torch.cuda.synchronize()
        got = _calls(engine)
        assert got[0] == (want[0], want[1:5]) and got[1] == want[5], (off_a, off_b)
    torch.cuda.synchronize()


def test_the_same_call_gives_the_same_bits(engine):
    a, b = _fields(LARGER[:3], LARGER[3], 3)
    _upload(engine, a, b)
    first = _calls(engine)
    assert _calls(engine) == first and _calls(engine) == first


# ---- refusals, instrumentation -----------------------------------------------------------------------------------------
def _refused(engine, code, fragment, **kw):
    with pytest.raises(CorrFieldError) as e:
        engine.field_kendall_similarity(**kw)
    assert e.value.code == code and fragment in e.value.message, e.value.message


def _still_usable(engine, a):
    _upload(engine, a, a)
    out = engine.compute(Measure.PEARSON, (1, 1, 1))
    assert out.shape == a.shape[1:] and np.isfinite(out).all()
    assert isinstance(engine.field_kendall_similarity(), float)


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
    _still_usable(engine, a)
    with monkeypatch.context() as m:                                            # a windowed context
        m.setenv("CRF_WINDOW_VOXELS", "1024")
        engine.set_grid(67, 61, 5, 2)
    assert engine.window_count() > 1
    wa, wb = _fields((67, 61, 5), 2, 2)
    engine.upload_members(wa)
    engine.upload_secondary_members(wb)
    _refused(engine, 4, "windowed")                                             # CRF_ERR_UNSUPPORTED
    _still_usable(engine, a)
    # more samples than the reference's int holds: 2048 members x 128 x 128 x 65 voxels, every member the same volume
    engine.set_grid(128, 128, 65, 2048)
    volume = torch.zeros(128 * 128 * 65, dtype=torch.float32, device="cuda")
    engine.bind_members([volume] * 2048)
    engine.bind_secondary_members([volume] * 2048)
    _refused(engine, 4, "samples")
    _still_usable(engine, a)


def test_the_other_entry_points_still_refuse_kendall(engine):
    """The split is deliberate: both keep their pinned refusals, Kendall has its own entry point."""
    a, b = _fields((16, 6, 5), 2, 9)
    _upload(engine, a, b)
    with pytest.raises(CorrFieldError) as e:
        engine.field_rank_similarity(Measure.KENDALL)
    assert e.value.code == 4 and "inversion count" in e.value.message
    with pytest.raises(CorrFieldError) as e:
        engine.field_similarity(Measure.KENDALL)
    assert e.value.code == 4 and "sort" in e.value.message
    assert isinstance(engine.field_kendall_similarity(), float)


def test_profiling_covers_the_call(engine):
    a, b = _fields(CHUNKY, 2, 4)
    _upload(engine, a, b)
    engine.set_profiling(True)
    try:
        engine.take_kernel_time()
        engine.field_kendall_similarity()
        ms, launches = engine.take_kernel_time()
        assert launches == 1 and ms > 0.0
    finally:
        engine.set_profiling(False)


def test_scratch_is_held_and_released(engine):
    a, b = _fields((16, 6, 5), 2, 10)
    _upload(engine, a, b)
    assert engine.rank_scratch_bytes() == 0                                     # a fresh grid
    engine.field_kendall_similarity()
    held = engine.rank_scratch_bytes()
    assert held >= 16 * a.size
    engine.field_kendall_similarity(member=0)                                   # fewer samples: no growth
    assert engine.rank_scratch_bytes() == held
    assert engine.last_kernel_name() == NAME
    engine.set_grid(16, 6, 5, 2)
    assert engine.rank_scratch_bytes() == 0
