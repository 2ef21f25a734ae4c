"""GPU: crf_rank_values_device / CorrField.rank_values -- fractional ranks of a device array by the device-wide radix
sort (kernels_rank_similarity.hip), bit-identical to rank_similarity_reference.ranks_restated, which
tests/test_rank_restatement.py pins to the reference's own computeRanks.

Sizes: a tile of the sort holds 4096 keys by default (4097 values: two tiles, two blocks); CRF_RANK_TILE_KEYS lowers it
so that a few thousand values span hundreds of tiles, and CRF_SIMILARITY_MAX_BLOCKS caps the persistent grids so that one
block, or five unevenly, walk all of them."""
import numpy as np
import pytest

from rank_similarity_reference import ranks_restated

pytestmark = pytest.mark.gpu

SMALL_SIZES = (1, 2, 3, 63, 64, 65, 4097)
MANY_TILES = 20435


def _normal(n, seed=0):
    """Both signs and every exponent around 1: all four digits live, the sign boundary crossed."""
    return (np.random.default_rng(100 + n + seed).standard_normal(n) * 3.0).astype(np.float32)


def _denormal(n):
    rng = np.random.default_rng(200 + n)
    bits = rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)
    return bits.view(np.float32)


def _zeros(n):
    rng = np.random.default_rng(300 + n)
    v = _normal(n, 1)
    v[rng.random(n) < 0.3] = np.float32(0.0)
    v[rng.random(n) < 0.3] = np.float32(-0.0)
    return v


def _infinite(n):
    rng = np.random.default_rng(400 + n)
    v = _normal(n, 2)
    v[rng.random(n) < 0.2] = np.float32(np.inf)
    v[rng.random(n) < 0.2] = np.float32(-np.inf)
    return v


def _quantised(n):
    return np.round(_normal(n, 3)).astype(np.float32)                   # about twenty levels: long runs


def _long_run(n):
    """A third of the values are equal: in sorted order one run that starts inside a tile and ends several tiles later."""
    v = _normal(n, 4)
    v[np.random.default_rng(500 + n).permutation(n)[:n // 3]] = np.float32(0.125)
    return v


def _constant(n):
    return np.full(n, np.float32(-7.5))                                 # every digit pass is skipped


def _one_digit(n):
    """Values that differ in the second byte only: three passes are skipped, one is not."""
    k = np.random.default_rng(600 + n).integers(0, 256, n).astype(np.uint32)
    return (np.uint32(0x3F800000) | (k << 8)).view(np.float32)


def _sorted(n):
    return np.sort(_normal(n, 5))


def _reversed(n):
    return np.sort(_normal(n, 6))[::-1].copy()


def _with_nans(n):
    rng = np.random.default_rng(700 + n)
    v = _quantised(n)
    v[rng.random(n) < 0.25] = np.float32(np.nan)
    v[rng.random(n) < 0.05] = np.float32(-np.nan)                       # either sign of NaN
    return v


KINDS = [_normal, _denormal, _zeros, _infinite, _quantised, _long_run, _constant, _one_digit, _sorted, _reversed,
         _with_nans]


def _rank(engine, v):
    import torch
    ranks, ranked = engine.rank_values(torch.from_numpy(v).cuda(), return_ranked=True)
    assert engine.last_kernel_name() == "similarity_rank_sort_kernel"
    return ranks.cpu().numpy(), ranked


def _check(engine, v, what):
    got, ranked = _rank(engine, v)
    want = ranks_restated(v)
    assert ranked == int((~np.isnan(v)).sum()), what
    assert (np.isnan(got) == np.isnan(v)).all(), f"{what}: NaN positions"
    keep = ~np.isnan(v)
    differ = np.flatnonzero(got[keep].view(np.uint32) != want[keep].view(np.uint32))
    assert differ.size == 0, f"{what}: {differ.size} of {v.size} ranks differ, first at kept index {differ[0]}: " \
                             f"{got[keep][differ[0]]!r} against {want[keep][differ[0]]!r}"


@pytest.mark.parametrize("kind", KINDS, ids=lambda f: f.__name__.strip("_"))
def test_small_sizes(engine, kind):
    for n in SMALL_SIZES:
        _check(engine, kind(n), f"{kind.__name__} n={n}")


@pytest.mark.parametrize("kind", KINDS, ids=lambda f: f.__name__.strip("_"))
def test_many_tiles(engine, monkeypatch, kind):
    """64 keys per tile: 320 tiles, runs that cross many of them, the carries between tiles and between blocks."""
    monkeypatch.setenv("CRF_RANK_TILE_KEYS", "64")
    _check(engine, kind(MANY_TILES), f"{kind.__name__} n={MANY_TILES} tile=64")


@pytest.mark.parametrize("tile", [100, 256, 320])
def test_a_tile_more_or_less(engine, monkeypatch, tile):
    """One key less than a tile, a whole tile, one more; tiles that are no multiple of a wave or of the block."""
    monkeypatch.setenv("CRF_RANK_TILE_KEYS", str(tile))
    for n in (tile - 1, tile, tile + 1, 3 * tile - 1, 3 * tile, 3 * tile + 1):
        for kind in (_normal, _quantised, _long_run, _with_nans):
            _check(engine, kind(n), f"{kind.__name__} n={n} tile={tile}")


@pytest.mark.parametrize("cap", [1, 5])
def test_capped_grids(engine, monkeypatch, cap):
    """One block walks all 320 tiles, or five blocks 64 each: the offsets a block carries from tile to tile."""
    monkeypatch.setenv("CRF_RANK_TILE_KEYS", "64")
    monkeypatch.setenv("CRF_SIMILARITY_MAX_BLOCKS", str(cap))
    for kind in (_normal, _quantised, _long_run, _constant, _with_nans):
        _check(engine, kind(MANY_TILES), f"{kind.__name__} n={MANY_TILES} tile=64 cap={cap}")


def test_two_to_the_twenty(engine):
    _check(engine, _normal(1 << 20), "2^20 random values")
    _check(engine, _quantised(1 << 20), "2^20 quantised values")


def test_exact_starts_beyond_2_to_24(engine):
    """2^24 + 4096 tie-free values: the run start is an exact integer rounded once (the reference's fp32 running sum
    stops at 2^24), in a 64 MiB sort."""
    n = (1 << 24) + 4096
    v = (np.random.default_rng(9).permutation(n) - (1 << 23)).astype(np.float32)     # |v| < 2^24: exact and distinct
    _check(engine, v, "2^24 + 4096 tie-free")


def test_the_same_call_gives_the_same_bits(engine, monkeypatch):
    monkeypatch.setenv("CRF_RANK_TILE_KEYS", "64")
    v = _with_nans(MANY_TILES)
    first, _ = _rank(engine, v)
    for _ in range(2):
        again, _ = _rank(engine, v)
        assert (again.view(np.uint32) == first.view(np.uint32)).all()


def test_arguments(engine):
    import torch
    from correrender_amd import CorrFieldError
    empty, ranked = engine.rank_values(torch.empty(0, dtype=torch.float32, device="cuda"), return_ranked=True)
    assert empty.numel() == 0 and ranked == 0
    with pytest.raises(ValueError):
        engine.rank_values(torch.zeros(4, dtype=torch.float64, device="cuda"))
    v = torch.zeros(8, dtype=torch.float32, device="cuda")
    import ctypes as C
    code = engine._lib.crf_rank_values_device(engine._ctx, C.c_void_p(v.data_ptr()), 8, C.c_void_p(v.data_ptr() + 16), None)
    assert code == 1                                                     # CRF_ERR_ARGUMENT: the ranks overlap the values
    _check(engine, _normal(65), "after a refusal")
