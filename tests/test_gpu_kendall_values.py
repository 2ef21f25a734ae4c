"""GPU: crf_kendall_values_device / CorrField.kendall_values -- Kendall's tau-b of two device arrays over all pairs without
a NaN (kernels_kendall_similarity.hip: two device-wide sorts, a tile kernel and merge levels that count inversions).
Everything is exact: the integers (n, n0, n1, n2, S) equal those of kendall_similarity_reference.kendall_restated, which
tests/test_kendall_restatement.py pins to the reference's object code, and the value has the bits of the restated
<int64_t> tail.  No tolerance anywhere.

Sizes: a tile of the inversion count holds 256 values by default and a merge chunk up to 2048 (4097 values: 17 tiles, five
levels, the last run one value); CRF_KENDALL_TILE_KEYS lowers the tile so that 4097 values are 65 runs and seven levels, CRF_RANK_TILE_KEYS does
the same for the sort and the run starts, and CRF_SIMILARITY_MAX_BLOCKS caps the persistent grids."""
import functools

import numpy as np
import pytest

from kendall_similarity_reference import f32_bits, kendall_restated, pin_pair
from rank_similarity_reference import PIN_KINDS

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 257, 4095, 4096, 4097, 20435)
MANY_TILES = 20435


def _nan_either_side(n):
    rng = np.random.default_rng(800 + n)
    x, y = pin_pair("tied", n)
    x[rng.random(n) < 0.1] = np.float32(np.nan)
    y[rng.random(n) < 0.1] = np.float32(-np.nan)                          # either sign of NaN
    return x, y


def _mostly_nan(n):
    """Half the pairs have a NaN: at 4097 values and up that is several whole tiles of them, and many 64-value runs."""
    rng = np.random.default_rng(900 + n)
    x, y = pin_pair("continuous", n)
    x[rng.random(n) < 0.3] = np.float32(np.nan)
    y[rng.random(n) < 0.3] = np.float32(np.nan)
    return x, y


KINDS = {**{kind: functools.partial(pin_pair, kind) for kind in PIN_KINDS}, "nan_either_side": _nan_either_side,
         "mostly_nan": _mostly_nan}


@functools.lru_cache(maxsize=None)
def _case(kind, n):
    """The data of a case and what the restatement makes of it: computed once, shared by every test that uses the case."""
    x, y = KINDS[kind](n)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, kendall_restated(x, y)


def _call(engine, x, y):
    import torch
    tx, ty = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda()
    value, kept, counts = engine.kendall_values(tx, ty, return_counts=True)
    if x.size:
        assert engine.last_kernel_name() == "similarity_kendall_merge_kernel"
    return value, kept, counts


def _check(engine, x, y, want, what):
    value, kept, counts = _call(engine, x, y)
    print(f"[kendall values] {what}: kept {kept} counts {counts} value {value!r}; restated {want}")
    assert kept == want[0], what
    assert counts == want[1:5], what
    assert f32_bits(value) == want[5], what


@pytest.mark.parametrize("kind", list(KINDS))
def test_sizes(engine, kind):
    for n in SIZES:
        x, y, want = _case(kind, n)
        _check(engine, x, y, want, f"{kind} n={n}")


@pytest.mark.parametrize("n", [2, 65, 4097, MANY_TILES])
def test_monotone_sequences(engine, n):
    x = np.arange(n, dtype=np.float32) - np.float32(n // 2)
    n0 = n * (n - 1) // 2
    want_up, want_down = kendall_restated(x, x * 3), kendall_restated(x, -x)
    assert want_up[1:5] == (n0, 0, 0, 0) and want_down[1:5] == (n0, 0, 0, n0)
    _check(engine, x, (x * 3).astype(np.float32), want_up, f"ascending n={n}")
    _check(engine, x, -x, want_down, f"descending n={n}")
    assert _call(engine, x, x * 3)[0] == 1.0 and _call(engine, x, -x)[0] == -1.0


def test_constant_x(engine):
    for n in (3, 4097):
        _, y, _ = _case("continuous", n)
        x = np.full(n, np.float32(-7.5))
        want = kendall_restated(x, y)
        assert want[2] == want[1] and want[4] == 0                          # every pair ties in x; y is sorted among them
        _check(engine, x, y, want, f"constant x n={n}")
        assert np.isnan(_call(engine, x, y)[0])
        assert np.isnan(_call(engine, y, x)[0])


def test_x_is_y(engine):
    import torch
    x, _, _ = _case("zeros", MANY_TILES)
    want = kendall_restated(x, x)
    assert want[2] == want[3] and want[4] == 0
    t = torch.from_numpy(np.array(x)).cuda()
    value, kept, counts = engine.kendall_values(t, t, return_counts=True)
    assert (kept, *counts, f32_bits(value)) == want


def test_doubling_keeps_the_bits(engine):
    x, _, _ = _case("infinite", MANY_TILES)
    same, doubled = _call(engine, x, x), _call(engine, x, (2.0 * x).astype(np.float32))
    assert doubled[1:] == same[1:] and f32_bits(doubled[0]) == f32_bits(same[0])


@pytest.mark.parametrize("n", [4097, 4160])
def test_sixty_five_runs(engine, monkeypatch, n):
    """Runs of 64: 65 of them, odd at every level but one; the last run holds one value (4097) or is full (4160)."""
    monkeypatch.setenv("CRF_KENDALL_TILE_KEYS", "64")
    monkeypatch.setenv("CRF_RANK_TILE_KEYS", "64")
    for kind in KINDS:
        if n == 4097:
            x, y, want = _case(kind, n)
        else:
            x, y = KINDS[kind](n)
            want = kendall_restated(x, y)
        _check(engine, x, y, want, f"{kind} n={n} runs of 64")
    x = np.arange(n, dtype=np.float32)
    _check(engine, x, -x, kendall_restated(x, -x), f"descending n={n} runs of 64")


@pytest.mark.parametrize("cap", [1, 5])
def test_capped_grids(engine, monkeypatch, cap):
    """One block walks every tile and every chunk of every level, or five blocks do unevenly."""
    monkeypatch.setenv("CRF_KENDALL_TILE_KEYS", "64")
    monkeypatch.setenv("CRF_RANK_TILE_KEYS", "64")
    monkeypatch.setenv("CRF_SIMILARITY_MAX_BLOCKS", str(cap))
    for kind in ("continuous", "tied", "mostly_nan"):
        x, y, want = _case(kind, MANY_TILES)
        _check(engine, x, y, want, f"{kind} n={MANY_TILES} cap={cap}")
    monkeypatch.delenv("CRF_KENDALL_TILE_KEYS")
    monkeypatch.delenv("CRF_RANK_TILE_KEYS")
    x, y, want = _case("tied", MANY_TILES)
    _check(engine, x, y, want, f"tied n={MANY_TILES} cap={cap} default tiles")


def test_counts_beyond_32_bits(engine):
    """262 144 values, y descending in x: S = n0 = 34 359 607 296; the last level is one merge of two runs of 131 072,
    which alone adds 2^34."""
    n = 262144
    x = np.arange(n, dtype=np.float32)
    n0 = n * (n - 1) // 2
    assert n0 > 1 << 34
    value, kept, counts = _call(engine, x, -x)
    assert kept == n and counts == (n0, 0, 0, n0) and value == -1.0


def test_the_same_call_gives_the_same_bits_and_leaves_its_inputs(engine, monkeypatch):
    import torch
    monkeypatch.setenv("CRF_KENDALL_TILE_KEYS", "64")
    x, y, want = _case("nan_either_side", MANY_TILES)
    tx, ty = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda()
    for _ in range(3):
        value, kept, counts = engine.kendall_values(tx, ty, return_counts=True)
        assert (kept, *counts, f32_bits(value)) == want
    assert (tx.cpu().numpy().view(np.uint32) == x.view(np.uint32)).all()
    assert (ty.cpu().numpy().view(np.uint32) == y.view(np.uint32)).all()


def test_arguments(engine):
    import torch
    empty = torch.empty(0, dtype=torch.float32, device="cuda")
    value, kept, counts = engine.kendall_values(empty, empty, return_counts=True)
    assert np.isnan(value) and kept == 0 and counts == (0, 0, 0, 0)
    assert np.isnan(engine.kendall_values(empty, empty))
    v = torch.zeros(4, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        engine.kendall_values(v, torch.zeros(4, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        engine.kendall_values(v, torch.zeros(5, dtype=torch.float32, device="cuda"))
    x, y, want = _case("continuous", 65)
    _check(engine, x, y, want, "after a refusal")
