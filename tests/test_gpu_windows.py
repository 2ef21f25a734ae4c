"""GPU: windowed evaluation.  A grid whose member volumes are 4 GiB or more is evaluated in windows (api.cpp: ensure_windows,
NarrowScope::select_window, for_each_window, compute_impl, run_windowed; the arithmetic: crf_windows.h), and only the 1024^3
test of test_gpu_fullsize.py reaches that code at its real size.  CRF_WINDOW_VOXELS, read by crf_set_grid, gives a small
grid windows, and this module sends every windowed route through them.

One grid, 67 x 61 x 53 = 216 611 voxels, odd in every dimension, under a window of 65 536 voxels: four windows, seams at
65 536, 131 072 and 196 608, the last window of 20 003 voxels = 312 waves and 35 lanes (ragged at the window level and at
the wave level).  Members are generated on the device and planted with the classes of test_gpu_host_ranges.py, so that every
window holds all of them: ties inside a sorted chunk (v % 5 == 0) and across chunks (v % 15 == 1) on about a quarter of
the voxels -- every window's deferred-voxel list is non-empty, and a counter carried over from the window before would show
--, near-ties that agree in their upper 25 bits (v % 7 == 3, at 50 and 100 members), a mask (all members equal) that
straddles the first seam, [65 400, 65 700), a second one on the last 200 voxels, and a NaN in one member every 1009 voxels.
The reference point lies in the last window.

Every checked evaluation is compared with
  1. the oracle on a sample of about 5 500 voxels (the other 211 000 are left to check 2): every seam +- 70 voxels, voxel 0,
     the last 200 voxels, the reference voxel, the whole seam-straddling mask, 100 voxels of every planted class out of
     every window, 3 000 random voxels -- bit for bit for Pearson / Spearman / Kendall and the reductions the oracle
     restates exactly, parity.assert_close for the MI and DKL families;
  2. the same call on the same members with the variable unset (window_count() == 1), bit for bit on the whole field with
     NaN equal to NaN: the ordinary route's kernels are pinned to the oracle by the rest of the suite;
  3. the output itself: it is a view into a larger tensor, 1024 elements on either side, all of it filled with -7.0 before
     every evaluation; afterwards no -7.0 remains in the field and both guards are untouched (a window offset applied
     twice, or `out + first` in the wrong unit, writes there).
Every case asserts window_count() before it evaluates.

The engine fixture is session-wide and the window size is captured by set_grid: every test here sets the variable through
monkeypatch around its own set_grid only, so it is restored when the test ends, and every test of the suite begins with a
set_grid of its own -- nothing of this module outlives a test.

Measured on an MI355X: the 29 cases of the file take 5 s together (pytest's own figure; the slowest, the one-reference
field at 300 members with its oracle calls, 0.8 s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import correrender_amd as ca
from correrender_amd import CorrFieldError, Measure
from correrender_amd.engine import default_kraskov_k
from parity import assert_bit_exact, assert_close, bit_identical
from test_gpu_member_formats import convert, to_device_members
from test_two_vector_route import two_vector_rule
import oracle_lib

pytestmark = pytest.mark.gpu

ENV = "CRF_WINDOW_VOXELS"
XS, YS, ZS = 67, 61, 53
N = XS * YS * ZS
WINDOW = 65536
WINDOWS = 4
SEAMS = (65536, 131072, 196608)
REF = (33, 30, 50)          # voxel 206 393: the last window, in none of the planted classes
OTHER = (20, 30, 10)        # voxel 42 900: the first window; poisoning evaluations, second reference vector (has a tie)
MASK_A = (65400, 65700)     # all members equal, across the first seam
MASK_TAIL = 200
SENTINEL = -7.0
GUARD = 1024

PEARSON = (Measure.PEARSON, oracle_lib.PEARSON)
SPEARMAN = (Measure.SPEARMAN, oracle_lib.SPEARMAN)
KENDALL = (Measure.KENDALL, oracle_lib.KENDALL)
BINNED = (Measure.MUTUAL_INFORMATION_BINNED, oracle_lib.MI_BINNED)
KRASKOV = (Measure.MUTUAL_INFORMATION_KRASKOV, oracle_lib.MI_KRASKOV)
BINNED_CC = (Measure.BINNED_MI_CORRELATION_COEFFICIENT, oracle_lib.BINNED_MI_CC)
KMI_CC = (Measure.KMI_CORRELATION_COEFFICIENT, oracle_lib.KMI_CC)


def _index(xyz, xs=XS, ys=YS):
    return (xyz[2] * ys + xyz[1]) * xs + xyz[0]


assert N == 216611 and N - 3 * WINDOW == 20003 == 312 * 64 + 35
assert _index(REF) >= SEAMS[-1] and _index(REF) < N - MASK_TAIL and _index(OTHER) < SEAMS[0]


def _plant(m, near_ties):
    """The planted classes on a (cs, N) tensor (module docstring)."""
    cs = m.shape[0]
    m[1, 0::5] = m[0, 0::5]                          # v % 5 == 0: a tie inside the first sorted chunk
    m[cs - 1, 1::15] = m[0, 1::15]                   # v % 15 == 1: a tie across the chunks
    if near_ties:                                    # v % 7 == 3: two values that agree in their upper 25 bits
        m[3, 3::7] = torch.nextafter(m[2, 3::7], torch.full_like(m[2, 3::7], float("inf")))
    for lo, hi in (MASK_A, (N - MASK_TAIL, N)):      # masks: all members equal
        m[:, lo:hi] = m[0:1, lo:hi] + 0
    m[cs // 2, 7::1009] = float("nan")               # v % 1009 == 7
    return m


def _randn(cs, seed):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return torch.randn((cs, N), generator=gen, device="cuda", dtype=torch.float32)


class _Data:
    def __init__(self, cs):
        self.cs = cs
        self.near_ties = cs in (50, 100)
        self.members = _plant(_randn(cs, 20261020 + cs), self.near_ties)
        torch.cuda.synchronize()                     # the engine computes on its own streams
        self._secondary = None
        self.idx = _sample(self.near_ties)
        self.cols = self.columns(self.members)

    @property
    def secondary(self):
        """A second field, correlated with the first, with ties of its own; NaN where the first has one."""
        if self._secondary is None:
            s = 0.6 * self.members + 0.8 * _randn(self.cs, 77 + self.cs)
            s[1, 2::5] = s[0, 2::5]
            self._secondary = s.contiguous()
            torch.cuda.synchronize()
        return self._secondary

    def columns(self, source):
        cols = source[:, torch.from_numpy(self.idx).cuda()].float().cpu().numpy()
        return np.ascontiguousarray(cols).reshape(source.shape[0], 1, 1, -1)

    def vector(self, xyz, source=None):
        return (self.members if source is None else source)[:, _index(xyz)].cpu().numpy().copy()


def _sample(near_ties=False):
    ref = _index(REF)
    for cls, hit in ((5, 0), (15, 1), (1009, 7), (7, 3)):
        assert ref % cls != hit                      # an ordinary voxel
    assert not MASK_A[0] <= ref < MASK_A[1]
    rng = np.random.default_rng(5)
    parts = [rng.choice(N, size=3000, replace=False), [0, ref, _index(OTHER)], np.arange(*MASK_A), np.arange(N - MASK_TAIL, N)]
    parts += [np.arange(s - 70, s + 70) for s in SEAMS]
    classes = [(5, 0), (15, 1), (1009, 7)] + ([(7, 3)] if near_ties else [])
    for w in range(WINDOWS):                         # every planted class out of every window
        lo, hi = w * WINDOW, min(N, (w + 1) * WINDOW)
        for cls, hit in classes:
            members_of_class = np.arange(lo + (hit - lo) % cls, hi, cls)
            assert members_of_class.size >= 19       # (NaN voxels: 19 in the last window, all taken)
            parts.append(rng.choice(members_of_class, size=min(100, members_of_class.size), replace=False))
    return np.unique(np.concatenate(parts)).astype(np.int64)


_cache = {}


def _data(cs):
    """The data set of one member count.  One set is alive at a time (cases are grouped by cs)."""
    if _cache.get("cs") != cs:
        _cache.clear()
        torch.cuda.empty_cache()
        _cache.update(cs=cs, data=_Data(cs))
    return _cache["data"]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
    torch.cuda.empty_cache()


def _set_grid(engine, monkeypatch, cs, window, grid=(XS, YS, ZS), count=None):
    """set_grid under CRF_WINDOW_VOXELS=window (None: unset); the variable is back to what it was on return."""
    with monkeypatch.context() as m:
        if window is None:
            m.delenv(ENV, raising=False)
        else:
            m.setenv(ENV, str(window))
        engine.set_grid(*grid, cs)
    if count is None:
        count = 1 if window is None else WINDOWS
    assert engine.window_count() == count


def _bind(engine, monkeypatch, data, window, secondary=False):
    _set_grid(engine, monkeypatch, data.cs, window)
    engine.bind_members(data.members)
    if secondary:
        engine.bind_secondary_members(data.secondary)
    assert engine.window_count() == (1 if window is None else WINDOWS)


class _Out:
    """The field as a view into a larger tensor (check 3 of the module docstring)."""

    def __init__(self, n=N):
        self.n = n
        self.whole = torch.empty(n + 2 * GUARD, dtype=torch.float32, device="cuda")
        self.field = self.whole[GUARD:GUARD + n]
        assert self.field.is_contiguous() and self.field.data_ptr() == self.whole.data_ptr() + 4 * GUARD

    def arm(self):
        self.whole.fill_(SENTINEL)
        torch.cuda.synchronize()                     # the engine computes on its own stream

    def run(self, call, what):
        self.arm()
        call(self.field)
        return self.check(what)

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.whole[:GUARD] == SENTINEL).all()), f"{what}: written in front of the output"
        assert bool((self.whole[GUARD + self.n:] == SENTINEL).all()), f"{what}: written behind the output"
        left = int((self.field == SENTINEL).sum())
        assert left == 0, f"{what}: {left} voxels were not written"
        return self.field.cpu().numpy().copy()


class _Eval:
    """One checked evaluation: call(engine, out tensor); want(): the oracle on data.idx (None: checks 2 and 3 only)."""

    def __init__(self, what, call, want=None, exact=True, launches=WINDOWS, kernel=None):
        self.what, self.call, self.want, self.exact, self.launches, self.kernel = what, call, want, exact, launches, kernel


def _field_eval(data, measure, om, what=None, kw=None, okw=None, ref=REF, ref_values=None, **how):
    """A one-reference field evaluation for the reference point, against oracle.field with that point's values."""
    kw, okw = dict(kw or {}), dict(okw or {})
    vec = data.vector(ref) if ref_values is None else ref_values

    def call(engine, out):
        engine.compute_device(measure, out, ref, **kw)

    def want(oracle):
        return oracle.field(om, data.cols, vec, **okw)
    return _Eval(what or f"{measure.name} cs={data.cs}", call, want, exact=om <= oracle_lib.KENDALL, **how)


def _run_pass(engine, out, evals, windowed, profiled=True):
    """Runs every evaluation on the grid that is set; returns [(field, kernel name)]."""
    results = []
    engine.take_kernel_time()
    engine.set_profiling(profiled)
    try:
        for ev in evals:
            what = f"{ev.what} ({'windowed' if windowed else 'one launch'})"
            field = out.run(lambda o: ev.call(engine, o), what)
            name = engine.last_kernel_name()
            if profiled:
                # api.cpp TimedLaunch: a field evaluation queues one event pair per launch of its per-voxel kernel (the
                # reference-side preparation queues none); run_windowed queues ONE pair for all its windows
                launches = engine.take_kernel_time()[1]
                assert launches == (ev.launches if windowed else 1), f"{what}: {launches} timed launches"
            results.append((field, name))
    finally:
        engine.set_profiling(False)
        engine.take_kernel_time()
    return results


def _check(oracle, data, evals, windowed, control):
    for ev, (got, name), (plain, plain_name) in zip(evals, windowed, control):
        assert name == plain_name and name, f"{ev.what}: windowed ran {name!r}, one launch ran {plain_name!r}"
        if ev.kernel:
            assert name == ev.kernel, f"{ev.what}: {name}"
        assert_bit_exact(got, plain, f"{ev.what}: windowed vs one launch, whole field")
        if ev.want is not None:
            want = ev.want(oracle)
            (assert_bit_exact if ev.exact else assert_close)(got[data.idx], want, f"{ev.what}: windowed vs oracle (sample)")


def _both(engine, oracle, monkeypatch, data, evals, secondary=False, between=None):
    """Checks 1-3 for every evaluation: all of them on the windowed grid, then all of them with the variable unset."""
    out = _Out()
    _bind(engine, monkeypatch, data, WINDOW, secondary)
    windowed = _run_pass(engine, out, evals, True)
    if between:
        between()
    _bind(engine, monkeypatch, data, None, secondary)
    control = _run_pass(engine, out, evals, False)
    _check(oracle, data, evals, windowed, control)
    return [w[0] for w in windowed]


# ---- one-reference field, fp32 members ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [16, 50, 100, 150, 300])
def test_windowed_one_reference_field_every_measure(engine, oracle, monkeypatch, cs):
    """16: register sorts; 50: the 33..64 split sort with its list; 100: 65..128; 150: the two-chunk merge; 300: the
    any-member-count kernels and pearson_split_kernel.  Default k and k = 3 for Kraskov, both estimators at 50 members."""
    data = _data(cs)
    _set_grid(engine, monkeypatch, cs, WINDOW)
    engine.bind_members(data.members)
    mm = engine.member_minmax()
    finite = data.members[~torch.isnan(data.members)]
    assert mm == (float(finite.min()), float(finite.max()))
    del finite
    bkw, bokw = dict(num_bins=80, minmax_ref=mm, minmax_query=mm), dict(num_bins=80, minmax_ref=mm)
    k0 = default_kraskov_k(cs)
    evals = [_field_eval(data, *PEARSON), _field_eval(data, *SPEARMAN), _field_eval(data, *KENDALL),
             _field_eval(data, *BINNED, kw=bkw, okw=bokw), _field_eval(data, *BINNED_CC, kw=bkw, okw=bokw),
             _field_eval(data, *KRASKOV, what=f"Kraskov default k={k0} cs={cs}", okw=dict(k=k0)),
             _field_eval(data, *KMI_CC, what=f"KMI-CC default k={k0} cs={cs}", okw=dict(k=k0))]
    if k0 != 3:
        evals.append(_field_eval(data, *KRASKOV, what=f"Kraskov k=3 cs={cs}", kw=dict(k=3), okw=dict(k=3)))
    if cs == 50:
        evals.append(_field_eval(data, *KRASKOV, what="Kraskov KSG-2 k=3 cs=50", kw=dict(k=3, kraskov_estimator_index=2),
                                 okw=dict(k=3, estimator=2)))
    got = _both(engine, oracle, monkeypatch, data, evals)
    assert float(got[0][_index(REF)]) == pytest.approx(1.0, abs=1e-6)
    nan_voxels = np.arange(7, N, 1009)
    for field in got:
        assert np.isnan(field[nan_voxels]).all()


@pytest.mark.parametrize("cs", [50, 100])
def test_windowed_pearson_never_reads_the_packed_copy(engine, oracle, monkeypatch, cs):
    """crf_set_member_layout(PACKED) packs at these member counts on an ordinary grid; a windowed grid reads the raw
    members.  Same field either way."""
    data = _data(cs)
    out = _Out()
    engine.set_member_layout("packed")
    try:
        ev = _field_eval(data, *PEARSON)
        _bind(engine, monkeypatch, data, WINDOW)
        windowed = out.run(lambda o: ev.call(engine, o), "Pearson, layout packed, windowed")
        assert engine.last_member_layout() == "raw"
        _bind(engine, monkeypatch, data, None)
        control = out.run(lambda o: ev.call(engine, o), "Pearson, layout packed, one launch")
        assert engine.last_member_layout() == "packed"
    finally:
        engine.set_member_layout("auto")
    assert_bit_exact(windowed, control, f"Pearson cs={cs}: windowed raw vs packed")
    assert_bit_exact(windowed[data.idx], ev.want(oracle), f"Pearson cs={cs}: windowed vs oracle (sample)")


# ---- reference sources --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["spearman", "binned"])
def test_windowed_reference_sources(engine, oracle, monkeypatch, which):
    """The reference point, a host vector, a device vector, the secondary members at a point of the last window, and
    prepared slots 0 and 5 (a phase-2-only call per window)."""
    data = _data(50)
    measure, om = SPEARMAN if which == "spearman" else BINNED
    exact = which == "spearman"
    _bind(engine, monkeypatch, data, WINDOW, secondary=True)
    mm, mm_s = engine.member_minmax(), engine.secondary_member_minmax()
    kw = {} if exact else dict(num_bins=80, minmax_ref=mm, minmax_query=mm)
    okw = {} if exact else dict(num_bins=80, minmax_ref=mm)
    kw_s = {} if exact else dict(num_bins=80, minmax_ref=mm_s, minmax_query=mm)
    okw_s = {} if exact else dict(num_bins=80, minmax_ref=mm_s, minmax_query=mm)
    vec = data.vector(OTHER)                                   # a vector with a tie of its own
    assert np.unique(vec).size < vec.size and np.isfinite(vec).all()
    dvec = torch.from_numpy(vec).cuda()
    sec_vec = data.vector(REF, data.secondary)
    assert np.isfinite(sec_vec).all()

    def want_for(values, o=okw):
        return lambda oracle_: oracle_.field(om, data.cols, values, **o)

    def prepared(slot, **source):
        def call(engine_, out):
            engine_.prepare_device(measure, slot, **source, **kw)
            engine_.compute_prepared_device(measure, [out], slot, **kw)
        return call

    evals = [
        _field_eval(data, measure, om, what=f"{which}: reference point", kw=kw, okw=okw),
        _Eval(f"{which}: host reference vector", lambda e, o: e.compute_device(measure, o, reference_values=vec, **kw),
              want_for(vec), exact),
        _Eval(f"{which}: device reference vector", lambda e, o: e.compute_device(measure, o, device_reference=dvec, **kw),
              want_for(vec), exact),
        _Eval(f"{which}: reference from the secondary members",
              lambda e, o: e.compute_device(measure, o, REF, reference_from_secondary=True, **kw_s), want_for(sec_vec, okw_s),
              exact),
        _Eval(f"{which}: prepared slot 0 (reference point)", prepared(0, ref=REF), want_for(data.vector(REF)), exact),
        _Eval(f"{which}: prepared slot 5 (device vector)", prepared(5, device_reference=dvec), want_for(vec), exact),
    ]
    got = _both(engine, oracle, monkeypatch, data, evals, secondary=True)
    assert not bit_identical(got[4], got[5]).all(), "the two prepared slots gave the same field"
    assert_bit_exact(got[4], got[0], "prepared slot 0 vs the reference point")
    assert_bit_exact(got[5], got[2], "prepared slot 5 vs the device vector")
    assert_bit_exact(got[1], got[2], "host vector vs device vector")


def test_windowed_prepare_rows_then_both_slots_in_one_call(engine, oracle, monkeypatch):
    """crf_prepare_rows_device into slots 5 and 6, crf_compute_prepared_device for both in one call."""
    data = _data(50)
    _bind(engine, monkeypatch, data, WINDOW)
    rows = torch.stack([data.members[:, _index(REF)], data.members[:, _index(OTHER)]]).contiguous()
    torch.cuda.synchronize()
    outs = [_Out(), _Out()]
    for o in outs:
        o.arm()
    engine.prepare_rows_device(Measure.SPEARMAN, rows, 5, 2)
    engine.compute_prepared_device(Measure.SPEARMAN, [o.field for o in outs], 5)
    for o, xyz in zip(outs, (REF, OTHER)):
        got = o.check(f"prepared rows, {xyz}")
        assert_bit_exact(got[data.idx], oracle.field(oracle_lib.SPEARMAN, data.cols, data.vector(xyz)),
                         f"Spearman from prepared rows, {xyz}")


def test_windowed_reference_gathers(engine, monkeypatch):
    data = _data(50)
    _bind(engine, monkeypatch, data, WINDOW)
    points = [OTHER, REF, (XS - 1, YS - 1, ZS - 1), (0, 0, 0)]
    for p in points:
        np.testing.assert_array_equal(engine.gather_reference(*p), data.vector(p))
    rows = torch.full((len(points) + 1, 50), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    engine.gather_reference_rows_device(points + [None], rows)
    torch.cuda.synchronize()
    got = rows.cpu().numpy()
    for r, p in enumerate(points):
        np.testing.assert_array_equal(got[r], data.vector(p))
    assert (got[-1] == 0).all()


# ---- symmetric mode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [16, 50, 150])
def test_windowed_symmetric_mode(engine, oracle, monkeypatch, cs):
    """compute_symmetric inside for_each_window, through the doubled table stride of window_has_secondary: the sorted
    kernels (16, 50 members) and the direct ones with their workspace (150)."""
    data = _data(cs)
    _bind(engine, monkeypatch, data, WINDOW, secondary=True)
    mm_a, mm_b = engine.member_minmax(), engine.secondary_member_minmax()
    sec_cols = data.columns(data.secondary)

    def sym(measure, om, kw=None, okw=None, exact=True):
        kw, okw = dict(kw or {}), dict(okw or {})
        rule = two_vector_rule(False, om, cs, kw.get("k", 0), kw.get("num_bins", 0))
        return _Eval(f"symmetric {measure.name} cs={cs}", lambda e, o: e.compute_device(measure, o, symmetric=True, **kw),
                     lambda oracle_: oracle_.symmetric_field(om, data.cols, sec_cols, **okw), exact, kernel=rule[1])

    evals = [sym(*PEARSON), sym(*SPEARMAN), sym(*KENDALL),
             sym(*BINNED, kw=dict(num_bins=20, minmax_ref=mm_a, minmax_query=mm_b),
                 okw=dict(num_bins=20, minmax_ref=mm_a, minmax_query=mm_b), exact=False),
             sym(*KRASKOV, kw=dict(k=3), okw=dict(k=3), exact=False)]
    _both(engine, oracle, monkeypatch, data, evals, secondary=True)


# ---- reductions through run_windowed -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [24, 150])
def test_windowed_reductions(engine, oracle, monkeypatch, cs):
    """Both ensemble statistics, the set predicate, DKL with both estimators (24 members: the sorting-network
    instantiations; 150: the counting-sort ones, which keep their columns in the workspace), the extrema."""
    data = _data(cs)
    _bind(engine, monkeypatch, data, WINDOW, secondary=True)
    for got, source in ((engine.member_minmax(), data.members), (engine.secondary_member_minmax(), data.secondary)):
        finite = source[~torch.isnan(source)]
        assert got == (float(finite.min()), float(finite.max()))
    k = default_kraskov_k(cs)
    lower, upper = cs // 4, cs // 2
    evals = [
        _Eval(f"ensemble mean cs={cs}", lambda e, o: e.ensemble_stat_device(0, o), lambda orc: orc.ensemble_stat(0, data.cols),
              launches=1),
        _Eval(f"ensemble spread cs={cs}", lambda e, o: e.ensemble_stat_device(1, o), lambda orc: orc.ensemble_stat(1, data.cols),
              launches=1),
        _Eval(f"set predicate > 0.25 in [{lower}, {upper}] cs={cs}",
              lambda e, o: e.set_predicate_device(">", 0.25, lower, upper, o),
              lambda orc: orc.set_predicate(0, 0.25, lower, upper, data.cols), launches=1),
        _Eval(f"DKL binned cs={cs}", lambda e, o: e.dkl_device("binned", o, num_bins=80),
              lambda orc: orc.dkl(0, data.cols, num_bins=80), exact=False, launches=1),
        _Eval(f"DKL k-NN k={k} cs={cs}", lambda e, o: e.dkl_device("knn", o, k=k), lambda orc: orc.dkl(1, data.cols, k=k),
              exact=False, launches=1),
    ]
    got = _both(engine, oracle, monkeypatch, data, evals, secondary=True)
    predicate = got[2][np.isfinite(got[2])]
    assert np.unique(predicate).size >= 2, "the predicate selects all voxels or none"


# ---- narrow members -----------------------------------------------------------------------------------------------------
def _narrow_members(fmt):
    """64 members of random codes with both masks (and, float16, the NaN class): (device tensor [64, N] whose rows are
    4-byte aligned, the float32 values the calculators see of them)."""
    cs = 64
    rng = np.random.default_rng({"u8": 1, "u16": 2, "f16": 3}[fmt])
    if fmt == "u8":
        narrow = rng.integers(0, 256, (cs, N), dtype=np.uint8)
    elif fmt == "u16":
        narrow = rng.integers(0, 65536, (cs, N), dtype=np.uint16)
    else:
        narrow = rng.standard_normal((cs, N), dtype=np.float32).astype(np.float16)
        narrow[cs // 2, 7::1009] = np.nan
    for lo, hi in (MASK_A, (N - MASK_TAIL, N)):
        narrow[:, lo:hi] = narrow[0:1, lo:hi]
    return to_device_members(narrow), convert(narrow)


@pytest.mark.parametrize("fmt", ["f16", "u16", "u8"])
def test_windowed_narrow_members(engine, oracle, monkeypatch, fmt):
    """Narrow members on a windowed grid: ensure_wide first, then window tables that point into the copy.  A reduction
    that is native on an ordinary grid comes first, so the copy appears before any table is built; the one-launch control
    on the same members reads them natively again."""
    cs = 64
    members, wide = _narrow_members(fmt)
    idx = _sample()
    cols = np.ascontiguousarray(wide[:, idx]).reshape(cs, 1, 1, -1)
    vec = wide[:, _index(REF)].copy()
    assert np.isfinite(vec).all()
    finite = wide[np.isfinite(wide)]
    mm = (float(finite.min()), float(finite.max()))
    bkw = dict(num_bins=80, minmax_ref=mm, minmax_query=mm)
    out = _Out()
    calls = [("ensemble mean", lambda o: engine.ensemble_stat_device(0, o), lambda: oracle.ensemble_stat(0, cols), True, False),
             ("Pearson", lambda o: engine.compute_device(Measure.PEARSON, o, REF),
              lambda: oracle.field(oracle_lib.PEARSON, cols, vec), True, True),
             ("Kendall", lambda o: engine.compute_device(Measure.KENDALL, o, REF),
              lambda: oracle.field(oracle_lib.KENDALL, cols, vec), True, True),
             ("binned MI", lambda o: engine.compute_device(Measure.MUTUAL_INFORMATION_BINNED, o, REF, **bkw),
              lambda: oracle.field(oracle_lib.MI_BINNED, cols, vec, num_bins=80, minmax_ref=mm), False, True),
             ("DKL binned", lambda o: engine.dkl_device("binned", o, num_bins=80), lambda: oracle.dkl(0, cols, num_bins=80),
              False, False)]
    results = {}
    for window in (WINDOW, None):
        _set_grid(engine, monkeypatch, cs, window)
        engine.bind_members(members)
        assert engine.member_format() == fmt and engine.wide_copy_bytes() == 0
        assert engine.member_minmax() == mm
        assert engine.wide_copy_bytes() == 0                       # the extrema read the members as stored
        for name, call, want, exact, is_field in calls:
            got = out.run(call, f"{fmt} {name} window={window}")
            if window is not None:
                assert engine.wide_copy_bytes() >= 4 * cs * N, f"{fmt} {name}: no fp32 copy on a windowed grid"
                if is_field:
                    assert engine.last_member_format() == "f32"
                (assert_bit_exact if exact else assert_close)(got[idx], want(), f"{fmt} {name}: windowed vs oracle (sample)")
                results[name] = got
            else:
                if is_field:                                           # native again, and no copy so far
                    assert engine.last_member_format() == fmt, f"{fmt} {name}: the control did not run natively"
                if name != "DKL binned":
                    assert engine.wide_copy_bytes() == 0
                assert_bit_exact(results[name], got, f"{fmt} {name}: windowed vs one launch, whole field")


# ---- invalidation of the window tables ----------------------------------------------------------------------------------
def test_windowed_tables_follow_the_members(engine, oracle, monkeypatch):
    """Replace the secondary members, the primary members, overwrite them in place, replace the secondary again, after the
    tables were built: every result follows the current members.  All tensors stay alive to the end, so a stale table
    reads wrong values, never freed memory."""
    cs = 16
    idx = _sample()
    didx = torch.from_numpy(idx).cuda()
    a, b, b2, s, s2 = (_randn(cs, 500 + i) for i in range(5))
    torch.cuda.synchronize()
    keep = [a, b, b2, s, s2]

    def cols(t):
        return np.ascontiguousarray(t[:, didx].cpu().numpy()).reshape(cs, 1, 1, -1)

    def vector(t):
        return t[:, _index(REF)].cpu().numpy().copy()

    out = _Out()

    def pearson(what, members, ref_source, **kw):
        got = out.run(lambda o: engine.compute_device(Measure.PEARSON, o, REF, **kw), what)
        assert_bit_exact(got[idx], oracle.field(oracle_lib.PEARSON, cols(members), vector(ref_source)), what)

    def symmetric(what, members, secondary):
        for measure, om in (PEARSON, SPEARMAN):
            got = out.run(lambda o: engine.compute_device(measure, o, symmetric=True), f"{what} {measure.name}")
            assert_bit_exact(got[idx], oracle.symmetric_field(om, cols(members), cols(secondary)), f"{what} {measure.name}")

    _set_grid(engine, monkeypatch, cs, WINDOW)
    engine.bind_members(a)
    pearson("members A, no secondary", a, a)
    engine.bind_secondary_members(s)
    assert engine.window_count() == WINDOWS
    pearson("members A, reference from secondary S", a, s, reference_from_secondary=True)
    symmetric("A against S", a, s)
    engine.bind_members(b)
    pearson("members B", b, b)
    symmetric("B against S", b, s)
    b.copy_(b2)
    torch.cuda.synchronize()
    engine.members_changed()
    pearson("members B overwritten in place", b2, b2)
    symmetric("B overwritten against S", b2, s)
    engine.bind_secondary_members(s2)
    symmetric("B overwritten against S2", b2, s2)
    pearson("reference from secondary S2", b2, s2, reference_from_secondary=True)
    assert engine.window_count() == WINDOWS
    del keep


# ---- host output --------------------------------------------------------------------------------------------------------
def test_windowed_host_output_and_absolute_value(engine, oracle, monkeypatch):
    """crf_compute on a windowed grid (no range pipeline: the context's result buffer, one copy) equals the device path
    bit for bit -- Pearson and one list-writing kernel --, a Pearson evaluation for another point in between; with
    CRF_FLAG_ABSOLUTE_VALUE every voxel of every window is |signed field|."""
    data = _data(50)
    out = _Out()
    _bind(engine, monkeypatch, data, WINDOW)
    for measure, om in (PEARSON, SPEARMAN):
        poison = engine.compute(Measure.PEARSON, OTHER).reshape(-1)
        host = engine.compute(measure, REF).reshape(-1)
        dev = out.run(lambda o: engine.compute_device(measure, o, REF), f"{measure.name} device")
        assert_bit_exact(host, dev, f"{measure.name}: windowed host output vs device output")
        assert_bit_exact(host[data.idx], oracle.field(om, data.cols, data.vector(REF)), f"{measure.name}: host output vs oracle")
        assert not (bit_identical(host, poison) & np.isfinite(host) & (np.abs(host) != 1.0)).any(), "a poison value survived"
        engine.compute(Measure.PEARSON, OTHER)
        host_abs = engine.compute(measure, REF, absolute_value=True).reshape(-1)
        dev_abs = out.run(lambda o: engine.compute_device(measure, o, REF, absolute_value=True), f"|{measure.name}| device")
        for got in (host_abs, dev_abs):
            assert_bit_exact(got, np.abs(host), f"|{measure.name}| on a windowed grid")
            assert (got[np.isfinite(got)] >= 0).all()
        assert (host[np.isfinite(host)] < 0).any()


# ---- the documented refusals --------------------------------------------------------------------------------------------
def test_windowed_refusals_leave_the_context_usable(engine, oracle, monkeypatch):
    data = _data(16)
    _bind(engine, monkeypatch, data, WINDOW)
    with pytest.raises(CorrFieldError, match="request mode") as e:
        engine.compute_requests(Measure.PEARSON, [[0, 0, 0, 1, 1, 1]])
    assert e.value.code == 4                                      # CRF_ERR_UNSUPPORTED
    linear = torch.zeros(N, dtype=torch.float32, device="cuda")
    tiled = torch.zeros(engine.tiled_element_count(), dtype=torch.float32, device="cuda")
    with pytest.raises(CorrFieldError, match="re-tiling") as e:
        engine.tile_field_device(linear, tiled)
    assert e.value.code == 4
    assert engine.window_count() == WINDOWS
    ev = _field_eval(data, *KENDALL)
    got = _Out().run(lambda o: ev.call(engine, o), "Kendall after the refusals")
    assert_bit_exact(got[data.idx], ev.want(oracle), "Kendall after the refusals")


# ---- the window size itself ---------------------------------------------------------------------------------------------
def _small_case(engine, oracle, monkeypatch, grid, window, count):
    xs, ys, zs = grid
    n, cs = xs * ys * zs, 16
    ens = _plant_small(np.random.default_rng(n).standard_normal((cs, n), dtype=np.float32))
    ref = (xs - 1, ys - 1, zs - 1)                               # the last voxel: the last window
    vec = ens[:, n - 1].copy()
    fields = {}
    for w in (window, None):
        _set_grid(engine, monkeypatch, cs, w, grid, count=count if w is not None else 1)
        engine.upload_members(ens)
        out = _Out(n)
        for measure, om in (PEARSON, KENDALL):
            got = out.run(lambda o: engine.compute_device(measure, o, ref), f"{measure.name} {grid} window={w}")
            fields[(measure, w)] = (got, engine.last_kernel_name())
            assert_bit_exact(got, oracle.field(om, ens, vec), f"{measure.name} {grid} window={w} vs oracle")
    for measure, _ in (PEARSON, KENDALL):
        assert fields[(measure, window)][1] == fields[(measure, None)][1] != ""
        assert_bit_exact(fields[(measure, window)][0], fields[(measure, None)][0], f"{measure.name} {grid}")


def _plant_small(ens):
    ens[1, 0::5] = ens[0, 0::5]
    ens[3, 11::97] = np.nan
    return ens


def test_window_of_1024_on_1025_voxels_last_window_of_one_voxel(engine, oracle, monkeypatch):
    _small_case(engine, oracle, monkeypatch, (5, 41, 5), 1024, 2)


def test_window_equal_to_the_grid_is_an_ordinary_grid(engine, oracle, monkeypatch):
    _small_case(engine, oracle, monkeypatch, (16, 16, 8), 2048, 1)


@pytest.mark.parametrize("value", ["-1", "1000", "1025", "1024abc"])
def test_rejected_window_sizes(engine, oracle, monkeypatch, value):
    engine.set_grid(8, 8, 4, 4)
    monkeypatch.setenv(ENV, value)
    with pytest.raises(CorrFieldError, match=ENV) as e:
        engine.set_grid(5, 41, 5, 16)
    assert e.value.code == 1                                      # CRF_ERR_ARGUMENT
    monkeypatch.delenv(ENV)
    _small_case(engine, oracle, monkeypatch, (5, 41, 5), 1024, 2)


# ---- a device group whose slabs are windowed -----------------------------------------------------------------------------
def test_group_of_two_windowed_slabs(engine, monkeypatch):
    """CorrFieldGroup([0, 0]) on 67 x 61 x 106: each slab is the grid of this module, four windows.  Host members with the
    same planting; the group's result equals a single context's one-launch device result bit for bit, the reference point
    in the last window of the second slab; one compute_batch of three points."""
    _cache.clear()
    torch.cuda.empty_cache()
    cs, zs = 50, 2 * ZS
    n = XS * YS * zs
    rng = np.random.default_rng(20261021)
    ens = rng.standard_normal((cs, n), dtype=np.float32)
    ens[1, 0::5] = ens[0, 0::5]
    ens[cs - 1, 1::15] = ens[0, 1::15]
    ens[:, N - 150:N + 150] = ens[0:1, N - 150:N + 150]           # a mask across the slab seam
    ens[cs // 2, 7::1009] = np.nan
    refs = [(REF[0], REF[1], REF[2] + ZS), OTHER, (XS - 1, YS - 1, ZS - 1)]
    _set_grid(engine, monkeypatch, cs, None, (XS, YS, zs))
    engine.upload_members(ens)
    dev = torch.empty(n, dtype=torch.float32, device="cuda")
    want = {}
    for measure in (Measure.PEARSON, Measure.SPEARMAN):
        for ref in refs:
            dev.fill_(SENTINEL)
            torch.cuda.synchronize()
            engine.compute_device(measure, dev, ref)
            torch.cuda.synchronize()
            want[(measure, ref)] = dev.cpu().numpy().copy()
    lib = ca.load_library()
    with ca.CorrFieldGroup([0, 0]) as grp:
        with monkeypatch.context() as m:
            m.setenv(ENV, str(WINDOW))
            grp.set_grid(XS, YS, zs, cs)
        assert [grp.slab(s)[1] for s in range(2)] == [ZS, ZS]
        for slot in range(2):
            assert lib.crf_window_count(C.c_void_p(lib.crf_group_context(grp._g, slot))) == WINDOWS
        grp.upload_members(ens)
        for measure in (Measure.PEARSON, Measure.SPEARMAN):
            grp.compute(Measure.PEARSON, OTHER)                    # another field in both slabs' result buffers
            got = grp.compute(measure, refs[0], out=np.full(n, SENTINEL, np.float32))
            assert_bit_exact(got, want[(measure, refs[0])], f"group of two windowed slabs, {measure.name}")
            outs = grp.compute_batch(measure, refs, outs=[np.full(n, SENTINEL, np.float32) for _ in refs])
            for ref, got in zip(refs, outs):
                assert_bit_exact(got, want[(measure, ref)], f"group of two windowed slabs, batch, {measure.name} {ref}")
