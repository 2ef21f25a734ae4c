"""GPU: the range pipeline of the host-output entry point (crf_compute on a result of 8 MiB or more: up to 13 voxel ranges
alternating between two streams, api.cpp compute_to_host) with every kernel that WRITES scratch while it runs -- the
deferred-voxel list of the rank kernels and the blockIdx-indexed workspace of direct_rank_kernel / generic_kernel.  Ranges
in flight together must not share either.

One grid, 161 x 127 x 103 = 2 106 041 voxels: just above the 2^21 voxels at which the pipeline turns on, odd in every
dimension (ragged last range, ragged last wave).  Members are generated on the device; about a quarter of all voxels carry
a tie, so every range defers voxels to its list.  Every checked evaluation is preceded by a Pearson evaluation for another
reference point, because the staging buffer survives between calls: a voxel that the checked evaluation fails to write
then holds a wrong value, not the right one from an earlier identical evaluation.  The host result must equal the device
path's bit for bit on the whole field, and the oracle on a sample that covers every range seam and every planted class.

The mask voxels (all members equal) are compared with the oracle's own answer, never with a constant: bit patterns for
Pearson / Spearman / Kendall, parity.assert_close for the MI estimators.  Binned MI of a constant column is H - H in fp64,
a pure summation-order residue: measured on the MI355X, the kernels return 0.0 on all 456 mask voxels where the oracle
returns 1.08e-15 or 6.4e-16 (161 members, 150 bins) and -3.6e-16 (16 members, 80 bins) -- the 1e-16-level difference of
fp64 sums that kernels_binned.hip documents.  Kraskov MI agrees with the oracle bit for bit on them.

The host half (crf_host_copy.h) has its own switches -- fault mode, huge pages, range count, copier threads -- and its own
edge, the caller's destination (never touched, resident, not page-aligned): each goes through the checked evaluation once,
on the 16-member Pearson control."""
import re

import numpy as np
import pytest
import torch

import correrender_amd as ca
from correrender_amd import Measure
from parity import assert_bit_exact, assert_close, bit_identical
import oracle_lib

pytestmark = pytest.mark.gpu

XS, YS, ZS = 161, 127, 103
N = XS * YS * ZS
REF = (83, 63, 51)          # an ordinary voxel: in none of the planted classes
OTHER_REF = (20, 30, 40)    # reference point of the poisoning evaluation
MASK_A = (4096, 4352)       # all members equal: [4096, 4352) and the last 200 voxels
MASK_TAIL = 200

SPEARMAN = (Measure.SPEARMAN, oracle_lib.SPEARMAN)
KENDALL = (Measure.KENDALL, oracle_lib.KENDALL)


def _index(xyz, xs=XS, ys=YS):
    return (xyz[2] * ys + xyz[1]) * xs + xyz[0]


def _plant(m, n, near_ties, xp):
    """The planted classes, on a (cs, n) array of either library (xp: torch or numpy; both index alike)."""
    cs = m.shape[0]
    m[1, 0::5] = m[0, 0::5]                          # v % 5 == 0: a tie inside the first sorted chunk
    m[cs - 1, 1::15] = m[0, 1::15]                   # v % 15 == 1: a tie across the chunks
    if near_ties:                                    # v % 7 == 3: two values that agree in their upper 25 bits
        inf = xp.full_like(m[2, 3::7], float("inf"))
        m[3, 3::7] = xp.nextafter(m[2, 3::7], inf)
    for lo, hi in (MASK_A, (n - MASK_TAIL, n)):      # masks: all members equal
        m[:, lo:hi] = m[0:1, lo:hi] + 0          # (a copy: source and destination overlap)
    m[cs // 2, 7::1009] = float("nan")               # v % 1009 == 7
    return m


class _Data:
    def __init__(self, cs, near_ties=False):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(20261000 + cs)
        self.cs = cs
        self.members = _plant(torch.randn((cs, N), generator=gen, device="cuda", dtype=torch.float32), N, near_ties, torch)
        torch.cuda.synchronize()                     # the engine computes on its own streams
        self.secondary = None

    def columns(self, idx, source=None):
        src = self.members if source is None else source
        cols = src[:, torch.from_numpy(idx).cuda()].cpu().numpy()
        return np.ascontiguousarray(cols).reshape(self.cs, 1, 1, -1)


_cache = {}


def _data(engine, cs, near_ties=False):
    """The data set of one member count, bound to the engine.  One set is alive at a time (cases are grouped by cs)."""
    if _cache.get("cs") != cs:
        _cache.clear()
        torch.cuda.empty_cache()
        _cache.update(cs=cs, data=_Data(cs, near_ties))
    data = _cache["data"]
    engine.set_grid(XS, YS, ZS, cs)
    engine.bind_members(data.members)
    return data


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
    torch.cuda.empty_cache()


def _sample(range_lengths):
    ref = _index(REF)
    for cls, hit in ((5, 0), (15, 1), (1009, 7), (7, 3)):
        assert ref % cls != hit
    rng = np.random.default_rng(5)
    seams = np.cumsum(range_lengths)[:-1]
    parts = [rng.choice(N, size=20000, replace=False), [0, N - 1, ref],
             np.arange(*MASK_A), np.arange(N - MASK_TAIL, N)]
    parts += [np.arange(s - 70, s + 70) for s in seams]
    classes = {"tie5": np.arange(0, N, 5), "tie15": np.arange(1, N, 15), "nan": np.arange(7, N, 1009)}
    picked = {name: rng.choice(v, size=500, replace=False) for name, v in classes.items()}
    idx = np.unique(np.concatenate(parts + list(picked.values()))).astype(np.int64)
    return idx, picked["nan"]


def _evaluate_checked(engine, oracle, data, capfd, monkeypatch, measure, om, *, exact=True, kw=None, okw=None, env=None,
                      ref_values=None, kernel=None, expect=lambda f: f, what="", out=None, ranges=None, copier_threads=None):
    """One checked evaluation (module docstring); returns the host field.
    out: the caller's destination (default: a new array); ranges, copier_threads: what the trace must report."""
    kw, okw = dict(kw or {}), dict(okw or {})
    what = f"{what or measure.name} cs={data.cs}"
    # 1. poison the staging buffer
    poison = engine.compute(Measure.PEARSON, OTHER_REF).reshape(-1)
    # 2. the evaluation, traced
    monkeypatch.setenv("CRF_HOST_TRACE", "1")
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    capfd.readouterr()
    where = dict(reference_values=ref_values) if ref_values is not None and "reference_from_secondary" not in kw else {}
    ref = None if where else REF
    if out is not None:
        kw["out"] = out
    host = engine.compute(measure, ref, **where, **kw).reshape(-1)
    kw.pop("out", None)
    assert out is None or np.shares_memory(host, out)
    trace = capfd.readouterr().err
    host_kernel = engine.last_kernel_name()
    monkeypatch.delenv("CRF_HOST_TRACE")
    for name in env or {}:
        monkeypatch.delenv(name)
    # 3. the pipeline ran
    landed = re.findall(r"crf_compute: range (\d+) \((\d+) voxels\) landed", trace)
    assert len(landed) >= 2, f"{what}: the range pipeline did not run:\n{trace}"
    assert [int(j) for j, _ in landed] == list(range(len(landed)))
    lengths = [int(v) for _, v in landed]
    assert sum(lengths) == N
    if ranges is not None:
        assert len(landed) == ranges, f"{what}: {len(landed)} ranges:\n{trace}"
    if copier_threads is not None:
        assert f"({len(landed)} ranges, {copier_threads} copier threads)" in trace, f"{what}:\n{trace}"
    # 4. the device path, one launch
    dev = torch.full((N,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    engine.compute_device(measure, dev, ref, **where, **kw)
    torch.cuda.synchronize()
    if kernel:
        assert (host_kernel, engine.last_kernel_name()) == (kernel, kernel), what
    # 5. bit for bit, the whole field
    assert_bit_exact(host, dev.cpu().numpy(), f"{what}: ranged host output vs device output")
    # 6. the oracle on the sample
    idx, nan_idx = _sample(lengths)
    if ref_values is None:
        ref_values = data.members[:, _index(REF)].cpu().numpy()
    want = expect(oracle.field(om, data.columns(idx), ref_values, **okw))
    (assert_bit_exact if exact else assert_close)(host[idx], want, f"{what}: ranged host output vs oracle (sample)")
    # 7. NaN voxels, masks, and the poison was a poison
    assert np.isnan(host[nan_idx]).all(), what
    masks = np.concatenate([np.arange(*MASK_A), np.arange(N - MASK_TAIL, N)])
    (assert_bit_exact if exact else assert_close)(host[masks], want[np.searchsorted(idx, masks)],
                                                  f"{what}: mask voxels vs oracle")
    finite = np.isfinite(host)
    assert not (bit_identical(host, poison) & finite).any(), f"{what}: a result equals the poisoning field"
    return host


RANK_CASES = [(24, "spearman_split_kernel", "kendall_split_kernel"), (64, "spearman_u32_kernel", "kendall_split_kernel"),
              (100, "spearman_u32_kernel", "kendall_split_kernel"), (130, "spearman_pair_kernel", "kendall_pair_kernel"),
              (257, "direct_rank_kernel", "direct_rank_kernel")]


@pytest.mark.parametrize("which", [0, 1], ids=["spearman", "kendall"])
@pytest.mark.parametrize("cs,spearman_kernel,kendall_kernel", RANK_CASES, ids=[f"cs{c[0]}" for c in RANK_CASES])
def test_ranged_rank_measures(engine, oracle, capfd, monkeypatch, cs, spearman_kernel, kendall_kernel, which):
    """First pass + list pass per range (24, 64, 100 members), the pair kernels whose list is walked by direct_rank_kernel
    with Spearman's workspace (130), direct_rank_kernel for every voxel (257: workspace slices)."""
    data = _data(engine, cs, near_ties=cs == 64)
    measure, om = (SPEARMAN, KENDALL)[which]
    _evaluate_checked(engine, oracle, data, capfd, monkeypatch, measure, om, kernel=(spearman_kernel, kendall_kernel)[which])


def test_ranged_kendall_absolute_value(engine, oracle, capfd, monkeypatch):
    """CRF_FLAG_ABSOLUTE_VALUE: results in HBM + DMA, launch_abs per range."""
    data = _data(engine, 64, near_ties=True)
    _evaluate_checked(engine, oracle, data, capfd, monkeypatch, *KENDALL, kw=dict(absolute_value=True), expect=np.abs,
                      kernel="kendall_split_kernel", what="|Kendall|")


def test_ranged_kendall_dma_path(engine, oracle, capfd, monkeypatch):
    data = _data(engine, 64, near_ties=True)
    _evaluate_checked(engine, oracle, data, capfd, monkeypatch, *KENDALL, env={"CRF_HOST_PATH": "dma"},
                      kernel="kendall_split_kernel", what="Kendall, CRF_HOST_PATH=dma")


def test_ranged_spearman_host_reference_vector_with_ties(engine, oracle, capfd, monkeypatch):
    data = _data(engine, 64, near_ties=True)
    vec = np.round(data.members[:, _index(REF)].cpu().numpy() * 3)
    assert np.unique(vec).size < vec.size
    _evaluate_checked(engine, oracle, data, capfd, monkeypatch, *SPEARMAN, ref_values=vec, kernel="spearman_u32_kernel",
                      what="Spearman, tied host reference vector")


def test_ranged_spearman_reference_from_secondary(engine, oracle, capfd, monkeypatch):
    data = _data(engine, 64, near_ties=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)
    secondary = torch.randn((64, N), generator=gen, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    engine.bind_secondary_members(secondary)
    vec = secondary[:, _index(REF)].cpu().numpy()
    _evaluate_checked(engine, oracle, data, capfd, monkeypatch, *SPEARMAN, kw=dict(reference_from_secondary=True),
                      ref_values=vec, kernel="spearman_u32_kernel", what="Spearman, reference from the secondary field")


def test_ranged_spearman_one_stream_equals_two_streams(engine, oracle, capfd, monkeypatch):
    data = _data(engine, 64, near_ties=True)
    two = _evaluate_checked(engine, oracle, data, capfd, monkeypatch, *SPEARMAN, kernel="spearman_u32_kernel")
    one = _evaluate_checked(engine, oracle, data, capfd, monkeypatch, *SPEARMAN, env={"CRF_HOST_STREAMS": "1"},
                            kernel="spearman_u32_kernel", what="Spearman, CRF_HOST_STREAMS=1")
    assert_bit_exact(one, two, "one stream vs two streams")


def test_ranged_binned_mi_tile_in_the_workspace(engine, oracle, capfd, monkeypatch):
    """161 members, 150 bins: the histogram kernel declines, generic_kernel keeps its tile in the global workspace."""
    data = _data(engine, 161)
    mm = engine.member_minmax()
    _evaluate_checked(engine, oracle, data, capfd, monkeypatch, Measure.MUTUAL_INFORMATION_BINNED, oracle_lib.MI_BINNED,
                      exact=False, kw=dict(num_bins=150, minmax_ref=mm, minmax_query=mm),
                      okw=dict(num_bins=150, minmax_ref=mm), kernel="generic_kernel")


@pytest.mark.parametrize("name", ["pearson", "binned", "kraskov"])
def test_ranged_scratch_free_controls(engine, oracle, capfd, monkeypatch, name):
    """16 members: kernels that write no scratch -- every measure family has been through the ranges once."""
    data = _data(engine, 16)
    if name == "pearson":
        _evaluate_checked(engine, oracle, data, capfd, monkeypatch, Measure.PEARSON, oracle_lib.PEARSON)
    elif name == "binned":
        mm = engine.member_minmax()
        _evaluate_checked(engine, oracle, data, capfd, monkeypatch, Measure.MUTUAL_INFORMATION_BINNED, oracle_lib.MI_BINNED,
                          exact=False, kw=dict(num_bins=80, minmax_ref=mm, minmax_query=mm),
                          okw=dict(num_bins=80, minmax_ref=mm))
    else:
        _evaluate_checked(engine, oracle, data, capfd, monkeypatch, Measure.MUTUAL_INFORMATION_KRASKOV,
                          oracle_lib.MI_KRASKOV, exact=False, kw=dict(k=3), okw=dict(k=3))


# ---- the host half's switches (crf_host_copy.h), each through the real pipeline once -----------------------------------
# The 16-member Pearson control: no scratch, the least GPU work per case.  Which copier finds which range landed already
# is a matter of timing here; tests/test_host_copy.py scripts those schedules on the CPU.
SENTINEL = np.float32(-3.0)


def _destination(kind):
    """(out, check): the array handed to compute and what must hold of its surroundings afterwards."""
    if kind == "fresh":
        return np.empty(N, dtype=np.float32), lambda: None
    if kind == "written":
        return np.full(N, SENTINEL, dtype=np.float32), lambda: None
    assert kind == "page_plus_4"
    whole = np.full(N + 4096, SENTINEL, dtype=np.float32)
    start = (-whole.ctypes.data % 4096) // 4 + 1
    out = whole[start:start + N]
    assert out.ctypes.data % 4096 == 4 and out.flags["C_CONTIGUOUS"]

    def untouched_around():
        assert (whole[:start] == SENTINEL).all() and (whole[start + N:] == SENTINEL).all(), "written outside the destination"
    return out, untouched_around


@pytest.mark.parametrize("destination", ["fresh", "written", "page_plus_4"])
@pytest.mark.parametrize("fault", ["0", "1", "2"])
def test_ranged_host_fault_modes_and_destinations(engine, oracle, capfd, monkeypatch, fault, destination):
    """CRF_HOST_FAULT 0 (the copy faults the pages in), 1 (touched ahead), 2 (populated ahead) into a never-touched
    array, a resident one, and one that starts one float past a page boundary inside a larger array."""
    data = _data(engine, 16)
    out, check = _destination(destination)
    host = _evaluate_checked(engine, oracle, data, capfd, monkeypatch, Measure.PEARSON, oracle_lib.PEARSON, out=out,
                             env={"CRF_HOST_FAULT": fault}, what=f"Pearson, CRF_HOST_FAULT={fault}, {destination} destination")
    assert host.ctypes.data == out.ctypes.data
    check()


def test_ranged_host_no_huge_pages(engine, oracle, capfd, monkeypatch):
    data = _data(engine, 16)
    _evaluate_checked(engine, oracle, data, capfd, monkeypatch, Measure.PEARSON, oracle_lib.PEARSON,
                      out=np.empty(N, dtype=np.float32), env={"CRF_HOST_HUGEPAGE": "0"}, what="Pearson, CRF_HOST_HUGEPAGE=0")


@pytest.mark.parametrize("name,value,ranges", [("CRF_HOST_CHUNKS", "2", 2), ("CRF_HOST_CHUNKS", "16", 16),
                                               ("CRF_HOST_SHARES", "32,32", 2)], ids=["chunks2", "chunks16", "shares32_32"])
def test_ranged_host_range_counts(engine, oracle, capfd, monkeypatch, name, value, ranges):
    """Another partition.  A context keeps its partition until the grid is set again, so the variable is set before
    _data sets the grid (the poisoning evaluation builds the partition), and the grid is set once more afterwards."""
    try:
        with monkeypatch.context() as m:
            m.setenv(name, value)
            data = _data(engine, 16)
            _evaluate_checked(engine, oracle, data, capfd, monkeypatch, Measure.PEARSON, oracle_lib.PEARSON, ranges=ranges,
                              what=f"Pearson, {name}={value}")
    finally:
        _data(engine, 16)


@pytest.mark.parametrize("threads", [1, 3])
def test_ranged_host_copier_threads(engine, oracle, capfd, monkeypatch, threads):
    """CRF_COPY_THREADS is read when a context builds its pool: a context of its own."""
    data = _data(engine, 16)
    monkeypatch.setenv("CRF_COPY_THREADS", str(threads))
    own = ca.CorrField(0)
    try:
        own.set_grid(XS, YS, ZS, 16)
        own.bind_members(data.members)
        _evaluate_checked(own, oracle, data, capfd, monkeypatch, Measure.PEARSON, oracle_lib.PEARSON,
                          copier_threads=threads, what=f"Pearson, CRF_COPY_THREADS={threads}")
    finally:
        own.close()


def test_group_of_two_ranged_slabs(engine):
    """CorrFieldGroup([0, 0]) on 161 x 127 x 206: both slabs are 2 106 041 voxels, so each context runs the range pipeline
    with first pass + list.  24 host volumes with the same planting; the group's host result equals the single context's
    device result bit for bit."""
    _cache.clear()
    torch.cuda.empty_cache()
    cs, zs = 24, 2 * ZS
    n = XS * YS * zs
    rng = np.random.default_rng(20261024)
    ens = _plant(rng.standard_normal((cs, n), dtype=np.float32), n, False, np)
    ref = (83, 63, 51 + ZS)                      # in the second slab
    engine.set_grid(XS, YS, zs, cs)
    engine.upload_members(ens)
    dev = torch.empty(n, dtype=torch.float32, device="cuda")
    with ca.CorrFieldGroup([0, 0]) as grp:
        grp.set_grid(XS, YS, zs, cs)
        assert [grp.slab(s)[1] for s in range(2)] == [ZS, ZS]
        grp.upload_members(ens)
        for measure, kernel in ((Measure.SPEARMAN, "spearman_split_kernel"), (Measure.KENDALL, "kendall_split_kernel")):
            dev.fill_(-7.0)
            torch.cuda.synchronize()
            engine.compute_device(measure, dev, ref)
            torch.cuda.synchronize()
            assert engine.last_kernel_name() == kernel
            grp.compute(Measure.PEARSON, (20, 30, 40))               # poison both slabs' staging buffers
            assert_bit_exact(grp.compute(measure, ref), dev.cpu().numpy(), f"group of two ranged slabs, {measure.name}")
