"""CPU: the inputs of tests/division_edge_inputs.py do what test_gpu_division_edges.py needs them for.

1. On every bin-edge lattice sample the kernels' own bin functions agree (query_bin_rcp == query_bin_div wherever a
   launcher takes the reciprocal form), and on every guard-edge vector that passes exact_div_guard the kernels' own
   exact_div is a / sd bit for bit (tests/native/division_edges.cpp, g++ -ffp-contract=off).
2. The inputs can fail a wrong kernel: dropping the correction (q = d * rcp alone) changes the bin of samples of every
   ordinary-range lattice, and ignoring the guard gives wrong quotients on the low-out and one-out families.  On high-out it
   cannot: a standard deviation just above 2^60 still has a normal, correctly rounded reciprocal and every product stays
   in range, so exact_div remains correctly rounded there -- the guard's upper bound is conservative -- and the test pins
   that as 0 wrong quotients instead.
3. The oracle's binned MI is finite and above 1e-3 at every voxel of every lattice case without plants, so
   parity.assert_close applies its pure relative bound everywhere.
4. On a subset, one member count per kernel family, the oracle is bit-identical to the reference's object code (skipped
   where oracle/_ref is absent; nothing is recorded for it)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import division_edge_inputs as dei
import oracle_lib
from parity import assert_bit_exact

ROOT = Path(__file__).resolve().parent.parent
ALL_RANGES = dei.ORDINARY_RANGES + [mm for mm, _ in dei.BOUNDARY_RANGES]
VECTOR_MEMBER_COUNTS = (2, 16, 17, 64, 81, 128, 340)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("division_edges") / "division_edges"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror",
                    f"-I{ROOT / 'correrender_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "division_edges.cpp"),
                    "-o", str(exe)], check=True)

    def run(records, path):
        with open(path, "wb") as f:
            for r in records:
                for part in r:
                    f.write(np.ascontiguousarray(part).tobytes())
        p = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = p.stdout.strip().splitlines()
        assert lines[-1] == f"OK division edges: {len(records)} records", p.stdout
        return [dict((k, int(v)) for k, v in re.findall(r"(\w+) (-?\d+)(?= |$)", ln.split(": ", 1)[1])) for ln in lines[:-1]]
    return run


def test_lattice_samples_rcp_equals_div_and_mutant_is_caught(program, tmp_path):
    cases, records = [], []
    for mm in ALL_RANGES:
        for nb in dei.NUM_BINS:
            ens = dei.lattice_case(64, mm, nb, plants=True)
            cases.append((mm, nb))
            records.append((np.int32(1), np.float32(mm[0]), np.float32(mm[1]), np.int32(nb), np.int64(ens.size), ens))
    for (mm, nb), r in zip(cases, program(records, tmp_path / "lattices.bin")):
        print(mm, nb, r)
        assert r["samples"] == 64 * 480
        assert r["rcp_form"] == int(dei.range_takes_rcp(mm)), (mm, nb)
        if r["rcp_form"]:
            assert r["rcp_vs_div"] == 0, f"range {mm} bins {nb}: {r['rcp_vs_div']} samples change their bin"
        if mm in dei.ORDINARY_RANGES:
            assert r["correction_dropped"] > 0, f"range {mm} bins {nb}: dropping the correction goes unnoticed"


def test_guard_vectors_exact_div_and_mutant_is_caught(program, tmp_path):
    n = 1024
    cases, records = [], []
    for cs in VECTOR_MEMBER_COUNTS:
        for name in dei.FAMILIES:
            ens = dei.guard_family(name, cs, n, seed=7)
            cases.append((cs, name))
            records.append((np.int32(2), np.int32(cs), np.int64(n), ens))
    for (cs, name), r in zip(cases, program(records, tmp_path / "vectors.bin")):
        print(cs, name, r)
        assert r["guarded"] == {"low-in": n, "high-in": n, "one-out": n - n // 64}.get(name, 0), (cs, name)
        assert r["wrong_guarded"] == 0, f"{name} cs={cs}: exact_div differs from a / sd under the guard"
        if name in ("low-out", "one-out") and cs >= 16:
            assert r["wrong_unguarded"] > 0, f"{name} cs={cs}: ignoring the guard goes unnoticed"
        if name == "high-out":
            assert r["wrong_unguarded"] == 0     # the window's upper bound is conservative (module docstring)


@pytest.mark.parametrize("cs", [17, 64, 128, 130])
def test_oracle_binned_mi_is_finite_and_above_the_absolute_floor(oracle, cs):
    for mm in ALL_RANGES:
        for nb in dei.NUM_BINS:
            ens = dei.lattice_case(cs, mm, nb)
            mi = oracle.field(oracle_lib.MI_BINNED, ens, dei.voxel(ens, dei.LATTICE_REF), num_bins=nb, minmax_ref=mm,
                              minmax_query=mm)
            assert np.isfinite(mi).all() and mi.min() > 1e-3, (cs, mm, nb, float(mi.min()))
    mm_a, mm_b = dei.ORDINARY_RANGES[0], dei.BOUNDARY_RANGES[0][0]
    for nb in dei.NUM_BINS:
        a, b = dei.lattice_case(cs, mm_a, nb), dei.lattice_case(cs, mm_b, nb, side=1)
        mi = oracle.symmetric_field(oracle_lib.MI_BINNED, a, b, num_bins=nb, minmax_ref=mm_a, minmax_query=mm_b)
        assert np.isfinite(mi).all() and mi.min() > 1e-3, (cs, nb, float(mi.min()))


@pytest.fixture(scope="module")
def ref():
    if not oracle_lib.reference_available():
        pytest.skip("oracle/_ref is absent")
    return oracle_lib.load_reference()


# one member count per kernel family: mi_binned_kernel, mi_binned_hist_kernel / generic_kernel
@pytest.mark.parametrize("cs,nb", [(64, 80), (130, 10), (130, 255)])
def test_oracle_vs_reference_binned_field(oracle, ref, cs, nb):
    for mm in (dei.ORDINARY_RANGES[0], dei.BOUNDARY_RANGES[1][0], dei.BOUNDARY_RANGES[5][0]):
        ens = dei.lattice_case(cs, mm, nb, plants=True)
        for r in (dei.LATTICE_REF, dei.PLANT_POS_INF):
            kw = dict(num_bins=nb, minmax_ref=mm, minmax_query=mm)
            for m in (oracle_lib.MI_BINNED, oracle_lib.BINNED_MI_CC):
                assert_bit_exact(oracle.field(m, ens, dei.voxel(ens, r), **kw), ref.mi_field(m, ens, dei.voxel(ens, r), **kw),
                                 f"binned measure {m} cs={cs} bins={nb} range={mm} ref={r}")


@pytest.mark.parametrize("cs", [64, 130])        # sorted_symmetric_kernel, direct_symmetric_kernel
def test_oracle_vs_reference_binned_symmetric_and_requests(oracle, ref, cs):
    mm_a, mm_b = dei.ORDINARY_RANGES[0], dei.BOUNDARY_RANGES[0][0]
    a, b = dei.lattice_case(cs, mm_a, 80, plants=True), dei.lattice_case(cs, mm_b, 80, side=1)
    kw = dict(num_bins=80, minmax_ref=mm_a, minmax_query=mm_b)
    assert_bit_exact(oracle.symmetric_field(oracle_lib.MI_BINNED, a, b, **kw),
                     ref.mi_symmetric_field(oracle_lib.MI_BINNED, a, b, **kw), f"symmetric binned cs={cs}")
    _, ii, jj = dei.request_pairs(dei.GRID, dei.REQUEST_COUNT, cs)
    assert_bit_exact(oracle.pair_requests(oracle_lib.MI_BINNED, a, ii, jj, num_bins=80),
                     ref.mi_pair_requests(oracle_lib.MI_BINNED, a, ii, jj, num_bins=80), f"binned requests cs={cs}")


# pearson_reg_kernel, pearson_reg_lds_kernel, pearson_split_kernel, pearson_big_kernel
@pytest.mark.parametrize("cs", [64, 256, 340, 1300])
def test_oracle_vs_reference_pearson_field(oracle, ref, cs):
    for name in ("low-in", "high-in", "one-out"):
        ens = dei.guard_field(name, cs, seed=cs)
        refv = dei.voxel(ens, dei.GUARD_REF)
        assert_bit_exact(oracle.field(oracle_lib.PEARSON, ens, refv), ref.field(oracle_lib.PEARSON, ens, refv),
                         f"pearson {name} cs={cs}")


@pytest.mark.parametrize("cs", [96, 150])        # the two-vector kernel, pair_request_kernel
def test_oracle_vs_reference_pearson_requests(oracle, ref, cs):
    ens, _, ii, jj = dei.guard_request_case(cs, seed=cs)
    assert_bit_exact(oracle.pair_requests(oracle_lib.PEARSON, ens, ii, jj), ref.pair_requests(oracle_lib.PEARSON, ens, ii, jj),
                     f"pearson requests cs={cs}")
