#!/usr/bin/env python3
"""Times crf_field_similarity (CorrField.field_similarity) on two resident fields and, beside it, the reference's own
functions on the host cores.

Workload: two size^3 box ensembles (seeds 1 and 2) of `--members` fp32 members, bound as primary and secondary members.
Per measure (Pearson; binned MI at 80 bins over the fields' extrema) and member selection (all members; one member):
after a warm-up, `--blocks` rounds of `--reps` calls -- wall ms per call (a host clock around the synchronous call) and
kernel ms (crf_take_kernel_time: one event pair around the call's launches), one median per block; the figure is the
median of the block medians.  Share of the HBM peak = algorithmic bytes / kernel time / 8 TB/s, the algorithmic bytes
being 2 passes x 2 fields x 4 B per sample for Pearson and 1 pass x 2 fields x 4 B for the binned measures.  (One member of
256^3 is 64 MiB per field: both fields fit the 256 MiB Infinity Cache, so in steady state that row is not an HBM figure.)

The histogram kernel is timed on two more inputs of the same shape: uniform random values (every sample its own cell, no
two neighbours alike) and all samples in one cell (a constant field).

--host-reference: computePearsonParallel<double> (oracle/_ref/libref_corr.so) and ref_mi_binned (computeMutualInformationBinned
<double>, oracle/_ref/libref_mi.so) on the gathered host copies of the same samples, wall time of one call each with the
OpenMP threads the host gives (the binned function is single-threaded in the reference).  Beyond 46 340 samples the
reference's binned VALUE is not defined (its int product overflows); its time is what is recorded.

usage: tools/measure_similarity.py --out TABLE.md [--json FILE] [--size 256] [--members 64] [--blocks 4] [--reps 8]
                                   [--host-reference]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_PEAK = 8.0e12           # bytes/s (MI355X)
BINS = 80
PASSES = {"pearson": 2, "mi_binned": 1}


def time_calls(eng, call, blocks, reps):
    for _ in range(3):
        call()
    eng.take_kernel_time()
    wall, kernel = [], []
    for _ in range(blocks):
        w, k = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            w.append((time.perf_counter() - t0) * 1e3)
            ms, launches = eng.take_kernel_time()
            assert launches == 1
            k.append(ms)
        wall.append(statistics.median(w))
        kernel.append(statistics.median(k))
    return {"wall_block_medians_ms": wall, "kernel_block_medians_ms": kernel}


def host_reference(x, y, mm_x, mm_y):
    """Wall seconds of the reference's own functions on host arrays x, y (fp32, no NaN)."""
    import numpy as np
    import oracle_lib
    from similarity_reference import PEARSON_PARALLEL_DOUBLE, normalise
    ref = oracle_lib.load_reference()
    pearson = getattr(ref.lib, PEARSON_PARALLEL_DOUBLE)
    pearson.restype = C.c_float
    pearson.argtypes = [oracle_lib.FP, oracle_lib.FP, C.c_int]
    rec = {"samples": int(x.size), "omp_threads": int(os.environ.get("OMP_NUM_THREADS", "0"))}
    t0 = time.perf_counter()
    rec["pearson_value"] = float(pearson(oracle_lib._fp(x), oracle_lib._fp(y), x.size))
    rec["pearson_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    x01, y01 = normalise(x, *mm_x), normalise(y, *mm_y)
    rec["normalise_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    rec["mi_binned_value"] = float(ref.mi.ref_mi_binned(oracle_lib._fp(x01), oracle_lib._fp(y01), BINS, x01.size))
    rec["mi_binned_s"] = time.perf_counter() - t0
    del x01, y01
    return rec


def measure(a):
    import torch
    import correrender_amd as ca
    from correrender_amd import Measure
    n, cs = a.size, a.members
    voxels = n * n * n
    eng = ca.CorrField(0)
    fields = []
    for seed in (1, 2):
        f = torch.empty((cs, voxels), dtype=torch.float32, device="cuda")
        for c in range(cs):
            eng.synth_box_member(f[c], n, n, n, 0, n, c, cs, seed)
        fields.append(f)
    torch.cuda.synchronize()
    eng.set_grid(n, n, n, cs)
    eng.set_profiling(True)
    result = {"library": str(ca._lib.library_path()), "size": n, "members": cs, "blocks": a.blocks, "reps": a.reps,
              "runs": {}, "histogram_inputs": {}, "host_reference": {}}

    def bind(x, y):
        eng.bind_members(x)
        eng.bind_secondary_members(y)
        return eng.member_minmax(), eng.secondary_member_minmax()

    mm_x, mm_y = bind(*fields)
    result["extrema"] = [mm_x, mm_y]
    one = cs // 2
    for name, measure_id in (("pearson", Measure.PEARSON), ("mi_binned", Measure.MUTUAL_INFORMATION_BINNED)):
        for member in (None, one):
            call = lambda: eng.field_similarity(measure_id, member=member, num_bins=BINS, minmax_x=mm_x, minmax_y=mm_y,
                                                return_samples=True)
            value, samples = call()
            rec = time_calls(eng, call, a.blocks, a.reps)
            rec.update(value=value, samples=samples, kernel=eng.last_kernel_name())
            result["runs"][f"{name}:{'all' if member is None else 'one'}"] = rec
            print(name, member, json.dumps(rec), flush=True)

    if a.host_reference:
        for key, sel in (("one", slice(one, one + 1)), ("all", slice(0, cs))):
            x = fields[0][sel].reshape(-1).cpu().numpy()
            y = fields[1][sel].reshape(-1).cpu().numpy()
            print(f"host reference on {x.size} samples ...", flush=True)
            result["host_reference"][key] = host_reference(x, y, mm_x, mm_y)
            print("host reference", key, json.dumps(result["host_reference"][key]), flush=True)
            del x, y

    # the histogram kernel on a uniform field and on a field in one cell
    del fields
    torch.cuda.empty_cache()
    gen = torch.Generator(device="cuda").manual_seed(3)
    inputs = {"uniform": lambda: torch.rand((cs, voxels), dtype=torch.float32, device="cuda", generator=gen),
              "one cell": lambda: torch.full((cs, voxels), 0.3, dtype=torch.float32, device="cuda")}
    for name, make in inputs.items():
        x, y = make(), make()
        bind(x, y)
        call = lambda: eng.field_similarity(Measure.MUTUAL_INFORMATION_BINNED, num_bins=BINS, return_samples=True)
        value, samples = call()
        rec = time_calls(eng, call, a.blocks, a.reps)
        rec.update(value=value, samples=samples, kernel=eng.last_kernel_name())
        result["histogram_inputs"][name] = rec
        print("histogram input", name, json.dumps(rec), flush=True)
        del x, y
        torch.cuda.empty_cache()
    eng.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(result, indent=1))
    write_table(a, result)


def write_table(a, result):
    n, cs = result["size"], result["members"]
    med = statistics.median
    lines = [f"crf_field_similarity on two resident fp32 fields, {n}^3 x {cs} members (box ensembles, seeds 1 and 2), binned MI at "
             f"{BINS} bins over the fields' extrema.  {result['blocks']} blocks of {result['reps']} calls after a warm-up; a figure is "
             "the median of the block medians, the spread max - min of the block medians.  ms per call: host clock around the "
             "synchronous call; kernel ms: crf_take_kernel_time (one event pair around the call's launches).  Share of the 8 TB/s "
             "HBM peak against the algorithmic bytes (Pearson 2 passes x 2 fields, binned 1 pass x 2 fields, 4 B per sample).", "",
             "| measure | members | samples | ms per call | kernel ms | spread of kernel ms | algorithmic GB | GB/s | share of 8 TB/s | kernel |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for key, rec in result["runs"].items():
        name, sel = key.split(":")
        k = med(rec["kernel_block_medians_ms"])
        spread = max(rec["kernel_block_medians_ms"]) - min(rec["kernel_block_medians_ms"])
        candidates = n ** 3 * (cs if sel == "all" else 1)
        bytes_ = PASSES[name] * 2 * 4 * candidates
        rate = bytes_ / (k * 1e-3)
        lines.append(f"| {name} | {sel} | {rec['samples']} | {med(rec['wall_block_medians_ms']):.3f} | {k:.3f} | {spread:.3f} | "
                     f"{bytes_ / 1e9:.3f} | {rate / 1e9:.0f} | {100 * rate / HBM_PEAK:.1f} % | {rec['kernel']} |")
    if result["histogram_inputs"]:
        lines += ["", f"similarity_histogram_kernel on two more inputs of the same shape ({BINS} bins, ranges (0, 1)):", "",
                  "| input | kernel ms | spread | GB/s | share of 8 TB/s |", "|---|---|---|---|---|"]
        ks = {}
        for name, rec in result["histogram_inputs"].items():
            ks[name] = med(rec["kernel_block_medians_ms"])
            spread = max(rec["kernel_block_medians_ms"]) - min(rec["kernel_block_medians_ms"])
            rate = 8 * n ** 3 * cs / (ks[name] * 1e-3)
            lines.append(f"| {name} | {ks[name]:.3f} | {spread:.3f} | {rate / 1e9:.0f} | {100 * rate / HBM_PEAK:.1f} % |")
        if len(ks) == 2:
            lines += ["", f"one cell / uniform = {ks['one cell'] / ks['uniform']:.3f}"]
    if result["host_reference"]:
        lines += ["", "The reference's own functions on the host cores (oracle/_ref, one call each, wall time; the binned function "
                  "is single-threaded in the reference and its input is normalised first, timed apart):", "",
                  "| members | samples | OpenMP threads | computePearsonParallel<double> s | normalisation s | computeMutualInformationBinned<double> s |",
                  "|---|---|---|---|---|---|"]
        for key, rec in result["host_reference"].items():
            lines.append(f"| {key} | {rec['samples']} | {rec['omp_threads']} | {rec['pearson_s']:.3f} | {rec['normalise_s']:.3f} | "
                         f"{rec['mi_binned_s']:.3f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--host-reference", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--from-json", help="rebuild the table from a --json file of an earlier run (no GPU)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.from_json:
        write_table(a, json.loads(Path(a.from_json).read_text()))
    else:
        measure(a)


if __name__ == "__main__":
    main()
