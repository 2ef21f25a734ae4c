#!/usr/bin/env python3
"""Kernel times of the symmetric Pearson field on two fields in a narrow native format: the native route
(pearson_symmetric_narrow_kernel on both fields as stored) against the copy route of the commit before it (narrow primary
members, fp32 secondary members holding the converted values: pearson_symmetric_kernel on the fp32 copy of the primary
field and the fp32 secondary field), both in ONE process on the same data, block by block in turns.

Workload: two size^3 box ensembles (seeds 1 and 2) of max(members) members, each rescaled to [0, 1] by its global extrema
and cast to u8 / u16 / f16; a run at `cs` members uses the first cs members of both.  Per format and member count, on two
fresh contexts: the wall time of the first call of each route (the copy route's contains the one-off fp32 copy); then, after
a warm-up of both, `--blocks` rounds of `--reps` calls per route, kernel time from crf_take_kernel_time, one median per
block; whether both routes gave the same bits; the sizes of the copies each route holds.

The routing rule of the project's narrow routes: the native kernel is routed where its time (median of its block medians)
is no more than the copy route's plus the copy route's run-to-run spread (max - min of its block medians).

usage: tools/measure_narrow_symmetric.py --out TABLE.md [--json FILE] [--size 256] [--members 16 24 ...] [--blocks 4] [--reps 16]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FORMATS = ("u8", "u16", "f16")
ELEMENT_BYTES = {"u8": 1, "u16": 2, "f16": 2}
# the exact counts 16 .. 128 and one guarded count per granule
DEFAULT_MEMBERS = [12, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120, 128]


def narrow_and_wide(base, fmt):
    """`base` (fp32 in [0, 1]) cast to `fmt`, and the fp32 values the calculators see of the cast."""
    import torch
    if fmt == "f16":
        narrow = base.to(torch.float16)
        return narrow, narrow.to(torch.float32)
    scale = 65535.0 if fmt == "u16" else 255.0
    codes = torch.round(base * scale).to(torch.int32)
    import numpy as np
    # float(code) / 255.0f, / 65535.0f as numpy rounds it (IEEE), through a table of every code
    table = torch.from_numpy(np.arange(int(scale) + 1, dtype=np.float32) / np.float32(scale)).cuda()
    wide = torch.empty_like(base)
    for c in range(base.shape[0]):  # (row by row: the int64 indices of a whole field would be four times its size)
        wide[c] = table[codes[c].to(torch.int64)]
    narrow = codes.to(torch.int16).view(torch.uint16) if fmt == "u16" else codes.to(torch.uint8)
    return narrow, wide


def measure(a):
    import torch
    import correrender_amd as ca
    from correrender_amd import Measure
    n = a.size
    voxels = n * n * n
    most = max(a.members)
    gen = ca.CorrField(0)
    base = []
    for seed in (1, 2):
        field = torch.empty((most, voxels), dtype=torch.float32, device="cuda")
        for c in range(most):
            gen.synth_box_member(field[c], n, n, n, 0, n, c, most, seed)
        torch.cuda.synchronize()
        lo, hi = field.min(), field.max()
        base.append((field - lo) / (hi - lo))
        del field
    gen.close()
    outs = {route: torch.empty(voxels, dtype=torch.float32, device="cuda") for route in ("native", "copy")}
    result = {"library": str(ca._lib.library_path()), "size": n, "blocks": a.blocks, "reps": a.reps, "runs": {}}
    for fmt in FORMATS:
        narrow_x, _ = narrow_and_wide(base[0], fmt)
        narrow_y, wide_y = narrow_and_wide(base[1], fmt)
        torch.cuda.synchronize()
        for cs in a.members:
            engines = {}
            rec = {}
            for route in ("native", "copy"):
                eng = ca.CorrField(0)
                eng.set_grid(n, n, n, cs)
                eng.bind_members(narrow_x[:cs])
                eng.bind_secondary_members(narrow_y[:cs] if route == "native" else wide_y[:cs])
                eng.set_profiling(True)
                t0 = time.perf_counter()
                eng.compute_device(Measure.PEARSON, outs[route], symmetric=True)
                torch.cuda.synchronize()
                rec[f"{route}_first_wall_ms"] = (time.perf_counter() - t0) * 1e3
                for _ in range(3):
                    eng.compute_device(Measure.PEARSON, outs[route], symmetric=True)
                torch.cuda.synchronize()
                eng.take_kernel_time()
                rec[f"{route}_kernel"] = eng.last_kernel_name()
                rec[f"{route}_member_format_read"] = eng.last_member_format()
                rec[f"{route}_copy_bytes"] = eng.wide_copy_bytes() + eng.secondary_wide_copy_bytes()
                engines[route] = eng
            rec["same_bits"] = bool(torch.equal(outs["native"].view(torch.int32), outs["copy"].view(torch.int32)))
            rec["checksum"] = float(torch.nan_to_num(outs["native"]).double().sum())
            medians = {"native": [], "copy": []}
            for _ in range(a.blocks):
                for route, eng in engines.items():  # the two routes in turns
                    times = []
                    for _ in range(a.reps):
                        eng.compute_device(Measure.PEARSON, outs[route], symmetric=True)
                        ms, launches = eng.take_kernel_time()
                        times.append(ms)  # main kernel and tail kernel are one launch record
                    medians[route].append(statistics.median(times))
            for route, eng in engines.items():
                rec[f"{route}_block_medians_ms"] = medians[route]
                eng.close()
            result["runs"][f"{fmt}:{cs}"] = rec
            print(fmt, cs, json.dumps(rec), flush=True)
            torch.cuda.empty_cache()
        del narrow_x, narrow_y, wide_y
        torch.cuda.empty_cache()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(result, indent=1))
    write_table(a, result)


def write_table(a, result):
    n = result["size"]
    voxels = n ** 3
    lines = [f"Symmetric Pearson field on two narrow fields, {n}^3, kernel ms from crf_take_kernel_time, one process, the two "
             f"routes in turns ({result['blocks']} blocks of {result['reps']} calls each; a figure is the median of the block "
             "medians).  (a) copy route, the commit before: narrow primary + fp32 secondary of the converted values, "
             "pearson_symmetric_kernel on the fp32 copy and the fp32 field, steady state; (b) native route: both fields "
             "narrow, pearson_symmetric_narrow_kernel.  spread = max - min of (a)'s block medians; routed = (b) <= (a) + spread.  "
             "GB/s = algorithmic bytes (2 cs e + 4 per voxel for (b), 8 cs + 4 for (a)) over the time.", "",
             "| format | members | (a) copy ms | spread of (a) | (b) native ms | (b) / (a) | (a) GB/s | (b) GB/s | routed | same bits | kernels (a) -> (b) |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    verdict = {}
    for key, rec in result["runs"].items():
        fmt, cs = key.split(":")
        cs = int(cs)
        ca_, na = statistics.median(rec["copy_block_medians_ms"]), statistics.median(rec["native_block_medians_ms"])
        spread = max(rec["copy_block_medians_ms"]) - min(rec["copy_block_medians_ms"])
        ok = na <= ca_ + spread and rec["native_kernel"] == "pearson_symmetric_narrow_kernel"
        verdict.setdefault((fmt, (cs + 15) // 16 * 16), []).append(ok)
        gbs = lambda bytes_per_voxel, ms: voxels * bytes_per_voxel / (ms * 1e-3) / 1e9
        lines.append(f"| {fmt} | {cs} | {ca_:.3f} | {spread:.3f} | {na:.3f} | {na / ca_:.3f} | {gbs(8 * cs + 4, ca_):.0f} | "
                     f"{gbs(2 * cs * ELEMENT_BYTES[fmt] + 4, na):.0f} | {'yes' if ok else 'NO'} | "
                     f"{'yes' if rec['same_bits'] else 'NO'} | {rec['copy_kernel']} -> {rec['native_kernel']} |")
    lines += ["", "Copies and first calls.  The copy route holds the fp32 copy of the primary members and the caller holds (and "
              "uploads, per evaluation in the C++ adapter) an fp32 secondary field; the native route holds neither.", "",
              "| format | members | fp32 copy held by (a) GiB | fp32 secondary field of (a) GiB | both narrow fields GiB | copies held by (b) | "
              "first call (a) wall ms | first call (b) wall ms |", "|---|---|---|---|---|---|---|---|"]
    for key, rec in result["runs"].items():
        fmt, cs = key.split(":")
        cs = int(cs)
        lines.append(f"| {fmt} | {cs} | {rec['copy_copy_bytes'] / 2**30:.2f} | {4 * cs * voxels / 2**30:.2f} | "
                     f"{2 * ELEMENT_BYTES[fmt] * cs * voxels / 2**30:.2f} | {rec['native_copy_bytes']} B | "
                     f"{rec['copy_first_wall_ms']:.1f} | {rec['native_first_wall_ms']:.1f} |")
    lines += ["", "Routing derived from the rows above (N = members rounded up to 16; every measured row of an N within the rule):", "",
              "| format | " + " | ".join(str(N) for N in sorted({N for _, N in verdict})) + " |",
              "|---|" + "---|" * len({N for _, N in verdict})]
    for fmt in FORMATS:
        lines.append(f"| {fmt} | " + " | ".join("native" if all(verdict[fmt, N]) else "copy"
                                                for N in sorted({N for f, N in verdict if f == fmt})) + " |")
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, nargs="+", default=DEFAULT_MEMBERS)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=16)
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
