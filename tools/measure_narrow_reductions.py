#!/usr/bin/env python3
"""Kernel times of the ensemble mean, spread and set predicate on members in a narrow native format, for ONE build of
libcorrfield.so (CORRFIELD_LIBRARY selects it) -- run it alternately on two builds and merge the JSON files.

Workload: the 256^3 x 64 box ensemble, rescaled to [0, 1] by its global extrema and cast to u8 / u16 / f16, bound as
narrow members.  Per format, on a fresh context: the wall time of crf_member_minmax; the wall time of the first mean
(on a build that widens, it contains the one-off fp32 copy); then, after a warm-up, `--blocks` blocks of `--reps` calls per
statistic, kernel time from crf_take_kernel_time, one median per block; free device memory at the end.

usage: tools/measure_narrow_reductions.py --out FILE [--size 256] [--members 64] [--blocks 5] [--reps 20]
       tools/measure_narrow_reductions.py --merge PARENT.json... --against NEW.json... --out TABLE.md
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

STATS = ("mean", "spread", "predicate >")


def call(eng, stat, out):
    if stat == "mean":
        eng.ensemble_stat_device(0, out)
    elif stat == "spread":
        eng.ensemble_stat_device(1, out)
    else:
        eng.set_predicate_device(">", 0.5, 16, 48, out)


def measure(a):
    import torch
    import correrender_amd as ca
    n, cs = a.size, a.members
    voxels = n * n * n
    gen = ca.CorrField(0)
    base = torch.empty((cs, voxels), dtype=torch.float32, device="cuda")
    for c in range(cs):
        gen.synth_box_member(base[c], n, n, n, 0, n, c, cs, 1)
    torch.cuda.synchronize()
    lo, hi = base.min(), base.max()
    base = (base - lo) / (hi - lo)
    out = torch.empty(voxels, dtype=torch.float32, device="cuda")
    result = {"library": str(ca._lib.library_path()), "size": n, "members": cs, "formats": {}}
    for fmt in ("u8", "u16", "f16"):
        if fmt == "f16":
            narrow = base.to(torch.float16)
        else:
            codes = torch.round(base * (65535.0 if fmt == "u16" else 255.0)).to(torch.int32)
            narrow = codes.to(torch.int16).view(torch.uint16) if fmt == "u16" else codes.to(torch.uint8)
            del codes
        torch.cuda.synchronize()
        eng = ca.CorrField(0)
        eng.set_grid(n, n, n, cs)
        eng.bind_members(narrow)
        eng.set_profiling(True)
        rec = {"kernels": {}, "block_medians_ms": {}}
        t0 = time.perf_counter()
        rec["minmax"] = eng.member_minmax()
        rec["minmax_wall_ms"] = (time.perf_counter() - t0) * 1e3
        eng.members_changed()  # (a build that widens built its copy for the extrema: the first mean pays for it again)
        t0 = time.perf_counter()
        call(eng, "mean", out)
        torch.cuda.synchronize()
        rec["first_mean_wall_ms"] = (time.perf_counter() - t0) * 1e3
        for stat in STATS:
            for _ in range(3):
                call(eng, stat, out)
            torch.cuda.synchronize()
            eng.take_kernel_time()
            medians = []
            for _ in range(a.blocks):
                times = []
                for _ in range(a.reps):
                    call(eng, stat, out)
                    ms, launches = eng.take_kernel_time()
                    times.append(ms / max(launches, 1))
                medians.append(statistics.median(times))
            rec["kernels"][stat] = eng.last_kernel_name()
            rec["block_medians_ms"][stat] = medians
        t0 = time.perf_counter()
        call(eng, "mean", out)
        torch.cuda.synchronize()
        rec["steady_mean_wall_ms"] = (time.perf_counter() - t0) * 1e3
        rec["free_device_bytes"] = int(torch.cuda.mem_get_info()[0])
        wide_copy = getattr(eng, "wide_copy_bytes", None)
        rec["wide_copy_bytes"] = wide_copy() if wide_copy else None
        result["formats"][fmt] = rec
        eng.close()
        del narrow
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1))
    print(json.dumps(result))


def merge(a):
    runs = {"parent": [json.loads(Path(p).read_text()) for p in a.merge],
            "native": [json.loads(Path(p).read_text()) for p in a.against]}
    n, cs = runs["parent"][0]["size"], runs["parent"][0]["members"]
    voxels = n ** 3
    element = {"u8": 1, "u16": 2, "f16": 2}
    lines = [f"Sibling reductions on narrow members, {n}^3 x {cs}, kernel ms from crf_take_kernel_time.  (a) parent: the fp32 "
             "kernel on the widened copy, steady state; (b) this commit: the native kernel.  Each figure is the median of "
             f"the block medians of {len(runs['parent'])} alternating processes per build; spread = max - min of the "
             "parent's block medians (the run-to-run spread the acceptance rule uses).", "",
             "| format | statistic | (a) parent ms | spread of (a) | (b) native ms | (b) / (a) | native GB/s | of 8 TB/s | kernels (a) -> (b) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for fmt in ("u8", "u16", "f16"):
        for stat in STATS:
            med = {side: [m for r in runs[side] for m in r["formats"][fmt]["block_medians_ms"][stat]] for side in runs}
            pa, na = statistics.median(med["parent"]), statistics.median(med["native"])
            spread = max(med["parent"]) - min(med["parent"])
            gbs = (element[fmt] * cs + 4) * voxels / (na * 1e-3) / 1e9
            names = " -> ".join(runs[side][0]["formats"][fmt]["kernels"][stat] for side in ("parent", "native"))
            lines.append(f"| {fmt} | {stat} | {pa:.4f} | {spread:.4f} | {na:.4f} | {na / pa:.3f} | {gbs:.0f} | "
                         f"{gbs / 80:.0f} % | {names} |")
    lines += ["", "| format | build | first mean wall ms | steady mean wall ms | one-off copy ms (difference) | "
              "crf_member_minmax wall ms | free device memory GiB | fp32 copy GiB |", "|---|---|---|---|---|---|---|---|"]
    for fmt in ("u8", "u16", "f16"):
        for side in ("parent", "native"):
            recs = [r["formats"][fmt] for r in runs[side]]
            md = lambda key: statistics.median(r[key] for r in recs)
            copy = recs[0]["wide_copy_bytes"]
            lines.append(f"| {fmt} | {side} | {md('first_mean_wall_ms'):.2f} | {md('steady_mean_wall_ms'):.2f} | "
                         f"{md('first_mean_wall_ms') - md('steady_mean_wall_ms'):.2f} | {md('minmax_wall_ms'):.2f} | "
                         f"{md('free_device_bytes') / 2**30:.2f} | {'n/a' if copy is None else f'{copy / 2**30:.2f}'} |")
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).write_text(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--against", nargs="+")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    merge(a) if a.merge else measure(a)


if __name__ == "__main__":
    main()
