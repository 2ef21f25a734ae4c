#!/usr/bin/env python3
"""Kernel times of the Spearman field on members in a narrow native format, for ONE build of libcorrfield.so
(CORRFIELD_LIBRARY selects it) -- run it alternately on two builds and merge the JSON files.

Workload and method are those of tools/measure_narrow_kendall.py: the size^3 box ensemble at each member count, rescaled
to [0, 1] by its global extrema and cast to u8 / u16 / f16, bound as narrow members.  Per format and member count, on a
fresh context: the wall time of the first Spearman call (on a build that widens, it contains the one-off fp32 copy); then,
after a warm-up, `--blocks` blocks of `--reps` calls, kernel time from crf_take_kernel_time (first pass and list pass
together where the build runs two), one median per block; the wall time of a steady call; free device memory and the
size of the fp32 copy at the end; the share of voxels with at least two equal members (every 16th voxel sampled).

usage: tools/measure_narrow_spearman.py --out FILE [--size 256] [--members 40 64 100 128] [--blocks 4] [--reps 8]
       tools/measure_narrow_spearman.py --merge PARENT.json... --against NEW.json... --out TABLE.md
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from measure_narrow_kendall import FORMATS, tied_share  # noqa: E402


def measure(a):
    import torch
    import correrender_amd as ca
    from correrender_amd import Measure
    n = a.size
    voxels = n * n * n
    ref = (n // 2, n // 2, n // 2)
    gen = ca.CorrField(0)
    out = torch.empty(voxels, dtype=torch.float32, device="cuda")
    result = {"library": str(ca._lib.library_path()), "size": n, "runs": {}}
    for cs in a.members:
        base = torch.empty((cs, voxels), dtype=torch.float32, device="cuda")
        for c in range(cs):
            gen.synth_box_member(base[c], n, n, n, 0, n, c, cs, 1)
        torch.cuda.synchronize()
        lo, hi = base.min(), base.max()
        base = (base - lo) / (hi - lo)
        for fmt in FORMATS:
            if fmt == "f16":
                narrow = base.to(torch.float16)
            else:
                codes = torch.round(base * (65535.0 if fmt == "u16" else 255.0)).to(torch.int32)
                narrow = codes.to(torch.int16).view(torch.uint16) if fmt == "u16" else codes.to(torch.uint8)
                del codes
            torch.cuda.synchronize()
            rec = {"tied_share": tied_share(narrow)}
            torch.cuda.empty_cache()
            eng = ca.CorrField(0)
            eng.set_grid(n, n, n, cs)
            eng.bind_members(narrow)
            eng.set_profiling(True)
            t0 = time.perf_counter()
            eng.compute_device(Measure.SPEARMAN, out, ref)
            torch.cuda.synchronize()
            rec["first_wall_ms"] = (time.perf_counter() - t0) * 1e3
            for _ in range(2):
                eng.compute_device(Measure.SPEARMAN, out, ref)
            torch.cuda.synchronize()
            eng.take_kernel_time()
            medians = []
            for _ in range(a.blocks):
                times = []
                for _ in range(a.reps):
                    eng.compute_device(Measure.SPEARMAN, out, ref)
                    ms, launches = eng.take_kernel_time()  # (one timed bracket per evaluation, around both passes)
                    times.append(ms / max(launches, 1))
                medians.append(statistics.median(times))
            rec["kernel"] = eng.last_kernel_name()
            rec["member_format_read"] = eng.last_member_format()
            rec["block_medians_ms"] = medians
            t0 = time.perf_counter()
            eng.compute_device(Measure.SPEARMAN, out, ref)
            torch.cuda.synchronize()
            rec["steady_wall_ms"] = (time.perf_counter() - t0) * 1e3
            rec["free_device_bytes"] = int(torch.cuda.mem_get_info()[0])
            rec["wide_copy_bytes"] = eng.wide_copy_bytes()
            rec["checksum"] = float(torch.nan_to_num(out).double().sum())
            result["runs"][f"{fmt}:{cs}"] = rec
            print(fmt, cs, json.dumps(rec), flush=True)
            eng.close()
            del narrow
            torch.cuda.empty_cache()
        del base
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1))


def merge(a):
    runs = {"parent": [json.loads(Path(p).read_text()) for p in a.merge],
            "native": [json.loads(Path(p).read_text()) for p in a.against]}
    n = runs["parent"][0]["size"]
    lines = [f"Spearman field on narrow members, {n}^3, kernel ms from crf_take_kernel_time.  (a) parent: the fp32 kernels on "
             "the widened copy, steady state; (b) this commit.  Each figure is the median of the block medians of "
             f"{len(runs['parent'])} alternating processes per build; spread = max - min of the parent's block medians (the "
             "run-to-run spread the acceptance rule uses).  tied = share of voxels with two equal members.", "",
             "| format | members | tied | (a) parent ms | spread of (a) | (b) native ms | (b) / (a) | within rule | kernels (a) -> (b) |",
             "|---|---|---|---|---|---|---|---|---|"]
    keys = list(runs["parent"][0]["runs"])
    for key in keys:
        fmt, cs = key.split(":")
        med = {side: [m for r in runs[side] for m in r["runs"][key]["block_medians_ms"]] for side in runs}
        pa, na = statistics.median(med["parent"]), statistics.median(med["native"])
        spread = max(med["parent"]) - min(med["parent"])
        names = " -> ".join(runs[side][0]["runs"][key]["kernel"] for side in ("parent", "native"))
        same = all(r["runs"][key]["checksum"] == runs["parent"][0]["runs"][key]["checksum"] for s in runs for r in runs[s])
        lines.append(f"| {fmt} | {cs} | {runs['parent'][0]['runs'][key]['tied_share']:.3f} | {pa:.3f} | {spread:.3f} | {na:.3f} | "
                     f"{na / pa:.3f} | {'yes' if na <= pa + spread else 'NO'} | {names}{'' if same else ' (CHECKSUMS DIFFER)'} |")
    lines += ["", "| format | members | build | first call wall ms | steady call wall ms | one-off copy ms (difference) | "
              "free device memory GiB | fp32 copy GiB |", "|---|---|---|---|---|---|---|---|"]
    for key in keys:
        fmt, cs = key.split(":")
        for side in ("parent", "native"):
            recs = [r["runs"][key] for r in runs[side]]
            md = lambda k: statistics.median(r[k] for r in recs)
            lines.append(f"| {fmt} | {cs} | {side} | {md('first_wall_ms'):.1f} | {md('steady_wall_ms'):.1f} | "
                         f"{md('first_wall_ms') - md('steady_wall_ms'):.1f} | {md('free_device_bytes') / 2**30:.2f} | "
                         f"{recs[0]['wide_copy_bytes'] / 2**30:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).write_text(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, nargs="+", default=[40, 64, 100, 128])
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--against", nargs="+")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    merge(a) if a.merge else measure(a)


if __name__ == "__main__":
    main()
