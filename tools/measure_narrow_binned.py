#!/usr/bin/env python3
"""Kernel times of the binned-MI field on members in a narrow native format, for ONE build of libcorrfield.so
(CORRFIELD_LIBRARY selects it) -- run it alternately on two builds and merge the JSON files.

Workload: the size^3 box ensemble at each member count, rescaled to [0, 1] by its global extrema and cast to u8 / u16 /
f16, bound as narrow members; num_bins 80, extrema from member_minmax (native on every build measured here).  Per format
and member count, on a fresh context: the wall time of the first binned-MI call (on a build that widens, it contains the
one-off fp32 copy); then, after a warm-up, `--blocks` blocks of `--reps` calls, kernel time from crf_take_kernel_time, one
median per block; the wall time of a steady call; free device memory and the size of the fp32 copy at the end.

usage: tools/measure_narrow_binned.py --out FILE [--size 256] [--members 24 64 100 128] [--formats u8 u16 f16]
                                      [--blocks 4] [--reps 8]
       tools/measure_narrow_binned.py --merge PARENT.json... --against NEW.json... [--variant OTHER.json...] --out TABLE.md
(--variant: a third build measured the same way, e.g. one whose u8 members go through the arithmetic front end; its
figures are listed next to --against's for the keys it holds.)
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FORMATS = ("u8", "u16", "f16")
NUM_BINS = 80


def measure(a):
    import torch
    import correrender_amd as ca
    from correrender_amd import Measure
    mi = Measure.MUTUAL_INFORMATION_BINNED
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
        for fmt in a.formats:
            if fmt == "f16":
                narrow = base.to(torch.float16)
            else:
                codes = torch.round(base * (65535.0 if fmt == "u16" else 255.0)).to(torch.int32)
                narrow = codes.to(torch.int16).view(torch.uint16) if fmt == "u16" else codes.to(torch.uint8)
                del codes
            torch.cuda.synchronize()
            rec = {}
            torch.cuda.empty_cache()
            eng = ca.CorrField(0)
            eng.set_grid(n, n, n, cs)
            eng.bind_members(narrow)
            eng.set_profiling(True)
            mm = eng.member_minmax()
            kw = dict(num_bins=NUM_BINS, minmax_ref=mm, minmax_query=mm)
            rec["minmax"] = list(mm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.compute_device(mi, out, ref, **kw)
            torch.cuda.synchronize()
            rec["first_wall_ms"] = (time.perf_counter() - t0) * 1e3
            for _ in range(2):
                eng.compute_device(mi, out, ref, **kw)
            torch.cuda.synchronize()
            eng.take_kernel_time()
            medians = []
            for _ in range(a.blocks):
                times = []
                for _ in range(a.reps):
                    eng.compute_device(mi, out, ref, **kw)
                    ms, launches = eng.take_kernel_time()
                    times.append(ms / max(launches, 1))
                medians.append(statistics.median(times))
            rec["kernel"] = eng.last_kernel_name()
            rec["member_format_read"] = eng.last_member_format()
            rec["block_medians_ms"] = medians
            t0 = time.perf_counter()
            eng.compute_device(mi, out, ref, **kw)
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
            "native": [json.loads(Path(p).read_text()) for p in a.against],
            "variant": [json.loads(Path(p).read_text()) for p in (a.variant or [])]}
    n = runs["parent"][0]["size"]
    lines = [f"Binned-MI field on narrow members, {n}^3, {NUM_BINS} bins, kernel ms from crf_take_kernel_time.  (a) parent: "
             "mi_binned_kernel on the widened copy, steady state; (b) this commit: mi_binned_narrow_kernel.  Each figure is the "
             f"median of the block medians of {len(runs['parent'])} alternating processes per build; spread = max - min of the "
             "parent's block medians (the run-to-run spread the acceptance rule uses).", "",
             "| format | members | (a) parent ms | spread of (a) | (b) native ms | (b) / (a) | within rule | variant ms | kernels (a) -> (b) |",
             "|---|---|---|---|---|---|---|---|---|"]
    keys = list(runs["parent"][0]["runs"])
    for key in keys:
        fmt, cs = key.split(":")
        med = {side: [m for r in runs[side] if key in r["runs"] for m in r["runs"][key]["block_medians_ms"]] for side in runs}
        pa, na = statistics.median(med["parent"]), statistics.median(med["native"])
        spread = max(med["parent"]) - min(med["parent"])
        var = f"{statistics.median(med['variant']):.3f}" if med["variant"] else ""
        names = " -> ".join(runs[side][0]["runs"][key]["kernel"] for side in ("parent", "native"))
        same = all(r["runs"][key]["checksum"] == runs["parent"][0]["runs"][key]["checksum"]
                   for s in runs for r in runs[s] if key in r["runs"])
        lines.append(f"| {fmt} | {cs} | {pa:.3f} | {spread:.3f} | {na:.3f} | {na / pa:.3f} | "
                     f"{'yes' if na <= pa + spread else 'NO'} | {var} | {names}{'' if same else ' (CHECKSUMS DIFFER)'} |")
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
    ap.add_argument("--members", type=int, nargs="+", default=[24, 64, 100, 128])
    ap.add_argument("--formats", nargs="+", default=list(FORMATS), choices=FORMATS)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--against", nargs="+")
    ap.add_argument("--variant", nargs="+")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    merge(a) if a.merge else measure(a)


if __name__ == "__main__":
    main()
