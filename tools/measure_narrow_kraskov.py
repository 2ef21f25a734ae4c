#!/usr/bin/env python3
"""Kernel times of the Kraskov-MI field on members in a narrow native format, for ONE build of libcorrfield.so
(CORRFIELD_LIBRARY selects it) -- run it alternately on two builds and merge the JSON files.

Workload: the size^3 box ensemble at each member count, rescaled to [0, 1] by its global extrema and cast to u8 / u16 /
f16, bound as narrow members; KSG-1.  Per format, member count and k, on a fresh context: the wall time of the first
Kraskov call (on a build that widens, it contains the one-off fp32 copy); then, after a warm-up, `--blocks` blocks of
`--reps` calls, kernel time from crf_take_kernel_time, one median per block; the wall time of a steady call; free device
memory and the size of the fp32 copy at the end.

Cases: every member count of --members with k = 3 and with the default k = max(ceil(3 cs / 100), 1), and the --extra
(members, k) pairs (k beyond 4: the K = 8 instantiation).

usage: tools/measure_narrow_kraskov.py --out FILE [--label NAME] [--size 256] [--members 24 40 64 100 128]
                                       [--extra 64:8] [--formats u8 u16 f16] [--blocks 4] [--reps 8]
       tools/measure_narrow_kraskov.py --merge PARENT.json... --against NEW.json... [--variant OTHER.json...] --out TABLE.md
(--variant: further builds measured the same way, e.g. ones that park the values elsewhere; their figures are listed next
to --against's under the --label they were measured with.)
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

FORMATS = ("u8", "u16", "f16")


def cases_of(a):
    from correrender_amd.engine import default_kraskov_k
    cases = []
    for cs in a.members:
        for k in dict.fromkeys((3, default_kraskov_k(cs))):
            cases.append((cs, k))
    for item in a.extra:
        cs, k = (int(x) for x in item.split(":"))
        cases.append((cs, k))
    return cases


def measure(a):
    import torch
    import correrender_amd as ca
    from correrender_amd import Measure
    mi = Measure.MUTUAL_INFORMATION_KRASKOV
    n = a.size
    voxels = n * n * n
    ref = (n // 2, n // 2, n // 2)
    gen = ca.CorrField(0)
    out = torch.empty(voxels, dtype=torch.float32, device="cuda")
    result = {"library": str(ca._lib.library_path()), "label": a.label, "size": n, "runs": {}}
    cases = cases_of(a)
    for cs in dict.fromkeys(c for c, _ in cases):
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
            for k in [k for c, k in cases if c == cs]:
                rec = {}
                torch.cuda.empty_cache()
                eng = ca.CorrField(0)
                eng.set_grid(n, n, n, cs)
                eng.bind_members(narrow)
                eng.set_profiling(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.compute_device(mi, out, ref, k=k)
                torch.cuda.synchronize()
                rec["first_wall_ms"] = (time.perf_counter() - t0) * 1e3
                for _ in range(2):
                    eng.compute_device(mi, out, ref, k=k)
                torch.cuda.synchronize()
                eng.take_kernel_time()
                medians = []
                for _ in range(a.blocks):
                    times = []
                    for _ in range(a.reps):
                        eng.compute_device(mi, out, ref, k=k)
                        ms, launches = eng.take_kernel_time()
                        times.append(ms / max(launches, 1))
                    medians.append(statistics.median(times))
                rec["kernel"] = eng.last_kernel_name()
                rec["member_format_read"] = eng.last_member_format()
                rec["block_medians_ms"] = medians
                t0 = time.perf_counter()
                eng.compute_device(mi, out, ref, k=k)
                torch.cuda.synchronize()
                rec["steady_wall_ms"] = (time.perf_counter() - t0) * 1e3
                rec["free_device_bytes"] = int(torch.cuda.mem_get_info()[0])
                rec["wide_copy_bytes"] = eng.wide_copy_bytes()
                rec["checksum"] = float(torch.nan_to_num(out).double().sum())
                result["runs"][f"{fmt}:{cs}:{k}"] = rec
                print(fmt, cs, k, json.dumps(rec), flush=True)
                eng.close()
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                Path(a.out).write_text(json.dumps(result, indent=1))  # after every case: a run cut short keeps its cells
            del narrow
            torch.cuda.empty_cache()
        del base
        torch.cuda.empty_cache()


def merge(a):
    load = lambda paths: [json.loads(Path(p).read_text()) for p in paths or []]
    runs = {"parent": load(a.merge), "native": load(a.against)}
    variants = {}
    for r in load(a.variant):
        variants.setdefault(r.get("label") or "variant", []).append(r)
    n = runs["parent"][0]["size"]
    lines = [f"Kraskov-MI field (KSG-1) on narrow members, {n}^3, kernel ms from crf_take_kernel_time.  (a) parent: the fp32 "
             "kernel on the widened copy, steady state; (b) this commit.  Each figure is the median of the block medians of "
             f"{len(runs['parent'])} alternating processes per build; spread = max - min of the parent's block medians (the "
             "run-to-run spread the acceptance rule uses).", "",
             "| format | members | k | (a) parent ms | spread of (a) | (b) native ms | (b) / (a) | within rule | "
             + "".join(f"{name} ms | " for name in variants) + "kernels (a) -> (b) |",
             "|---|---|---|---|---|---|---|---|" + "---|" * (len(variants) + 1)]
    keys = [key for key in runs["parent"][0]["runs"] if all(key in r["runs"] for s in runs for r in runs[s])]
    for key in keys:
        fmt, cs, k = key.split(":")
        med = {side: [m for r in runs[side] for m in r["runs"][key]["block_medians_ms"]] for side in runs}
        pa, na = statistics.median(med["parent"]), statistics.median(med["native"])
        spread = max(med["parent"]) - min(med["parent"])
        var = ""
        for recs in variants.values():
            vm = [m for r in recs if key in r["runs"] for m in r["runs"][key]["block_medians_ms"]]
            var += (f"{statistics.median(vm):.3f}" if vm else "") + " | "
        names = " -> ".join(runs[side][0]["runs"][key]["kernel"] for side in ("parent", "native"))
        everyone = [r for s in runs for r in runs[s]] + [r for recs in variants.values() for r in recs]
        same = all(r["runs"][key]["checksum"] == runs["parent"][0]["runs"][key]["checksum"] for r in everyone if key in r["runs"])
        lines.append(f"| {fmt} | {cs} | {k} | {pa:.3f} | {spread:.3f} | {na:.3f} | {na / pa:.3f} | "
                     f"{'yes' if na <= pa + spread else 'NO'} | {var}{names}{'' if same else ' (CHECKSUMS DIFFER)'} |")
    lines += ["", "| format | members | k | build | first call wall ms | steady call wall ms | one-off copy ms (difference) | "
              "free device memory GiB | fp32 copy GiB |", "|---|---|---|---|---|---|---|---|---|"]
    for key in keys:
        fmt, cs, k = key.split(":")
        for side in ("parent", "native"):
            recs = [r["runs"][key] for r in runs[side]]
            md = lambda name: statistics.median(r[name] for r in recs)
            lines.append(f"| {fmt} | {cs} | {k} | {side} | {md('first_wall_ms'):.1f} | {md('steady_wall_ms'):.1f} | "
                         f"{md('first_wall_ms') - md('steady_wall_ms'):.1f} | {md('free_device_bytes') / 2**30:.2f} | "
                         f"{recs[0]['wide_copy_bytes'] / 2**30:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).write_text(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, nargs="+", default=[24, 40, 64, 100, 128])
    ap.add_argument("--extra", nargs="*", default=["64:8"])
    ap.add_argument("--formats", nargs="+", default=list(FORMATS), choices=FORMATS)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--label", default="")
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--against", nargs="+")
    ap.add_argument("--variant", nargs="+")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    merge(a) if a.merge else measure(a)


if __name__ == "__main__":
    main()
