#!/usr/bin/env python3
"""Kernel times of DKL (both estimators) on members in a narrow native format, for ONE build of libcorrfield.so
(CORRFIELD_LIBRARY selects it) -- run it alternately on two builds and merge the JSON files.

Workload: the size^3 box ensemble at each member count, rescaled to [0, 1] by its global extrema and cast to u8 / u16 /
f16, bound as narrow members.  Three calls per format and member count: the binned estimator (80 bins), the k-NN estimator
with the default k = ceil(3 cs / 100), and with k = 1 (up to 96 members: the register descent).  Per call kind, on a fresh
context: the wall time of the first call (on a build that widens, it contains the one-off fp32 copy); then, after a warm-up
of 3 calls, `--blocks` blocks of `--reps` calls, kernel time from crf_take_kernel_time, one median per block; the wall time
of a steady call; free device memory and the size of the fp32 copy at the end.

usage: tools/measure_narrow_dkl.py --out FILE [--size 256] [--members 24 64 100 128 200] [--formats u8 u16 f16]
                                   [--kinds binned knn knn_k1] [--blocks 4] [--reps 8]
       tools/measure_narrow_dkl.py --merge PARENT.json... --against NEW.json... --out TABLE.md
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
KINDS = ("binned", "knn", "knn_k1")


def default_k(cs):
    return max(-(-3 * cs // 100), 1)


def instantiation(cs, kind):
    """The kernel instantiation a call runs (launch_dkl_format, kernels_dkl.hip): the padded network size, or the counting sort."""
    networks = cs <= (96 if kind == "binned" else 128)
    return f"N = {(cs + 15) // 16 * 16}" if networks else "counting sort"


def measure(a):
    import torch
    import correrender_amd as ca
    n = a.size
    voxels = n * n * n
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
            for kind in a.kinds:
                estimator = "binned" if kind == "binned" else "knn"
                kw = dict(num_bins=NUM_BINS, k=1 if kind == "knn_k1" else default_k(cs))
                rec = {"k": kw["k"], "instantiation": instantiation(cs, kind)}
                torch.cuda.empty_cache()
                eng = ca.CorrField(0)
                eng.set_grid(n, n, n, cs)
                eng.bind_members(narrow)
                eng.set_profiling(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.dkl_device(estimator, out, **kw)
                torch.cuda.synchronize()
                rec["first_wall_ms"] = (time.perf_counter() - t0) * 1e3
                for _ in range(3):
                    eng.dkl_device(estimator, out, **kw)
                torch.cuda.synchronize()
                eng.take_kernel_time()
                medians = []
                for _ in range(a.blocks):
                    times = []
                    for _ in range(a.reps):
                        eng.dkl_device(estimator, out, **kw)
                        ms, launches = eng.take_kernel_time()
                        times.append(ms / max(launches, 1))
                    medians.append(statistics.median(times))
                rec["kernel"] = eng.last_kernel_name()
                rec["block_medians_ms"] = medians
                t0 = time.perf_counter()
                eng.dkl_device(estimator, out, **kw)
                torch.cuda.synchronize()
                rec["steady_wall_ms"] = (time.perf_counter() - t0) * 1e3
                rec["free_device_bytes"] = int(torch.cuda.mem_get_info()[0])
                rec["wide_copy_bytes"] = eng.wide_copy_bytes()
                rec["checksum"] = float(torch.nan_to_num(out).double().sum())
                rec["nan_voxels"] = int(torch.isnan(out).sum())
                result["runs"][f"{fmt}:{cs}:{kind}"] = rec
                print(fmt, cs, kind, json.dumps(rec), flush=True)
                eng.close()
            del narrow
            torch.cuda.empty_cache()
        del base
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1))


def merge(a):
    def load(paths):  # files of one process may be split by member count / call kind: same stem up to the last '.'
        merged = {}
        for p in paths:
            d = json.loads(Path(p).read_text())
            merged.setdefault(Path(p).name.split(".")[0], {"size": d["size"], "runs": {}})["runs"].update(d["runs"])
        return list(merged.values())
    runs = {"parent": load(a.merge), "native": load(a.against)}
    n = runs["parent"][0]["size"]
    lines = [f"DKL on narrow members, {n}^3, kernel ms from crf_take_kernel_time ({NUM_BINS} bins; k-NN with the default "
             "k = ceil(3 cs / 100) and with k = 1).  (a) parent: dkl_kernel on the widened copy, steady state; (b) this commit: "
             f"dkl_narrow_kernel.  Each figure is the median of the block medians of {len(runs['parent'])} alternating "
             "processes per build; spread = max - min of the parent's block medians (the run-to-run spread the acceptance "
             "rule uses).", "",
             "| format | members | estimator | k | instantiation | (a) parent ms | spread of (a) | (b) native ms | (b) / (a) | "
             "within rule | NaN voxels | kernels (a) -> (b) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    keys = list(runs["parent"][0]["runs"])
    for key in keys:
        fmt, cs, kind = key.split(":")
        med = {side: [m for r in runs[side] if key in r["runs"] for m in r["runs"][key]["block_medians_ms"]] for side in runs}
        pa, na = statistics.median(med["parent"]), statistics.median(med["native"])
        spread = max(med["parent"]) - min(med["parent"])
        first = runs["parent"][0]["runs"][key]
        names = " -> ".join(runs[side][0]["runs"][key]["kernel"] for side in ("parent", "native"))
        same = all(r["runs"][key]["checksum"] == first["checksum"] and r["runs"][key]["nan_voxels"] == first["nan_voxels"]
                   for s in runs for r in runs[s] if key in r["runs"])
        lines.append(f"| {fmt} | {cs} | {'binned' if kind == 'binned' else 'k-NN'} | {first['k'] if kind != 'binned' else ''} | "
                     f"{first['instantiation']} | {pa:.3f} | {spread:.3f} | {na:.3f} | {na / pa:.3f} | "
                     f"{'yes' if na <= pa + spread else 'NO'} | {first['nan_voxels']} | "
                     f"{names}{'' if same else ' (CHECKSUMS DIFFER)'} |")
    lines += ["", "| format | members | call | build | first call wall ms | steady call wall ms | one-off copy ms (difference) | "
              "free device memory GiB | fp32 copy GiB |", "|---|---|---|---|---|---|---|---|---|"]
    for key in keys:
        fmt, cs, kind = key.split(":")
        for side in ("parent", "native"):
            recs = [r["runs"][key] for r in runs[side] if key in r["runs"]]
            md = lambda k: statistics.median(r[k] for r in recs)
            lines.append(f"| {fmt} | {cs} | {kind} | {side} | {md('first_wall_ms'):.1f} | {md('steady_wall_ms'):.1f} | "
                         f"{md('first_wall_ms') - md('steady_wall_ms'):.1f} | {md('free_device_bytes') / 2**30:.2f} | "
                         f"{recs[0]['wide_copy_bytes'] / 2**30:.2f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).write_text(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, nargs="+", default=[24, 64, 100, 128, 200])
    ap.add_argument("--formats", nargs="+", default=list(FORMATS), choices=FORMATS)
    ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=KINDS)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--against", nargs="+")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    merge(a) if a.merge else measure(a)


if __name__ == "__main__":
    main()
