#!/usr/bin/env python3
"""Times crf_kendall_values_device (CorrField.kendall_values) and crf_field_kendall_similarity
(CorrField.field_kendall_similarity) -- kernels_kendall_similarity.hip: two device-wide sorts, a tile kernel and merge
levels that count inversions -- and, beside every figure, crf_field_rank_similarity (Spearman) on the same data in the same
run: that call's code is the yardstick.

Workloads:
  kendall_values             2^24 and 2^28 pairs (--log2): "normal" (x normal, y = x / 2 + normal: all digit passes run) and
                             "quantised" (both rounded to a dozen levels: long runs of equal values in both sorts and of
                             equal run starts in the merges).  The same two arrays are bound as a primary and a secondary
                             field of 256^3 voxels per member for the Spearman call and for the field call.
  field_kendall_similarity   two size^3 box ensembles (seeds 1 and 2) of --members fp32 members, one member and all members
  tile sweep                 kendall_values on the "normal" pairs with CRF_KENDALL_TILE_KEYS = 64, 128, 256, 512 and 1024
After a warm-up, `--blocks` rounds of `--reps` calls: wall ms per call (a host clock around the synchronous call) and
kernel ms (crf_take_kernel_time: one event pair around all launches of the call, the host's read of the digit histograms
in between included), one median per block; the figure is the median of the block medians, the spread max - min of them.

Algorithmic bytes of a Kendall call over n pairs of which k are kept, with p digit passes run in all and L merge levels:
keys 16 n (x and y read, two keys stored); per pass 20 n (count 4 n; scatter: key and payload read and stored); run starts
4 n + 16 n after the first sort (heads; keys and payload read, the next pair stored) and 4 n + 4 n after the second; tile
kernel 8 k; 8 k per merge level.  The field call adds the masking pass (16 n).  The Spearman call's bytes are those of
tools/measure_rank_similarity.py.

--one-call LOG2 makes a single kendall_values call on "normal" pairs and nothing else: the workload of a
`rocprofv3 --kernel-trace` run of its own, whose kernel-trace csv --trace turns into the per-kernel table.

usage: tools/measure_kendall_similarity.py --out TABLE.md [--json FILE] [--size 256] [--members 64] [--log2 24 28]
                                           [--blocks 3] [--reps 2] [--trace CSV ...]
       tools/measure_kendall_similarity.py --one-call 28
       tools/measure_kendall_similarity.py --from-json FILE --trace CSV --out TABLE.md
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
from collections import defaultdict
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from measure_rank_similarity import passes_run, sort_bytes, time_calls  # noqa: E402

DEFAULT_TILE, CHUNK = 256, 2048
TILES = (64, 128, 256, 512, 1024)


def merge_levels(kept, tile=DEFAULT_TILE):
    levels, run = 0, tile
    while run < kept:
        levels, run = levels + 1, run * 2
    return levels


def kendall_bytes(n, kept, passes, levels, field):
    return n * (16 + 20 * passes + 20 + 8 + (16 if field else 0)) + kept * 8 * (1 + levels)


def spearman_bytes(n, passes):
    return 32 * n + sum(sort_bytes(n, p) for p in passes)


def pairs(log2, kind, seed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = 1 << log2
    x = torch.randn(n, dtype=torch.float32, device="cuda", generator=gen)
    y = 0.5 * x + torch.randn(n, dtype=torch.float32, device="cuda", generator=gen)
    if kind == "quantised":                                                  # twelve levels a side
        x, y = torch.round(x * 2.0).clamp_(-6.0, 5.0), torch.round(y * 2.0).clamp_(-6.0, 5.0)
    return x.contiguous(), y.contiguous()


def one_call(log2):
    import torch
    import correrender_amd as ca
    eng = ca.CorrField(0)
    x, y = pairs(log2, "normal", log2)
    torch.cuda.synchronize()
    print("kendall_values", log2, eng.kendall_values(x, y, return_counts=True), flush=True)
    eng.close()


def measure(a):
    import torch
    import correrender_amd as ca
    from correrender_amd import Measure
    eng = ca.CorrField(0)
    eng.set_profiling(True)
    result = {"library": str(ca._lib.library_path()), "size": a.size, "members": a.members, "blocks": a.blocks,
              "reps": a.reps, "values": {}, "field": {}, "tiles": {}}

    def kernel_ms():
        ms, launches = eng.take_kernel_time()
        assert launches == 1
        return ms

    def both(n, passes, member, reps):
        """The field call and the Spearman call on the bound fields; Kendall first, on a fresh scratch buffer."""
        call = lambda: eng.field_kendall_similarity(member=member, return_samples=True, return_counts=True)
        value, kept, counts = call()
        eng.take_kernel_time()
        levels = merge_levels(kept)
        rec = time_calls(call, kernel_ms, a.blocks, reps)
        rec.update(value=value, samples=kept, counts=counts, passes=passes, levels=levels, kernel=eng.last_kernel_name(),
                   bytes=kendall_bytes(n, kept, sum(passes), levels, True), scratch_bytes=eng.rank_scratch_bytes())
        call = lambda: eng.field_rank_similarity(Measure.SPEARMAN, member=member, return_samples=True)
        call()
        eng.take_kernel_time()
        rec["spearman"] = time_calls(call, kernel_ms, a.blocks, reps)
        rec["spearman"].update(bytes=spearman_bytes(n, passes), scratch_bytes=eng.rank_scratch_bytes())
        return rec

    side = 256
    for log2 in a.log2:
        n = 1 << log2
        cs = n // side ** 3
        for kind in ("normal", "quantised"):
            x, y = pairs(log2, kind, log2)
            passes = [passes_run(x), passes_run(y)]
            call = lambda: eng.kendall_values(x, y, return_counts=True)
            value, kept, counts = call()
            eng.take_kernel_time()
            levels = merge_levels(kept)
            reps = a.reps if log2 < 28 else max(1, a.reps // 2)
            rec = time_calls(call, kernel_ms, a.blocks, reps)
            rec.update(values=n, value=value, kept=kept, counts=counts, passes=passes, levels=levels,
                       bytes=kendall_bytes(n, kept, sum(passes), levels, False), scratch_bytes=eng.rank_scratch_bytes())
            if kind == "normal":
                for tile in TILES:
                    os.environ["CRF_KENDALL_TILE_KEYS"] = str(tile)
                    again = call()
                    assert again == (value, kept, counts)
                    eng.take_kernel_time()
                    t = time_calls(call, kernel_ms, a.blocks, reps)
                    t["levels"] = merge_levels(kept, tile)
                    result["tiles"][f"2^{log2}:{tile}"] = t
                del os.environ["CRF_KENDALL_TILE_KEYS"]
            eng.set_grid(side, side, side, cs)                               # a fresh scratch buffer
            eng.bind_members(x.view(cs, side ** 3))
            eng.bind_secondary_members(y.view(cs, side ** 3))
            rec["as_fields"] = both(n, passes, None, reps)
            assert rec["as_fields"]["counts"] == counts
            result["values"][f"2^{log2}:{kind}"] = rec
            print("values", log2, kind, json.dumps(rec), flush=True)
            eng.set_grid(side, side, side, cs)
            del x, y
            torch.cuda.empty_cache()

    n, cs = a.size, a.members
    voxels = n * n * n
    fields = []
    for seed in (1, 2):
        f = torch.empty((cs, voxels), dtype=torch.float32, device="cuda")
        eng.set_grid(n, n, n, cs)
        for c in range(cs):
            eng.synth_box_member(f[c], n, n, n, 0, n, c, cs, seed)
        fields.append(f)
    torch.cuda.synchronize()
    for member in (cs // 2, None):
        eng.set_grid(n, n, n, cs)
        eng.bind_members(fields[0])
        eng.bind_secondary_members(fields[1])
        sel = slice(0, cs) if member is None else slice(member, member + 1)
        passes = [passes_run(f[sel]) for f in fields]
        samples = voxels * (cs if member is None else 1)
        rec = both(samples, passes, member, max(1, a.reps // 2) if member is None else a.reps)
        result["field"]["all" if member is None else "one"] = rec
        print("field", member, json.dumps(rec), flush=True)
    eng.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(result, indent=1))
    write_table(a, result)


def kernel_split(paths):
    """{kernel: (launches, total ms)} of the library's kernels in rocprofv3 kernel-trace csv files."""
    total = defaultdict(lambda: [0, 0.0])
    for path in paths:
        with open(path, newline="") as fh:
            for r in csv.DictReader(fh):
                found = re.search(r"\b((?:kendall|rank|similarity)_\w*_kernel)\b", r["Kernel_Name"])
                if not found:
                    continue
                name = found.group(1)
                total[name][0] += 1
                total[name][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    return total


def write_table(a, result):
    med = statistics.median
    spread = lambda v: max(v) - min(v)
    k_of = lambda rec: med(rec["kernel_block_medians_ms"])

    def row(label, n, rec, field):
        sp = rec["spearman"] if field else rec["as_fields"]["spearman"]
        k, s = k_of(rec), k_of(sp)
        rate = sp["bytes"] / (s * 1e-3)
        return (f"| {label} | {n} | {rec['passes'][0]}, {rec['passes'][1]} | {rec['levels']} | {med(rec['wall_block_medians_ms']):.2f} | "
                f"{k:.2f} | {spread(rec['kernel_block_medians_ms']):.2f} | {rec['bytes'] / 1e9:.2f} | "
                f"{rec['bytes'] / (k * 1e-3) / 1e9:.0f} | {med(sp['wall_block_medians_ms']):.2f} | {s:.2f} | {sp['bytes'] / 1e9:.2f} | "
                f"{rate / 1e9:.0f} | {rec['bytes'] / rate * 1e3:.2f} | {k - rec['bytes'] / rate * 1e3:+.2f} | "
                f"{rec['scratch_bytes'] / 2 ** 20:.0f} | {sp['scratch_bytes'] / 2 ** 20:.0f} |")

    head = ("| {} | samples | digit passes run (x, y) | merge levels | Kendall ms per call | Kendall kernel ms | spread | Kendall "
            "algorithmic GB | GB/s | Spearman ms per call | Spearman kernel ms | Spearman algorithmic GB | Spearman GB/s | Kendall "
            "bytes at Spearman's GB/s, ms | excess ms | Kendall scratch MiB | Spearman scratch MiB |")
    rule = "|" + "---|" * 17
    n, cs = result["size"], result["members"]
    lines = [f"Kendall's tau-b over all samples (kernels_kendall_similarity.hip), tiles of {DEFAULT_TILE} values and merge chunks of up to "
             f"{CHUNK}.  {result['blocks']} blocks of {result['reps']} calls after a warm-up (half as many at 2^28 pairs and with all "
             "members); a figure is the median of the block medians, the spread max - min of them.  ms per call: host clock around "
             "the synchronous call; kernel ms: crf_take_kernel_time (one event pair around all launches of the call, the host's "
             "reads of the digit histograms in between included).  Bytes: the algorithmic bytes of the passes and levels that ran "
             "(tools/measure_kendall_similarity.py).  Spearman: crf_field_rank_similarity on the same data in the same run, its "
             "code unchanged from the parent commit.  Excess: the Kendall kernel ms beyond what its bytes take at the Spearman "
             "call's measured rate.", "",
             "crf_kendall_values_device (the Spearman call, and its scratch, on the same two arrays bound as fields of 256^3 voxels "
             "per member):", "", head.format("input"), rule]
    for key, rec in result["values"].items():
        size, kind = key.split(":")
        lines.append(row(f"{size} {kind}", rec["values"], rec, False))
    lines += ["", "crf_field_kendall_similarity on the same arrays bound as fields (the masking pass added):", "",
              head.format("input"), rule]
    for key, rec in result["values"].items():
        size, kind = key.split(":")
        lines.append(row(f"{size} {kind}", rec["values"], rec["as_fields"], True))
    lines += ["", f"crf_field_kendall_similarity, two resident fp32 box ensembles of {n}^3 x {cs} members:", "",
              head.format("members"), rule]
    for sel, rec in result["field"].items():
        lines.append(row(sel, rec["samples"], rec, True))
    lines += ["", "The tile sweep: crf_kendall_values_device on the \"normal\" pairs with CRF_KENDALL_TILE_KEYS set:", "",
              "| pairs | tile | merge levels | kernel ms | spread |", "|---|---|---|---|---|"]
    for key, rec in result["tiles"].items():
        size, tile = key.split(":")
        lines.append(f"| {size} | {tile} | {rec['levels']} | {k_of(rec):.2f} | {spread(rec['kernel_block_medians_ms']):.2f} |")
    if a.trace:
        split = kernel_split(a.trace)
        whole = sum(ms for _, ms in split.values())
        lines += ["", f"Per kernel, one crf_kendall_values_device call on 2^{a.trace_log2} \"normal\" pairs under `rocprofv3 "
                  "--kernel-trace`, a run of its own (no warm-up call; the library's kernels only):", "",
                  "| kernel | launches | total ms | share |", "|---|---|---|---|"]
        for name, (launches, ms) in sorted(split.items(), key=lambda kv: -kv[1][1]):
            lines.append(f"| {name} | {launches} | {ms:.3f} | {100 * ms / whole:.1f} % |")
        lines.append(f"| all | {sum(c for c, _ in split.values())} | {whole:.3f} | 100 % |")
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 28])
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json")
    ap.add_argument("--from-json", help="rebuild the table from a --json file of an earlier run (no GPU)")
    ap.add_argument("--trace", nargs="+", help="rocprofv3 kernel-trace csv files of a --one-call run")
    ap.add_argument("--trace-log2", type=int, default=28)
    ap.add_argument("--one-call", type=int, metavar="LOG2")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not a.one_call and not a.out:
        ap.error("--out is required")
    if a.one_call:
        one_call(a.one_call)
    elif a.from_json:
        write_table(a, json.loads(Path(a.from_json).read_text()))
    else:
        measure(a)


if __name__ == "__main__":
    main()
