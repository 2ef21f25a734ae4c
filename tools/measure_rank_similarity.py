#!/usr/bin/env python3
"""Times the device-wide radix sort behind crf_rank_values_device (CorrField.rank_values) and crf_field_rank_similarity
(CorrField.field_rank_similarity, Spearman) and, beside them from the same run and device, two yardsticks: torch.sort of
the same values (rocPRIM's sort, values and indices) and, with --host-reference, the reference's own functions on the
host cores at 2^24 values.

Workloads:
  rank_values                2^24 and 2^28 values (--rank-log2), normally distributed ("normal": all four digit passes
                             run) and with 16 varying bits in the two middle bytes ("two digits": two passes are skipped)
  field_rank_similarity      two size^3 box ensembles (seeds 1 and 2) of --members fp32 members, all members and one
                             member; and two fields of the "two digits" kind of the same shape
After a warm-up, `--blocks` rounds of `--reps` calls: wall ms per call (a host clock around the synchronous call) and
kernel ms (crf_take_kernel_time: one event pair around all launches of the call, the host's read of the digit histograms
in between included), one median per block; the figure is the median of the block medians, the spread max - min of them.

Algorithmic bytes of a sort of n values with p passes run: keys 8 n (values read, keys stored); per pass 4 n (count) +
16 n (scatter: key and payload read and stored; 12 n for the first, whose payload is the identity); heads 4 n; assign
12 n (8 n without a pass).  The field similarity adds the masking pass (16 B per candidate sample) and the two passes of
the moments kernels over the rank arrays (16 B).  Share = bytes / kernel time / 6.3 TB/s, the streaming rate the device
reaches.

usage: tools/measure_rank_similarity.py --out TABLE.md [--json FILE] [--size 256] [--members 64] [--rank-log2 24 28]
                                        [--blocks 3] [--reps 3] [--host-reference]
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

STREAM_RATE = 6.3e12        # bytes/s: what streaming kernels reach on the MI355X


def sort_bytes(n, passes):
    if passes == 0:
        return n * (8 + 4 + 8)
    return n * (8 + 20 * passes - 4 + 4 + 12)


def passes_run(values):
    """How many of the four digit passes a sort of the tensor runs: the digits that are not constant over the keys."""
    import torch
    u = values.reshape(-1).view(torch.int32)
    u = torch.where(values.reshape(-1) == 0, torch.zeros_like(u), u)
    key = torch.where(u < 0, ~u, u ^ (-2 ** 31))
    key = torch.where(torch.isnan(values.reshape(-1)), torch.full_like(key, -1), key)
    run = 0
    for d in range(4):
        digit = (key >> (8 * d)) & 255
        run += int(digit.min() != digit.max())
    return run


def two_digit_values(shape, seed):
    """fp32 values in [1, 4) whose low and high bytes are constant: 65 536 levels in the two middle bytes."""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    k = torch.randint(0, 1 << 16, shape, dtype=torch.int32, device="cuda", generator=gen)
    return ((k << 8) | 0x3F800000).view(torch.float32)


def time_calls(call, take, blocks, reps):
    import torch
    for _ in range(2):
        call()
        take()
    wall, kernel = [], []
    for _ in range(blocks):
        w, k = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            w.append((time.perf_counter() - t0) * 1e3)
            k.append(take())
        wall.append(statistics.median(w))
        kernel.append(statistics.median(k))
    return {"wall_block_medians_ms": wall, "kernel_block_medians_ms": kernel}


def host_reference(x, y):
    """Wall seconds of the reference's own functions on host arrays (fp32, no NaN): computeRanks of either, then
    computePearsonParallel<double> over the two rank arrays."""
    import ctypes as C
    import oracle_lib
    from similarity_reference import PEARSON_PARALLEL_DOUBLE
    ref = oracle_lib.load_reference()
    pearson = getattr(ref.lib, PEARSON_PARALLEL_DOUBLE)
    pearson.restype = C.c_float
    pearson.argtypes = [oracle_lib.FP, oracle_lib.FP, C.c_int]
    rec = {"samples": int(x.size), "omp_threads": int(os.environ.get("OMP_NUM_THREADS", "0"))}
    t0 = time.perf_counter()
    rx = ref.ranks(x)
    rec["ranks_x_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ry = ref.ranks(y)
    rec["ranks_y_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    rec["spearman_value"] = float(pearson(oracle_lib._fp(rx), oracle_lib._fp(ry), rx.size))
    rec["pearson_of_ranks_s"] = time.perf_counter() - t0
    return rec


def measure(a):
    import torch
    import correrender_amd as ca
    from correrender_amd import Measure
    eng = ca.CorrField(0)
    eng.set_profiling(True)
    result = {"library": str(ca._lib.library_path()), "size": a.size, "members": a.members, "blocks": a.blocks,
              "reps": a.reps, "rank_values": {}, "field": {}, "host_reference": {}}

    def kernel_ms():
        ms, launches = eng.take_kernel_time()
        assert launches == 1
        return ms

    # ---- rank_values against torch.sort
    for log2 in a.rank_log2:
        n = 1 << log2
        gen = torch.Generator(device="cuda").manual_seed(log2)
        inputs = {"normal": torch.randn(n, dtype=torch.float32, device="cuda", generator=gen),
                  "two digits": two_digit_values((n,), log2)}
        for name, v in inputs.items():
            passes = passes_run(v)
            rec = time_calls(lambda: eng.rank_values(v), kernel_ms, a.blocks, a.reps)
            rec.update(values=n, passes=passes, bytes=sort_bytes(n, passes), scratch_bytes=eng.rank_scratch_bytes())
            events = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

            def sort_call():
                events[0].record()
                torch.sort(v)
                events[1].record()

            def sort_ms():
                torch.cuda.synchronize()
                return events[0].elapsed_time(events[1])
            rec["torch_sort"] = time_calls(sort_call, sort_ms, a.blocks, a.reps)
            result["rank_values"][f"2^{log2}:{name}"] = rec
            print("rank_values", log2, name, json.dumps(rec), flush=True)
            if a.host_reference and log2 == 24 and name == "normal":
                x = v.cpu().numpy()
                y = (0.5 * v + torch.randn(n, dtype=torch.float32, device="cuda", generator=gen)).cpu().numpy()
                result["host_reference"] = host_reference(x, y)
                print("host reference", json.dumps(result["host_reference"]), flush=True)
        del inputs, v
        torch.cuda.empty_cache()

    # ---- field_rank_similarity
    n, cs = a.size, a.members
    voxels = n * n * n
    eng.set_grid(n, n, n, cs)
    for kind in ("box ensembles", "two digits"):
        fields = []
        for seed in (1, 2):
            if kind == "two digits":
                fields.append(two_digit_values((cs, voxels), seed))
                continue
            f = torch.empty((cs, voxels), dtype=torch.float32, device="cuda")
            for c in range(cs):
                eng.synth_box_member(f[c], n, n, n, 0, n, c, cs, seed)
            fields.append(f)
        torch.cuda.synchronize()
        eng.bind_members(fields[0])
        eng.bind_secondary_members(fields[1])
        for member in (cs // 2, None):
            sel = slice(0, cs) if member is None else slice(member, member + 1)
            passes = [passes_run(f[sel]) for f in fields]
            samples = voxels * (cs if member is None else 1)
            call = lambda: eng.field_rank_similarity(Measure.SPEARMAN, member=member, return_samples=True)
            value, kept = call()
            eng.take_kernel_time()
            reps = max(1, a.reps // 2) if member is None else a.reps
            rec = time_calls(call, kernel_ms, a.blocks, reps)
            rec.update(value=value, samples=kept, passes=passes, kernel=eng.last_kernel_name(),
                       bytes=32 * samples + sum(sort_bytes(samples, p) for p in passes),
                       scratch_bytes=eng.rank_scratch_bytes())
            result["field"][f"{kind}:{'all' if member is None else 'one'}"] = rec
            print("field", kind, member, json.dumps(rec), flush=True)
        del fields
        torch.cuda.empty_cache()
    eng.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(result, indent=1))
    write_table(a, result)


def write_table(a, result):
    med = statistics.median
    spread = lambda v: max(v) - min(v)
    n, cs = result["size"], result["members"]
    lines = [f"The device-wide radix sort of kernels_rank_similarity.hip.  {result['blocks']} blocks of {result['reps']} calls "
             "after a warm-up (half as many per block with all members); a figure is the median of the block medians, the spread "
             "max - min of them.  ms per call: host clock around the synchronous call; kernel ms: crf_take_kernel_time (one event "
             "pair around all launches of the call).  Bytes: the algorithmic bytes of the passes that ran "
             "(tools/measure_rank_similarity.py); share of the 6.3 TB/s streaming rate.  torch.sort: the same values on the same "
             "device in the same run (values and int64 indices; device events around the call).", "",
             "crf_rank_values_device:", "",
             "| values | input | digit passes run | ms per call | kernel ms | spread | algorithmic GB | GB/s | share of 6.3 TB/s | "
             "torch.sort ms | spread | kernel ms / torch.sort ms | scratch MiB |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for key, rec in result["rank_values"].items():
        size, name = key.split(":")
        k, t = med(rec["kernel_block_medians_ms"]), med(rec["torch_sort"]["kernel_block_medians_ms"])
        rate = rec["bytes"] / (k * 1e-3)
        lines.append(f"| {size} | {name} | {rec['passes']} | {med(rec['wall_block_medians_ms']):.3f} | {k:.3f} | "
                     f"{spread(rec['kernel_block_medians_ms']):.3f} | {rec['bytes'] / 1e9:.3f} | {rate / 1e9:.0f} | "
                     f"{100 * rate / STREAM_RATE:.1f} % | {t:.3f} | {spread(rec['torch_sort']['kernel_block_medians_ms']):.3f} | "
                     f"{k / t:.2f} | {rec['scratch_bytes'] / 2 ** 20:.0f} |")
    lines += ["", f"crf_field_rank_similarity (Spearman), two resident fp32 fields of {n}^3 x {cs} members:", "",
              "| fields | members | samples | digit passes run (x, y) | ms per call | kernel ms | spread | algorithmic GB | GB/s | "
              "share of 6.3 TB/s | scratch MiB |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for key, rec in result["field"].items():
        kind, sel = key.split(":")
        k = med(rec["kernel_block_medians_ms"])
        rate = rec["bytes"] / (k * 1e-3)
        lines.append(f"| {kind} | {sel} | {rec['samples']} | {rec['passes'][0]}, {rec['passes'][1]} | "
                     f"{med(rec['wall_block_medians_ms']):.3f} | {k:.3f} | {spread(rec['kernel_block_medians_ms']):.3f} | "
                     f"{rec['bytes'] / 1e9:.3f} | {rate / 1e9:.0f} | {100 * rate / STREAM_RATE:.1f} % | "
                     f"{rec['scratch_bytes'] / 2 ** 20:.0f} |")
    if result["host_reference"]:
        rec = result["host_reference"]
        lines += ["", "The reference's own functions on the host cores (oracle/_ref, one call each, wall time): computeRanks is a "
                  "single-threaded std::sort of (value, index) pairs.", "",
                  "| samples | OpenMP threads | computeRanks(x) s | computeRanks(y) s | computePearsonParallel<double> over the ranks s |",
                  "|---|---|---|---|---|",
                  f"| {rec['samples']} | {rec['omp_threads']} | {rec['ranks_x_s']:.3f} | {rec['ranks_y_s']:.3f} | "
                  f"{rec['pearson_of_ranks_s']:.3f} |"]
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--rank-log2", type=int, nargs="+", default=[24, 28])
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
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
