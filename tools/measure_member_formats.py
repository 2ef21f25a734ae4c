#!/usr/bin/env python3
"""A/B of the Pearson field kernel on narrow native members against fp32 members that hold the same converted values.

Workload: the 256^3 x 64 box ensemble, rescaled to [0, 1] by its global extrema and cast to u8 / u16 / f16.  Metric: the
per-voxel kernel's time from crf_set_profiling (HIP events around the kernel).  Both sides run in ONE process on one
context pair, alternating native / fp32 (raw layout: the parent commit's kernel) `--alternations` times with `--reps`
evaluations each after a warm-up; reported are the median of the per-alternation medians and the spread (max - min) of
those medians.  Prints a markdown table; `--out` also writes it to a file.

usage: tools/measure_member_formats.py [--size 256] [--members 64] [--alternations 7] [--reps 20] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import correrender_amd as ca  # noqa: E402
from correrender_amd import Measure  # noqa: E402


def kernel_ms(eng, out, ref, reps):
    eng.compute_device(Measure.PEARSON, out, ref)  # warm-up (and any one-time copy)
    eng.take_kernel_time()
    times = []
    for _ in range(reps):
        eng.compute_device(Measure.PEARSON, out, ref)
        ms, n = eng.take_kernel_time()
        times.append(ms / max(n, 1))
    return statistics.median(times)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, cs = a.size, a.members
    voxels = n * n * n
    ref = (n // 2, n // 2, n // 2)
    gen = ca.CorrField(0)
    base = torch.empty((cs, voxels), dtype=torch.float32, device="cuda")
    for c in range(cs):
        gen.synth_box_member(base[c], n, n, n, 0, n, c, cs, 1)
    torch.cuda.synchronize()
    lo, hi = base.min(), base.max()
    base = (base - lo) / (hi - lo)
    out = torch.empty(voxels, dtype=torch.float32, device="cuda")
    lines = [f"Pearson field kernel, {n}^3 x {cs}, {a.alternations} alternations x {a.reps} evaluations, kernel ms "
             "(median of the alternations' medians; spread = max - min of those medians)", "",
             "| format | native ms | spread | fp32 ms | spread | native / fp32 | bit-identical |", "|---|---|---|---|---|---|---|"]
    for fmt in ("f16", "u16", "u8"):
        if fmt == "f16":
            narrow = base.to(torch.float16)
            wide = narrow.to(torch.float32)
        else:
            top = 65535.0 if fmt == "u16" else 255.0
            codes = torch.round(base * top)
            # (uint16 through the int16 of the same bits: torch converts to uint16 in few releases)
            narrow = (codes.to(torch.int32).to(torch.int16).view(torch.uint16) if fmt == "u16"
                      else codes.to(torch.int32).to(torch.uint8))
            # the table's value: the IEEE quotient by a TENSOR (a scalar divisor becomes a multiply by its reciprocal)
            wide = torch.div(codes.to(torch.float32), torch.full_like(codes, top, dtype=torch.float32))
        engines = {}
        for name, members in (("native", narrow), ("fp32", wide)):
            eng = ca.CorrField(0)
            eng.set_grid(n, n, n, cs)
            eng.set_member_layout("raw")
            eng.bind_members(members)
            eng.set_profiling(True)
            engines[name] = eng
        results = {}
        for name, eng in engines.items():
            eng.compute_device(Measure.PEARSON, out, ref)
            torch.cuda.synchronize()
            results[name] = out.clone()
        assert engines["native"].last_member_format() == fmt and engines["fp32"].last_member_format() == "f32"
        same = bool(((results["native"].view(torch.int32) == results["fp32"].view(torch.int32))
                     | (results["native"].isnan() & results["fp32"].isnan())).all())
        medians = {"native": [], "fp32": []}
        for _ in range(a.alternations):
            for name in ("native", "fp32"):
                medians[name].append(kernel_ms(engines[name], out, ref, a.reps))
        nat, f32 = statistics.median(medians["native"]), statistics.median(medians["fp32"])
        lines.append(f"| {fmt} | {nat:.4f} | {max(medians['native']) - min(medians['native']):.4f} | {f32:.4f} | "
                     f"{max(medians['fp32']) - min(medians['fp32']):.4f} | {nat / f32:.3f} | {same} |")
        for eng in engines.values():
            eng.close()
        del narrow, wide, engines, results
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
