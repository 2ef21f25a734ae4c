#!/usr/bin/env python3
"""Pearson field per step from the raw members and from the packed copy (crf_set_member_layout), same process, the two
layouts alternated: which member counts the packed copy pays off at.  Synthetic box ensemble, one reference point per
step, kernel times from HIP events (crf_set_profiling).
Usage: tools/measure_member_layout.py [--grid 256 256 256] [--steps 30] [--rounds 3] CS [CS ...]"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("members", type=int, nargs="+")
    ap.add_argument("--grid", type=int, nargs=3, default=[256, 256, 256])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    import correrender_amd as ca
    xs, ys, zs = args.grid
    n = xs * ys * zs
    eng = ca.CorrField(0)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    print(f"grid {xs}x{ys}x{zs}, {args.steps} steps x {args.rounds} rounds per layout; kernel ms (median of rounds)")
    print("| members | raw ms | packed ms | packed / raw | B/voxel raw | B/voxel packed |")
    print("|---|---|---|---|---|---|")
    for cs in args.members:
        eng.set_grid(xs, ys, zs, cs)
        members = torch.empty((cs, zs, ys, xs), dtype=torch.float32, device="cuda")
        for c in range(cs):
            eng.synth_box_member(members[c], xs, ys, zs, 0, zs, c, cs, 20260130, stream)
        torch.cuda.synchronize()
        eng.bind_members(members)
        times = {"raw": [], "packed": []}
        for r in range(args.rounds):
            for layout in ("raw", "packed"):
                eng.set_member_layout(layout)
                eng.compute_device(ca.Measure.PEARSON, out, (1, 2, 3))  # builds the packed copy (untimed)
                torch.cuda.synchronize()
                eng.set_profiling(True)
                eng.take_kernel_time()
                for i in range(args.steps):
                    eng.compute_device(ca.Measure.PEARSON, out, ((7 * i) % xs, (5 * i) % ys, (3 * i) % zs))
                ms, k = eng.take_kernel_time()
                eng.set_profiling(False)
                assert eng.last_member_layout() == layout
                times[layout].append(ms / k)
        raw, packed = statistics.median(times["raw"]), statistics.median(times["packed"])
        slots = (cs + 15) // 16 * 16
        pb = 16 * (slots // 8 + slots // 16 + (slots + 31) // 32) + slots / 64 + 4
        print(f"| {cs} | {raw:.4f} | {packed:.4f} | {packed / raw:.3f} | {4 * cs + 4} | {pb:.1f} |", flush=True)
        del members
        eng.set_member_layout("auto")
    eng.close()


if __name__ == "__main__":
    main()
