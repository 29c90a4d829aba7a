#!/usr/bin/env python3
"""Times the per-node statistics pass (fognet_node_stats_dev) and its job reduction
(fognet_reduce_node_stats_dev) against the stand-alone replication pass
(fognet_rep_stats_dev), which streams the same 33 B per task and is the yardstick.

Shapes: C3 (R = 4,096, T = 100k, N = 256) and C5 flat (R = 1,024, T = 10k, N = 10,000),
traces generated on the device as bench.py does.  Each pass: warm-up launches, then
timed repeats between events on the stream; the median is reported, with the achieved
GB/s over the bytes the pass must move (33 B per task + its records).

  python tools/node_stats_timing.py [--out profiles/node_stats_timing.txt] [--reps N]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fognetsimpp_amd as fa  # noqa: E402
from fognetsimpp_amd import _abi  # noqa: E402

SHAPES = {"c3": (4096, 100_000, 256), "c5flat": (1024, 10_000, 10_000)}


def timed(fn, warmup: int, reps: int) -> list[float]:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="c3,c5flat")
    args = ap.parse_args()
    ctx = fa.Context(0)
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.reps} timed launches after {args.warmup} warm-up"]
    for name in args.shapes.split(","):
        R, T, N = SHAPES[name]
        mg, sc = (fa.c5_params if name == "c5flat" else fa.sweep_params)(np.arange(R), N)
        d = fa.generate_trace(ctx, 0x5EED0003, R, T, N, mg, sc)
        tr = {k: v for k, v in d.items() if not k.startswith("_")}
        out = fa.run_batch(ctx, tr)
        torch.cuda.synchronize()
        ok = int((out.rep_stats()["status"] == 0).sum())
        nodes = torch.empty(R * N * _abi.NODE_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        job = torch.empty(N * _abi.NODE_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        task_bytes = 33 * R * T
        rec_bytes = R * N * _abi.NODE_STATS_DTYPE.itemsize
        passes = {
            "rep_stats": (lambda: fa.run_batch(ctx, tr, out=out, stage="stats"), task_bytes),
            "node_stats": (lambda: fa.node_stats(ctx, tr, out, res=nodes), task_bytes + rec_bytes),
            "node_stats[hbm]": (lambda: fa.node_stats(ctx, tr, out, res=nodes), task_bytes + rec_bytes),
            "reduce_node_stats": (lambda: fa.reduce_node_stats(ctx, nodes, out.stats, R, N, out=job), rec_bytes),
        }
        med = {}
        for pname, (fn, nbytes) in passes.items():
            if pname.endswith("[hbm]"):
                os.environ["FOGNET_NODE_STATS"] = "hbm"
            ms = timed(fn, args.warmup, args.reps)
            os.environ.pop("FOGNET_NODE_STATS", None)
            med[pname] = statistics.median(ms)
            lines.append(f"{name} R={R} T={T} N={N} ok={ok} {pname}: median {med[pname]:.3f} ms (min {min(ms):.3f}, max "
                         f"{max(ms):.3f}), {nbytes / 1e6:.1f} MB, {nbytes / med[pname] / 1e6:.1f} GB/s")
        lines.append(f"{name}: node_stats / rep_stats = {med['node_stats'] / med['rep_stats']:.3f} (bytes ratio "
                     f"{(task_bytes + rec_bytes) / task_bytes:.3f})")
        del d, tr, out, nodes, job
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
