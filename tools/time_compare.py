#!/usr/bin/env python3
"""Times the paired comparison (fognet_compare_dev) and its job reduction
(fognet_reduce_compare_dev) beside the yardstick: fognet_node_stats_dev on A's outputs, which
streams one replay's rows (33 B per decided task) and commits per node with keyed atomics.

Bytes the comparison must move: node, status, start_tick and done_tick of both replays, 42 B per
decided task, and one 400-B record per replication; the reduction reads the R records.

Shapes: C3 (R = 4,096, T = 100k, N = 256), C5 flat (R = 64, T = 100k, N = 10,000) and the
driver's (R = 4, T = 600, N = 5), traces generated on the device as bench.py does.  A is the
REF_V3 replay, B the same traces under round-robin decisions (fognet_run_assigned_dev); both
outputs are replayed once and reused.  Each: warm-up launches, then timed repeats between events
on the stream; the minimum and the median are reported.

  python tools/time_compare.py [--out profiles/compare_timing.txt] [--shapes c3,c5,driver] [--tag T]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fognetsimpp_amd import _abi  # noqa: E402

if os.environ.get("FOGNET_LIB"):  # a variant build (tools/build_variant.sh)
    _abi.LIB_PATH = os.environ["FOGNET_LIB"]
import fognetsimpp_amd as fa  # noqa: E402

SHAPES = {"c3": (4096, 100_000, 256), "c5": (64, 100_000, 10_000), "driver": (4, 600, 5)}
ROW_BYTES, NODE_ROW_BYTES = 42, 33


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
    ap.add_argument("--tag", default="")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="c3,c5,driver")
    args = ap.parse_args()
    ctx = fa.Context(0)
    dev = torch.device("cuda", 0)
    tag = f"[{args.tag}] " if args.tag else ""
    lines = [f"{tag}device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH)}; minimum and median of "
             f"{args.reps} timed launches after {args.warmup} warm-up"]

    def report(name, ms, nbytes):
        lo, med = min(ms), statistics.median(ms)
        lines.append(f"{tag}{name}: min {lo:.3f} ms, median {med:.3f} ms (max {max(ms):.3f}); {nbytes / 1e6:.1f} MB read, "
                     f"{nbytes / med / 1e6:.1f} GB/s at the median ({nbytes / lo / 1e6:.1f} at the minimum)")
        return med

    for shape in args.shapes.split(","):
        R, T, N = SHAPES[shape]
        mg, sc = (fa.c5_params if shape == "c5" else fa.sweep_params)(np.arange(R), N)
        d = fa.generate_trace(ctx, 0x5EED0003, R, T, N, mg, sc)
        tr = {k: v for k, v in d.items() if not k.startswith("_")}
        out_a = fa.run_batch(ctx, tr)
        out_b = fa.run_assigned(ctx, tr, fa.assign_round_robin(R, T, N, dev))
        torch.cuda.synchronize()
        sa, sb = out_a.rep_stats(), out_b.rep_stats()
        both = (sa["status"] == 0) & (sb["status"] == 0)
        pairs = int(np.minimum(sa["n_tasks"], sb["n_tasks"])[both].sum())
        decided_a = int(sa["n_tasks"][sa["status"] == 0].sum())
        rec_bytes = _abi.COMPARE_STATS_DTYPE.itemsize
        nodes = torch.empty(R * N * _abi.NODE_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        cmp = torch.empty(R * rec_bytes, dtype=torch.uint8, device=dev)
        job = torch.empty(rec_bytes, dtype=torch.uint8, device=dev)
        hist = torch.zeros((2, _abi.HIST_BINS), dtype=torch.int64, device=dev)
        unit = report(f"{shape} node_stats on A (the yardstick)", timed(lambda: fa.node_stats(ctx, tr, out_a, res=nodes),
                                                                        args.warmup, args.reps), NODE_ROW_BYTES * decided_a)
        pas = report(f"{shape} compare", timed(lambda: fa.compare(ctx, out_a, out_b, res=cmp, hist=hist), args.warmup, args.reps),
                     ROW_BYTES * pairs)
        plain = report(f"{shape} compare without hist", timed(lambda: fa.compare(ctx, out_a, out_b, res=cmp), args.warmup, args.reps),
                       ROW_BYTES * pairs)
        red = report(f"{shape} reduce_compare", timed(lambda: ctx.check(ctx._lib.fognet_reduce_compare_dev(
            ctx.handle, fa.engine._ptr(cmp), R, fa.engine._ptr(job), fa.engine._stream_ptr(dev))), args.warmup, args.reps),
            R * rec_bytes)
        j = job.cpu().numpy().view(_abi.COMPARE_STATS_DTYPE)[0]
        lines.append(f"{tag}{shape} R={R} T={T} N={N} compared={int(j['n_reps'])} pairs={int(j['n_pairs'])} moved={int(j['n_moved'])} "
                     f"better/equal/worse={int(j['n_better'])}/{int(j['n_equal'])}/{int(j['n_worse'])}")
        lines.append(f"{tag}{shape} compare {pas:.3f} ms = {pas / unit:.2f} x node_stats in time, "
                     f"{(ROW_BYTES * pairs / pas) / (NODE_ROW_BYTES * decided_a / unit):.2f} x node_stats in bytes/s "
                     f"(without hist {plain:.3f} ms); reduction {red:.3f} ms")
        del d, tr, out_a, out_b, nodes, cmp
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.tag else "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
