#!/usr/bin/env python3
"""Times the queue-length pass (fognet_queue_stats_dev): count + build (FOGNET_QUEUE_STAGES=1) and
the whole pass, so build and measure are reported separately, beside the yardstick:
fognet_node_stats_dev on the same replay outputs, which streams the same rows once and commits
per node.

Bytes each part must move: count + build read node and status twice and arrive and start_tick
once (26 B per decided task) and write one element (28 B) per queued task; measure reads every
element once and writes the records (176 B per replication and node).

Shapes: C3 (R = 4,096, T = 100k, N = 256), C5 flat (R = 64, T = 100k, N = 10,000) and the
driver's (R = 4, T = 600, N = 5), traces generated on the device as bench.py does, one replay's
outputs reused.  Each: warm-up launches, then timed repeats between events on the stream; the
median is reported.  The range covers every replication; the levels are the driver's defaults.

  python tools/time_queue_stats.py [--out profiles/queue_stats_timing.txt] [--shapes c3,c5,driver] [--tag T]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="c3,c5,driver")
    args = ap.parse_args()
    ctx = fa.Context(0)
    dev = torch.device("cuda", 0)
    tag = f"[{args.tag}] " if args.tag else ""
    lines = [f"{tag}device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH)}; median of "
             f"{args.reps} timed launches after {args.warmup} warm-up"]

    def report(name, ms):
        med = statistics.median(ms)
        lines.append(f"{tag}{name}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})")
        return med

    for shape in args.shapes.split(","):
        R, T, N = SHAPES[shape]
        mg, sc = (fa.c5_params if shape == "c5" else fa.sweep_params)(np.arange(R), N)
        d = fa.generate_trace(ctx, 0x5EED0003, R, T, N, mg, sc)
        tr = {k: v for k, v in d.items() if not k.startswith("_")}
        out = fa.run_batch(ctx, tr)
        torch.cuda.synchronize()
        st = out.rep_stats()
        ok = st["status"] == 0
        t1 = int(st["last_tick"][ok].max()) + 1
        decided = int(st["n_tasks"][ok].sum())
        nodes = torch.empty(R * N * _abi.NODE_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        rows = torch.empty(R * N * _abi.QUEUE_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        unit = report(f"{shape} node_stats (the yardstick)", timed(lambda: fa.node_stats(ctx, tr, out, res=nodes), args.warmup, args.reps))
        call = lambda: fa.queue_stats(ctx, tr, out, fa.engine.QUEUE_LEVELS, 0, t1, res=rows)  # noqa: E731
        os.environ["FOGNET_QUEUE_STAGES"] = "1"
        build = report(f"{shape} queue_stats count + build", timed(call, args.warmup, args.reps))
        os.environ.pop("FOGNET_QUEUE_STAGES")
        whole = report(f"{shape} queue_stats whole pass", timed(call, args.warmup, args.reps))
        rec = rows.cpu().numpy().view(_abi.QUEUE_STATS_DTYPE).reshape(R, N)
        elements = int(rec["n_enq"].sum())
        measure = max(whole - build, 1e-6)
        b_build = 26 * decided + 28 * elements
        b_meas = 28 * elements + R * N * _abi.QUEUE_STATS_DTYPE.itemsize
        rounds = -(-R // max(1, min(R, (1 << 30) // (28 * T))))
        lines.append(f"{tag}{shape} R={R} T={T} N={N} ok={int(ok.sum())} decided={decided} queued elements={elements} "
                     f"longest queue={int(rec['max_len'].max())} rounds={rounds}")
        lines.append(f"{tag}{shape} count + build {build:.3f} ms ({b_build / build / 1e6:.1f} GB/s of {b_build / 1e6:.1f} MB), "
                     f"measure {measure:.3f} ms ({b_meas / measure / 1e6:.1f} GB/s of {b_meas / 1e6:.1f} MB), "
                     f"sum {whole:.3f} ms = {whole / unit:.2f} x node_stats")
        del d, tr, out, nodes, rows
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
