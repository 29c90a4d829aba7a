#!/usr/bin/env python3
"""Times the per-node statistics pass (fognet_node_stats_dev) and its job reduction
(fognet_reduce_node_stats_dev) against the stand-alone replication pass
(fognet_rep_stats_dev), which streams the same 33 B per task and is the yardstick.

Shapes: C3 (R = 4,096, T = 100k, N = 256) and C5 flat (R = 1,024, T = 10k, N = 10,000),
traces generated on the device as bench.py does.  Each pass: warm-up launches, then
timed repeats between events on the stream; the median is reported, with the achieved
GB/s over the bytes the pass must move (33 B per task + its records).

``--shapes c5hier,c5sat``: C5 under EXT_HIER (bench.py's light recipe, where no region
escalates, and its saturating recipe, T = 32,768, where every replication does): the replay
without and with the per-task escalation flags (fognet_batch_out.escalated, one more byte
per task), then the user-signal and per-node passes that read them (34 B per task).

FOGNET_LIB=build/live/<name>/libfognet_hip.so times a variant build (tools/build_variant.sh).

  python tools/node_stats_timing.py [--out profiles/node_stats_timing.txt] [--reps N] [--shapes c3,c5flat]
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

SHAPES = {"c3": (4096, 100_000, 256), "c5flat": (1024, 10_000, 10_000),
          "c5hier": (1024, 10_000, 10_000), "c5sat": (1024, 32_768, 10_000)}
HIER = dict(policy="EXT_HIER", hier_threshold_s=60, hier_up_tick=20 * 10**9)  # bench.py's defaults


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


def time_hier(ctx, dev, name: str, R: int, T: int, N: int, args) -> list[str]:
    """C5 under EXT_HIER: the replay without / with the escalation flags and the two passes that read them."""
    if name == "c5sat":
        tr = fa.as_device_trace(fa.saturating_trace(0x5EED0005, R, T, N), dev)
    else:
        mg, sc = fa.c5_params(np.arange(R), N)
        d = fa.generate_trace(ctx, 0x5EED0005, R, T, N, mg, sc)
        tr = {k: v for k, v in d.items() if not k.startswith("_")}
        tr["region"] = fa.mobility_regions(tr["arrive"], N)
    plain = fa.allocate_outputs(R, T, dev)
    out = fa.allocate_outputs(R, T, dev, escalated=True)
    fa.run_batch(ctx, tr, out=out, **HIER)
    torch.cuda.synchronize()
    ok = int((out.rep_stats()["status"] == 0).sum())
    n_esc = int(out.escalated.sum(dtype=torch.int64))
    uu = torch.full((R,), 2 * 10**9, dtype=torch.int64, device=dev)
    ud = torch.full((R,), 3 * 10**9, dtype=torch.int64, device=dev)
    users = torch.empty(R * _abi.USER_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    nodes = torch.empty(R * N * _abi.NODE_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    rec_bytes = R * N * _abi.NODE_STATS_DTYPE.itemsize
    passes = {
        "replay": (lambda: fa.run_batch(ctx, tr, out=plain, **HIER), None),
        "replay+escalated": (lambda: fa.run_batch(ctx, tr, out=out, **HIER), None),
        "user_stats": (lambda: fa.user_stats(ctx, tr, out, uu, ud, res=users), 22 * R * T),
        "node_stats": (lambda: fa.node_stats(ctx, tr, out, policy="EXT_HIER", res=nodes), 34 * R * T + rec_bytes),
    }
    lines = [f"{name} R={R} T={T} N={N} EXT_HIER ok={ok} escalated tasks={n_esc}"]
    for pname, (fn, nbytes) in passes.items():
        ms = timed(fn, args.warmup, args.reps)
        med = statistics.median(ms)
        rate = f", {nbytes / 1e6:.1f} MB, {nbytes / med / 1e6:.1f} GB/s" if nbytes else ""
        lines.append(f"{name} {pname}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}){rate}")
    return lines


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="c3,c5flat")
    args = ap.parse_args()
    ctx = fa.Context(0)
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH)}; median of {args.reps} "
             f"timed launches after {args.warmup} warm-up"]
    for name in args.shapes.split(","):
        R, T, N = SHAPES[name]
        if name in ("c5hier", "c5sat"):
            lines += time_hier(ctx, dev, name, R, T, N, args)
            continue
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
