#!/usr/bin/env python3
"""Times the assigned replay (fognet_replay_assigned_dev, fognet_run_assigned_dev) against the
sequential replay (fognet_replay_dev) on the same trace, which is the yardstick: the assignment is
that replay's own node output, so both produce identical arrays.

Shapes: C3 (R = 4,096, T = 100,000, N = 256), C5 flat (R = 1,024, T = 10,000, N = 10,000) and the
driver's (R = 64, T = 20,000, N = 5), traces generated on the device as bench.py does.  The two
stages are timed cumulatively -- FOGNET_ASSIGNED_STAGES=1 (validation + count), unset (+ chain) --
and reported as a difference; each figure is the median of --reps launches between events on the
stream after --warmup warm-up launches.  FOGNET_ASSIGNED=hbm (a test mode) keeps the counts and the
per-node carries in the workspace.  The HBM share is the pass's least traffic, 37 B per task (16 B
in: arrive, req, assign; 21 B out), over the time, against bench.py's HBM figure.

  python tools/time_assigned.py [--out profiles/assigned_timing.txt] [--reps N] [--shapes R,T,N;...]
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

SHAPES = "4096,100000,256;1024,10000,10000;64,20000,5"
HBM_PEAK_GBS = 8000.0  # bench.py's roofline figure
BYTES_PER_TASK = 37


def timed(fn, warmup: int, reps: int) -> float:
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
    return statistics.median(ms)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=SHAPES)
    args = ap.parse_args()
    ctx = fa.Context(0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    say(f"device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH)}; median of {args.reps} timed "
        f"launches after {args.warmup} warm-up")
    for shape in args.shapes.split(";"):
        R, T, N = (int(x) for x in shape.split(","))
        mg, sc = fa.c5_params(np.arange(R), N) if N > 256 else fa.sweep_params(np.arange(R), N)
        d = fa.generate_trace(ctx, 0x5EED0003, R, T, N, mg, sc)
        tr = {k: v for k, v in d.items() if not k.startswith("_")}
        ref = fa.run_batch(ctx, tr, stage="replay")
        torch.cuda.synchronize()
        ok = int((ref.rep_stats()["status"] == 0).sum())
        assign = ref.node.clone()
        out = fa.allocate_outputs(R, T, assign.device, hist=True)
        fa.run_assigned(ctx, tr, assign, out=out, stats=False)
        torch.cuda.synchronize()
        good = torch.from_numpy(ref.rep_stats()["status"] == 0).to(assign.device)
        same = all(torch.equal(a[good], b[good]) for a, b in ((out.node, ref.node), (out.status, ref.status),
                                                              (out.start_tick, ref.start_tick),
                                                              (out.done_tick, ref.done_tick)))
        say(f"R={R} T={T} N={N} ok={ok}: assigned outputs equal the sequential replay's: {same}")
        scratch = fa.allocate_outputs(R, T, assign.device)
        base = timed(lambda: fa.run_batch(ctx, tr, out=scratch, stage="replay"), args.warmup, args.reps)
        say(f"  fognet_replay_dev (yardstick): {base:.3f} ms")
        gb = R * T * BYTES_PER_TASK / 1e9
        for mode in ("default", "hbm"):
            if mode == "hbm":
                os.environ["FOGNET_ASSIGNED"] = "hbm"
            replay = lambda: fa.run_assigned(ctx, tr, assign, out=out, stats=False)  # noqa: E731
            os.environ["FOGNET_ASSIGNED_STAGES"] = "1"
            count = timed(replay, args.warmup, args.reps)
            os.environ.pop("FOGNET_ASSIGNED_STAGES", None)
            whole = timed(replay, args.warmup, args.reps)
            full = timed(lambda: fa.run_assigned(ctx, tr, assign, out=out, stats=True), args.warmup, args.reps)
            os.environ.pop("FOGNET_ASSIGNED", None)
            say(f"  replay_assigned [{mode}]: count {count:.3f} ms, chain {whole - count:.3f} ms, whole pass {whole:.3f} ms "
                f"= {whole / base:.2f} x the yardstick; {gb / (whole * 1e-3):.0f} GB/s of the least traffic = "
                f"{100 * gb / (whole * 1e-3) / HBM_PEAK_GBS:.1f} % of {HBM_PEAK_GBS:.0f} GB/s; with the statistics "
                f"(run_assigned) {full:.3f} ms")
        del tr, d, ref, out, scratch, assign
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
