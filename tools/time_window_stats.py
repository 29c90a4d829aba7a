#!/usr/bin/env python3
"""Times the time-window pass (fognet_window_stats_dev) and its job reduction
(fognet_reduce_window_stats_dev) against the yardstick: fognet_node_stats_dev plus
fognet_per_user_stats_dev on the same replay, which together read the same rows (33 + 25 B per
task against the window pass's 33 B) and make the same emissions.

Shapes: C3 (R = 4,096, T = 100k, N = 256), C5 flat (R = 64, T = 100k, N = 10,000) and the
driver's (R = 4, T = 600, N = 5), traces generated on the device as bench.py does, one replay's
outputs reused.  user_of is round-robin over 10 users.  The range covers the replay ([0, the
latest completion + 100 s)), cut into W = 64, 1,024 and 16,384 windows; W = 64 runs in both
layouts (records in LDS; FOGNET_WINDOW_STATS=hbm).  Each: warm-up launches, then timed repeats
between events on the stream; the median is reported, with the GB/s over the bytes the pass
must move (33 B per task, the records once, and the 16 B of deltas per window twice where they
live in the workspace).

The wave-summing thresholds are compile-time constants (FOGNET_WINDOW_REDUCE_LDS and _HBM in
window_stats.hip); a variant build is timed with FOGNET_LIB:

  EXTRA=-DFOGNET_WINDOW_REDUCE_LDS=8 tools/build_variant.sh wl8
  FOGNET_LIB=build/live/wl8/libfognet_hip.so python tools/time_window_stats.py --tag wl8

and so is the LDS limit (FOGNET_WINDOW_LDS_WINDOWS in fognet_hip.h; --lds-max tells this tool the build's):

  EXTRA=-DFOGNET_WINDOW_LDS_WINDOWS=96 tools/build_variant.sh lds96
  FOGNET_LIB=build/live/lds96/libfognet_hip.so python tools/time_window_stats.py --tag lds96 --lds-max 96 --shapes c3 --windows 96,97,128,150

  python tools/time_window_stats.py [--out profiles/window_stats_timing.txt] [--shapes c3,c5,driver] [--windows 64,1024,16384]
"""
from __future__ import annotations

import argparse
import ctypes as C
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
REC = _abi.WINDOW_STATS_DTYPE.itemsize
U = 10


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
    ap.add_argument("--windows", default="64,1024,16384")
    ap.add_argument("--lds-max", type=int, default=_abi.WINDOW_LDS_WINDOWS, help="the timed build's FOGNET_WINDOW_LDS_WINDOWS")
    args = ap.parse_args()
    ctx = fa.Context(0)
    dev = torch.device("cuda", 0)
    tag = f"[{args.tag}] " if args.tag else ""
    lines = [f"{tag}device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH)}; median of "
             f"{args.reps} timed launches after {args.warmup} warm-up"]

    def report(name, ms, nbytes):
        med = statistics.median(ms)
        lines.append(f"{tag}{name}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), {nbytes / 1e6:.1f} MB, "
                     f"{nbytes / med / 1e6:.1f} GB/s")
        return med

    for shape in args.shapes.split(","):
        R, T, N = SHAPES[shape]
        mg, sc = (fa.c5_params if shape == "c5" else fa.sweep_params)(np.arange(R), N)
        d = fa.generate_trace(ctx, 0x5EED0003, R, T, N, mg, sc)
        tr = {k: v for k, v in d.items() if not k.startswith("_")}
        out = fa.run_batch(ctx, tr)
        torch.cuda.synchronize()
        st = out.rep_stats()
        ok = int((st["status"] == 0).sum())
        last = int(st["last_tick"][st["status"] == 0].max()) + 100 * 10**12  # (the last acks arrive a relay later)
        lines.append(f"{tag}{shape} R={R} T={T} N={N} ok={ok} range=[0, {last / 1e12:.3f} s)")
        rng = torch.Generator(device=dev).manual_seed(1)
        who = ((torch.arange(T, dtype=torch.int32, device=dev)[None, :] +
                3 * torch.arange(R, dtype=torch.int32, device=dev)[:, None]) % U).contiguous()
        uu = torch.randint(0, 5 * 10**9, (U,), dtype=torch.int64, device=dev, generator=rng)
        ud = torch.randint(0, 5 * 10**9, (U,), dtype=torch.int64, device=dev, generator=rng)
        cnt = torch.empty(R, dtype=torch.int64, device=dev)
        outside = torch.empty((R, 2), dtype=torch.int64, device=dev)
        # the yardstick: the node pass and the per-user pass of the same replay
        nodes = torch.empty(R * N * _abi.NODE_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        users = torch.empty(R * U * _abi.USER_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        t_node = report(f"{shape} node_stats", timed(lambda: fa.node_stats(ctx, tr, out, res=nodes), args.warmup, args.reps),
                        33 * R * T + nodes.numel())
        t_user = report(f"{shape} per_user_stats U={U}",
                        timed(lambda: fa.per_user_stats(ctx, tr, out, who, uu, ud, res=users, n_unassigned=cnt,
                                                        allow_unassigned=True), args.warmup, args.reps),
                        25 * R * T + users.numel())
        del nodes, users
        torch.cuda.empty_cache()
        p, stream = fa.engine._ptr, fa.engine._stream_ptr(dev)
        for W in (int(w) for w in args.windows.split(",")):
            window = last // W + 1
            recs = torch.empty(R * W * REC, dtype=torch.uint8, device=dev)
            job = torch.empty(W * REC, dtype=torch.uint8, device=dev)
            fn = lambda: fa.window_stats(ctx, tr, out, who, uu, ud, 0, window, W, res=recs, n_outside=outside, n_unassigned=cnt)
            lds = W <= args.lds_max
            nbytes = 33 * R * T + R * W * REC + (0 if lds else 2 * 16 * R * W)
            med = report(f"{shape} window_stats W={W} [{'lds' if lds else 'hbm'}]", timed(fn, args.warmup, args.reps), nbytes)
            assert int(cnt.sum()) == 0
            lines.append(f"{tag}{shape} window_stats W={W}: {int(outside.sum())} point events outside the range")
            lines.append(f"{tag}{shape} window_stats W={W} / (node_stats + per_user_stats) = {med / (t_node + t_user):.3f} "
                         f"(bytes per task 33 / 58 = {33 / 58:.3f})")
            if lds:
                os.environ["FOGNET_WINDOW_STATS"] = "hbm"
                report(f"{shape} window_stats W={W} [hbm forced]", timed(fn, args.warmup, args.reps),
                       33 * R * T + 2 * R * W * REC + 2 * 16 * R * W)
                os.environ.pop("FOGNET_WINDOW_STATS", None)

            def reduce():
                ctx.check(ctx._lib.fognet_reduce_window_stats_dev(ctx.handle, p(recs), p(out.stats), R, W, p(job), stream),
                          "reduce_window_stats")
            report(f"{shape} reduce_window_stats W={W}", timed(reduce, args.warmup, args.reps), R * W * REC)
            del recs, job
            torch.cuda.empty_cache()
        del d, tr, out, who
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
