#!/usr/bin/env python3
"""Times the signal-vector pass (fognet_signal_vectors_dev) stage by stage, in both sort
modes, against the per-user statistics pass (fognet_per_user_stats_dev) on the same arrays,
which is the yardstick: it reads the same per-task rows once.

Shapes: C1 (R = 64, T = 20,000, N = 5, U = 10) and R = 64, T = 100,000, N = 256, U = 10, traces
generated on the device as bench.py does, one replay's outputs reused.  user_of is round-robin
(mqttApp2's users publish in turn).  The stages are timed cumulatively -- FOGNET_VEC_STAGES=1
(count), =2 (count + place), unset (count + place + order) -- and reported as differences;
each figure is the median of --reps launches between events on the stream after --warmup
warm-up launches.  FOGNET_VEC_SORT=hbm (a test mode) sorts in chunks of 64 rows and keeps the counters in HBM.

  python tools/time_signal_vectors.py [--out profiles/signal_vectors_timing.txt] [--reps N] [--shapes R,T,N,U;...]
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

SHAPES = "64,20000,5,10;64,100000,256,10"
REC = _abi.USER_STATS_DTYPE.itemsize


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
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    say(f"device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH)}; median of {args.reps} timed "
        f"launches after {args.warmup} warm-up")
    for shape in args.shapes.split(";"):
        R, T, N, U = (int(x) for x in shape.split(","))
        mg, sc = fa.sweep_params(np.arange(R), N)
        d = fa.generate_trace(ctx, 0x5EED0003, R, T, N, mg, sc)
        tr = {k: v for k, v in d.items() if not k.startswith("_")}
        out = fa.run_batch(ctx, tr)
        torch.cuda.synchronize()
        ok = int((out.rep_stats()["status"] == 0).sum())
        step = torch.arange(T, dtype=torch.int32, device=dev)[None, :] + 3 * torch.arange(R, dtype=torch.int32, device=dev)[:, None]
        who = (step % U).contiguous()
        rng = torch.Generator(device=dev).manual_seed(1)
        uu = torch.randint(0, 5 * 10**9, (U,), dtype=torch.int64, device=dev, generator=rng)
        ud = torch.randint(0, 5 * 10**9, (U,), dtype=torch.int64, device=dev, generator=rng)
        V = N + 1 + 3 * U
        bufs = dict(offset=torch.empty((R, V + 1), dtype=torch.int64, device=dev),
                    time=torch.empty((R, 6 * T), dtype=torch.int64, device=dev),
                    value=torch.empty((R, 6 * T), dtype=torch.int64, device=dev),
                    task=torch.empty((R, 6 * T), dtype=torch.int32, device=dev),
                    n_unassigned=torch.empty((R,), dtype=torch.int64, device=dev))
        recs = torch.empty(R * U * REC, dtype=torch.uint8, device=dev)
        cnt = torch.empty(R, dtype=torch.int64, device=dev)
        base = timed(lambda: fa.per_user_stats(ctx, tr, out, who, uu, ud, res=recs, n_unassigned=cnt, allow_unassigned=True),
                     args.warmup, args.reps)
        vectors = lambda: fa.signal_vectors(ctx, tr, out, who, uu, ud, bufs=bufs, to_host=False)
        vectors()
        torch.cuda.synchronize()
        off = bufs["offset"].cpu().numpy()
        seg = np.diff(off, axis=1)
        # the delay vector of a replication without unassigned publishes is placed in order and not sorted
        seg[seg[:, N] == out.rep_stats()["n_tasks"], N] = 0
        say(f"R={R} T={T} N={N} U={U} ok={ok}: rows per replication mean {off[:, -1].mean():.0f}, longest sorted segment "
            f"{int(seg.max())} rows (vector {int(np.unravel_index(seg.argmax(), seg.shape)[1])}), sorted segments above the "
            f"LDS sort's 2,048 rows: {int((seg > 2048).sum())} of {seg.size}")
        say(f"  per_user_stats (yardstick): {base:.3f} ms")
        for mode in ("default", "hbm"):
            if mode == "hbm":
                os.environ["FOGNET_VEC_SORT"] = "hbm"
            cum = []
            for stages in ("1", "2", None):
                if stages:
                    os.environ["FOGNET_VEC_STAGES"] = stages
                cum.append(timed(vectors, args.warmup, args.reps))
                os.environ.pop("FOGNET_VEC_STAGES", None)
            os.environ.pop("FOGNET_VEC_SORT", None)
            count, place, order = cum[0], cum[1] - cum[0], cum[2] - cum[1]
            say(f"  signal_vectors [{mode}]: count {count:.3f} ms, place {place:.3f} ms, order {order:.3f} ms, whole pass "
                f"{cum[2]:.3f} ms = {cum[2] / base:.1f} x the yardstick (count {count / base:.2f} x, place {place / base:.2f} x, "
                f"order {order / base:.1f} x)")
        del bufs, recs, who, tr, d, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
