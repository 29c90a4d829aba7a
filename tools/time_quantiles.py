#!/usr/bin/env python3
"""Times the quantile passes (fognet_quantiles_dev per replication, fognet_job_quantiles_dev over
the job), each with the skipped rounds and with FOGNET_QUANTILES=full, beside the natural unit:
fognet_window_stats_dev with W = 1 on the same replay outputs, which is one stream of the same
rows with the same emissions.  A select costs one stream for the extents and one per round.

Shapes: C3 (R = 4,096, T = 100k, N = 256), C5 flat (R = 64, T = 100k, N = 10,000) and the
driver's (R = 4, T = 600, N = 5), traces generated on the device as bench.py does, one replay's
outputs reused.  user_of is round-robin over 10 users.  Each: warm-up launches, then timed repeats
between events on the stream; the median is reported.  The rounds actually run are worked out from
the results: a signal starts behind the leading bytes that its minimum and maximum share, and a
replication (or the job) streams every round from its earliest signal's on.

The two ways of sharing counter updates are compile-time switches (FOGNET_QUANTILE_WAVE_SUM and
FOGNET_QUANTILE_SHARE_HISTOGRAMS in quantiles.hip); a build without one is timed with FOGNET_LIB:

  EXTRA=-DFOGNET_QUANTILE_WAVE_SUM=0 tools/build_variant.sh qnosum
  FOGNET_LIB=build/live/qnosum/libfognet_hip.so python tools/time_quantiles.py --tag qnosum --shapes c3

  python tools/time_quantiles.py [--out profiles/quantiles_timing.txt] [--shapes c3,c5,driver] [--ranks 50,99,99.9]
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


def first_round(lo: np.ndarray, hi: np.ndarray, count: np.ndarray) -> np.ndarray:
    """The first round of each population: the leading bytes its extreme keys share (8: none runs)."""
    diff = (lo.astype(np.uint64) ^ hi.astype(np.uint64)).astype(np.uint64)
    start = np.full(diff.shape, 8, np.int64)
    for b in range(8):  # the highest byte that differs
        start = np.where((start == 8) & ((diff >> np.uint64(56 - 8 * b)) & np.uint64(255) != 0), b, start)
    return np.where(count > 0, start, 8)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="c3,c5,driver")
    ap.add_argument("--ranks", default="50,99,99.9", help="percents; a second timing uses eight ranks")
    args = ap.parse_args()
    ctx = fa.Context(0)
    dev = torch.device("cuda", 0)
    tag = f"[{args.tag}] " if args.tag else ""
    lines = [f"{tag}device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH)}; median of "
             f"{args.reps} timed launches after {args.warmup} warm-up"]
    ranks3 = [round(float(p) * 10000) for p in args.ranks.split(",")]
    ranks8 = [500000, 900000, 950000, 990000, 999000, 999900, 0, 1000000]

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
        last = int(st["last_tick"][st["status"] == 0].max()) + 100 * 10**12
        lines.append(f"{tag}{shape} R={R} T={T} N={N} ok={int((st['status'] == 0).sum())}")
        rng = torch.Generator(device=dev).manual_seed(1)
        who = ((torch.arange(T, dtype=torch.int32, device=dev)[None, :] +
                3 * torch.arange(R, dtype=torch.int32, device=dev)[:, None]) % U).contiguous()
        uu = torch.randint(0, 5 * 10**9, (U,), dtype=torch.int64, device=dev, generator=rng)
        ud = torch.randint(0, 5 * 10**9, (U,), dtype=torch.int64, device=dev, generator=rng)
        cnt1 = torch.empty(R, dtype=torch.int64, device=dev)
        outside = torch.empty((R, 2), dtype=torch.int64, device=dev)
        rec = torch.empty(R * _abi.WINDOW_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        unit = report(f"{shape} window_stats W=1 (one stream of the rows)",
                      timed(lambda: fa.window_stats(ctx, tr, out, who, uu, ud, 0, last, 1, res=rec, n_outside=outside,
                                                    n_unassigned=cnt1), args.warmup, args.reps))
        # the rounds that run, from the extremes
        v, c, _ = fa.quantiles(ctx, tr, out, who, uu, ud, [0, 1000000])
        v, c = v.cpu().numpy(), c.cpu().numpy()
        start = first_round(v[:, :, 0], v[:, :, 1], c)
        per_rep = 8 - start.min(axis=1)
        lines.append(f"{tag}{shape} rounds run per replication: mean {per_rep.mean():.2f} (min {per_rep.min()}, max "
                     f"{per_rep.max()}) of 8; first round per signal (median over replications) "
                     f"{[int(np.median(start[:, s])) for s in range(5)]}; populations (mean) {[int(x) for x in c.mean(axis=0)]}")
        jv, jc = fa.job_quantiles(ctx, tr, out, who, uu, ud, [0, 1000000])
        jstart = first_round(jv[:, 0], jv[:, 1], jc)
        lines.append(f"{tag}{shape} rounds run by the job: {8 - int(jstart.min())} of 8; first round per signal "
                     f"{[int(x) for x in jstart]}; populations {[int(x) for x in jc]}")
        for ranks in (ranks3, ranks8):
            Q = len(ranks)
            val = torch.empty((R, 5, Q), dtype=torch.int64, device=dev)
            cnt = torch.empty((R, 5), dtype=torch.int64, device=dev)
            jval = torch.empty((5, Q), dtype=torch.int64, device=dev)
            jcnt = torch.empty(5, dtype=torch.int64, device=dev)
            bi, bo = fa.engine._pass_descriptors(tr, out, fa.engine._dims(tr), fa.engine._policy_of(out, None), None)
            p, stream = fa.engine._ptr, fa.engine._stream_ptr(dev)
            carr = (fa.engine.C.c_int32 * Q)(*ranks)

            def per_rep_call():
                fa.quantiles(ctx, tr, out, who, uu, ud, ranks, value=val, count=cnt, n_unassigned=cnt1)

            def job_call():  # (the binding's job call copies the results to the host: the entry point itself)
                ctx.check(ctx._lib.fognet_job_quantiles_dev(ctx.handle, fa.engine.C.byref(bi), fa.engine.C.byref(bo), p(who), U, 0,
                                                            p(uu), p(ud), carr, Q, p(jval), p(jcnt), stream), "job_quantiles")
            for mode in ("skip", "full"):
                if mode == "full":
                    os.environ["FOGNET_QUANTILES"] = "full"
                a = report(f"{shape} quantiles Q={Q} [{mode}]", timed(per_rep_call, args.warmup, args.reps))
                b = report(f"{shape} job_quantiles Q={Q} [{mode}]", timed(job_call, args.warmup, args.reps))
                os.environ.pop("FOGNET_QUANTILES", None)
                lines.append(f"{tag}{shape} Q={Q} [{mode}] / window_stats W=1: per replication {a / unit:.2f}, job {b / unit:.2f}")
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
