#!/usr/bin/env python3
"""Times the per-user signal pass (fognet_per_user_stats_dev) and its job reduction
(fognet_reduce_user_stats_dev) against the existing whole-replication pass
(fognet_user_stats_dev with per-task links), which is the yardstick: it streams 37 B per
task where the keyed pass streams 25 B.

Shape: C3 (R = 4,096, T = 100k, N = 256), trace generated on the device as bench.py does,
one replay's outputs reused.  user_of is round-robin (mqttApp2's users publish in turn).
The pass runs at U = 1, 10, 64, 128 (accumulators in LDS) and U = 129, 1,024 (the caller's
records in HBM).  Each: warm-up launches, then timed repeats between events on the stream;
the median is reported, with the achieved GB/s over the bytes the pass must move.

The grouping thresholds are compile-time constants (FOGNET_USER_GROUP_REDUCE_LDS and _HBM in
per_user_stats.hip); a variant build is timed with FOGNET_LIB:

  EXTRA=-DFOGNET_USER_GROUP_REDUCE_LDS=4 tools/build_variant.sh g4
  FOGNET_LIB=build/live/g4/libfognet_hip.so python tools/time_per_user_stats.py --tag g4

  python tools/time_per_user_stats.py [--out profiles/per_user_stats_timing.txt] [--reps N] [--R R --T T]
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

USERS = (1, 10, 64, 128, 129, 1024)
REC = _abi.USER_STATS_DTYPE.itemsize


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
    ap.add_argument("--R", type=int, default=4096)
    ap.add_argument("--T", type=int, default=100_000)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--users", default=",".join(str(u) for u in USERS))
    args = ap.parse_args()
    R, T, N = args.R, args.T, args.N
    ctx = fa.Context(0)
    dev = torch.device("cuda", 0)
    tag = f"[{args.tag}] " if args.tag else ""
    lines = [f"{tag}device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH)}; median of "
             f"{args.reps} timed launches after {args.warmup} warm-up"]
    mg, sc = fa.sweep_params(np.arange(R), N)
    d = fa.generate_trace(ctx, 0x5EED0003, R, T, N, mg, sc)
    tr = {k: v for k, v in d.items() if not k.startswith("_")}
    out = fa.run_batch(ctx, tr)
    torch.cuda.synchronize()
    ok = int((out.rep_stats()["status"] == 0).sum())
    lines.append(f"{tag}C3 R={R} T={T} N={N} ok={ok}")

    def report(name, ms, nbytes):
        med = statistics.median(ms)
        lines.append(f"{tag}{name}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), {nbytes / 1e6:.1f} MB, "
                     f"{nbytes / med / 1e6:.1f} GB/s")
        return med

    # the yardstick: the existing pass with per-task links (37 B per task)
    rng = torch.Generator(device=dev).manual_seed(1)
    tu = torch.randint(0, 5 * 10**9, (R, T), dtype=torch.int64, device=dev, generator=rng)
    td = torch.randint(0, 5 * 10**9, (R, T), dtype=torch.int64, device=dev, generator=rng)
    whole = torch.empty(R * REC, dtype=torch.uint8, device=dev)
    # (the C entry points directly: fa.user_stats and fa.reduce_user_stats copy their records to the host)
    p, stream = fa.engine._ptr, fa.engine._stream_ptr(dev)
    bi = _abi.BatchIn(R, T, N, _abi.FOGNET_POLICY_REF_V3, N if tr["mips"].dim() == 2 else 0, 0,
                      *(p(tr[k]) for k in ("arrive", "req", "mips", "dl", "ul", "init")))
    bo = _abi.BatchOut(p(out.node), p(out.status), p(out.start_tick), p(out.done_tick), p(out.stats))

    def user_stats():
        ctx.check(ctx._lib.fognet_user_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), p(tu), p(td), 1, p(whole), stream),
                  "user_stats")
    base = report("user_stats (per-task links)", timed(user_stats, args.warmup, args.reps), 37 * R * T + R * REC)
    del tu, td
    torch.cuda.empty_cache()

    step = torch.arange(T, dtype=torch.int32, device=dev)[None, :] + 3 * torch.arange(R, dtype=torch.int32, device=dev)[:, None]
    cnt = torch.empty(R, dtype=torch.int64, device=dev)
    med = {}
    for U in (int(u) for u in args.users.split(",")):
        who = (step % U).contiguous()
        uu = torch.randint(0, 5 * 10**9, (U,), dtype=torch.int64, device=dev, generator=rng)
        ud = torch.randint(0, 5 * 10**9, (U,), dtype=torch.int64, device=dev, generator=rng)
        recs = torch.empty(R * U * REC, dtype=torch.uint8, device=dev)
        job = torch.empty(U * REC, dtype=torch.uint8, device=dev)
        fn = lambda: fa.per_user_stats(ctx, tr, out, who, uu, ud, res=recs, n_unassigned=cnt, allow_unassigned=True)
        layout = "lds" if U <= 128 else "hbm"
        med[U] = report(f"per_user_stats U={U} [{layout}]", timed(fn, args.warmup, args.reps), 25 * R * T + R * U * REC)
        assert int(cnt.sum()) == 0
        if U <= 128:
            os.environ["FOGNET_USER_STATS"] = "hbm"
            report(f"per_user_stats U={U} [hbm forced]", timed(fn, args.warmup, args.reps), 25 * R * T + 2 * R * U * REC)
            os.environ.pop("FOGNET_USER_STATS", None)

        def reduce():
            ctx.check(ctx._lib.fognet_reduce_user_stats_dev(ctx.handle, p(recs), p(out.stats), R, U, p(job), stream),
                      "reduce_user_stats")
        report(f"reduce_user_stats U={U}", timed(reduce, args.warmup, args.reps), R * U * REC)
        del who, recs, job
        torch.cuda.empty_cache()
    if 10 in med:
        lines.append(f"{tag}per_user_stats U=10 / user_stats = {med[10] / base:.3f} (bytes ratio {25 / 37:.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.tag else "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
