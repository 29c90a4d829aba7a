#!/usr/bin/env python3
"""Times the replication-group pass (fognet_reduce_groups_dev) beside the plain job reduction
(fognet_reduce_stats_dev) on the same records.

Both read the R per-replication records (200 B each); the group pass forms nine metrics per record,
merges eleven signals per replication where the plain reduction adds four sums, and first clears
its G records (848 B each).

Records: synthetic, R = 4,096 (C3's count) and 2^20 (C4's).  Groups: G = 1 (NULL group_of), 9
(r % 9, C3's sweep points), 65 (r % 65, the first G past the LDS limit) and 65,536 (r % 65,536),
each with the accumulators in LDS where G allows it and forced into the caller's records
(FOGNET_GROUP_STATS=hbm).  Each: warm-up launches, then timed repeats between events on the stream;
the median is reported with its ratio to the plain reduction's.

  python tools/time_group_stats.py [--out profiles/group_timing.txt] [--reps 9]
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

SIZES = (4096, 1 << 20)
GROUPS = (1, 9, 65, 65536)


def synthetic(R: int, seed: int = 1) -> np.ndarray:
    """R plausible OK records (a few failed among them): random counts and moments, vectorised."""
    rng = np.random.default_rng(seed)
    r = np.zeros(R, _abi.REP_STATS_DTYPE)
    t = rng.integers(1000, 100_000, R)
    q = (t * rng.random(R)).astype(np.int64)
    r["n_tasks"], r["n_queued"], r["n_started"], r["n_qtime"] = t, q, t - q, q
    r["events"] = t * 516
    r["last_tick"] = rng.integers(10**12, 10**15, R)
    r["queue_min_raw"], r["queue_max_raw"] = rng.integers(0, 10**9, R), rng.integers(10**9, 10**15, R)
    r["resp_min_ticks"], r["resp_max_ticks"] = rng.integers(10**8, 10**9, R), rng.integers(10**12, 10**14, R)
    for k in ("queue_sum_lo", "queue_sq_lo", "queue_sq_hi", "resp_sum_lo", "resp_sq_lo", "resp_sq_hi"):
        r[k] = rng.integers(0, 2**62, R).astype(np.uint64)
    r["resp_sum_hi"] = rng.integers(0, 4, R).astype(np.uint64)   # a mean response that needs the 128-bit division
    r["max_pending"] = rng.integers(0, 2048, R)
    r["busy_s"] = rng.integers(0, 10**6, R)
    r["energy_j"] = rng.uniform(0, 1e6, R)
    r["abort_tick"], r["abort_task"] = np.iinfo(np.int64).max, -1
    r["status"][rng.random(R) < 0.001] = _abi.FOGNET_ERR_CAPACITY
    return r


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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = fa.Context(0)
    dev = torch.device("cuda", 0)
    ptr, sp = fa.engine._ptr, fa.engine._stream_ptr
    lines = [f"device: {torch.cuda.get_device_name(0)}; library {os.path.relpath(_abi.LIB_PATH)}; median of {args.reps} "
             f"timed launches after {args.warmup} warm-up", "| R | G | accumulators | median ms | x fognet_reduce_stats_dev |",
             "|---|---|---|---|---|"]
    for R in SIZES:
        recs = synthetic(R)
        stats = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev)
        job = torch.empty(_abi.JOB_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        plain = statistics.median(timed(lambda: ctx.check(ctx._lib.fognet_reduce_stats_dev(
            ctx.handle, ptr(stats), R, ptr(job), sp(dev))), args.warmup, args.reps))
        lines.append(f"| {R} | - | fognet_reduce_stats_dev | {plain:.4f} | 1.00 |")
        want = None
        for G in GROUPS:
            gof = None if G == 1 else (torch.arange(R, device=dev, dtype=torch.int64) % G).to(torch.int32)
            out = torch.empty(G * _abi.GROUP_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            ung = torch.empty(1, dtype=torch.int64, device=dev)
            for mode in ("lds", "hbm"):
                if mode == "lds" and G > _abi.GROUP_LDS_MAX:
                    continue
                os.environ.pop("FOGNET_GROUP_STATS", None)
                if mode == "hbm":
                    os.environ["FOGNET_GROUP_STATS"] = "hbm"
                med = statistics.median(timed(lambda: ctx.check(ctx._lib.fognet_reduce_groups_dev(
                    ctx.handle, ptr(stats), R, ptr(gof), G, ptr(out), None, None, ptr(ung), sp(dev))), args.warmup, args.reps))
                lines.append(f"| {R} | {G} | {mode} | {med:.4f} | {med / plain:.2f} |")
                # the folded groups equal the one-group record: the timed calls computed the same thing
                folded = fa.merge_group_stats(out.cpu().numpy().view(_abi.GROUP_STATS_DTYPE)).tobytes()
                want = want or folded
                assert folded == want and int(ung.item()) == 0, (R, G, mode)
            os.environ.pop("FOGNET_GROUP_STATS", None)
        jr = job.cpu().numpy().view(_abi.JOB_STATS_DTYPE)[0]
        gj = fa.group_job(np.frombuffer(want, dtype=_abi.GROUP_STATS_DTYPE)[0])
        assert all(np.array_equal(jr[n], gj[n]) for n in jr.dtype.names if n != "energy_j"), R
        del stats
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
