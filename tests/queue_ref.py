"""Event-level restatement of the queue-length statistics (fognet_hip.h "Queue-length
statistics"; test infrastructure, no GPU needed).

Per fog node a future-event set ordered by (tick, insertion sequence) with the publishes
pre-inserted, as OMNeT++ keeps it: a publish at the broker inserts the task's arrival at the
node one downlink later, an arrival either starts the task (and inserts its RELEASERESOURCE
timer) or pushes it onto a real list, a timer pops the list's head and inserts the next timer.
L is read off the list after every event.  Nothing here uses the closed form of the device
pass (ranks, binary searches over sorted keys), so the two check each other; the statuses and
start ticks that fall out of the events are compared with the replay's on the way.
"""
from __future__ import annotations

import heapq

import numpy as np

from fognetsimpp_amd import _abi

QUEUE = _abi.QUEUE_STATS_DTYPE
OK_STATUSES = (_abi.FOGNET_OK, _abi.FOGNET_REF_ABORTED)
NEVER = np.iinfo(np.int64).max
TPS = 10**12
MASK = (1 << 64) - 1
PUB, ARR, REL, CRASH = "pub", "arr", "rel", "crash"


def node_events(t, req, mips: int, dl: int, down: int = NEVER, tie: str = "fes"):
    """One node's run over its tasks (publish ticks ``t`` at the broker and requirements ``req``,
    in trace order).  Returns (status, start, done, trail): per task what the node model gives,
    and the trail [(tick, L after the event, "enq" | "deq" | "crash")] of every change of its
    list, in the order the events ran.

    ``tie``: "fes" is the model.  "arrival" and "dequeue" are two wrong same-tick orders, kept
    to show that the traces tell them apart: every arrival of a tick before / after every timer
    of that tick."""
    n = len(t)
    status, start, done = [0] * n, [-1] * n, [-1] * n
    serve = [(int(req[i]) // int(mips)) * TPS for i in range(n)]
    fes: list = []
    seq = n  # the publishes hold the sequence numbers 0 .. n - 1: they were inserted before the run

    def insert(tick, kind, i):
        nonlocal seq
        rank = seq
        if tie == "arrival" and kind == ARR:
            rank = -1 - (n - i)       # before every timer of its tick, arrivals in trace order
        if tie == "dequeue" and kind == REL:
            rank = -1                 # before every arrival of its tick
        heapq.heappush(fes, (tick, rank, seq, kind, i))
        seq += 1

    for i in range(n):
        heapq.heappush(fes, (int(t[i]), i, i, PUB, i))
    if down != NEVER:
        heapq.heappush(fes, (int(down), -(1 << 62), -1, CRASH, -1))  # precedes every model event of its tick
    requests: list = []
    trail: list = []
    busy = crashed = False
    while fes:
        now, _, _, kind, i = heapq.heappop(fes)
        if kind == PUB:
            insert(now + int(dl), ARR, i)
        elif kind == CRASH:
            crashed = True
            if requests:
                requests.clear()  # the tasks still waiting leave with the node
                trail.append((now, 0, "crash"))
        elif kind == ARR:
            if crashed:
                status[i] = 9
            elif not busy:
                busy, status[i], start[i] = True, 5, now
                insert(now + serve[i], REL, i)
            else:
                status[i] = 4
                requests.append(i)
                trail.append((now, len(requests), "enq"))
        elif not crashed:  # (the crash cancelled the timer)
            done[i] = now
            if requests:
                j = requests.pop(0)
                trail.append((now, len(requests), "deq"))
                start[j] = now
                insert(now + serve[j], REL, j)
            else:
                busy = False
    return status, start, done, trail


def measure(trail, levels, t0: int, t1: int) -> dict:
    """The record of one node from its trail: L is a step function that holds, from each tick on,
    the value after the last event of that tick."""
    rec = dict(n_enq=0, max_len=0, observed=t1 - t0, area=0, time_ge=[0] * len(levels))
    for tick, L, kind in trail:
        if kind == "enq" and t0 <= tick < t1:
            rec["n_enq"] += 1
            rec["max_len"] = max(rec["max_len"], L)
    for (tick, L, _), nxt in zip(trail, trail[1:] + [(NEVER, 0, "")]):
        lo, hi = max(tick, t0), min(nxt[0], t1)
        if hi > lo:
            rec["area"] += L * (hi - lo)
            for q, lv in enumerate(levels):
                if L >= lv:
                    rec["time_ge"][q] += hi - lo
    return rec


def to_record(rec: dict) -> np.ndarray:
    out = np.zeros((), QUEUE)
    out["n_enq"], out["max_len"] = rec["n_enq"], rec["max_len"]
    for name in ("observed", "area"):
        out[name + "_lo"], out[name + "_hi"] = rec[name] & MASK, rec[name] >> 64
    for q, v in enumerate(rec["time_ge"]):
        out["time_ge"][q] = (v & MASK, v >> 64)
    return out


def from_record(r, Q: int) -> dict:
    wide = lambda lo, hi: int(lo) | (int(hi) << 64)  # noqa: E731
    return dict(n_enq=int(r["n_enq"]), max_len=int(r["max_len"]), observed=wide(r["observed_lo"], r["observed_hi"]),
                area=wide(r["area_lo"], r["area_hi"]), time_ge=[wide(*r["time_ge"][q]) for q in range(Q)])


def merged(recs, Q: int) -> np.ndarray:
    """The exact merge of records (the job reduction's rule), in Python integers."""
    acc = dict(n_enq=0, max_len=0, observed=0, area=0, time_ge=[0] * Q)
    for r in recs:
        d = from_record(r, Q)
        acc["n_enq"] += d["n_enq"]
        acc["max_len"] = max(acc["max_len"], d["max_len"])
        acc["observed"] += d["observed"]
        acc["area"] += d["area"]
        acc["time_ge"] = [a + b for a, b in zip(acc["time_ge"], d["time_ge"])]
    return to_record(acc)


def node_row(tr: dict, r: int, k: int):
    """(mips, dl, down) of node k in replication r of a trace with shared or per-replication node rows."""
    pick = lambda a: a[r, k] if np.asarray(a).ndim == 2 else a[k]  # noqa: E731
    down = int(pick(tr["down"])) if tr.get("down") is not None else NEVER
    return int(pick(tr["mips"])), int(pick(tr["dl"])), down


def expected(tr: dict, o: dict, levels, t0: int, t1: int, tie: str = "fes", check: bool = True) -> np.ndarray:
    """QUEUE_STATS_DTYPE [R, N]: the records of a finished replay ``o`` (node, status, start, done
    [R, T] and stats [R]) of the trace ``tr``; a failed replication's row is all zero.  ``check``:
    the statuses and start ticks of the events equal the replay's."""
    arrive, req = np.atleast_2d(tr["arrive"]), np.atleast_2d(tr["req"])
    R, N = arrive.shape[0], int(np.asarray(tr["mips"]).shape[-1])
    out = np.zeros((R, N), QUEUE)
    for r in range(R):
        if int(o["stats"]["status"][r]) not in OK_STATUSES:
            continue
        n = int(o["stats"]["n_tasks"][r])
        node = np.asarray(o["node"][r][:n])
        for k in range(N):
            idx = np.nonzero(node == k)[0]
            mips, dl, down = node_row(tr, r, k)
            status, start, done, trail = node_events(arrive[r][idx], req[r][idx], mips, dl, down, tie)
            if check and tie == "fes":
                assert status == [int(x) for x in o["status"][r][idx]], (r, k, "status")
                assert start == [int(x) for x in o["start"][r][idx]], (r, k, "start")
                assert done == [int(x) for x in o["done"][r][idx]], (r, k, "done")
            out[r, k] = to_record(measure(trail, levels, t0, t1))
    return out


def tie_heavy_trace(seed: int, R: int, N: int, T: int) -> dict:
    """Coarse ticks, so that arrivals and completions collide: gaps, latencies and services are
    small multiples of one base, services are often 0, and some downlinks reach whole seconds (an
    arrival inserted before the timer it meets)."""
    rng = np.random.default_rng(seed)
    base = 10**11
    mips = rng.choice([1000, 2000, 500], size=(R, N)).astype(np.int32)
    dl = rng.choice([0, base, 2 * base, 10 * base, 20 * base, 30 * base], size=(R, N)).astype(np.int64)
    ul = rng.choice([0, base, 3 * base], size=(R, N)).astype(np.int64)
    init = ul + rng.integers(0, 3, size=(R, N)) * base
    first = init.max(axis=1, keepdims=True) + base
    arrive = first + np.cumsum(rng.choice([0, 0, base, 5 * base, 10 * base], size=(R, T)).astype(np.int64), axis=1)
    req = rng.choice([0, 400, 999, 1000, 1500, 2000, 3000], size=(R, T)).astype(np.int32)
    return dict(arrive=arrive, req=req, mips=mips, dl=dl, ul=ul, init=init)


def assert_records_equal(got, want, Q: int, what: str = "") -> None:
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    for ix in np.ndindex(got.shape):
        if got[ix].tobytes() != want[ix].tobytes():
            raise AssertionError(f"{what} record {ix}: got {from_record(got[ix], Q)}, want {from_record(want[ix], Q)}")
