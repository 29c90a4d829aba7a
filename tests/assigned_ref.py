"""Plain-Python restatement of the assigned replay (fognet_hip.h "Assigned replay": the node
model under a caller's decisions), with Python integers.  Test infrastructure only."""
from __future__ import annotations

import bisect

import numpy as np

TPS = 10**12
NEVER = int(np.iinfo(np.int64).max)
MAX_TICK = 1 << 61
MAX_S = 1 << 22          # service seconds a task that starts may have
OK, ERR_ARG = 0, 1
STATS = np.dtype([("n_tasks", np.int64), ("max_pending", np.int32), ("events", np.int64), ("status", np.int32)])


def replay_one(arrive, req, assign, mips, dl, ul, init, down=None):
    """One replication.  Returns (status [T], start [T], done [T], record) with record a
    STATS scalar; a refused replication has record status ERR_ARG, n_tasks = events =
    max_pending = 0 and undefined rows."""
    T, N = len(arrive), len(mips)
    arrive, req, assign = [int(x) for x in arrive], [int(x) for x in req], [int(x) for x in assign]
    mips, dl, ul, init = ([int(x) for x in v] for v in (mips, dl, ul, init))
    down = [NEVER] * N if down is None else [int(x) for x in down]
    status, start, done = np.full(T, 9, np.uint8), np.full(T, -1, np.int64), np.full(T, -1, np.int64)
    refused = np.zeros((), STATS)
    refused["status"] = ERR_ARG
    bad = False
    a0 = arrive[0] if T else NEVER
    for j in range(N):
        bad |= mips[j] <= 0 or dl[j] < 0 or ul[j] < 0 or dl[j] > MAX_TICK or ul[j] > MAX_TICK
        bad |= init[j] < ul[j] or init[j] >= a0
        bad |= down[j] != NEVER and (down[j] < init[j] or down[j] > MAX_TICK)
    for i in range(T):
        bad |= not 0 <= assign[i] < N or req[i] < 0 or arrive[i] > MAX_TICK or (i > 0 and arrive[i] < arrive[i - 1])
    if bad:
        return status, start, done, refused
    last = {}      # node -> (computed done, service ticks) of its last queued task
    adverts = {}   # node -> advert ticks of the tasks sent to it, in order (NEVER: never completes)
    max_pending = shorts = 0
    for i in range(T):
        k = assign[i]
        sec = req[i] // mips[k]
        s, a = sec * TPS, arrive[i] + dl[k]
        adv = adverts.setdefault(k, [])
        # pending at the broker when it publishes: earlier tasks whose advert is not strictly before
        # (a FIFO node's adverts are nondecreasing, NEVER last: the count of x >= arrive[i] is a suffix)
        max_pending = max(max_pending, 1 + len(adv) - bisect.bisect_left(adv, arrive[i]))
        if a >= down[k]:  # lost: takes no place in the queue
            adv.append(NEVER)
            shorts += 1
            continue
        if a > MAX_TICK:
            return status, start, done, refused
        if k not in last:
            st, begin = 5, a
        else:
            done_p, s_p = last[k]
            begin = max(a, done_p)
            st = 5 if a > done_p or (a == done_p and dl[k] < s_p) else 4
        end = begin + s
        last[k] = (end, s)
        status[i] = st
        if begin < down[k]:
            if sec >= MAX_S or end > MAX_TICK:  # it starts: its timer cannot be armed
                return status, start, done, refused
            start[i] = begin
            if end < down[k]:
                done[i] = end
        adv.append(end + ul[k] if done[i] >= 0 else NEVER)
        shorts += done[i] < 0
    rec = np.zeros((), STATS)
    rec["n_tasks"], rec["max_pending"], rec["events"] = T, max_pending, 2 * N + 4 * T - 2 * shorts
    return status, start, done, rec


def replay(tr: dict, assign) -> dict:
    """[R, T] batch (node parameters [N] or [R, N]): status / start / done [R, T], stats [R]."""
    arrive, req, assign = np.atleast_2d(tr["arrive"]), np.atleast_2d(tr["req"]), np.atleast_2d(assign)
    R, T = arrive.shape
    out = dict(node=np.array(assign, np.int32), status=np.zeros((R, T), np.uint8), start=np.zeros((R, T), np.int64),
               done=np.zeros((R, T), np.int64), stats=np.zeros(R, STATS))
    for r in range(R):
        par = [tr[k][r] if np.ndim(tr[k]) == 2 else tr[k] for k in ("mips", "dl", "ul", "init")]
        down = tr.get("down")
        if down is not None:
            down = down[r] if np.ndim(down) == 2 else down
        out["status"][r], out["start"][r], out["done"][r], out["stats"][r] = replay_one(
            arrive[r], req[r], assign[r], *par, down=down)
    return out


def assert_equals_oracle(got: dict, o: dict, what=""):
    """The four arrays and the replay fields of a result against the oracle's (oracle_lib.run_batch)."""
    for k in ("status", "start", "done"):
        np.testing.assert_array_equal(got[k], o[k], err_msg=f"{what} {k}")
    for f in ("n_tasks", "max_pending", "events", "status"):
        np.testing.assert_array_equal(got["stats"][f], o["stats"][f], err_msg=f"{what} stats.{f}")
