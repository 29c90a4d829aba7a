"""Expected per-node records (fognet_node_stats) from the ORACLE's per-task outputs,
in Python integers (test infrastructure for test_node_stats*.py; no GPU needed).

A record is built exactly as include/fognet_hip.h defines it; the sums are
unbounded Python ints cut to their limbs at the end, so carries cannot be lost.
"""
from __future__ import annotations

import numpy as np

import oracle_lib as ol
from fognetsimpp_amd import _abi

I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
NODE = _abi.NODE_STATS_DTYPE
M64 = (1 << 64) - 1
OK_STATUSES = (_abi.FOGNET_OK, _abi.FOGNET_REF_ABORTED)


class Mom:
    """count / overflow / extrema / exact sum and sum of squares of raw values."""

    def __init__(self):
        self.n = self.ovf = self.s = self.q = 0
        self.mn, self.mx = I64_MAX, I64_MIN

    def add(self, v: int):
        self.n += 1
        self.s += v
        self.q += v * v
        self.mn, self.mx = min(self.mn, v), max(self.mx, v)

    def merge(self, o: "Mom"):
        self.n += o.n
        self.ovf += o.ovf
        self.s += o.s
        self.q += o.q
        self.mn, self.mx = min(self.mn, o.mn), max(self.mx, o.mx)

    def store(self, rec):
        s = self.s % (1 << 128)  # two's complement
        assert self.q < 1 << 192
        rec["count"], rec["overflow"], rec["min_raw"], rec["max_raw"] = self.n, self.ovf, self.mn, self.mx
        rec["sum_lo"], rec["sum_hi"] = s & M64, s >> 64
        rec["sq_lo"], rec["sq_hi"], rec["sq_top"] = self.q & M64, (self.q >> 64) & M64, self.q >> 128

    @staticmethod
    def load(rec) -> "Mom":
        m = Mom()
        m.n, m.ovf, m.mn, m.mx = int(rec["count"]), int(rec["overflow"]), int(rec["min_raw"]), int(rec["max_raw"])
        s = int(rec["sum_lo"]) | (int(rec["sum_hi"]) << 64)
        m.s = s - (1 << 128) if s >> 127 else s
        m.q = int(rec["sq_lo"]) | (int(rec["sq_hi"]) << 64) | (int(rec["sq_top"]) << 128)
        return m


class Node:
    def __init__(self):
        self.tasks = self.queued = self.started = self.lost = self.busy = 0
        self.last = I64_MIN
        self.queue, self.resp = Mom(), Mom()

    def merge(self, o: "Node"):
        for k in ("tasks", "queued", "started", "lost", "busy"):
            setattr(self, k, getattr(self, k) + getattr(o, k))
        self.last = max(self.last, o.last)
        self.queue.merge(o.queue)
        self.resp.merge(o.resp)

    def store(self, rec):
        rec["n_tasks"], rec["n_queued"], rec["n_started"], rec["n_lost"] = self.tasks, self.queued, self.started, self.lost
        rec["busy_s"], rec["last_tick"] = self.busy, self.last
        self.queue.store(rec["queue"])
        self.resp.store(rec["resp"])

    @staticmethod
    def load(rec) -> "Node":
        n = Node()
        n.tasks, n.queued, n.started, n.lost = (int(rec[k]) for k in ("n_tasks", "n_queued", "n_started", "n_lost"))
        n.busy, n.last = int(rec["busy_s"]), int(rec["last_tick"])
        n.queue, n.resp = Mom.load(rec["queue"]), Mom.load(rec["resp"])
        return n


def to_records(nodes) -> np.ndarray:
    out = np.zeros(len(nodes), NODE)
    for j, n in enumerate(nodes):
        n.store(out[j])
    return out


def empty_records(n: int) -> np.ndarray:
    return to_records([Node() for _ in range(n)])


def expected(tr: dict, o: dict) -> np.ndarray:
    """[R, N] records of a trace (host arrays; node parameters [N] or [R, N]) from
    the oracle's result ``o`` (oracle_lib.run_batch)."""
    arrive, req = np.atleast_2d(tr["arrive"]), np.atleast_2d(tr["req"])
    R = arrive.shape[0]
    N = np.shape(tr["mips"])[-1]
    out = np.zeros((R, N), NODE)
    for r in range(R):
        mips = tr["mips"][r] if np.ndim(tr["mips"]) == 2 else tr["mips"]
        dl = tr["dl"][r] if np.ndim(tr["dl"]) == 2 else tr["dl"]
        nodes = [Node() for _ in range(N)]
        if int(o["stats"]["status"][r]) in OK_STATUSES:
            for i in range(int(o["stats"]["n_tasks"][r])):
                k, st = int(o["node"][r, i]), int(o["status"][r, i])
                t, start, done = int(arrive[r, i]), int(o["start"][r, i]), int(o["done"][r, i])
                nd = nodes[k]
                nd.tasks += 1
                nd.queued += st == 4
                nd.started += st == 5
                nd.lost += st == 9
                if done >= 0:  # completed
                    nd.busy += int(req[r, i]) // int(mips[k])
                    nd.last = max(nd.last, done)
                    nd.resp.add(done - t)
                if st == 4 and start >= 0:  # queueTime emission (ComputeBrokerApp3.cc:238)
                    raw = ol.qtime_raw(start, t + int(dl[k]))
                    if raw is None:
                        nd.queue.ovf += 1
                    else:
                        nd.queue.add(raw)
        out[r] = to_records(nodes)
    return out


def merged(recs) -> Node:
    acc = Node()
    for rec in recs:
        acc.merge(Node.load(rec))
    return acc


def assert_merge_is_rep_record(recs, rep) -> None:
    """The defining invariant (fognet_hip.h): the exact merge of a replication's N
    node records is its fognet_rep_stats (``rep``: one REP_STATS_DTYPE / oracle record)."""
    m = merged(recs)
    got = dict(n_tasks=m.tasks, n_queued=m.queued, n_started=m.started, busy_s=m.busy, last_tick=m.last,
               n_qtime=m.queue.n, n_qtime_overflow=m.queue.ovf, queue_min_raw=m.queue.mn, queue_max_raw=m.queue.mx,
               queue_sum_lo=m.queue.s % (1 << 128) & M64, queue_sum_hi=m.queue.s % (1 << 128) >> 64,
               queue_sq_lo=m.queue.q & M64, queue_sq_hi=(m.queue.q >> 64) & M64, queue_sq_top=m.queue.q >> 128,
               resp_min_ticks=m.resp.mn, resp_max_ticks=m.resp.mx, resp_sum_lo=m.resp.s & M64,
               resp_sum_hi=(m.resp.s >> 64) & M64, resp_sq_lo=m.resp.q & M64, resp_sq_hi=(m.resp.q >> 64) & M64)
    for k, v in got.items():
        assert int(rep[k]) == v, (k, int(rep[k]), v)


def assert_records_equal(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    """Every field of every record (the records of nodes without a task too)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    for idx in np.ndindex(got.shape):
        for k in NODE.names:
            if NODE[k].names:
                for f in NODE[k].names:
                    assert got[idx][k][f] == want[idx][k][f], (what, idx, k, f, got[idx][k][f], want[idx][k][f])
            else:
                assert got[idx][k] == want[idx][k], (what, idx, k, got[idx][k], want[idx][k])


def same_tick_negative(lo: int, dl: int) -> int:
    """The first publish tick t >= lo whose task, enqueued at t + dl and popped in
    that same tick, emits a NEGATIVE queueTime (the enqueue time's double round trip
    lands one tick later: fognet_hip.h "Reference signal values"; it needs ticks of
    2^52 and more, where 1e12 * (a * 1e-12) is no longer a itself)."""
    for t in range(lo, lo + 100000):
        raw = ol.qtime_raw(t + dl, t + dl)
        if raw is not None and raw < 0:
            return t
    raise AssertionError("no same-tick negative queueTime near %d" % lo)


def herded_trace(N: int = 256, T: int = 320, burst: int = 260):
    """C3's herding in the small: until node 0's first completion is advertised, the
    broker's view shows every node idle, so every publish goes to node 0 (strict '<':
    ties -> lowest index).  Task 0 (1 s) starts on arrival; task 1 reaches node 0
    exactly at task 0's completion tick (the downlink, 2 s, is not below the service
    time, so the arrival is first: queued, then popped in the same tick); ``burst``
    more publishes of 64 s each follow before that completion's advert reaches the
    broker, and node 0's queue passes the ~9,223 s at which a queueTime emission
    overflows simtime_t; the remaining publishes come later and spread."""
    S = 10**12
    mips = np.full(N, 1000, np.int32)
    dl = np.full(N, 2 * S, np.int64)
    ul = np.full(N, 2 * S, np.int64)
    init = ul.copy()
    t0 = same_tick_negative(6000 * S, 2 * S) - S  # task 1 is published 1 s after task 0
    arrive = [t0, t0 + S] + [t0 + S + 1 + 10**9 * i for i in range(burst)]  # within 0.26 s: before t0 + S + 4 s
    req = [1000, 64000] + [64000] * burst
    rest = T - len(arrive)
    arrive += [t0 + 30 * S + 10**10 * i for i in range(rest)]
    req += [1000 + 500 * (i % 9) for i in range(rest)]
    return dict(arrive=np.array([arrive], np.int64), req=np.array([req], np.int32), mips=mips, dl=dl, ul=ul, init=init)
