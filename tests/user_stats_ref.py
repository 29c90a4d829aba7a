"""Expected user-side signal records (fognet_user_stats) from a finished replay's
per-task outputs, in plain Python ints and floats (test infrastructure for
test_user_stats*.py; no GPU needed).

An independent restatement: nothing here comes from oracle/ or the package.  The
signals are worded as include/fognet_hip.h words them ("Reference signal values"
and the fognet_user_stats comment); numpy only carries the arrays in and the
finished limbs out, no value is computed with it.

  created    = arrive - user_ul                    (the publish's send time at the user)
  delay      raw = user_ul, every publish          (a simtime_t in ticks)
  latencyH1  ms_raw(user_ul + user_dl), every publish: the broker's own status-4
             pubAck reaches the user at arrive + user_dl
  node ack   sent when the task reaches its node, at arrive + dl_k; at the broker
             ul_k later, at the user user_dl later:
             status 5 -> latency, status 4 -> latencyH1, status 9 (lost) -> none
  taskTime   done >= 0: ms_raw(done + ul_k + user_dl - created)
  ms_raw(d)  = to_int64(float(d) * 1000.0); to_int64(x) = floor(x + 0.5), an
             emission lost (overflow) where that leaves the int64 range

Python's float(int) is correctly rounded (to nearest, ties to even), which is
what the reference's (double) conversion of an int64 does.
"""
from __future__ import annotations

import math

import numpy as np

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
M64 = (1 << 64) - 1
SIGNALS = ("delay", "latency", "latencyH1", "taskTime")
FIELDS = ("count", "min_raw", "max_raw", "sum_lo", "sum_hi", "sq_lo", "sq_hi", "sq_top", "overflow")
# struct fognet_moments / fognet_user_stats (include/fognet_hip.h), field by field
MOMENTS_DTYPE = np.dtype([("count", np.int64), ("min_raw", np.int64), ("max_raw", np.int64),
                          ("sum_lo", np.uint64), ("sum_hi", np.uint64), ("sq_lo", np.uint64), ("sq_hi", np.uint64),
                          ("sq_top", np.uint64), ("overflow", np.int64)])
USER_STATS_DTYPE = np.dtype([(n, MOMENTS_DTYPE) for n in SIGNALS])
OK_STATUSES = (0, 9)  # FOGNET_OK, FOGNET_REF_ABORTED: every other status is a failed replication


def to_int64(x: float):
    """SimTime::toInt64: floor(x + 0.5), None where the reference throws."""
    f = math.floor(x + 0.5)
    if abs(f) >= 2.0**63:
        return None
    return int(f)


def ms_raw(d: int):
    """Raw simtime_t of (simTime() - created) * 1000 for a difference of d ticks."""
    return to_int64(float(d) * 1000.0)


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

    def add_ms(self, d: int):
        raw = ms_raw(d)
        if raw is None:
            self.ovf += 1
        else:
            self.add(raw)

    def store(self, rec):
        s = self.s % (1 << 128)  # two's complement
        assert self.q < 1 << 192
        rec["count"], rec["overflow"], rec["min_raw"], rec["max_raw"] = self.n, self.ovf, self.mn, self.mx
        rec["sum_lo"], rec["sum_hi"] = s & M64, s >> 64
        rec["sq_lo"], rec["sq_hi"], rec["sq_top"] = self.q & M64, (self.q >> 64) & M64, self.q >> 128


def signals(arrive, node, status, done, dl, ul, user_ul, user_dl, n_tasks) -> dict:
    """The four signals' moments of one replication's first ``n_tasks`` publishes.
    arrive/node/status/done: [T]; dl/ul: [N]; user_ul/user_dl: [T] (per task) or scalars."""
    per_task = np.ndim(user_ul) == 1
    m = {s: Mom() for s in SIGNALS}
    for i in range(int(n_tasks)):
        t, k, st, dn = int(arrive[i]), int(node[i]), int(status[i]), int(done[i])
        uu, ud = (int(user_ul[i]), int(user_dl[i])) if per_task else (int(user_ul), int(user_dl))
        created = t - uu
        m["delay"].add(t - created)
        m["latencyH1"].add_ms(t + ud - created)  # the broker's own pubAck, status 4
        at_user = t + int(dl[k]) + int(ul[k]) + ud  # the node's ack, sent at the task's arrival
        if st == 5:
            m["latency"].add_ms(at_user - created)
        elif st == 4:
            m["latencyH1"].add_ms(at_user - created)
        if dn >= 0:
            m["taskTime"].add_ms(dn + int(ul[k]) + ud - created)
    return m


def to_record(m: dict) -> np.ndarray:
    rec = np.zeros((), USER_STATS_DTYPE)
    for s in SIGNALS:
        m[s].store(rec[s])
    return rec


def empty_record() -> np.ndarray:
    return to_record({s: Mom() for s in SIGNALS})


def expected(tr: dict, o: dict, user_ul, user_dl, statuses=None) -> np.ndarray:
    """[R] records of a trace (host arrays; node parameters [N] or [R, N]; user links [R]
    or [R, T]) from per-task outputs ``o`` (node / status / done [R, T], stats [R] with
    n_tasks and status).  ``statuses``: replication statuses to go by instead of
    o["stats"]["status"]; a failed replication gets the empty record."""
    arrive = np.atleast_2d(tr["arrive"])
    R = arrive.shape[0]
    out = np.zeros(R, USER_STATS_DTYPE)
    for r in range(R):
        status = int(o["stats"]["status"][r]) if statuses is None else int(statuses[r])
        if status not in OK_STATUSES:
            out[r] = empty_record()
            continue
        dl = tr["dl"][r] if np.ndim(tr["dl"]) == 2 else tr["dl"]
        ul = tr["ul"][r] if np.ndim(tr["ul"]) == 2 else tr["ul"]
        out[r] = to_record(signals(arrive[r], o["node"][r], o["status"][r], o["done"][r], dl, ul, user_ul[r],
                                   user_dl[r], o["stats"]["n_tasks"][r]))
    return out


def assert_user_parity(g_user, o_user):
    """Exact equality of all nine fognet_moments fields of all four signals."""
    for n in SIGNALS:
        for f in FIELDS:
            np.testing.assert_array_equal(g_user[n][f], o_user[n][f], err_msg=f"{n}.{f}")


def is_empty(rec) -> bool:
    """``rec`` (one USER_STATS_DTYPE record) is the count == 0 record in all four signals."""
    return np.asarray(rec).tobytes() == empty_record().tobytes()
