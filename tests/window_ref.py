"""Expected time-window records (fognet_window_stats_dev's [R][W] fognet_window_stats) from a
finished replay's per-task outputs, in plain Python ints (test infrastructure for
test_window_stats*.py; no GPU needed).

Worded as include/fognet_hip.h words them ("Time-window statistics"), in two ways that must
agree: expected() goes through every task's events (task_events) and, for the two intervals,
through every window an interval overlaps; binned() takes the five signals from the rows of
signal_vectors_ref.replication_rows, whose order and times are held to the reference's
recordings, and bins them by their times.

  window w           the ticks [t0 + w * window, t0 + (w + 1) * window), w in [0, W)
  point events       the emissions of the five signals at the times of "Signal vectors" (task_events
                     spells them out on its own, and binned() holds them to signal_vectors_ref's
                     rows), n_publish at arrive, n_complete at done.  at_node = arrive + dl_k (+ the
                     hop where escalated).
  intervals          busy: [start, done), insys: [at_node, done), of every completed task
  n_outside          point events before t0 / at or past t0 + W * window
"""
from __future__ import annotations

import numpy as np

import node_stats_ref as ns
import oracle_lib as ol
import user_stats_ref as us
from fognetsimpp_amd import _abi

WINDOW = _abi.WINDOW_STATS_DTYPE
SIGNALS = _abi.WINDOW_SIGNALS  # queue, delay, latency, latencyH1, taskTime
USER_SIGNALS = us.SIGNALS
COUNTS = ("n_publish", "n_complete")
INTERVALS = ("busy", "insys")
M64 = (1 << 64) - 1
OK_STATUSES = us.OK_STATUSES


def _row(a, r):
    a = np.asarray(a)
    return a[r] if a.ndim == 2 else a


class Win:
    """One window's record on unbounded ints."""

    def __init__(self):
        self.n_publish = self.n_complete = self.busy = self.insys = 0
        self.sig = {s: ns.Mom() for s in SIGNALS}

    def merge(self, o: "Win"):
        for k in COUNTS + INTERVALS:
            setattr(self, k, getattr(self, k) + getattr(o, k))
        for s in SIGNALS:
            self.sig[s].merge(o.sig[s])

    def store(self, rec):
        rec["n_publish"], rec["n_complete"] = self.n_publish, self.n_complete
        for k in INTERVALS:
            v = getattr(self, k)
            assert 0 <= v < 1 << 128
            rec[k + "_lo"], rec[k + "_hi"] = v & M64, v >> 64
        for s in SIGNALS:
            self.sig[s].store(rec[s])

    @staticmethod
    def load(rec) -> "Win":
        w = Win()
        w.n_publish, w.n_complete = int(rec["n_publish"]), int(rec["n_complete"])
        for k in INTERVALS:
            setattr(w, k, int(rec[k + "_lo"]) | (int(rec[k + "_hi"]) << 64))
        w.sig = {s: ns.Mom.load(rec[s]) for s in SIGNALS}
        return w


def to_records(wins) -> np.ndarray:
    out = np.zeros(len(wins), WINDOW)
    for j, w in enumerate(wins):
        w.store(out[j])
    return out


def empty_records(n: int) -> np.ndarray:
    return to_records([Win() for _ in range(n)])


def merged(recs, wrap: bool = False) -> Win:
    """The exact merge of records (any iterable); ``wrap``: limbs modulo their width (random limbs)."""
    acc = Win()
    for rec in recs:
        acc.merge(Win.load(rec))
    if wrap:
        acc.busy %= 1 << 128
        acc.insys %= 1 << 128
        for s in SIGNALS:
            acc.sig[s].q %= 1 << 192
            acc.sig[s].s = (acc.sig[s].s + (1 << 127)) % (1 << 128) - (1 << 127)
    return acc


def task_events(t, k, st, start, done, dl, ul, user, hop):
    """(points, intervals) of one decided publish.  points: (signal or count, time, raw value or
    None for a lost emission); intervals: (name, a, b).  ``user``: (ul_u, dl_u) or None for a
    publish without a user in range; ``hop``: the ticks an escalated task reaches its node later."""
    at_node = t + int(dl[k]) + hop
    points = [("n_publish", t, 0)]
    if st == 4 and start >= 0:
        points.append(("queue", start, ol.qtime_raw(start, at_node)))
    if user is not None:
        uu, ud = user
        created = t - uu
        relay = int(ul[k]) + ud
        points.append(("delay", t, uu))
        points.append(("latencyH1", t + ud, us.ms_raw(t + ud - created)))
        if st in (4, 5):
            points.append(("latency" if st == 5 else "latencyH1", at_node + relay, us.ms_raw(at_node + relay - created)))
        if done >= 0:
            points.append(("taskTime", done + relay, us.ms_raw(done + relay - created)))
    intervals = []
    if done >= 0:
        points.append(("n_complete", done, 0))
        intervals = [("busy", start, done), ("insys", at_node, done)]
    return points, intervals


def replication_events(arrive, node, status, start, done, dl, ul, user_of, user_ul, user_dl, n_tasks, flags=None, up=0):
    """task_events of a replication's first n_tasks publishes, and the number without a user."""
    U = 0 if user_ul is None else len(user_ul)
    points, intervals, unassigned = [], [], 0
    for i in range(int(n_tasks)):
        u = int(user_of[i]) if U else -1
        user = (int(user_ul[u]), int(user_dl[u])) if 0 <= u < U else None
        unassigned += user is None
        hop = int(up) if flags is not None and int(flags[i]) else 0
        p, iv = task_events(int(arrive[i]), int(node[i]), int(status[i]), int(start[i]), int(done[i]), dl, ul, user, hop)
        points += p
        intervals += iv
    return points, intervals, unassigned


def window_records(points, intervals, t0: int, window: int, W: int):
    """([W] Win, [before, after]) of one replication's events."""
    wins = [Win() for _ in range(W)]
    outside = [0, 0]
    end = t0 + W * window
    for what, at, raw in points:
        if at < t0:
            outside[0] += 1
        elif at >= end:
            outside[1] += 1
        else:
            w = wins[(at - t0) // window]
            if what in COUNTS:
                setattr(w, what, getattr(w, what) + 1)
            elif raw is None:
                w.sig[what].ovf += 1
            else:
                w.sig[what].add(raw)
    for what, a, b in intervals:
        a, b = max(a, t0), min(b, end)
        if a >= b:
            continue
        for j in range((a - t0) // window, (b - 1 - t0) // window + 1):  # every window it overlaps
            lo = t0 + j * window
            part = min(b, lo + window) - max(a, lo)
            assert part > 0
            setattr(wins[j], what, getattr(wins[j], what) + part)
    return wins, outside


def _replications(tr, o, user_of, user_ul, user_dl, flags, up, statuses):
    arrive = np.atleast_2d(tr["arrive"])
    R = arrive.shape[0]
    who = None if user_of is None else np.atleast_2d(user_of)
    for r in range(R):
        status = int(o["stats"]["status"][r]) if statuses is None else int(statuses[r])
        if status not in OK_STATUSES:
            yield r, None
            continue
        yield r, replication_events(arrive[r], o["node"][r], o["status"][r], o["start"][r], o["done"][r],
                                    _row(tr["dl"], r), _row(tr["ul"], r), None if who is None else who[r],
                                    None if user_ul is None else _row(user_ul, r),
                                    None if user_dl is None else _row(user_dl, r), int(o["stats"]["n_tasks"][r]),
                                    None if flags is None else flags[r], up)


def expected(tr: dict, o: dict, user_of, user_ul, user_dl, t0: int, window: int, W: int, flags=None, up: int = 0,
             statuses=None):
    """([R, W] records, [R, 2] n_outside, [R] n_unassigned).  user_of [R, T], user_ul / user_dl [U]
    or [R, U], or all three None (no user side); ``flags`` [R, T]: the replay's escalation flags
    (EXT_HIER), ``up`` the hop in ticks; ``statuses``: replication statuses to go by instead of
    o["stats"]["status"] (a failed replication gets empty records and zero counts)."""
    R = np.atleast_2d(tr["arrive"]).shape[0]
    out = np.zeros((R, W), WINDOW)
    outside, unassigned = np.zeros((R, 2), np.int64), np.zeros(R, np.int64)
    for r, ev in _replications(tr, o, user_of, user_ul, user_dl, flags, up, statuses):
        if ev is None:
            out[r] = empty_records(W)
            continue
        wins, outside[r] = window_records(ev[0], ev[1], t0, window, W)
        out[r] = to_records(wins)
        unassigned[r] = ev[2]
    return out, outside, unassigned


def latest_tick(tr: dict, o: dict, user_of, user_ul, user_dl, flags=None, up: int = 0) -> int:
    """The latest tick of any event of any readable replication (0 if there is none): a range
    [0, latest_tick + 1) leaves nothing outside."""
    last = 0
    for _, ev in _replications(tr, o, user_of, user_ul, user_dl, flags, up, None):
        if ev is not None:
            last = max([last] + [at for _, at, _ in ev[0]] + [b for _, _, b in ev[1]])
    return last


def event_ticks(tr: dict, o: dict, user_of, user_ul, user_dl, r: int = 0) -> list:
    """The sorted distinct ticks of replication r's point events (to put window edges on them)."""
    for q, ev in _replications(tr, o, user_of, user_ul, user_dl, None, 0, None):
        if q == r:
            return sorted({at for _, at, _ in ev[0]})
    return []


def binned(vec, N: int, U: int, t0: int, window: int, W: int):
    """The five signals of [W] Win from the vectors of signal_vectors_ref.replication_rows (rows
    (key, time, value, task, kind)), each row into the window of its time; rows outside are
    dropped.  Lost emissions are no rows, so ``ovf`` stays 0."""
    wins = [Win() for _ in range(W)]
    names = ["queue"] * N + ["delay"] + ["latency"] * U + ["latencyH1"] * U + ["taskTime"] * U
    for name, rows in zip(names, vec):
        for _, at, value, _, _ in rows:
            if t0 <= at < t0 + W * window:
                wins[(at - t0) // window].sig[name].add(value)
    return wins


def assert_signals_match_rows(recs, wins) -> None:
    """Count, extrema and sums of every signal of records [W] equal those binned from rows."""
    for j, (rec, w) in enumerate(zip(recs, wins)):
        for s in SIGNALS:
            g, m = ns.Mom.load(rec[s]), w.sig[s]
            assert (g.n, g.mn, g.mx, g.s, g.q) == (m.n, m.mn, m.mx, m.s, m.q), (j, s)


def assert_records_equal(got, want, what: str = "") -> None:
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    for idx in np.ndindex(got.shape):
        for k in WINDOW.names:
            if WINDOW[k].names:
                for f in WINDOW[k].names:
                    assert got[idx][k][f] == want[idx][k][f], (what, idx, k, f, got[idx][k][f], want[idx][k][f])
            else:
                assert got[idx][k] == want[idx][k], (what, idx, k, got[idx][k], want[idx][k])
