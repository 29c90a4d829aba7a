"""Expected signal vectors (fognet_signal_vectors_dev's CSR) from a finished replay's
per-task outputs, in plain Python ints (test infrastructure for test_signal_vectors*.py;
no GPU needed).

The rows and their order are worded as include/fognet_hip.h words them ("Signal vectors"):
V = N + 1 + 3U vectors per replication -- the N nodes' queueTime, the broker's delay, then
U x latency, U x latencyH1, U x taskTime -- whose rows are the emissions that
fognet_node_stats_dev and fognet_per_user_stats_dev count, each vector ascending by

  (time, relayed, tick the node sent the ack, tick its sending event was inserted,
   completion ack, task)

where the broker's own pubAck has relayed = 0 and the two ticks 0, a node's first ack
(sent at arrive + dl_k, from the arrival event created at the decision: arrive) and its
completion ack (sent at done, from the RELEASERESOURCE timer armed at start) relayed = 1.
queueTime and delay rows come in task order (their key is the task alone).
"""
from __future__ import annotations

import numpy as np

import oracle_lib as ol
import user_stats_ref as us

PUBACK, FIRST, COMPLETION = 0, 1, 2  # the kind of a user-side row
ACK_STATUS = {PUBACK: 4, COMPLETION: 6}  # (a first ack carries the task's status, 4 or 5)
LEVELS = ("time", "pubAck first", "send tick", "insertion tick", "first before completion", "task")
OK_STATUSES = us.OK_STATUSES


def n_vectors(N: int, U: int) -> int:
    return N + 1 + 3 * U


def capacity(T: int) -> int:
    return 6 * T


def _row(a, r):
    a = np.asarray(a)
    return a[r] if a.ndim == 2 else a


def replication_rows(arrive, node, status, start, done, dl, ul, user_of, user_ul, user_dl, n_tasks):
    """The V vectors of one replication, each a list of rows (key, time, value, task, kind)
    in emission order.  user_of [T]; user_ul / user_dl [U]."""
    N, U = len(dl), len(user_ul)
    vec = [[] for _ in range(n_vectors(N, U))]
    lat, h1, tt = N + 1, N + 1 + U, N + 1 + 2 * U
    for i in range(int(n_tasks)):
        t, k, st, s0, dn, u = int(arrive[i]), int(node[i]), int(status[i]), int(start[i]), int(done[i]), int(user_of[i])
        if st == 4 and s0 >= 0:  # queueTime (ComputeBrokerApp3.cc:238), at the service start
            raw = ol.qtime_raw(s0, t + int(dl[k]))
            if raw is not None:
                vec[k].append(((i,), s0, raw, i, None))
        if not 0 <= u < U:
            continue
        uu, ud = int(user_ul[u]), int(user_dl[u])
        created = t - uu
        vec[N].append(((i,), t, uu, i, None))  # delay (BrokerBaseApp3.cc:143), at the publish's arrival

        def emit(v, time, key, kind):
            raw = us.ms_raw(time - created)
            if raw is not None:
                vec[v].append(((time,) + key + (i,), time, raw, i, kind))
        emit(h1 + u, t + ud, (0, 0, 0, 0), PUBACK)
        relay = int(ul[k]) + ud
        sent = t + int(dl[k])
        if st == 5:
            emit(lat + u, sent + relay, (1, sent, t, 0), FIRST)
        elif st == 4:
            emit(h1 + u, sent + relay, (1, sent, t, 0), FIRST)
        if dn >= 0:
            emit(tt + u, dn + relay, (1, dn, s0, 1), COMPLETION)
    for v in vec:
        v.sort(key=lambda row: row[0])
    return vec


def to_csr(vec, cap: int):
    """(offset [V + 1], time [cap], value [cap], task [cap]); rows past offset[V] are 0."""
    off = np.zeros(len(vec) + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in vec])
    assert off[-1] <= cap
    time, value, task = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.int32)
    p = 0
    for v in vec:
        for _, tm, val, i, _ in v:
            time[p], value[p], task[p] = tm, val, i
            p += 1
    return off, time, value, task


def expected(tr: dict, o: dict, user_of, user_ul, user_dl, r0: int = 0, Rv: int | None = None, statuses=None,
             with_rows: bool = False):
    """dict(offset [Rv, V + 1], time / value / task [Rv, 6T]) of replications [r0, r0 + Rv) of a
    trace from per-task outputs ``o`` (node / status / start / done [R, T], stats [R]); a failed
    replication gets all-zero offsets.  ``with_rows``: also the row lists, "rows" [Rv]."""
    arrive = np.atleast_2d(tr["arrive"])
    user_of = np.atleast_2d(user_of)
    R, T = arrive.shape
    Rv = R - r0 if Rv is None else Rv
    N, U = np.shape(tr["dl"])[-1], np.shape(user_ul)[-1]
    V, cap = n_vectors(N, U), capacity(T)
    out = dict(offset=np.zeros((Rv, V + 1), np.int64), time=np.zeros((Rv, cap), np.int64),
               value=np.zeros((Rv, cap), np.int64), task=np.zeros((Rv, cap), np.int32), rows=[])
    for q in range(Rv):
        r = r0 + q
        status = int(o["stats"]["status"][r]) if statuses is None else int(statuses[r])
        vec = [[] for _ in range(V)]
        if status in OK_STATUSES:
            vec = replication_rows(arrive[r], o["node"][r], o["status"][r], o["start"][r], o["done"][r], _row(tr["dl"], r),
                                   _row(tr["ul"], r), user_of[r], _row(user_ul, r), _row(user_dl, r),
                                   int(o["stats"]["n_tasks"][r]))
        out["offset"][q], out["time"][q], out["value"][q], out["task"][q] = to_csr(vec, cap)
        out["rows"].append(vec)
    if not with_rows:
        del out["rows"]
    return out


def user_sequence(vec, N: int, U: int, u: int):
    """User u's three vectors merged into the one sequence in which the module made the
    emissions: rows (key, time, value, task, kind), ascending by the key."""
    rows = vec[N + 1 + u] + vec[N + 1 + U + u] + vec[N + 1 + 2 * U + u]
    return sorted(rows, key=lambda row: row[0])


def deciding_levels(seq) -> list:
    """How many adjacent pairs of a user's sequence each level of the key decided (the first
    word in which the two keys differ), in LEVELS' order."""
    n = [0] * len(LEVELS)
    for a, b in zip(seq, seq[1:]):
        n[next(w for w in range(len(LEVELS)) if a[0][w] != b[0][w])] += 1
    return n


def same_tick_rows(seq) -> int:
    """Rows of a sequence that share their time with a neighbour."""
    times = [row[1] for row in seq]
    return sum(1 for j, t in enumerate(times) if (j > 0 and times[j - 1] == t) or (j + 1 < len(times) and times[j + 1] == t))


def assert_equal(got: dict, want: dict, what="") -> None:
    """Offsets, and times, values and tasks up to offset[V], byte for byte."""
    np.testing.assert_array_equal(got["offset"], want["offset"], err_msg=f"{what} offset")
    for q in range(want["offset"].shape[0]):
        n = int(want["offset"][q, -1])
        for k in ("time", "value", "task"):
            g, w = np.asarray(got[k][q][:n]), want[k][q][:n]
            assert g.dtype == w.dtype
            np.testing.assert_array_equal(g, w, err_msg=f"{what} replication {q} {k}")
            assert g.tobytes() == w.tobytes()
