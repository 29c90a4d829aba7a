"""Expected per-user signal records (fognet_per_user_stats_dev's [R][U] fognet_user_stats)
from a finished replay's per-task outputs, in plain Python ints (test infrastructure for
test_per_user_stats*.py; no GPU needed).

Record [r][u] is user_stats_ref.signals over the publishes i < n_tasks of replication r
with user_of[r][i] == u, with that user's links.  Under EXT_HIER the node ack of an
escalated task leaves its node a hop later; signals() takes the node downlinks as an
array indexed by the task's node, so the hop is fed in as N further node entries
(node k + N: dl_k + up, ul_k) that the escalated tasks are pointed at.  A failed
replication gets U empty records; decided publishes whose user lies outside [0, U) are
counted and belong to no record.  The exact merge of records is done on Python ints too.
"""
from __future__ import annotations

import numpy as np

import user_stats_ref as us

USER = us.USER_STATS_DTYPE


def _row(a, r):
    a = np.asarray(a)
    return a[r] if a.ndim == 2 else a


def expected(tr: dict, o: dict, user_of, user_ul, user_dl, flags=None, up: int = 0, statuses=None):
    """([R, U] records, [R] n_unassigned).  user_of [R, T]; user_ul / user_dl [U] or [R, U];
    ``flags`` [R, T]: the replay's escalation flags (EXT_HIER), ``up`` the hop in ticks;
    ``statuses``: replication statuses to go by instead of o["stats"]["status"]."""
    arrive = np.atleast_2d(tr["arrive"])
    user_of = np.atleast_2d(user_of)
    R = arrive.shape[0]
    U = np.shape(user_ul)[-1]
    out = np.zeros((R, U), USER)
    unassigned = np.zeros(R, np.int64)
    for r in range(R):
        status = int(o["stats"]["status"][r]) if statuses is None else int(statuses[r])
        if status not in us.OK_STATUSES:
            out[r] = us.empty_record()
            continue
        n = int(o["stats"]["n_tasks"][r])
        dl, ul = [int(x) for x in _row(tr["dl"], r)], [int(x) for x in _row(tr["ul"], r)]
        N = len(dl)
        node = np.asarray(o["node"][r][:n], np.int64)
        if flags is not None:
            node = node + N * (np.asarray(flags[r][:n]) != 0)
            dl, ul = dl + [d + int(up) for d in dl], ul + ul
        uu, ud = _row(user_ul, r), _row(user_dl, r)
        who = user_of[r][:n]
        unassigned[r] = int(((who < 0) | (who >= U)).sum())
        for u in range(U):
            idx = np.nonzero(who == u)[0]
            out[r, u] = us.to_record(us.signals(arrive[r][idx], node[idx], o["status"][r][idx], o["done"][r][idx], dl, ul,
                                                int(uu[u]), int(ud[u]), len(idx)))
    return out, unassigned


def expand_links(user_of, user_ul, user_dl):
    """Per-task links [R, T] of user_of [R, T] and links [U] or [R, U] (ids in range)."""
    user_of = np.atleast_2d(user_of)
    uu = np.stack([np.asarray(_row(user_ul, r))[user_of[r]] for r in range(user_of.shape[0])])
    ud = np.stack([np.asarray(_row(user_dl, r))[user_of[r]] for r in range(user_of.shape[0])])
    return uu.astype(np.int64), ud.astype(np.int64)


def load_mom(rec) -> us.Mom:
    m = us.Mom()
    m.n, m.ovf, m.mn, m.mx = int(rec["count"]), int(rec["overflow"]), int(rec["min_raw"]), int(rec["max_raw"])
    s = int(rec["sum_lo"]) | (int(rec["sum_hi"]) << 64)
    m.s = s - (1 << 128) if s >> 127 else s
    m.q = int(rec["sq_lo"]) | (int(rec["sq_hi"]) << 64) | (int(rec["sq_top"]) << 128)
    return m


def merged(records, wrap: bool = False) -> np.ndarray:
    """The exact merge of fognet_user_stats records (any iterable) as one record; ``wrap``:
    sums of squares modulo 2^192 (random limbs), else they must fit."""
    acc = {s: us.Mom() for s in us.SIGNALS}
    for rec in records:
        for s in us.SIGNALS:
            b, a = load_mom(rec[s]), acc[s]
            a.n, a.ovf, a.s, a.q = a.n + b.n, a.ovf + b.ovf, a.s + b.s, a.q + b.q
            a.mn, a.mx = min(a.mn, b.mn), max(a.mx, b.mx)
    if wrap:
        for s in us.SIGNALS:
            acc[s].q %= 1 << 192
    return us.to_record(acc)


def empty_records(*shape) -> np.ndarray:
    out = np.zeros(shape, USER)
    out[...] = us.empty_record()
    return out


def assert_records_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for s in us.SIGNALS:
        for f in us.FIELDS:
            np.testing.assert_array_equal(got[s][f], want[s][f], err_msg=f"{what} {s}.{f}")
    assert got.tobytes() == want.tobytes(), what
