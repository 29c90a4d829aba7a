"""The paired comparison of two replays (fognet_hip.h "Paired comparison") in plain Python
integers: the record of one replication, the job merge and the two histogram rows.  A record is
a dict of Python ints (sums unbounded and signed); to_record() folds it into the ABI's limbs."""
from __future__ import annotations

import numpy as np

from fognetsimpp_amd import _abi

CMP = _abi.COMPARE_STATS_DTYPE
OK, ABORTED = _abi.FOGNET_OK, _abi.FOGNET_REF_ABORTED
I64_MAX, I64_MIN = 2**63 - 1, -2**63
BINS = _abi.HIST_BINS
STATUS_INDEX = {5: 0, 4: 1, 9: 2}
COUNTS = ("n_reps", "n_pairs", "n_moved") + _abi.COMPARE_COUNTS
SIGNALS = _abi.COMPARE_SIGNALS


def wrap64(v: int) -> int:
    """v modulo 2^64 as a signed 64-bit value (the differences are formed modulo 2^64)."""
    v &= 2**64 - 1
    return v - 2**64 if v >= 2**63 else v


def hist_bin(ticks: int) -> int:
    """Histogram metric 1's rule: the bit length of the whole milliseconds, capped."""
    return min((ticks // 10**9).bit_length(), BINS - 1)


def moments() -> dict:
    return dict(count=0, min=I64_MAX, max=I64_MIN, sum=0, sq=0)


def moments_add(m: dict, v: int):
    m["count"] += 1
    m["min"], m["max"] = min(m["min"], v), max(m["max"], v)
    m["sum"] += v
    m["sq"] += v * v


def empty(status_a: int = OK, status_b: int = OK) -> dict:
    d = dict(status_a=int(status_a), status_b=int(status_b), trans=[[0] * 3 for _ in range(3)])
    d.update({k: 0 for k in COUNTS})
    d.update({s: moments() for s in SIGNALS})
    return d


def new_hist() -> list:
    return [[0] * BINS, [0] * BINS]


def replication(a: dict, b: dict, r: int, hist: list | None = None) -> dict:
    """The record of replication r.  a, b: host copies of the two outputs (node, status, start,
    done [R, T]; stats [R] records).  hist: [2][BINS], added to under the job rule."""
    sa, sb = int(a["stats"]["status"][r]), int(b["stats"]["status"][r])
    rec = empty(sa, sb)
    if sa not in (OK, ABORTED) or sb not in (OK, ABORTED):
        return rec  # (none of its rows is read)
    T = a["node"].shape[1]
    n = max(0, min(int(a["stats"]["n_tasks"][r]), int(b["stats"]["n_tasks"][r]), T))
    rec["n_reps"], rec["n_pairs"] = 1, n
    in_hist = hist is not None and sa == OK and sb == OK
    for i in range(n):
        rec["n_moved"] += int(a["node"][r, i]) != int(b["node"][r, i])
        ia, ib = STATUS_INDEX.get(int(a["status"][r, i])), STATUS_INDEX.get(int(b["status"][r, i]))
        if ia is not None and ib is not None:
            rec["trans"][ia][ib] += 1
        da, db = int(a["done"][r, i]), int(b["done"][r, i])
        key = {(True, True): "n_done_both", (True, False): "n_done_only_a", (False, True): "n_done_only_b",
               (False, False): "n_done_neither"}[(da >= 0, db >= 0)]
        rec[key] += 1
        if key != "n_done_both":
            continue
        ds = wrap64(int(b["start"][r, i]) - int(a["start"][r, i]))
        dr = wrap64(db - da)
        dv = wrap64(dr - ds)
        moments_add(rec["d_start"], ds)
        moments_add(rec["d_service"], dv)
        moments_add(rec["d_resp"], dr)
        rec["n_better" if dr < 0 else "n_worse" if dr > 0 else "n_equal"] += 1
        if in_hist and dr != 0:
            hist[0 if dr < 0 else 1][hist_bin(abs(dr))] += 1
    s = rec["d_resp"]["sum"]
    s = s % 2**128  # the sign of the signed 128-bit sum
    s = s - 2**128 if s >= 2**127 else s
    rec["rep_better" if s < 0 else "rep_worse" if s > 0 else "rep_equal"] = 1
    return rec


def merge(acc: dict, other: dict) -> dict:
    """acc (+) other, field by field; acc's statuses stay."""
    for k in COUNTS:
        acc[k] += other[k]
    for i in range(3):
        for j in range(3):
            acc["trans"][i][j] += other["trans"][i][j]
    for s in SIGNALS:
        m, o = acc[s], other[s]
        m["count"] += o["count"]
        m["min"], m["max"] = min(m["min"], o["min"]), max(m["max"], o["max"])
        m["sum"] += o["sum"]
        m["sq"] += o["sq"]
    return acc


def job(recs) -> dict:
    """The job record: the merge of the records whose two statuses are OK."""
    acc = empty()
    for rec in recs:
        if rec["status_a"] == OK and rec["status_b"] == OK:
            merge(acc, rec)
    return acc


def compare(a: dict, b: dict):
    """([R] records, the job record, hist [2][BINS]) of two outputs."""
    hist = new_hist()
    recs = [replication(a, b, r, hist) for r in range(len(a["stats"]))]
    return recs, job(recs), hist


def to_record(d: dict) -> np.ndarray:
    rec = np.zeros((), CMP)
    rec["status_a"], rec["status_b"] = d["status_a"], d["status_b"]
    for k in COUNTS:
        rec[k] = wrap64(d[k])
    rec["trans"] = np.array(d["trans"], np.int64)
    for s in SIGNALS:
        m = d[s]
        rec[s]["count"], rec[s]["min_raw"], rec[s]["max_raw"], rec[s]["overflow"] = m["count"], m["min"], m["max"], 0
        tot, sq = m["sum"] % 2**128, m["sq"] % 2**192
        rec[s]["sum_lo"], rec[s]["sum_hi"] = tot & (2**64 - 1), tot >> 64
        rec[s]["sq_lo"], rec[s]["sq_hi"], rec[s]["sq_top"] = sq & (2**64 - 1), (sq >> 64) & (2**64 - 1), sq >> 128
    return rec


def from_record(rec) -> dict:
    d = empty(int(rec["status_a"]), int(rec["status_b"]))
    for k in COUNTS:
        d[k] = int(rec[k])
    d["trans"] = [[int(x) for x in row] for row in rec["trans"]]
    for s in SIGNALS:
        m = rec[s]
        tot = int(m["sum_lo"]) | (int(m["sum_hi"]) << 64)
        d[s] = dict(count=int(m["count"]), min=int(m["min_raw"]), max=int(m["max_raw"]),
                    sum=tot - 2**128 if tot >= 2**127 else tot,
                    sq=int(m["sq_lo"]) | (int(m["sq_hi"]) << 64) | (int(m["sq_top"]) << 128))
    return d


def to_records(recs) -> np.ndarray:
    out = np.zeros(len(recs), CMP)
    for i, d in enumerate(recs):
        out[i] = to_record(d)
    return out


def assert_equal(got: np.ndarray, want: np.ndarray, what: str = ""):
    """Byte equality of record arrays, naming the first field that differs."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    for r in range(got.size):
        for k in CMP.names:
            if got[r][k].tobytes() != want[r][k].tobytes():
                raise AssertionError(f"{what}: record {r} field {k}: got {got[r][k]} want {want[r][k]}")
    raise AssertionError(f"{what}: records differ")
