"""Replication groups restated in Python integers (fognet_hip.h "Replication groups"): the nine
metrics of one fognet_rep_stats record, the group record of any set of records, its merge and its
job record.  Nothing here calls the library; the tests hold the host twins and the device pass to
these bytes.  Also: the crafted records the CPU and GPU tests share."""
import math
import struct

import numpy as np

from fognetsimpp_amd import _abi

I64_MIN, I64_MAX = -2**63, 2**63 - 1
M64, M128, M192 = 2**64 - 1, 2**128 - 1, 2**192 - 1
OK, REF_ABORTED = _abi.FOGNET_OK, _abi.FOGNET_REF_ABORTED
NMET = len(_abi.REP_METRICS)
UNIT_EXP = (9, 9, 12, 12, 6, 12, 0, 0, 6)   # the writer's unit of metric m is 10^-UNIT_EXP[m]
SCA_NAMES = ("respMean", "respMax", "queueMean", "queueMax", "queuedShare", "makespan", "busySeconds", "maxPending",
             "energy")


def signed(v: int, bits: int) -> int:
    return v - (1 << bits) if v >> (bits - 1) else v


def _u128(rec, name) -> int:
    return int(rec[name + "_lo"]) | (int(rec[name + "_hi"]) << 64)


def energy_uj(e: float):
    """toInt64(e * 1e6): one IEEE multiply, floor(x + 0.5) with its own rounding; None outside int64."""
    x = float(np.float64(e) * np.float64(1e6))
    if math.isnan(x):
        return None
    y = float(np.float64(x) + np.float64(0.5))
    if math.isinf(y):
        return None
    f = math.floor(y)
    return f if abs(f) < 2**63 else None


def metrics(rec):
    """[(defined, value or None)] * 9: value None = defined but outside int64 (lost)."""
    n, nq = int(rec["n_tasks"]), int(rec["n_qtime"])
    out = [(False, None)] * NMET

    def put(k, v):
        out[k] = (True, v if v is not None and I64_MIN <= v <= I64_MAX else None)

    if n > 0:
        put(0, _u128(rec, "resp_sum") // n)
        put(1, int(rec["resp_max_ticks"]))
        put(4, int(rec["n_queued"]) * 10**6 // n)
    if nq > 0:
        put(2, signed(_u128(rec, "queue_sum"), 128) // nq)   # Python's // floors towards minus infinity
        put(3, int(rec["queue_max_raw"]))
    if int(rec["last_tick"]) != I64_MIN:
        put(5, int(rec["last_tick"]))
    put(6, int(rec["busy_s"]))
    put(7, int(rec["max_pending"]))
    put(8, energy_uj(float(rec["energy_j"])))
    return out


def metrics_row(rec):
    """The device's metrics row and defined word of one record (status looked at)."""
    row, bits = [I64_MIN] * NMET, 0
    if int(rec["status"]) == OK:
        for k, (d, v) in enumerate(metrics(rec)):
            if d and v is not None:
                row[k], bits = v, bits | (1 << k)
    return row, bits


class Mom:
    def __init__(self):
        self.count = self.overflow = self.sum = self.sq = 0
        self.mn, self.mx = I64_MAX, I64_MIN

    def merge(self, count, mn, mx, s, q, overflow):
        self.count = (self.count + count) & M64
        self.overflow = (self.overflow + overflow) & M64
        self.mn, self.mx = min(self.mn, mn), max(self.mx, mx)
        self.sum = (self.sum + s) & M128
        self.sq = (self.sq + q) & M192

    def add_value(self, v):
        self.merge(1, v, v, v & M128, v * v, 0)

    def merge_mom(self, o):
        self.merge(o.count, o.mn, o.mx, o.sum, o.sq, o.overflow)

    def pack(self) -> bytes:
        return struct.pack("<qqqQQQQQq", signed(self.count, 64), self.mn, self.mx, self.sum & M64, self.sum >> 64,
                           self.sq & M64, (self.sq >> 64) & M64, self.sq >> 128, signed(self.overflow, 64))


class Group:
    def __init__(self):
        self.head = [0] * 7     # n_reps, n_failed, n_ref_aborted, n_tasks, n_queued, n_started, events
        self.queue, self.resp = Mom(), Mom()
        self.across = [Mom() for _ in range(NMET)]

    def add_rep(self, rec):
        st = int(rec["status"])
        self.head[0] += 1
        if st in (OK, REF_ABORTED) and int(rec["abort_tick"]) != I64_MAX:
            self.head[2] += 1
        if st != OK:
            self.head[1] += 1
            return
        for w, k in enumerate(("n_tasks", "n_queued", "n_started", "events")):
            self.head[3 + w] = (self.head[3 + w] + int(rec[k])) & M64
        self.queue.merge(int(rec["n_qtime"]) & M64, int(rec["queue_min_raw"]), int(rec["queue_max_raw"]),
                         _u128(rec, "queue_sum"), _u128(rec, "queue_sq") | (int(rec["queue_sq_top"]) << 128),
                         int(rec["n_qtime_overflow"]) & M64)
        self.resp.merge(int(rec["n_tasks"]) & M64, int(rec["resp_min_ticks"]), int(rec["resp_max_ticks"]),
                        _u128(rec, "resp_sum"), _u128(rec, "resp_sq"), 0)
        for k, (d, v) in enumerate(metrics(rec)):
            if d and v is None:
                self.across[k].overflow += 1
            elif d:
                self.across[k].add_value(v)

    def merge(self, o):
        self.head = [(a + b) & M64 for a, b in zip(self.head, o.head)]
        self.queue.merge_mom(o.queue)
        self.resp.merge_mom(o.resp)
        for a, b in zip(self.across, o.across):
            a.merge_mom(b)

    def pack(self) -> bytes:
        return struct.pack("<7q", *[signed(h, 64) for h in self.head]) + self.queue.pack() + self.resp.pack() + \
            b"".join(m.pack() for m in self.across)

    def record(self) -> np.ndarray:
        return np.frombuffer(self.pack(), dtype=_abi.GROUP_STATS_DTYPE)[0]


def reduce_groups(reps, group_of=None, G=1):
    """([G] Group, n_ungrouped) of REP_STATS_DTYPE records under group_of (None: all in group 0)."""
    groups, lost = [Group() for _ in range(G)], 0
    for r, rec in enumerate(reps):
        g = 0 if group_of is None else int(group_of[r])
        if 0 <= g < G:
            groups[g].add_rep(rec)
        else:
            lost += 1
    return groups, lost


def records(groups) -> np.ndarray:
    return np.frombuffer(b"".join(g.pack() for g in groups), dtype=_abi.GROUP_STATS_DTYPE)


# The same reduction by columns, for the many (G, membership) cases of one record set: every record's
# share is formed once (a Group of one), a group is then sums and extrema over its members' rows.
_MOM_FIELDS = 6   # count, min, max, sum, sq, overflow


def rows(reps):
    """One row per record: the 7 counts, then (count, min, max, sum, sq, overflow) of its 11 signals."""
    out = []
    for rec in reps:
        g = Group()
        g.add_rep(rec)
        row = list(g.head)
        for m in [g.queue, g.resp] + g.across:
            row += [m.count, m.mn, m.mx, m.sum, m.sq, m.overflow]
        out.append(row)
    return out


def reduce_rows(rws, group_of, G):
    """(bytes of the [G] records, n_ungrouped) from rows()."""
    members = [[] for _ in range(G)]
    lost = 0
    for r in range(len(rws)):
        g = 0 if group_of is None else int(group_of[r])
        if 0 <= g < G:
            members[g].append(rws[r])
        else:
            lost += 1
    empty = Group().pack()
    parts = []
    for mem in members:
        if not mem:
            parts.append(empty)
            continue
        cols = list(zip(*mem))
        b = struct.pack("<7q", *[signed(sum(cols[w]) & M64, 64) for w in range(7)])
        for k in range(2 + NMET):
            c = cols[7 + k * _MOM_FIELDS: 7 + (k + 1) * _MOM_FIELDS]
            s, q = sum(c[3]) & M128, sum(c[4]) & M192
            b += struct.pack("<qqqQQQQQq", signed(sum(c[0]) & M64, 64), min(c[1]), max(c[2]), s & M64, s >> 64,
                             q & M64, (q >> 64) & M64, q >> 128, signed(sum(c[5]) & M64, 64))
        parts.append(b)
    return b"".join(parts), lost


# ---------------------------------------------------------------- crafted records

def blank(n=1) -> np.ndarray:
    """n records of a replication that decided nothing (the header's empty-set values), status OK."""
    r = np.zeros(n, _abi.REP_STATS_DTYPE)
    r["queue_min_raw"] = r["resp_min_ticks"] = r["abort_tick"] = I64_MAX
    r["queue_max_raw"] = r["resp_max_ticks"] = r["last_tick"] = I64_MIN
    r["abort_task"] = -1
    return r


def _set128(rec, name, v):
    rec[name + "_lo"], rec[name + "_hi"] = v & M64, (v >> 64) & M64


def plain(rng, n) -> np.ndarray:
    """n consistent-looking OK records with random moments."""
    r = blank(n)
    for x in r:
        t = int(rng.integers(1, 5000))
        q = int(rng.integers(0, t + 1))
        x["n_tasks"], x["n_queued"], x["n_started"] = t, q, t - q
        x["events"] = t * 20
        x["last_tick"] = int(rng.integers(1, 2**50))
        x["n_qtime"] = q
        qs = int(rng.integers(-2**40, 2**62)) if q else 0
        _set128(x, "queue_sum", qs)
        _set128(x, "queue_sq", int(rng.integers(0, 2**63)) ** 2 if q else 0)
        x["queue_sq_top"] = int(rng.integers(0, 3)) if q else 0
        if q:
            x["queue_min_raw"], x["queue_max_raw"] = int(rng.integers(-5, 10)), int(rng.integers(10, 2**55))
        _set128(x, "resp_sum", int(rng.integers(0, 2**62)) * int(rng.integers(1, 8)))
        _set128(x, "resp_sq", int(rng.integers(0, 2**63)) * int(rng.integers(0, 2**63)))
        x["resp_min_ticks"], x["resp_max_ticks"] = int(rng.integers(0, 1000)), int(rng.integers(1000, 2**45))
        x["max_pending"] = int(rng.integers(0, 2000))
        x["busy_s"] = int(rng.integers(0, 10**6))
        x["energy_j"] = float(rng.uniform(0, 5e4))
        x["n_qtime_overflow"] = int(rng.integers(0, 2))
    return r


FAILED = (_abi.FOGNET_ERR_ARG, _abi.FOGNET_ERR_NO_NODES, _abi.FOGNET_ERR_DIV0, _abi.FOGNET_ERR_STATE,
          _abi.FOGNET_ERR_DEVICE, _abi.FOGNET_ERR_OOM, _abi.FOGNET_ERR_CAPACITY, _abi.FOGNET_ERR_UNSUPPORTED,
          _abi.FOGNET_ERR_INTERNAL)


def edge_cases() -> np.ndarray:
    """The issue's crafted records, each an otherwise plain OK record unless said."""
    rng = np.random.default_rng(0xED6E)
    out = []

    def case(**kw):
        x = plain(rng, 1)
        for k, v in kw.items():
            if k in ("queue_sum", "queue_sq", "resp_sum", "resp_sq"):
                _set128(x[0], k, v)
            else:
                x[k] = v
        out.append(x)

    case(n_qtime=2, queue_sum=-7 & M128)                       # negative with remainder: -7 / 2 -> -4
    case(n_qtime=2, queue_sum=-8 & M128)                       # negative, no remainder
    case(n_qtime=3, queue_sum=-(2**127) & M128)                # the most negative sum: quotient past int64
    case(n_qtime=1, queue_sum=-(2**127) & M128)
    case(n_qtime=2**62, queue_sum=-(2**127) & M128)            # ... and with a quotient that fits
    case(n_qtime=1, queue_sum=I64_MIN & M128)                  # the quotient is INT64_MIN itself
    case(n_qtime=1, queue_sum=(I64_MIN - 1) & M128)            # one past it
    case(n_qtime=1, queue_sum=I64_MAX)
    case(n_qtime=1, queue_sum=I64_MAX + 1)
    case(n_tasks=7, resp_sum=2**64 + 5)                        # resp_sum >= 2^64
    case(n_tasks=3, resp_sum=2**127 + 11)                      # ... with the top bit set: unsigned
    case(n_tasks=1, resp_sum=2**63)                            # a quotient past int64 (lost)
    case(n_tasks=2, resp_sum=2**64 - 2)                        # 2^63 - 1: the largest that fits
    case(n_tasks=1, n_queued=2**62)                            # queued share past int64
    case(n_tasks=3, n_queued=-5)                               # a negative count of an inconsistent record
    case(queue_min_raw=I64_MIN, queue_max_raw=I64_MAX, resp_min_ticks=I64_MIN, resp_max_ticks=I64_MAX,
         last_tick=I64_MAX, busy_s=I64_MIN)                    # extrema at +-2^63
    case(busy_s=I64_MAX, last_tick=I64_MIN + 1)
    case(queue_sq=M128, queue_sq_top=M64, resp_sq=M128)        # square sums that carry into the top limb
    case(queue_sq=M128, queue_sq_top=1, resp_sq=M128)
    case(n_tasks=0, n_qtime=0, last_tick=I64_MIN)              # nothing decided: most metrics undefined
    case(n_tasks=-3, n_qtime=-1)                               # negative divisors: undefined
    for e in (float("nan"), float("inf"), float("-inf"), -12.25, 9.3e12, -9.3e12, 9.2e12, 2.5e-6, 0.5e-6, -0.5e-6,
              1.0000005, 0.0, -0.0, 4503599627370497e-6):
        case(energy_j=e)
    for st in FAILED:
        case(status=st)
    case(status=REF_ABORTED, abort_tick=12345, abort_task=7)   # counted as aborted and as failed
    case(status=REF_ABORTED)                                   # (no abort point: failed only)
    case(status=OK, abort_tick=777, abort_task=1)              # the extension ran on: aborted and OK
    case(status=_abi.FOGNET_ERR_CAPACITY, abort_tick=5)        # failed otherwise: not counted as aborted
    return np.concatenate(out)


def crafted(R: int, seed: int = 1) -> np.ndarray:
    """R records: the edge cases cycled among plain ones, with failed and REF_ABORTED records at
    lanes 0 and 63 of wavefronts and on either side of a 256-record workgroup boundary."""
    rng = np.random.default_rng(seed)
    r = plain(rng, R)
    edges = edge_cases()
    if R:
        pos = rng.permutation(R)[: min(R, len(edges))]
        r[pos] = edges[: len(pos)]
    for i, st in ((0, _abi.FOGNET_ERR_CAPACITY), (63, REF_ABORTED), (64, REF_ABORTED), (127, _abi.FOGNET_ERR_DIV0),
                  (255, REF_ABORTED), (256, _abi.FOGNET_ERR_STATE), (R - 1, _abi.FOGNET_ERR_ARG)):
        if 0 <= i < R and R > 1:
            r[i]["status"] = st
            if st == REF_ABORTED:
                r[i]["abort_tick"] = 99 + i
    return r
