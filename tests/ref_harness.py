"""The reference harness seen from Python (test infrastructure).

``oracle/_ref/ref_v3`` (oracle/ref_shim/README.md) runs the reference's own
BrokerBaseApp3 / ComputeBrokerApp3 handlers under a stand-in kernel.  This
module feeds it traces in ``fognet_batch_in`` terms, reads back what it
recorded, and holds the one comparison of such a recording with the oracle
that tests/test_reference_pin.py applies to the committed fixtures and to
live runs alike.
"""
from __future__ import annotations

import json
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "ref_v3")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")  # as oracle/Makefile
I64_MAX = int(np.iinfo(np.int64).max)
CONNACK_TO_ADVERT = 10**10  # ComputeBrokerApp3.cc:265: scheduleAt(simTime() + 0.01)


def have_reference() -> bool:
    return os.path.exists(os.path.join(REFERENCE, "src", "mqttapp", "BrokerBaseApp3.cc"))


def have_binary() -> bool:
    return os.path.exists(BIN)


def node_starts(ul):
    """Node start ticks under which CONNECT k reaches the broker at max(ul) + k:
    in index order, whatever the uplinks."""
    ul = np.asarray(ul, np.int64)
    return int(ul.max()) + np.arange(ul.size, dtype=np.int64) - ul


def handshake_init(dl, ul):
    """Arrival tick of each node's first advert under node_starts(): CONNECT up,
    CONNACK down, 0.01 s, advert up.  The harness reports the ticks it saw; the
    fixture generator checks that they are these."""
    dl, ul = np.asarray(dl, np.int64), np.asarray(ul, np.int64)
    return int(ul.max()) + np.arange(ul.size, dtype=np.int64) + dl + CONNACK_TO_ADVERT + ul


def rebase(tr, r=0, grid=10**11):
    """Replication r of a tracegen / tie_heavy batch as the harness can run it:
    ``init`` becomes the handshake's and the arrivals move up by a whole number
    of ``grid`` ticks (every relative tick, and so every tie, is kept) until the
    first one is later than the last handshake advert."""
    def row(a):
        a = np.asarray(a)
        return a[r] if a.ndim == 2 else a
    mips, dl, ul = (row(tr[k]) for k in ("mips", "dl", "ul"))
    arrive, req = np.asarray(tr["arrive"])[r].astype(np.int64), np.asarray(tr["req"])[r].astype(np.int32)
    init = handshake_init(dl, ul)
    if arrive.size:
        short = int(init.max()) + 1 - int(arrive[0])
        if short > 0:
            arrive = arrive + -(-short // grid) * grid
    return dict(arrive=arrive, req=req, mips=mips.astype(np.int32), dl=dl.astype(np.int64), ul=ul.astype(np.int64),
                init=init)


def per_task(x, T):
    x = np.asarray(x, np.int64)
    return np.broadcast_to(x, (T,)) if x.ndim == 0 or x.size == 1 else x


def _replay_text(tr, uu, ud):
    N, T = len(tr["mips"]), len(tr["arrive"])
    st = node_starts(tr["ul"])
    uu, ud = per_task(uu, T), per_task(ud, T)
    lines = [f"replay {N} {T}"]
    lines += [f"{int(tr['mips'][j])} {int(tr['dl'][j])} {int(tr['ul'][j])} {int(st[j])}" for j in range(N)]
    lines += [f"{int(tr['arrive'][t])} {int(tr['req'][t])} {int(uu[t])} {int(ud[t])}" for t in range(T)]
    return "\n".join(lines) + "\n"


def _run(text):
    p = subprocess.run([BIN], input=text, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"ref_v3 exit {p.returncode}: {p.stderr.strip()}")
    return [json.loads(line) for line in p.stdout.splitlines()]


def run_replays(jobs):
    """jobs: [(trace, user_ul, user_dl)], one replication each (1-D arrays;
    user links scalar or [T]).  Returns the harness's records, in order."""
    return _run("".join(_replay_text(*j) for j in jobs)) if jobs else []


def bits(x) -> str:
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def run_decides(views):
    """views: [(busy doubles, mips ints, req)].  Returns the chosen node of each."""
    text = []
    for busy, mips, req in views:
        text.append(f"decide {len(busy)} {int(req)}\n")
        text.append("".join(f"{int(m)} {bits(b)}\n" for b, m in zip(busy, mips)))
    return [r["node"] for r in _run("".join(text))] if views else []


# ------------------------------------------------------------------ the comparison

def _moments(values):
    """count / min / max / sum / sum of squares of a list of Python ints."""
    return dict(count=len(values), min=min(values) if values else I64_MAX,
                max=max(values) if values else -I64_MAX - 1, sum=sum(values), sq=sum(v * v for v in values))


def _limbs_signed(lo, hi):
    s = int(lo) | (int(hi) << 64)
    return s - (1 << 128) if s >> 127 else s


def queue_moments_of(st):
    """The queueTime moments of a fognet_rep_stats / orc_rep_stats record as Python ints."""
    return dict(count=int(st["n_qtime"]), min=int(st["queue_min_raw"]), max=int(st["queue_max_raw"]),
                sum=_limbs_signed(st["queue_sum_lo"], st["queue_sum_hi"]),
                sq=int(st["queue_sq_lo"]) | (int(st["queue_sq_hi"]) << 64) | (int(st["queue_sq_top"]) << 128))


def user_moments_of(m):
    """One signal of a fognet_user_stats / orc_user_stats record as Python ints."""
    return dict(count=int(m["count"]), min=int(m["min_raw"]), max=int(m["max_raw"]),
                sum=_limbs_signed(m["sum_lo"], m["sum_hi"]),
                sq=int(m["sq_lo"]) | (int(m["sq_hi"]) << 64) | (int(m["sq_top"]) << 128), overflow=int(m["overflow"]))


def expected_user(tr, uu, ud, rec, ms_raw):
    """The four user signals from what the harness recorded: the broker's delay
    emissions as they are, and (ack arrival - creation) * 1000 through ``ms_raw``
    (the written SimTime rule) for every ack that reached the user."""
    T = len(tr["arrive"])
    uu = per_task(uu, T)
    by = {"latency": [], "latencyH1": [], "taskTime": []}
    lost = {"latency": 0, "latencyH1": 0, "taskTime": 0}
    for task, status, tick in rec["user_acks"]:
        name = {5: "latency", 4: "latencyH1", 6: "taskTime"}[status]
        raw = ms_raw(tick - (int(tr["arrive"][task]) - int(uu[task])))
        if raw is None:
            lost[name] += 1
        else:
            by[name].append(raw)
    out = {n: dict(_moments(v), overflow=lost[n]) for n, v in by.items()}
    out["delay"] = dict(_moments([int(v) for v in rec["delay"]]), overflow=0)
    return out


def compare_with_oracle(tr, uu, ud, rec, ol):
    """Every value a reference run defines against oracle_lib's stop-at-abort
    replay of the same trace.  Returns how many values were compared."""
    T, N = len(tr["arrive"]), len(tr["mips"])
    o = ol.run_batch(tr["arrive"][None], tr["req"][None], tr["mips"], tr["dl"], tr["ul"], tr["init"],
                     stop_at_ref_abort=True, user_ul=np.ascontiguousarray(per_task(uu, T))[None],
                     user_dl=np.ascontiguousarray(per_task(ud, T))[None])
    st = o["stats"][0]
    n = 0
    assert st["status"] == 0
    assert rec["connect_order"] == list(range(N)) and rec["init_adv_tick"] == [int(x) for x in tr["init"]]
    assert rec["last_handshake_adv"] < int(tr["arrive"][0]) if T else True
    n += 2 * N
    for k in ("node", "status", "start", "done"):  # all T tasks; what an aborted run never reached is -1 / 0 in both
        np.testing.assert_array_equal(o[k][0].astype(np.int64), np.array(rec[k], np.int64), err_msg=k)
        n += T
    ab = rec["abort"]
    if ab is None:
        assert (np.array(rec["done"]) >= 0).all(), "a run without abort completes every task"
    # each emission: the node, the task it starts, the tick and the value, one by one ...
    for raw, tick, node, task in rec["qtime"]:
        assert rec["status"][task] == 4 and rec["node"][task] == node and rec["start"][task] == tick
        assert ol.qtime_raw(tick, int(tr["arrive"][task]) + int(tr["dl"][node])) == raw
        n += 4
    # ... and the record's moments from Python integers over the recorded emissions
    want = _moments([e[0] for e in rec["qtime"]])
    assert queue_moments_of(st) == want, (queue_moments_of(st), want)
    assert int(st["n_qtime_overflow"]) == (0 if ab is None else 1)
    assert int(st["abort_tick"]) == (I64_MAX if ab is None else ab["tick"])
    # stopped where the reference stops, the oracle names the task the reference threw at
    assert int(st["abort_task"]) == (-1 if ab is None else ab["task"])
    if ab is not None:
        assert "SimTime" in ab["what"] and rec["node"][ab["task"]] == ab["node"]
    assert int(st["n_tasks"]) == sum(1 for x in rec["node"] if x >= 0)
    assert int(st["n_queued"]) == rec["status"].count(4) and int(st["n_started"]) == rec["status"].count(5)
    n += 5 + 3 + 3
    want_user = expected_user(tr, uu, ud, rec, ol.ms_raw)
    for name in ol.USER_SIGNALS:
        got = user_moments_of(o["user"][0][name])
        assert got == want_user[name], (name, got, want_user[name])
        n += 6
    return n


def values_compared(T, N, n_emissions):
    """What compare_with_oracle returns for a trace of that shape."""
    return 2 * N + 4 * T + 4 * n_emissions + 11 + 24
