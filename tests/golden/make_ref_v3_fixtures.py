"""Generates tests/golden/ref_v3_*.json: what the reference's own v3 handlers do.

Each replay case is a trace in ``fognet_batch_in`` terms (arrive, req, mips, dl,
ul, init, and the publishing users' links user_ul / user_dl) together with what
``oracle/_ref/ref_v3`` recorded when it ran BrokerBaseApp3 and
ComputeBrokerApp3, compiled in place, over that trace (oracle/ref_shim/README.md):

  connect_order, init_adv_tick, last_handshake_adv   the registration handshake
  node / status / start / done   per task: the node the FognetMsgTask went to, the
          node's ack (5 assigned, 4 queued), the tick its service started and its
          RELEASERESOURCE tick; -1 (status 0) where an aborted run never got there
  qtime   every queueTime emission: [raw int64, tick, node, task it starts]
  user_acks   every ack that reached the user: [task, status, tick]
  delay   the broker's delay emissions (raw)
  abort   null, or the cRuntimeError that left handleMessage: tick, node, the
          task the node was about to start, the message

``init`` is what the harness reported, not an input: the nodes go through the
reference's own start -> CONNECT -> CONNACK -> first ADVERTISEMIPS path.

What the recordings pin is the handlers' logic.  SimTime arithmetic, the fixed
link latencies and the order of two deliveries at one tick are the project's
written model, restated in the stand-in kernel.  The
``past_2p53`` cases lie wholly inside that part: the queueStartTime round trip
above 2^53 ticks is computed by two restatements of one written rule (oracle
and stand-in), so they check consistency and are NOT a reference pin.

Needs the harness binary (make -C oracle ref).  Deterministic: running it again
reproduces the committed bytes, which tests/test_reference_pin.py asserts.

Run: python tests/golden/make_ref_v3_fixtures.py
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))

import ref_harness as rh  # noqa: E402
import tracegen as tg  # noqa: E402

MS = 10**9
TPS = 10**12
MAX_BYTES = 64 * 1024


def tie_heavy(seed, R, N, T):
    from test_parity_gpu import tie_heavy as th  # the suite's generator (imports the engine package)
    return th(seed, R, N, T)


def small(name, mips, dl, ul, arrive_after, req, uu, ud, note=None):
    """A hand-made trace: ``arrive_after`` are ticks after the first whole second past the handshake."""
    mips, dl, ul = np.array(mips, np.int32), np.array(dl, np.int64), np.array(ul, np.int64)
    init = rh.handshake_init(dl, ul)
    t0 = -(-(int(init.max()) + 1) // TPS) * TPS
    tr = dict(arrive=t0 + np.array(arrive_after, np.int64), req=np.array(req, np.int32), mips=mips, dl=dl, ul=ul,
              init=init)
    return name, tr, uu, ud, note


def replay_groups():
    rng = np.random.default_rng(0x5EED0007)
    g = {}
    # arrivals, completions and adverts on shared ticks; dl on both sides of S * 1e12; zero-service tasks
    for seed, N in ((0, 1), (1, 3), (2, 5)):
        tr = rh.rebase(tie_heavy(seed, 1, N, 200))
        T = 200
        # user links on the same coarse grid, so acks collide with everything else too
        uu = rng.integers(0, 3, T) * 10**11
        ud = rng.integers(0, 3, T) * 10**11
        g[f"tie_n{N}"] = [(f"tie_heavy_n{N}", tr, uu, ud, None)]
    # herding: heterogeneous MIPS, req around mips_0 (the estimate uses node 0's MIPS only)
    for N, T in ((5, 200), (64, 200)):
        mips, dl, ul, _ = tg.gen_nodes(0x5EED0011, N, N, 1)
        req = rng.integers(500, 2501, T).astype(np.int32)
        gaps = (rng.exponential(0.9 / N, T) * TPS).astype(np.int64)
        tr = rh.rebase(dict(arrive=np.cumsum(gaps)[None], req=req[None], mips=mips, dl=dl, ul=ul))
        g[f"herd_n{N}"] = [(f"herding_n{N}", tr, 3 * MS, 2 * MS, None)]
    # More than one wavefront lane per node set.  Every view starts at 0 and ties go to the lowest
    # index, so a node above 63 is chosen only while every node below it shows a backlog: publishes
    # come in pairs, a 1-s task a node starts at once and a long one that queues behind it, so each
    # node's first completion advertises the long task and moves the broker on by one node, up to
    # node 99; after that the decisions are minima over 100 different positive views.
    N, T = 100, 300
    _, dl, ul, _ = tg.gen_nodes(0x5EED0012, 0, N, 1)
    req = np.where(np.arange(T) % 2 == 0, rng.integers(1000, 2000, T), rng.integers(170_000, 400_000, T))
    gaps = (rng.uniform(0.6, 0.9, T) * TPS).astype(np.int64)
    tr = rh.rebase(dict(arrive=np.cumsum(gaps)[None], req=req[None], mips=np.full(N, 1000, np.int32), dl=dl, ul=ul))
    g["many_n100"] = [("many_nodes_n100", tr, 4 * MS + 1, 3 * MS + 7, None)]  # one user: the file stays under 64 KB

    e = []
    # req = 0 (zero service at every node), and N = 1: the loop at BrokerBaseApp3.cc:271 is skipped
    e.append(small("req_zero", [1000, 500, 2000], [MS, 0, 2 * MS], [MS, MS, 0],
                   [0, 0, 1, MS, MS, 2 * MS, 2 * MS + 1], [0, 0, 0, 1500, 0, 0, 999], 5, 7))
    e.append(small("one_node", [1000], [MS], [MS], [0, 1, 2, TPS, TPS + MS, 3 * TPS, 9 * TPS],
                   [3000, 0, 1000, 999, 2000, 1000, 0], 4 * MS, 3 * MS))
    # queueTime overflow: mips = 1, services of thousands of seconds.  The wait of task 2
    # (9223 s + 1 s - 2 ticks) leaves int64 when multiplied by 1000: the run ends at that emit.
    e.append(small("overflow_one_node", [1, 1], [MS, MS], [MS, MS], [0, 1, 2, 3, 5000 * TPS],
                   [9223, 1, 1, 1, 1], 2 * MS, 2 * MS))
    # Two nodes overflow at the SAME tick with different task indices.
    #  low_first: node 0 serves task 0 (1 s), then task 1 (9300 s) from d0 = a0 + 1 s; task 2 queues
    #  behind it.  Node 0's completion advert (busy 9301) sends task 3 (9299 s, published 2 s after
    #  task 0) and task 4 to node 1.  Both long services end at a0 + 9301 s; node 0's timer was set
    #  first (at d0 < a3), so its emission -- for task 2, the lowest index -- throws first.
    e.append(small("overflow_same_tick_low_first", [1, 1], [MS, MS], [MS, MS], [0, 1, 2, 2 * TPS, 2 * TPS + 1],
                   [1, 9300, 1, 9299, 1], 2 * MS, 2 * MS))
    #  high_first: node 0 serves 1 s, then 100 s, then task 2 (9300 s) from a0 + 101 s with task 3
    #  queued behind; node 1 gets task 4 (9399 s) at a0 + 2 s with task 5 behind.  Both end at
    #  a0 + 9401 s; node 1's timer was set first (a0 + 2 s < a0 + 101 s), so the emission for
    #  task 5 throws first although task 3 overflows at the same tick.
    e.append(small("overflow_same_tick_high_first", [1, 1], [MS, MS], [MS, MS],
                   [0, 1, 2, 3, 2 * TPS, 2 * TPS + 1], [1, 100, 9300, 1, 9399, 1], 2 * MS, 2 * MS))
    g["edges"] = e

    # Above 2^53 ticks queueStartTime = simTime().dbl() no longer round-trips.  Consistency
    # of two restatements of the written SimTime rule -- not a reference pin (see above).
    note = "consistency of the written SimTime rule; not a reference pin"
    p = []
    for name, base in (("past_2p53_round_trip", 2**54), ("past_2p60_round_trip", 2**60 + 1000)):
        t0 = base + 5 - MS
        p.append((name, dict(arrive=np.array([t0, t0 + 1], np.int64), req=np.array([3000, 1000], np.int32),
                             mips=np.array([1000], np.int32), dl=np.array([MS], np.int64), ul=np.array([MS], np.int64),
                             init=rh.handshake_init([MS], [MS])), MS, MS, note))
    a = 2**54 + 3 - MS
    p.append(("past_2p53_same_tick", dict(arrive=np.array([a, a], np.int64), req=np.array([500, 2000], np.int32),
                                          mips=np.array([1000], np.int32), dl=np.array([MS], np.int64),
                                          ul=np.array([MS], np.int64), init=rh.handshake_init([MS], [MS])), MS, MS,
              note))
    g["past_2p53"] = p
    return g


def enc(x):
    """A double as kat_decide.json holds it: a JSON number, or a string where JSON has none."""
    x = float(x)
    if math.isnan(x):
        return "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return x


def decide_views():
    rng = np.random.default_rng(0x5EED0008)
    big = 2**31 - 1
    special = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, -1.5, -1e300, 5e-324, -5e-324, 2.2250738585072014e-308,
               1e300, 1e16, 1e16 + 2, 1.0, 1.0 + 2.0**-52, 3.0, 4.0, 0.5, 9007199254740992.0, 9007199254740994.0]
    views = []
    # the rounding tie: 1e16 + 1 is no double, so 1e16 + req/mips_0 = 1e16 + 1 rounds to even
    # and two views that differ by 2 meet after the addition
    for busy, mips, req in (([1e16 + 2, 1e16], [1000, 1000], 1000), ([1e16, 1e16 + 2], [1000, 1000], 1000),
                            ([1e16 + 2, 1e16, 1e16], [1000, 1, 1], 3000), ([1e16, 1e16 + 2], [1000, 7], 0),
                            ([1e16 + 2, 1e16 + 4, 1e16], [1, 1, 1], 1), ([1e16 + 4, 1e16 + 2], [1, 1], 3),
                            ([9007199254740992.0, 9007199254740994.0, 9007199254740992.0], [1000, 1, 1], 1000),
                            ([float("nan"), 1.0], [1000, 1000], 1000), ([1.0, float("nan"), 0.5], [1000, 1000, 1000], 0),
                            ([float("inf"), float("inf")], [1, 1], 5), ([float("inf"), 1e300, float("-inf")], [1, 1, 1], 5),
                            ([0.0, -0.0], [1000, 1000], 999), ([-0.0, 0.0, -5e-324], [1000, 1000, 1000], 999),
                            ([5e-324, 0.0], [big, 1], big), ([3.0, 2.0, 2.0], [big, 1, 1], big),
                            ([3.0, 2.0], [1, 1], -5000), ([1.0, 5001.0], [1, 1], -5000), ([7.0], [1], -1)):
        views.append((busy, mips, req))
    while len(views) < 200:
        n = int(rng.choice([1, 2, 2, 3, 3, 4, 5, 6, 7, 8]))
        kind = rng.integers(0, 3)
        if kind == 0:   # small integer views with many ties, as the replay sees them
            busy = rng.integers(0, 4, n).astype(np.float64)
        elif kind == 1:  # the special values
            busy = rng.choice(special, n)
        else:
            busy = np.where(rng.random(n) < 0.5, rng.choice(special, n), rng.integers(-3, 6, n) + rng.choice([0, 0.5, 1e-16], n))
        mips = rng.choice([1, 7, 500, 1000, 3000, big], n)
        req = int(rng.choice([-5000, -1, 0, 1, 999, 1000, 3000, 64000, big]))
        views.append(([float(b) for b in busy], [int(m) for m in mips], req))
    for n in (64, 65, 257, 64, 65, 257):  # past one wavefront, and past the kernel-argument view
        busy = rng.integers(2, 5, n).astype(np.float64)
        busy[rng.integers(0, n, 3)] = rng.choice(special, 3)
        lo = int(rng.integers(n - 3, n))
        busy[lo] = 1.0  # a late strict minimum ...
        if n != 64:
            busy[n - 1] = 1.0  # ... and its tie on the last slot
        mips = rng.choice([1, 1000, big], n)
        mips[0] = 1000
        views.append(([float(b) for b in busy], [int(m) for m in mips], int(rng.choice([0, 3000, -1]))))
    return views


def dump(about, cases):
    body = ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases)
    return '{"_about":%s,\n"cases":[\n%s\n]}\n' % (json.dumps(about), body)


def generate():
    """{file name: text} of every fixture."""
    out = {}
    about = ("Recorded from the reference's own BrokerBaseApp3 / ComputeBrokerApp3 handlers by oracle/_ref/ref_v3; "
             "see tests/golden/make_ref_v3_fixtures.py for the fields.")
    for group, cases in replay_groups().items():
        recs = rh.run_replays([(tr, uu, ud) for _, tr, uu, ud, _ in cases])
        js = []
        for (name, tr, uu, ud, note), rec in zip(cases, recs):
            N = len(tr["mips"])
            assert rec["connect_order"] == list(range(N)), name
            assert rec["init_adv_tick"] == [int(x) for x in tr["init"]], name  # the handshake's, as predicted
            c = dict(name=name)
            if note:
                c["note"] = note
            for k in ("arrive", "req", "mips", "dl", "ul"):
                c[k] = [int(x) for x in tr[k]]
            c["init"] = rec["init_adv_tick"]
            c["user_ul"] = [int(x) for x in np.atleast_1d(uu)]
            c["user_dl"] = [int(x) for x in np.atleast_1d(ud)]
            c["ref"] = rec
            js.append(c)
        out[f"ref_v3_{group}.json"] = dump(about, js)
    views = decide_views()
    nodes = rh.run_decides(views)
    out["ref_v3_decide.json"] = dump(
        "Decisions of the reference's own BrokerBaseApp3::sendPubAck(status=false) on arbitrary advertised views, "
        "recorded by oracle/_ref/ref_v3 (decide mode).  Non-finite busy values are strings, as in kat_decide.json.",
        [dict(name=f"v{i:03d}_n{len(b)}", busy=[enc(x) for x in b], mips=m, req=r, node=k)
         for i, ((b, m, r), k) in enumerate(zip(views, nodes))])
    for name, text in out.items():
        assert len(text.encode()) <= MAX_BYTES, (name, len(text))
    return out


def main():
    for name, text in generate().items():
        with open(os.path.join(HERE, name), "w") as f:
            f.write(text)
        print(f"{name}: {len(text)} bytes")


if __name__ == "__main__":
    main()
