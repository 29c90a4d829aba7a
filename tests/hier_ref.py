"""EXT_HIER escalation flags and the statistics that need them, rebuilt from the
ORACLE's per-task outputs (test infrastructure for test_hier_flags*.py; no GPU needed).

The oracle does not say which tasks the parent broker decided.  expected_flags
rebuilds each publish's broker view from the oracle's own node / start / done
(fognet_hip.h FOGNET_POLICY_EXT_HIER), asks the oracle's decision
function for it and checks that it names the oracle's node, so the `escalated`
result it returns is the decision the oracle's run took.  With those flags the
closed forms of user_stats_ref / node_stats_ref, the hop hier_up_tick added to an
escalated task's arrival at its node, are compared with the oracle's event-level
records by the tests.
"""
from __future__ import annotations

import bisect

import numpy as np

import node_stats_ref as ns
import oracle_lib as ol
import user_stats_ref as us

MS, TPS = 10**9, 10**12
REGION_NODES = 1024  # FOGNET_HIER_REGION_NODES


def _row(a, r):
    a = np.asarray(a)
    return a[r] if a.ndim == 2 else a


def _flags_rep(t, req, region, mips, dl, ul, node, status, start, done, thr, up):
    T, N = len(t), len(mips)
    S = [int(req[i]) // int(mips[int(node[i])]) for i in range(T)]  # service seconds (int division)
    flags = np.zeros(T, np.uint8)
    chains: dict[int, list] = {}  # node -> its tasks in arrival order: (arrival tick, task)
    busy = np.zeros(N, np.float64)
    for i in range(T):
        ti = int(t[i])
        for k, ch in chains.items():
            # 1. the last completion whose advert reached the broker strictly before the publish
            pos = -1
            for p, (_, j) in enumerate(ch):
                if int(done[j]) + int(ul[k]) < ti:
                    pos = p
                else:
                    break  # (FIFO: completions in arrival order)
            if pos < 0:
                continue  # still the first advert: busy 0
            j = ch[pos][1]
            dj, sj = int(done[j]), S[j] * TPS
            # 2. it advertised the service of the later tasks that had arrived by then; an arrival
            #    at the completion's own tick comes first iff its event was inserted no later
            #    (DESIGN.md §3.3): its downlink, hop included, is at least the completing service
            b = 0
            for a2, i2 in ch[pos + 1:]:
                if a2 < dj or (a2 == dj and int(dl[k]) + up * int(flags[i2]) >= sj):
                    b += S[i2]
            busy[k] = b
        # 3. the oracle's decision on that view names the oracle's node
        rc, k, e = ol.decide_hier(busy, mips, int(region[i]), thr, int(req[i]))
        assert rc == 0 and k == int(node[i]), (i, rc, k, int(node[i]), e)
        # 4. and the task reaches it the hop later iff the parent decided
        a = ti + int(dl[k]) + up * e
        if int(status[i]) == 5:
            assert int(start[i]) == a, (i, e, int(start[i]), a)
        else:
            assert int(status[i]) == 4 and int(start[i]) >= a, (i, e, int(status[i]), int(start[i]), a)
        flags[i] = e
        bisect.insort(chains.setdefault(k, []), (a, i))
    return flags


def expected_flags(tr: dict, o: dict, region, thr: int, up: int) -> np.ndarray:
    """[R, T] uint8: 1 where the parent broker took the decision of the oracle's run ``o``
    (oracle_lib.run_batch under EXT_HIER with threshold ``thr`` s and hop ``up`` ticks;
    replications without a crash, status OK)."""
    arrive, req, region = np.atleast_2d(tr["arrive"]), np.atleast_2d(tr["req"]), np.atleast_2d(region)
    out = np.zeros(arrive.shape, np.uint8)
    for r in range(arrive.shape[0]):
        assert int(o["stats"]["status"][r]) == 0
        out[r] = _flags_rep(arrive[r], req[r], region[r], _row(tr["mips"], r), _row(tr["dl"], r), _row(tr["ul"], r),
                            o["node"][r], o["status"][r], o["start"][r], o["done"][r], int(thr), int(up))
    return out


def user_expected(tr: dict, o: dict, user_ul, user_dl, flags, up: int, statuses=None) -> np.ndarray:
    """user_stats_ref.expected with the node ack of task i leaving at t + dl_k + up * flags[i]
    (only that term moves: delay, the broker's own pubAck and taskTime do not)."""
    arrive = np.atleast_2d(tr["arrive"])
    R = arrive.shape[0]
    out = np.zeros(R, us.USER_STATS_DTYPE)
    for r in range(R):
        status = int(o["stats"]["status"][r]) if statuses is None else int(statuses[r])
        m = {s: us.Mom() for s in us.SIGNALS}
        if status in us.OK_STATUSES:
            dl, ul = _row(tr["dl"], r), _row(tr["ul"], r)
            per_task = np.ndim(user_ul[r]) == 1
            for i in range(int(o["stats"]["n_tasks"][r])):
                t, k, st, dn = int(arrive[r, i]), int(o["node"][r, i]), int(o["status"][r, i]), int(o["done"][r, i])
                uu, ud = (int(user_ul[r][i]), int(user_dl[r][i])) if per_task else (int(user_ul[r]), int(user_dl[r]))
                created = t - uu
                m["delay"].add(uu)
                m["latencyH1"].add_ms(t + ud - created)
                at_user = t + int(dl[k]) + up * int(flags[r, i]) + int(ul[k]) + ud
                if st == 5:
                    m["latency"].add_ms(at_user - created)
                elif st == 4:
                    m["latencyH1"].add_ms(at_user - created)
                if dn >= 0:
                    m["taskTime"].add_ms(dn + int(ul[k]) + ud - created)
        out[r] = us.to_record(m)
    return out


def node_expected(tr: dict, o: dict, flags, up: int, statuses=None) -> np.ndarray:
    """node_stats_ref.expected with task i enqueued at t + dl_k + up * flags[i]."""
    arrive, req = np.atleast_2d(tr["arrive"]), np.atleast_2d(tr["req"])
    R, N = arrive.shape[0], np.shape(tr["mips"])[-1]
    out = np.zeros((R, N), ns.NODE)
    for r in range(R):
        mips, dl = _row(tr["mips"], r), _row(tr["dl"], r)
        nodes = [ns.Node() for _ in range(N)]
        status = int(o["stats"]["status"][r]) if statuses is None else int(statuses[r])
        if status in ns.OK_STATUSES:
            for i in range(int(o["stats"]["n_tasks"][r])):
                k, st = int(o["node"][r, i]), int(o["status"][r, i])
                t, start, done = int(arrive[r, i]), int(o["start"][r, i]), int(o["done"][r, i])
                nd = nodes[k]
                nd.tasks += 1
                nd.queued += st == 4
                nd.started += st == 5
                nd.lost += st == 9
                if done >= 0:
                    nd.busy += int(req[r, i]) // int(mips[k])
                    nd.last = max(nd.last, done)
                    nd.resp.add(done - t)
                if st == 4 and start >= 0:
                    raw = ol.qtime_raw(start, t + int(dl[k]) + up * int(flags[r, i]))
                    if raw is None:
                        nd.queue.ovf += 1
                    else:
                        nd.queue.add(raw)
        out[r] = ns.to_records(nodes)
    return out


# ---------------------------------------------------------------- the traces

def make_trace(seed: int, R: int, N: int, T: int, gap: int, region_of):
    """arrive = 100 ms + cumsum of odd gaps in [gap / 2, 3 gap / 2); req in [1000, 5000);
    every node 1000 MIPS; dl, ul = 1-8 ms + an even sub-µs offset; first adverts at 50 ms;
    per-task user links of 1-50 ms + a sub-µs offset.  ``region_of(rng, shape)`` draws the
    regions.  Returns (trace, user_ul, user_dl)."""
    rng = np.random.default_rng(seed)
    arrive = 100 * MS + np.cumsum(rng.integers(gap // 2, 3 * gap // 2, (R, T)) | 1, axis=1)
    req = rng.integers(1000, 5000, (R, T)).astype(np.int32)
    dl = rng.integers(1, 9, N) * MS + 2 * rng.integers(0, 500, N)
    ul = rng.integers(1, 9, N) * MS + 2 * rng.integers(0, 500, N)
    region = np.asarray(region_of(rng, (R, T)), np.int32)
    uu = rng.integers(1, 51, (R, T)) * MS + rng.integers(0, 10**6, (R, T))
    ud = rng.integers(1, 51, (R, T)) * MS + rng.integers(0, 10**6, (R, T))
    tr = dict(arrive=arrive.astype(np.int64), req=req, mips=np.full(N, 1000, np.int32), dl=dl.astype(np.int64),
              ul=ul.astype(np.int64), init=np.full(N, 50 * MS, np.int64), region=region)
    return tr, uu.astype(np.int64), ud.astype(np.int64)


# name -> (seed, N, T, gap, regions, threshold s, hop ticks)
CASES = {
    "B": (5, 1030, 400, 200 * MS, lambda g, s: (g.random(s) < 0.7).astype(np.int32), 0, 3 * TPS),
    "B2": (5, 1030, 400, 200 * MS, lambda g, s: (g.random(s) < 0.7).astype(np.int32), 2, 20 * MS),
    "C": (6, 2052, 300, 150 * MS, lambda g, s: np.array([0, 1, 2, 2], np.int32)[g.integers(0, 4, s)], 1, 5 * TPS),
    "D": (7, 5, 300, 300 * MS, lambda g, s: np.zeros(s, np.int32), 1, 2 * TPS),
}
_cache: dict = {}


def run_oracle(tr, uu, ud, thr, up, **kw):
    return ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=4, user_ul=uu,
                        user_dl=ud, policy=ol.POLICY_EXT_HIER, region=tr["region"], hier_threshold_s=thr,
                        hier_up_tick=up, down=tr.get("down"), **kw)


def case(name: str):
    """(trace, user_ul, user_dl, oracle result, flags, threshold, hop) of CASES[name], computed
    once and left unchanged: two replications of the recipe and, for B and C, a third whose
    publishes are all region 0's, which never escalates (1,024 mostly idle nodes)."""
    if name not in _cache:
        seed, N, T, gap, region_of, thr, up = CASES[name]
        quiet = N > REGION_NODES
        tr, uu, ud = make_trace(seed, 3 if quiet else 2, N, T, gap, region_of)
        if quiet:
            tr["region"][2] = 0
        o = run_oracle(tr, uu, ud, thr, up)
        _cache[name] = (tr, uu, ud, o, expected_flags(tr, o, tr["region"], thr, up), thr, up)
    return _cache[name]
