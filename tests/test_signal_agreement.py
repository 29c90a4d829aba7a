"""The vectors are the rows the records count (no GPU): for every replication, the values of
every signal vector against the fognet_moments record of the same signal -- the rows' count,
minimum, maximum, sum (128-bit two's complement) and sum of squares (192 bits) equal the
record's count, min_raw, max_raw, (sum_lo, sum_hi) and (sq_lo, sq_hi, sq_top):

  node vector k        node_stats[r][k].queue
  latency vector u     per_user[r][u].latency      (latencyH1, taskTime likewise)
  delay vector         the exact merge over u of per_user[r][u].delay

A record's overflow count has no rows; a failed replication's all-zero offsets stand against
empty records.  Here the three independent restatements are held to it on the oracle's
outputs; test_signal_agreement_gpu.py holds the device's three passes to it on one replay."""
import pytest

import node_stats_ref as ns
import per_user_ref as pu
import signal_vectors_ref as sv
import user_stats_ref as us
from test_per_user_stats import carry_case, draw_links, draw_users, replay_oracle, trace_case
from test_signal_vectors import herded_case

M64 = (1 << 64) - 1
SHAPES = [(1, 1), (5, 3), (300, 129)]  # (N, U); N = 300: wide-kernel rows, and both layouts of the record passes
TS = [1, 63, 65, 129]  # one lane, the chunk edge either side of 64, three chunks
KINDS = ("queueTime", "delay", "latency", "latencyH1", "taskTime")


def moments_of(values) -> dict:
    """The fognet_moments fields that rows can state, from their values in Python ints."""
    vals = [int(v) for v in values]
    s, q = sum(vals) % (1 << 128), sum(v * v for v in vals)
    assert q < 1 << 192
    return dict(count=len(vals), min_raw=min(vals, default=us.I64_MAX), max_raw=max(vals, default=us.I64_MIN),
                sum_lo=s & M64, sum_hi=s >> 64, sq_lo=q & M64, sq_hi=(q >> 64) & M64, sq_top=q >> 128)


def assert_vectors_are_the_records(vec: dict, nodes, users, what="") -> dict:
    """``vec``: offset [R, V + 1] and value [R, cap] of signal vectors; ``nodes`` [R, N]
    fognet_node_stats and ``users`` [R, U] fognet_user_stats records of the same replications.
    Returns the rows per kind and the emissions the records count as lost, per side."""
    R, N, U = nodes.shape[0], nodes.shape[1], users.shape[1]
    assert vec["offset"].shape == (R, sv.n_vectors(N, U) + 1) and users.shape[0] == R and U > 0
    n = dict.fromkeys(KINDS + ("lost queueTime", "lost user-side"), 0)
    for r in range(R):
        off = vec["offset"][r]
        assert off[0] == 0

        def check(v, rec, kind):
            got = moments_of(vec["value"][r][off[v]:off[v + 1]])
            for f, x in got.items():
                assert int(rec[f]) == x, (what, r, kind, v, f, int(rec[f]), x)
            n[kind] += got["count"]
            n["lost queueTime" if kind == "queueTime" else "lost user-side"] += int(rec["overflow"])
        for k in range(N):
            check(k, nodes[r, k]["queue"], "queueTime")
        check(N, pu.merged(users[r])["delay"], "delay")
        for s, sig in enumerate(KINDS[2:]):
            for u in range(U):
                check(N + 1 + s * U + u, users[r, u][sig], sig)
    return n


def relayed_h1_rows(rows, N, U) -> int:
    """latencyH1 rows of the restatement's row lists that are a node's "task queued" ack."""
    return sum(1 for vec in rows for v in range(N + 1 + U, N + 1 + 2 * U) for row in vec[v] if row[4] == sv.FIRST)


def check_restatements(tr, o, who, uu, ud, what="", statuses=None) -> dict:
    """signal_vectors_ref against per_user_ref and node_stats_ref on the oracle's outputs."""
    want = sv.expected(tr, o, who, uu, ud, statuses=statuses, with_rows=True)
    users, un = pu.expected(tr, o, who, uu, ud, statuses=statuses)
    assert (un == 0).all()
    nodes = ns.expected(tr, o)
    if statuses is not None:  # (node_stats_ref goes by the oracle's statuses)
        for r, st in enumerate(statuses):
            if st not in us.OK_STATUSES:
                nodes[r] = ns.empty_records(nodes.shape[1])
    n = assert_vectors_are_the_records(want, nodes, users, what)
    n["relayed"] = relayed_h1_rows(want["rows"], nodes.shape[1], users.shape[1])
    n["pubAck"] = n["latencyH1"] - n["relayed"]
    return n


def total(counts) -> dict:
    return {k: sum(c[k] for c in counts) for k in counts[0]}


def assert_every_kind(n: dict, what=""):
    for k in ("queueTime", "latency", "pubAck", "relayed", "taskTime"):
        assert n[k] > 0, (what, k, n)


def trace_users(N, U, T):
    """The users and links test_signal_agreement_gpu.py gives trace_case(N, T)."""
    return draw_users(1000 * U + T, 3, T, U, "rr"), *draw_links(1000 * U + T + 1, 3, U, True)


@pytest.mark.parametrize("N,U", SHAPES)
def test_restatements_agree_on_oracle_runs(N, U):
    counts = []
    for T in TS:
        tr, o = trace_case(N, T)
        assert (o["stats"]["status"] == 0).all()
        counts.append(check_restatements(tr, o, *trace_users(N, U, T), what=f"N={N} U={U} T={T}"))
        assert counts[-1]["delay"] == counts[-1]["pubAck"] == 3 * T and counts[-1]["lost user-side"] == 0
        if T >= 63:  # (what the GPU test asserts of each such case: no kind without a row)
            assert_every_kind(counts[-1], (N, U, T))
    assert_every_kind(total(counts), (N, U))


def test_restatements_agree_under_ext_lat():
    tr, o = trace_case(5, 129, "EXT_LAT")
    n = check_restatements(tr, o, *trace_users(5, 3, 129), what="EXT_LAT")
    assert_every_kind(n)
    assert n["delay"] == n["pubAck"] == 3 * 129 and n["lost user-side"] == 0


def test_restatements_agree_where_emissions_are_lost():
    """Links near the simtime_t range (user side) and a herded node whose queue passes it (node side):
    the records count the lost emissions, the vectors have no row for them."""
    tr, who, uu, ud = carry_case()
    n = check_restatements(tr, replay_oracle(tr), who, uu, ud, what="carry")
    assert_every_kind(n)
    assert n["lost user-side"] > 0 and n["pubAck"] < n["delay"] == 96
    tr, o, who, uu, ud = herded_case()
    h = check_restatements(tr, o, who, uu, ud, what="herded")
    assert_every_kind(h)
    assert h["lost queueTime"] == int(o["stats"]["n_qtime_overflow"][0]) > 0


def test_a_failed_replication_has_no_rows_and_empty_records():
    tr, o = trace_case(5, 65)
    who, uu, ud = trace_users(5, 3, 65)
    n = check_restatements(tr, o, who, uu, ud, statuses=[0, 1, 9])
    full = check_restatements(tr, o, who, uu, ud)
    assert n["delay"] == 2 * 65 and full["delay"] == 3 * 65 and 0 < n["queueTime"] < full["queueTime"]
