"""User-side signals, host side (no GPU): the independent Python restatement
(user_stats_ref) against the oracle's event-level records, bit for bit, on the
shapes and edges test_user_stats_gpu.py then runs on the device; the emission rule
ms_raw around 2^53 and 2^63 / 1000; and the reason fognet_user_stats_dev refuses
EXT_HIER, pinned as a number."""
import numpy as np
import pytest

import oracle_lib as ol
import tracegen as tg
import user_stats_ref as us

MS, TPS = 10**9, 10**12
NEVER = np.iinfo(np.int64).max
B = 2**63 // 1000  # the largest d whose exact d * 1000 is still below 2^63
assert B == 9223372036854775
_cache: dict = {}


def run_oracle(tr, uu, ud, policy="REF_V3", **kw):
    return ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=4, user_ul=uu,
                        user_dl=ud, policy=ol.POLICIES[policy], down=tr.get("down"), region=tr.get("region"), **kw)


def case(key, make, policy="REF_V3", **kw):
    """(trace, user_ul, user_dl, oracle result, restatement's records), computed once per
    key and left unchanged; ``make`` returns (trace, user_ul, user_dl)."""
    if key not in _cache:
        tr, uu, ud = make()
        o = run_oracle(tr, uu, ud, policy, **kw)
        _cache[key] = (tr, uu, ud, o, us.expected(tr, o, uu, ud))
    return _cache[key]


def user_links(seed, shape):
    """Links drawn from [0, 5 ms)."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 5 * MS, shape).astype(np.int64), rng.integers(0, 5 * MS, shape).astype(np.int64)


# ---------------------------------------------------------------- the cases (shared with the GPU tests)

def batch_case(N, T, policy="REF_V3", R=3, per_task=True, shared=False, rho=0.9):
    def make():
        tr = tg.make_batch(0x05E2 + 7 * N + T, R, N, T, rho=rho)
        if shared:  # node_stride = 0
            tr = dict(tr, **{k: tr[k][0] for k in ("mips", "dl", "ul", "init")})
        return (tr, *user_links(1000 * N + T, (R, T) if per_task else (R,)))
    return case(("batch", N, T, policy, R, per_task, shared, rho), make, policy)


def down_case():
    """T = 257: node 0 crashes in mid-run (12,345 ticks before its 21st task would
    complete) and node 3 at publish 128, so tasks are lost at a crashed node (status 9)
    and accepted tasks never complete (done = -1)."""
    def make():
        tr = tg.make_batch(0xD0D1, 3, 5, 257, rho=1.5, lat_scale=10)
        free = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=3)
        down = np.full(tr["mips"].shape, NEVER, np.int64)
        for r in range(3):
            i = int(np.nonzero(free["node"][r] == 0)[0][20])
            down[r, 0] = int(free["done"][r, i]) - 12345
            down[r, 3] = int(tr["arrive"][r, 128])
        return (dict(tr, down=down), *user_links(0xD0, (3, 257)))
    return case("down", make)


SWEEP_D = ([0, 1, 2**53 - 1, 2**53, 2**53 + 1] + list(range(B - 40, B + 41)) + [2**62, 2**61 + 12345])


def sweep_case():
    """Every d of SWEEP_D fed straight into the emission rule: the broker's own pubAck
    term of latencyH1 is ms_raw(user_ul + user_dl) and depends on nothing else, so
    task i gets user_ul = d_i // 2, user_dl = d_i - d_i // 2.  One replication, four
    1000-MIPS nodes 1 ms away, 1-s tasks published 50 ms apart."""
    def make():
        T = len(SWEEP_D)
        n = np.full(4, MS, np.int64)
        tr = dict(arrive=(100 * MS + 50 * MS * np.arange(T, dtype=np.int64))[None], req=np.full((1, T), 1000, np.int32),
                  mips=np.full(4, 1000, np.int32), dl=n, ul=n.copy(), init=n.copy())
        uu = np.array([[d // 2 for d in SWEEP_D]], np.int64)
        ud = np.array([[d - d // 2 for d in SWEEP_D]], np.int64)
        return tr, uu, ud
    return case("sweep", make)


HIER_UP = 20 * MS


def hier_case(threshold_s, N=2, T=200, gap=100 * MS, up=HIER_UP):
    """One region over N 1000-MIPS nodes 1 ms away, 3-s tasks every ``gap``: the nodes
    fall behind at once, and with ``threshold_s`` = 0 the regional broker escalates as
    soon as every node advertises queued work."""
    def make():
        n = np.full(N, MS, np.int64)
        tr = dict(arrive=(gap * np.arange(1, T + 1, dtype=np.int64))[None], req=np.full((1, T), 3000, np.int32),
                  mips=np.full(N, 1000, np.int32), dl=n, ul=n.copy(), init=n.copy(),
                  region=np.zeros((1, T), np.int32))
        return tr, np.array([2 * MS], np.int64), np.array([3 * MS], np.int64)
    return case(("hier", threshold_s, N, T, gap, up), make, "EXT_HIER", hier_threshold_s=threshold_s, hier_up_tick=up)


def abort_case():
    """make_ref_v3_fixtures.py's overflow_one_node shape: MIPS 1, a service of 9223 s; the
    wait of task 2 (9223 s + 1 s - 2 ticks) leaves int64 when multiplied by 1000, so the
    reference run ends at that queueTime emission.  The oracle (and the engine) replay on."""
    def make():
        n = np.full(2, MS, np.int64)
        tr = dict(arrive=(TPS + np.array([0, 1, 2, 3, 5000 * TPS], np.int64))[None],
                  req=np.array([[9223, 1, 1, 1, 1]], np.int32), mips=np.ones(2, np.int32), dl=n, ul=n.copy(), init=n.copy())
        return tr, np.array([2 * MS], np.int64), np.array([2 * MS], np.int64)
    return case("abort", make)


def sum_of(m) -> int:
    s = int(m["sum_lo"]) | (int(m["sum_hi"]) << 64)
    return s - (1 << 128) if s >> 127 else s


# ---------------------------------------------------------------- the emission rule

def test_ms_raw_known_values():
    assert us.to_int64(0.25) == 0 and us.to_int64(0.5) == 1 and us.to_int64(-0.5) == 0
    assert us.to_int64(0.49999999999999994) == 1  # floor(x + 0.5) as written: the sum itself rounds to 1.0
    assert us.to_int64(-1.5) == -1 and us.to_int64(2.0**63) is None and us.to_int64(-(2.0**63)) is None
    assert us.to_int64(2.0**63 - 1024) == 2**63 - 1024  # the largest double below 2^63
    assert (us.ms_raw(0), us.ms_raw(1), us.ms_raw(10**12 + 1)) == (0, 1000, 10**15 + 1000)
    # from 2^53 on the conversion rounds to even (2 apart), and near 2^63 the product to a multiple of 1024
    assert us.ms_raw(2**53 - 1) == 2**53 * 1000 - 1024  # exact conversion; the product ... - 1000 rounds
    assert us.ms_raw(2**53) == us.ms_raw(2**53 + 1) == 2**53 * 1000  # 2^53 + 1 -> 2^53
    assert us.ms_raw(2**53 + 3) == 2**53 * 1000 + 4096  # -> 2^53 + 4; the product ... + 4000 rounds
    assert us.ms_raw(2**62) is None and us.ms_raw(2**61 + 12345) is None


def test_ms_raw_equals_the_oracles_rule_at_the_edges():
    """The restatement and oracle/fognet_oracle.c's orc_ms_raw, two writings of
    toInt64((double)d * 1000.0), on every d near 2^53 (the conversion starts to round)
    and near 2^63 / 1000 (the product leaves the range), and both outcomes occur."""
    ds = list(range(2**53 - 70, 2**53 + 70)) + list(range(B - 2100, B + 2100)) + [2**k for k in range(64 - 11, 63)]
    got = [us.ms_raw(d) for d in ds]
    assert got == [ol.ms_raw(d) for d in ds]
    assert None in got and any(v is not None and v >= 2**63 - 2048 * 1000 for v in got)
    edge = [d for d in range(B - 2100, B + 2100) if us.ms_raw(d) is None]
    # Doubles are 2 apart here and 1024 apart at the product.  B is odd and converts to B + 1 (ties to even), whose
    # product 2^63 + 192 rounds to 2^63: B itself is lost although B * 1000 < 2^63.  B - 1 converts exactly and
    # its product 2^63 - 1808 rounds to 2^63 - 2048; B - 2 is odd and converts to B - 3, product 2^63 - 3808.
    assert edge == list(range(B, B + 2100))
    assert us.ms_raw(B - 1) == 2**63 - 2048 and us.ms_raw(B - 2) == us.ms_raw(B - 3) == 2**63 - 4096


# ---------------------------------------------------------------- restatement against the oracle's events

@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
@pytest.mark.parametrize("N", [1, 5, 64])
def test_restatement_equals_oracle_events(N, policy):
    for per_task in (True, False):
        tr, uu, ud, o, want = batch_case(N, 600, policy, per_task=per_task)
        assert (o["stats"]["status"] == 0).all() and (o["stats"]["n_tasks"] == 600).all()
        assert (o["status"] == 4).any() and (o["status"] == 5).any()
        us.assert_user_parity(want, o["user"])
        assert (want["delay"]["count"] == 600).all() and (want["latencyH1"]["count"] > 600).all()


def test_restatement_equals_oracle_events_node_down():
    tr, uu, ud, o, want = down_case()
    assert (o["stats"]["status"] == 0).all()
    assert (o["status"] == 9).any() and ((o["status"] != 9) & (o["done"] == -1)).any()
    us.assert_user_parity(want, o["user"])
    # a lost task sends no node ack, a task that never completes no status-6 ack
    acks = want["latency"]["count"] + want["latencyH1"]["count"] - 257
    np.testing.assert_array_equal(acks, 257 - (o["status"] == 9).sum(axis=1))
    np.testing.assert_array_equal(want["taskTime"]["count"], (o["done"] >= 0).sum(axis=1))


def test_boundary_sweep():
    tr, uu, ud, o, want = sweep_case()
    assert len(SWEEP_D) == 88 and int(o["stats"]["status"][0]) == 0 and int(o["stats"]["n_tasks"][0]) == 88
    us.assert_user_parity(want, o["user"])
    h1, tt, dly = (want[0][k] for k in ("latencyH1", "taskTime", "delay"))
    # all three outcomes are present: emitted, lost to the range, and squares that carry into the top limb
    assert int(h1["count"]) > 0 and int(h1["overflow"]) > 0 and int(h1["sq_top"]) > 0
    assert (int(h1["count"]), int(h1["overflow"]), int(h1["sq_top"])) == (49, 123, 11)
    assert (int(tt["count"]), int(tt["overflow"])) == (5, 83)
    assert (int(dly["count"]), int(dly["overflow"])) == (88, 0)
    # the pubAck term alone, d by d: the sweep reaches the device function with exactly these arguments
    raws = [us.ms_raw(d) for d in SWEEP_D]
    assert raws == [ol.ms_raw(d) for d in SWEEP_D]
    assert raws.count(None) == 43 and raws[SWEEP_D.index(B)] is None and raws[SWEEP_D.index(B - 1)] == 2**63 - 2048


def test_ext_hier_closed_form_misses_the_escalation_hop():
    """Why fognet_user_stats_dev refuses EXT_HIER: the closed form takes every node ack to
    leave at t + dl_k, but an escalated task reaches its node hier_up_tick later (oracle:
    e.tick = now + dl[k] + (escalated ? hier_up_tick : 0)) and the per-task outputs do not
    say which.  Over the oracle's own outputs the restatement's latencyH1 sum falls short
    of the event-level one by exactly 1000 * hier_up_tick per escalated status-4 ack; delay
    (no node involved) and taskTime (which goes by done_tick) agree.  A change that makes
    the outputs carry the escalation replaces this test with a parity test."""
    for key, acks in (((0,), 138), ((1,), None), ((2, 3, 300, 50 * MS, 7 * MS), 117)):
        tr, uu, ud, o, want = hier_case(*key)
        up = key[4] if len(key) > 1 else HIER_UP
        assert int(o["stats"]["status"][0]) == 0
        for sig in ("delay", "taskTime"):
            for f in us.FIELDS:
                assert want[0][sig][f] == o["user"][0][sig][f], (key, sig, f)
        for sig in ("latency", "latencyH1"):
            assert want[0][sig]["count"] == o["user"][0][sig]["count"], (key, sig)
        diff = sum_of(o["user"][0]["latencyH1"]) - sum_of(want[0]["latencyH1"])
        assert diff > 0 and diff % (1000 * up) == 0, (key, diff)
        if acks is not None:
            assert diff == acks * 1000 * up, (key, diff // (1000 * up))
    # a threshold nothing reaches: no task is escalated, and all four signals agree
    tr, uu, ud, o, want = hier_case(10**6)
    assert int(o["stats"]["status"][0]) == 0
    us.assert_user_parity(want, o["user"])


def test_ref_abort_shape_overflows_task_time():
    """The ref_abort case of the GPU tests, on the oracle: the replication has an abort
    point and a taskTime emission lost to the range, and the restatement agrees."""
    tr, uu, ud, o, want = abort_case()
    assert int(o["stats"]["status"][0]) == 0 and int(o["stats"]["abort_tick"][0]) != NEVER
    assert int(o["stats"]["n_qtime_overflow"][0]) > 0 and int(want[0]["taskTime"]["overflow"]) > 0
    us.assert_user_parity(want, o["user"])


def test_failed_replication_is_the_empty_record():
    tr, uu, ud, o, _ = batch_case(5, 600)
    want = us.expected(tr, o, uu, ud, statuses=[0, 1, 9])  # FOGNET_OK, FOGNET_ERR_ARG, FOGNET_REF_ABORTED
    assert us.is_empty(want[1]) and not us.is_empty(want[0])
    e = want[1]
    for sig in us.SIGNALS:
        assert (int(e[sig]["min_raw"]), int(e[sig]["max_raw"])) == (us.I64_MAX, us.I64_MIN)
        assert all(int(e[sig][f]) == 0 for f in us.FIELDS if f not in ("min_raw", "max_raw"))
    assert want[2].tobytes() == us.expected(tr, o, uu, ud)[2].tobytes()  # a REF_ABORTED one keeps its full record
