"""Quantiles on the device (fognet_quantiles_dev, fognet_job_quantiles_dev) against the restatement
in Python integers (quantile_ref): exact equality of int64, every case with and without the skipped
rounds (FOGNET_QUANTILES=full) and identical bytes from both; against the device's own signal
vectors and window records on the same replay.  test_quantiles.py checks the restatement without
a GPU."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import quantile_ref as qr
import stream_gate
import tracegen as tg
import window_ref as wr
from fognetsimpp_amd import _abi
from guarded import Arena
from test_per_user_stats import draw_links, draw_users, replay_oracle, trace_case
from test_user_stats import HIER_UP, hier_case
from test_window_stats import oracle_case

pytestmark = pytest.mark.gpu

REP = _abi.REP_STATS_DTYPE
MODES = ("skip", "full")
I64_MAX = 2**63 - 1
I32_MAX = 2**31 - 1
PPM = 10**6
PPM8 = [990000, 0, PPM, 500000, 500000, 1, 999999, 250000]  # unsorted, repeated, both ends
_replays: dict = {}


def set_mode(monkeypatch, mode):
    if mode == "full":
        monkeypatch.setenv("FOGNET_QUANTILES", "full")
    else:
        monkeypatch.delenv("FOGNET_QUANTILES", raising=False)


def device_replay(ctx, key, tr, policy="REF_V3", **kw):
    """(device trace, replay outputs) of a trace, replayed once per key and left unchanged."""
    if key not in _replays:
        d = fa.as_device_trace(tr, torch.device("cuda", ctx.device))
        _replays[key] = (d, fa.run_batch(ctx, d, policy=policy, **kw))
    return _replays[key]


def both_modes(ctx, monkeypatch, d, out, who, uu, ud, ppm, **kw):
    """Both calls in both modes: identical bytes; returns (value, count, n_unassigned, job value, job count)."""
    got = {}
    for mode in MODES:
        set_mode(monkeypatch, mode)
        v, c, un = fa.quantiles(ctx, d, out, who, uu, ud, ppm, **kw)
        jv, jc = fa.job_quantiles(ctx, d, out, who, uu, ud, ppm, **kw)
        got[mode] = (v.cpu().numpy().copy(), c.cpu().numpy().copy(), un.cpu().numpy().copy(), jv.copy(), jc.copy())
    for a, b in zip(got["skip"], got["full"]):
        assert a.dtype == np.int64 and a.tobytes() == b.tobytes()
    return got["skip"]


def check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, ppm, what="", flags=None, up=0, statuses=None, **kw):
    want = qr.expected(tr, o, who, uu, ud, ppm, flags, up, statuses) + qr.expected_job(tr, o, who, uu, ud, ppm, flags, up, statuses)
    got = both_modes(ctx, monkeypatch, d, out, who, uu, ud, ppm, **kw)
    for g, w, name in zip(got, want, ("value", "count", "n_unassigned", "job value", "job count")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")
    return got


def handmade(ctx, arrive, node, status, start, done, dl, ul):
    """Replay outputs written by hand (rows [T] of one replication, or [R][T]) over len(dl) nodes:
    (trace, o, device trace, out)."""
    dev = torch.device("cuda", ctx.device)
    arrive = np.atleast_2d(np.array(arrive, np.int64))
    R, T = arrive.shape
    N = len(dl)
    tr = dict(arrive=arrive, req=np.ones((R, T), np.int32), mips=np.ones(N, np.int32), dl=np.array(dl, np.int64),
              ul=np.array(ul, np.int64), init=np.array(ul, np.int64))
    stats = np.zeros(R, REP)
    stats["n_tasks"] = T
    rows = lambda a, dt: np.array(np.broadcast_to(np.atleast_2d(np.array(a, dt)), (R, T)))
    o = dict(node=rows(node, np.int32), status=rows(status, np.uint8), start=rows(start, np.int64), done=rows(done, np.int64),
             stats=stats)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = fa.BatchResult(t(o["node"]), t(o["status"]), t(o["start"]), t(o["done"]), t(stats.view(np.uint8)))
    return tr, o, fa.as_device_trace(tr, dev), out


def delays(ctx, values):
    """One replication whose delay population is exactly ``values`` (the delay of a publish is its
    user's uplink, to the tick): (trace, o, device trace, out, user_of, user_ul, user_dl)."""
    T = len(values)
    distinct = sorted(set(values))
    who = np.array([[distinct.index(v) for v in values]], np.int32)
    arrive = [1000 + 10 * i for i in range(T)]
    tr, o, d, out = handmade(ctx, arrive, [0] * T, [5] * T, [a + 1 for a in arrive], [a + 2 for a in arrive], [1], [1])
    return tr, o, d, out, who, np.array(distinct, np.int64), np.full(len(distinct), 3, np.int64)


def ranks_around(n_low: int, n: int):
    """ppm whose ranks are n_low and n_low + 1 of n values (either side of a boundary), and the ends."""
    below = n_low * PPM // n          # k = ceil(n * ppm / 10^6) <= n_low
    above = below + 1
    while qr.rank_of(n, above) <= n_low:
        above += 1
    assert qr.rank_of(n, below) == n_low and qr.rank_of(n, above) == n_low + 1
    return [below, above, 0, PPM]


# ---------------------------------------------------------------- parity over the shapes

@pytest.mark.parametrize("N", [1, 5, 300])
def test_parity_over_shapes(ctx, monkeypatch, N):
    """T around a wavefront step and past one workgroup round, U = 1, 3 and none, Q = 1 and 8:
    per replication and the job of R = 3."""
    for ti, T in enumerate((1, 63, 65, 257)):
        tr, o = trace_case(N, T)
        assert (o["stats"]["status"] == 0).all()
        d, out = device_replay(ctx, ("trace", N, T), tr)
        for qi, ppm in enumerate((PPM8, [500000], [PPM], PPM8[:3])):
            U = (1, 3, 0)[(qi + ti) % 3]
            if U:
                who, (uu, ud) = draw_users(100 * T + qi, 3, T, U, "rr"), draw_links(100 * T + qi + 1, 3, U, qi % 2 == 0)
            else:
                who = uu = ud = None
            v, c, un, jv, jc = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, ppm, f"N{N} T{T} U{U} Q{len(ppm)}")
            assert list(un) == ([0, 0, 0] if U else [T, T, T])
            assert (c[:, 1] == (T if U else 0)).all() and int(jc[1]) == (3 * T if U else 0)
            if not U:
                assert (v[:, 1:] == I64_MAX).all() and (jv[1:] == I64_MAX).all()


# ---------------------------------------------------------------- handmade populations

@pytest.mark.parametrize("n", [64, 65])
def test_all_equal_population(ctx, monkeypatch, n):
    """Every lane of a step adds to one counter: the summed path, a full wavefront and one past it."""
    tr, o, d, out, who, uu, ud = delays(ctx, [123456789] * n)
    v, c, _, jv, jc = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, PPM8, f"all equal {n}")
    assert (v[0, 1] == 123456789).all() and int(c[0, 1]) == n and (jv[1] == 123456789).all()


@pytest.mark.parametrize("byte", range(8))
def test_two_values_that_differ_in_one_byte(ctx, monkeypatch, byte):
    """The select must take the byte's round to tell them apart; the rank on either side."""
    lo = 0x0102030405060708
    hi = lo ^ (0x30 << (8 * byte))  # (byte 7: 0x31..., still below 2^62)
    assert lo < hi < 2**62 and [(lo ^ hi) >> (8 * b) & 255 != 0 for b in range(8)].count(True) == 1
    values = [lo, hi, hi, lo, lo, hi, lo] * 11  # 44 x lo, 33 x hi, interleaved over two steps
    tr, o, d, out, who, uu, ud = delays(ctx, values)
    ppm = ranks_around(44, 77)
    v, c, _, jv, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, ppm, f"byte {byte}")
    assert list(v[0, 1]) == [lo, hi, lo, hi] == list(jv[1]) and int(c[0, 1]) == 77


def test_negative_queue_times_beside_positive_ones(ctx, monkeypatch):
    """A task that starts in the tick before it is enqueued has a negative queueTime: the key's
    sign flip orders it below the positive ones."""
    T = 70
    arrive = [10**9 * (1 + i) for i in range(T)]
    start = [a + 10 + (i % 7 - 3) * 1000 for i, a in enumerate(arrive)]  # at_node = arrive + 10: -3000 .. +3000 ticks
    tr, o, d, out = handmade(ctx, arrive, [0] * T, [4] * T, start, [s + 5 for s in start], [10], [7])
    v, c, _, _, _ = check(ctx, monkeypatch, d, out, tr, o, None, None, None, PPM8, "negative queueTime")
    assert int(c[0, 0]) == T and v[0, 0, 1] < 0 < v[0, 0, 2]  # (PPM8[1] = 0: the minimum, PPM8[2]: the maximum)
    members = qr.replication_populations(tr, o, None, None, None)[0][0]["queue"]
    assert sum(m < 0 for m in members) >= 20 and sum(m > 0 for m in members) >= 20


def test_large_ticks_and_values_near_2_62(ctx, monkeypatch):
    """Ticks above 2^53 (no double holds them all) and delays near 2^62."""
    base = 2**56 + 1
    T = 66
    arrive = [base + 3 * i for i in range(T)]
    start = [a + 5 + (i % 5) for i, a in enumerate(arrive)]
    tr, o, d, out = handmade(ctx, arrive, [i % 2 for i in range(T)], [4 + i % 2 for i in range(T)], start,
                             [s + 2**40 + i for i, s in enumerate(start)], [1, 2], [3, 4])
    who = np.array([[i % 3 for i in range(T)]], np.int32)
    uu = np.array([2**62 - 1, 2**62 - 2**33, 2**61 + 12345], np.int64)
    ud = np.array([7, 2**31, 2**50], np.int64)
    v, c, _, _, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, PPM8, "2^56 / 2^62")
    assert int(v[0, 1, 2]) == 2**62 - 1 and int(v[0, 1, 1]) == 2**61 + 12345 and int(c[0, 1]) == T
    assert int(c[0, 3]) < 2 * T  # most user-side products leave the simtime_t range


def test_tie_group_straddles_the_rank(ctx, monkeypatch):
    values = [1] * 10 + [5] * 50 + [9] * 10
    tr, o, d, out, who, uu, ud = delays(ctx, values[::-1])
    ppm = ranks_around(10, 70)[:2] + ranks_around(60, 70)[:2] + [500000]
    v, _, _, _, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, ppm, "ties")
    assert list(v[0, 1]) == [1, 5, 5, 9, 5]


def test_one_member_no_member_and_a_lost_emission(ctx, monkeypatch):
    """n = 1; a signal without a member gives INT64_MAX and count 0; an emission that leaves the
    simtime_t range is no member, and the count is the window record's count."""
    tr, o, d, out, who, uu, ud = delays(ctx, [42])
    v, c, _, jv, jc = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, PPM8, "n = 1")
    assert (v[0, 1] == 42).all() and list(c[0]) == [0, 1, 1, 1, 1] and (v[0, 0] == I64_MAX).all() and (jv[0] == I64_MAX).all()
    # taskTime of task 2 completes 2^61 ticks after its publish: (done - created) * 1000 leaves int64
    arrive = [1000, 2000, 3000, 4000]
    done = [1500, 2500, 3000 + 2**61, 4500]
    tr, o, d, out = handmade(ctx, arrive, [0] * 4, [4] * 4, [a + 20 for a in arrive], done, [10], [5])
    who, uu, ud = np.zeros((1, 4), np.int32), np.array([3], np.int64), np.array([2], np.int64)
    v, c, _, _, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, [0, PPM], "lost emission")
    buf, outside, _ = fa.window_stats(ctx, d, out, who, uu, ud, 0, 2**62, 1)
    rec = buf.cpu().numpy().view(_abi.WINDOW_STATS_DTYPE).reshape(1, 1)[0, 0]
    assert not outside.cpu().numpy().any() and int(rec["taskTime"]["overflow"]) == 1
    for s, sig in enumerate(qr.SIGNALS):
        assert int(c[0, s]) == int(rec[sig]["count"]), sig
    assert int(c[0, 4]) == 3 and int(c[0, 2]) == 0 and int(v[0, 2, 0]) == I64_MAX
    assert int(v[0, 4, 1]) == int(rec["taskTime"]["max_raw"])


# ---------------------------------------------------------------- the device's own passes

@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
def test_against_the_devices_own_vectors_and_window_record(ctx, monkeypatch, policy):
    tr, o = trace_case(5, 191, policy)
    d, out = device_replay(ctx, ("trace", 5, 191, policy), tr, policy)
    who, (uu, ud) = draw_users(21, 3, 191, 7, "random"), draw_links(22, 3, 7, True)
    N, U = 5, 7
    ppm = [0, PPM, 500000, 990000, 999000, 10000, 333333, 750000]
    v, c, _, jv, jc = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, ppm, policy, policy=policy)
    vec = fa.signal_vectors(ctx, d, out, who, uu, ud, policy=policy)
    last = wr.latest_tick(tr, o, who, uu, ud)
    buf, outside, _ = fa.window_stats(ctx, d, out, who, uu, ud, 0, last + 1, 1, policy=policy)
    recs = buf.cpu().numpy().view(_abi.WINDOW_STATS_DTYPE).reshape(3, 1)
    assert not outside.cpu().numpy().any()
    names = ["queue"] * N + ["delay"] + ["latency"] * U + ["latencyH1"] * U + ["taskTime"] * U
    job = {s: [] for s in qr.SIGNALS}
    for r in range(3):
        off = vec["offset"][r]
        for s, sig in enumerate(qr.SIGNALS):
            pooled = sorted(int(vec["value"][r][p]) for j, name in enumerate(names) if name == sig
                            for p in range(int(off[j]), int(off[j + 1])))
            job[sig] += pooled
            m = recs[r, 0][sig]
            assert len(pooled) == int(c[r, s]) == int(m["count"]), (r, sig)
            if pooled:
                assert [int(x) for x in v[r, s]] == [pooled[qr.rank_of(len(pooled), p) - 1] for p in ppm], (r, sig)
                assert int(v[r, s, 0]) == int(m["min_raw"]) and int(v[r, s, 1]) == int(m["max_raw"])
    for s, sig in enumerate(qr.SIGNALS):
        pooled = sorted(job[sig])
        assert [int(x) for x in jv[s]] == [pooled[qr.rank_of(len(pooled), p) - 1] for p in ppm] and int(jc[s]) == len(pooled)


# ---------------------------------------------------------------- the other policies and replays

def test_ext_hier_with_the_replays_flags_and_refused_without(ctx, monkeypatch):
    tr, _, _, o, _ = hier_case(0)
    T = tr["arrive"].shape[1]
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_batch(ctx, d, policy="EXT_HIER", hier_threshold_s=0, hier_up_tick=HIER_UP, escalated=True)
    flags = out.escalated.cpu().numpy()
    assert 0 < int(flags.sum()) < T
    who, (uu, ud) = draw_users(0xE, 1, T, 4, "rr"), draw_links(0xF, 1, 4, False)
    v, _, _, _, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, PPM8, "hier", flags=flags, up=HIER_UP)
    flat, _, _ = qr.expected(tr, o, who, uu, ud, PPM8)
    assert v.tobytes() != flat.tobytes()  # the hop shows
    bare = fa.BatchResult(out.node, out.status, out.start_tick, out.done_tick, out.stats)
    for mode in MODES:
        set_mode(monkeypatch, mode)
        val = torch.full((1, 5, 8), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        cnt = torch.full((1, 5), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        un = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        for call in (lambda: fa.quantiles(ctx, d, bare, who, uu, ud, PPM8, policy="EXT_HIER", hier_up_tick=HIER_UP, value=val,
                                          count=cnt, n_unassigned=un),
                     lambda: fa.job_quantiles(ctx, d, bare, who, uu, ud, PPM8, policy="EXT_HIER", hier_up_tick=HIER_UP,
                                              value=val[0], count=cnt[0])):
            with pytest.raises(fa.FognetError) as e:
                call()
            assert e.value.code == _abi.FOGNET_ERR_UNSUPPORTED and "escalated" in str(e.value)
        torch.cuda.synchronize()
        assert (val.cpu().numpy() == 0x5A5A5A5A).all() and (cnt.cpu().numpy() == 0x5A5A5A5A).all() and int(un[0]) == 0x5A5A5A5A


def test_assigned_replay_outputs(ctx, monkeypatch):
    tr, _ = trace_case(5, 191)
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_assigned(ctx, d, fa.assign_random(3, 191, 5, 7, dev))
    o = dict(node=out.node.cpu().numpy(), status=out.status.cpu().numpy(), start=out.start_tick.cpu().numpy(),
             done=out.done_tick.cpu().numpy(), stats=out.rep_stats())
    assert (o["stats"]["status"] == 0).all() and (o["status"] == 4).any()
    who, (uu, ud) = draw_users(5, 3, 191, 6, "random"), draw_links(6, 3, 6, True)
    _, c, _, _, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, PPM8, "assigned", policy="REF_V3")
    assert (c[:, 1] == 191).all() and (c[:, 0] > 0).all()


def test_down_nodes_and_tasks_that_never_complete(ctx, monkeypatch):
    tr, o, who, uu, ud, _, _ = oracle_case("down")
    d, out = device_replay(ctx, "down", tr)
    np.testing.assert_array_equal(out.done_tick.cpu().numpy(), o["done"])
    assert (o["status"] == 9).any() and (o["done"] == -1).any()
    _, c, _, _, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, PPM8, "down")
    assert (c[:, 4] == (o["done"] >= 0).sum(axis=1)).all() and (c[:, 4] < c[:, 1]).all()


def test_good_failed_aborted_good_and_unassigned(ctx, monkeypatch):
    """[good, failed, REF_ABORTED, good]: the failed one gets the empty results and nothing of it is
    read; the aborted one keeps its results and is absent from the job; publishes of no known user
    keep their queueTime and are counted."""
    tr = tg.make_batch(0x600D, 4, 5, 129, rho=0.9)
    o = replay_oracle(tr)
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_batch(ctx, d)
    torch.cuda.synchronize()
    statuses = [0, _abi.FOGNET_ERR_ARG, _abi.FOGNET_REF_ABORTED, 0]
    st = out.rep_stats().copy()
    st["status"] = statuses
    out.stats.copy_(torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).to(dev))
    who, (uu, ud) = draw_users(4, 4, 129, 3, "rr"), draw_links(5, 4, 3, True)
    who[1] = I32_MAX
    uu[1] = ud[1] = 0x5A5A5A5A5A5A5A5A
    out.node[1].fill_(I32_MAX)  # nothing of a failed replication's rows is read
    who[0, 5], who[3, 7], who[3, 9] = 3, -1, I32_MAX  # one past the last user, negative, far out
    v, c, un, jv, jc = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, PPM8, "statuses", statuses=statuses)
    assert (v[1] == I64_MAX).all() and not c[1].any() and list(un) == [1, 0, 0, 2]
    assert int(c[2, 1]) == 129 and list(jc) == list(c[0] + c[3]) and int(c[0, 1]) == 128 and int(c[3, 1]) == 127


# ---------------------------------------------------------------- the job's pooling

def test_job_of_many_short_replications(ctx, monkeypatch):
    """More workgroups than are resident at once add their bins to the workspace's table."""
    R, T = 1500, 40
    tr = tg.make_batch(0x1500, R, 5, T, rho=0.9)
    o = replay_oracle(tr)
    assert (o["stats"]["status"] == 0).all()
    d, out = device_replay(ctx, "many", tr)
    who, (uu, ud) = draw_users(15, R, T, 3, "rr"), draw_links(16, R, 3, False)
    ppm = [500000, 990000, 999000, 0, PPM]
    want_v, want_c = qr.expected_job(tr, o, who, uu, ud, ppm)
    for mode in MODES:
        set_mode(monkeypatch, mode)
        jv, jc = fa.job_quantiles(ctx, d, out, who, uu, ud, ppm)
        np.testing.assert_array_equal(jv, want_v, err_msg=mode)
        np.testing.assert_array_equal(jc, want_c, err_msg=mode)
    assert int(want_c[1]) == R * T


def test_job_pools_the_values_and_merges_no_results(ctx, monkeypatch):
    """Delays 1, 2, 3 in one replication and 10, 20, 30 in the other: the job's median is 3, which is
    neither replication's median (2 and 20); two job calls in a row, the second over the table and the
    state the first left in the workspace."""
    arrive = [[1000, 2000, 3000], [1000, 2000, 3000]]
    tr, o, d, out = handmade(ctx, arrive, [0] * 3, [5] * 3, [[1001, 2001, 3001]] * 2, [[1002, 2002, 3002]] * 2, [1], [1])
    who = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
    uu, ud = np.array([[1, 2, 3], [30, 20, 10]], np.int64), np.full((2, 3), 4, np.int64)
    v, _, _, jv, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, [500000], "pooled")
    assert int(jv[1, 0]) == 3 and [int(v[r, 1, 0]) for r in range(2)] == [2, 20]
    first = fa.job_quantiles(ctx, d, out, who, uu, ud, PPM8)
    second = fa.job_quantiles(ctx, d, out, who, uu, ud, [PPM, 0])
    again = fa.job_quantiles(ctx, d, out, who, uu, ud, PPM8)
    for got, ppm in ((first, PPM8), (second, [PPM, 0]), (again, PPM8)):
        want = qr.expected_job(tr, o, who, uu, ud, ppm)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    assert list(second[0][1]) == [30, 1]


# ---------------------------------------------------------------- argument errors, empty shapes

def test_argument_errors_and_empty_shapes(ctx):
    dev = torch.device("cuda", ctx.device)
    tr, o = trace_case(5, 65)
    d, out = device_replay(ctx, ("trace", 5, 65), tr)
    who = torch.from_numpy(draw_users(1, 3, 65, 4, "rr")).to(dev)
    uu, ud = (torch.from_numpy(x).to(dev) for x in draw_links(2, 3, 4, False))
    so = fa.run_batch(ctx, d, out=fa.allocate_outputs(3, 65, dev, per_task=False))
    for f in (fa.quantiles, fa.job_quantiles):
        with pytest.raises(fa.FognetError) as e:
            f(ctx, d, so, who, uu, ud, [500000])  # a statistics-only out
        assert e.value.code == _abi.FOGNET_ERR_ARG
    p = fa.engine._ptr
    bi = _abi.BatchIn(3, 65, 5, 1, 5, 0, *(p(d[k]) for k in ("arrive", "req", "mips", "dl", "ul", "init")))
    outs = dict(node=out.node, status=out.status, start_tick=out.start_tick, done_tick=out.done_tick, stats=out.stats)
    val = torch.full((3, 5, 8), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((3, 5), -7, dtype=torch.int64, device=dev)
    un = torch.full((3,), -7, dtype=torch.int64, device=dev)
    ranks = lambda *a: (C.c_int32 * len(a))(*a)

    def call(job, user_of=p(who), U=4, stride=0, ul=p(uu), dl=p(ud), ppm=ranks(500000, 990000), Q=2, value=p(val), count=p(cnt),
             unassigned=p(un), drop=None):
        bo = _abi.BatchOut(**{k: p(v) for k, v in outs.items() if k != drop})
        head = (ctx.handle, C.byref(bi), C.byref(bo), user_of, U, stride, ul, dl, ppm, Q, value, count)
        if job:
            return ctx._lib.fognet_job_quantiles_dev(*head, None)
        return ctx._lib.fognet_quantiles_dev(*head, unassigned, None)
    for job in (False, True):
        for bad in (dict(Q=0), dict(Q=9, ppm=ranks(*[1] * 9)), dict(Q=-1), dict(ppm=ranks(-1, 5)), dict(ppm=ranks(5, PPM + 1)),
                    dict(ppm=None), dict(value=None), dict(count=None), dict(drop="start_tick"), dict(drop="node"),
                    dict(drop="stats"), dict(U=-1), dict(stride=3), dict(stride=5), dict(ul=None), dict(dl=None),
                    dict(user_of=None)):
            assert call(job, **bad) == _abi.FOGNET_ERR_ARG, (job, bad)
    torch.cuda.synchronize()
    assert (val.cpu().numpy() == -7).all() and (cnt.cpu().numpy() == -7).all() and (un.cpu().numpy() == -7).all()
    # U = 0 with NULL users: the node side alone; n_unassigned is optional
    assert call(False, user_of=None, U=0, ul=None, dl=None, unassigned=None) == _abi.FOGNET_OK
    torch.cuda.synchronize()
    want_v, want_c, _ = qr.expected(tr, o, None, None, None, [500000, 990000])
    got = val.cpu().numpy().reshape(-1)[:30].reshape(3, 5, 2)
    np.testing.assert_array_equal(got, want_v)
    np.testing.assert_array_equal(cnt.cpu().numpy(), want_c)
    assert (un.cpu().numpy() == -7).all() and (val.cpu().numpy().reshape(-1)[30:] == -7).all()
    # T = 0: empty populations; R = 0: nothing per replication, five empty populations for the job
    t0 = {k: (v[:, :0] if k in ("arrive", "req") else v) for k, v in tr.items()}
    d0 = fa.as_device_trace(t0, dev)
    o0 = fa.run_batch(ctx, d0)
    v, c, u0 = fa.quantiles(ctx, d0, o0, np.zeros((3, 0), np.int32), uu, ud, [0, PPM])
    jv, jc = fa.job_quantiles(ctx, d0, o0, np.zeros((3, 0), np.int32), uu, ud, [0, PPM])
    assert (v.cpu().numpy() == I64_MAX).all() and not c.cpu().numpy().any() and not u0.cpu().numpy().any()
    assert (jv == I64_MAX).all() and jv.shape == (5, 2) and not jc.any()
    empty = fa.as_device_trace({k: v[:0] for k, v in tr.items()}, dev)
    oe = fa.allocate_outputs(0, 65, dev)
    v, c, u0 = fa.quantiles(ctx, empty, oe, np.zeros((0, 65), np.int32), uu, ud, [0, PPM])
    assert v.numel() == 0 and c.numel() == 0 and u0.numel() == 0
    jv, jc = fa.job_quantiles(ctx, empty, oe, np.zeros((0, 65), np.int32), uu, ud, [0, PPM],
                              value=torch.full((5, 2), -7, dtype=torch.int64, device=dev),
                              count=torch.full((5,), -7, dtype=torch.int64, device=dev))
    assert (jv == I64_MAX).all() and not jc.any()


# ---------------------------------------------------------------- buffer contract, streams

def guarded_run(ctx, tr, who, uu, ud, ppm, poison, misalign):
    dev = torch.device("cuda", ctx.device)
    ain, aout = Arena(dev, poison), Arena(dev, poison)
    d = {k: ain.put(v, misalign, name=k) for k, v in tr.items()}
    g_who, g_uu, g_ud = ain.put(who, misalign, "user_of"), ain.put(uu, misalign, "user_ul"), ain.put(ud, misalign, "user_dl")
    R, T = d["arrive"].shape
    Q = len(ppm)
    out = fa.BatchResult(node=aout.alloc((R, T), torch.int32, misalign, "node"), status=aout.alloc((R, T), torch.uint8, misalign, "status"),
                         start_tick=aout.alloc((R, T), torch.int64, misalign, "start"),
                         done_tick=aout.alloc((R, T), torch.int64, misalign, "done"),
                         stats=aout.alloc(R * REP.itemsize // 8, torch.int64, misalign, name="stats").view(torch.uint8))
    fa.run_batch(ctx, d, out=out)
    val, cnt = aout.alloc((R, 5, Q), torch.int64, misalign, "value"), aout.alloc((R, 5), torch.int64, misalign, "count")
    un = aout.alloc((R,), torch.int64, misalign, "n_unassigned")
    jval, jcnt = aout.alloc((5, Q), torch.int64, misalign, "job_value"), aout.alloc((5,), torch.int64, misalign, "job_count")
    if misalign:
        assert g_who.data_ptr() % 8 == 4 and val.data_ptr() % 16 == 8  # natural alignment only
    fa.quantiles(ctx, d, out, g_who, g_uu, g_ud, ppm, value=val, count=cnt, n_unassigned=un)
    jv, jc = fa.job_quantiles(ctx, d, out, g_who, g_uu, g_ud, ppm, value=jval, count=jcnt)
    torch.cuda.synchronize()
    ain.check()
    aout.check()
    return val.cpu().numpy().copy(), cnt.cpu().numpy().copy(), un.cpu().numpy().copy(), jv.copy(), jc.copy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,ppm", [(65, [500000]), (191, PPM8)])
def test_buffer_contract(ctx, monkeypatch, mode, T, ppm):
    """Guard bands around every array, two poisons, and pointers at their natural alignment only."""
    set_mode(monkeypatch, mode)
    tr, o = trace_case(5, T)
    who = draw_users(T, 3, T, 4, "random")
    who[1, T // 2] = 4  # one past the last user
    uu, ud = draw_links(T + 1, 3, 4, True)
    want = qr.expected(tr, o, who, uu, ud, ppm) + qr.expected_job(tr, o, who, uu, ud, ppm)
    runs = [guarded_run(ctx, tr, who, uu, ud, ppm, p, m) for p, m in ((0xA5, False), (0x5A, False), (0xA5, True))]
    for got in runs:
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w, err_msg=mode)
        assert list(got[2]) == [0, 1, 0]


@pytest.mark.parametrize("ppm", [[990000], PPM8])
def test_gated_on_a_side_stream(ctx, tmp_path, monkeypatch, ppm):
    """Both calls behind a gate on a side stream: only enqueued, and they read the inputs that the
    stream's own copies put there."""
    monkeypatch.setenv(stream_gate.REPORT_ENV, str(tmp_path / "gate.json"))
    dev = torch.device("cuda", ctx.device)
    tr, o = trace_case(5, 65)
    decoy = tg.make_batch(0xDEC0, 3, 5, 65, rho=0.9)
    who, (uu, ud) = draw_users(31, 3, 65, 4, "rr"), draw_links(32, 3, 4, True)
    Q = len(ppm)
    want = qr.expected(tr, o, who, uu, ud, ppm) + qr.expected_job(tr, o, who, uu, ud, ppm)
    names = ("arrive", "req", "mips", "dl", "ul", "init")
    plain = fa.as_device_trace(tr, dev)
    fa.job_quantiles(ctx, plain, fa.run_batch(ctx, plain), who, uu, ud, ppm)
    torch.cuda.synchronize()  # (the workspace has grown)
    ranks = (C.c_int32 * Q)(*ppm)

    class Job:
        def __init__(self):
            self.d = fa.as_device_trace(tr, dev)
            self.who, self.uu, self.ud = (torch.from_numpy(x).to(dev) for x in (who, uu, ud))
            self.inputs = dict({k: self.d[k] for k in names}, user_of=self.who, user_ul=self.uu, user_dl=self.ud)
            self.out = fa.allocate_outputs(3, 65, dev)
            self.val = torch.empty((3, 5, Q), dtype=torch.int64, device=dev)
            self.cnt = torch.empty((3, 5), dtype=torch.int64, device=dev)
            self.un = torch.empty(3, dtype=torch.int64, device=dev)
            self.jval = torch.empty((5, Q), dtype=torch.int64, device=dev)
            self.jcnt = torch.empty(5, dtype=torch.int64, device=dev)

    def enqueue(job):
        fa.run_batch(ctx, job.d, out=job.out)
        fa.quantiles(ctx, job.d, job.out, job.who, job.uu, job.ud, ppm, value=job.val, count=job.cnt, n_unassigned=job.un)
        bi, bo = fa.engine._pass_descriptors(job.d, job.out, fa.engine._dims(job.d), _abi.FOGNET_POLICY_REF_V3, None)
        p = fa.engine._ptr
        ctx.check(ctx._lib.fognet_job_quantiles_dev(ctx.handle, C.byref(bi), C.byref(bo), p(job.who), 4, 4, p(job.uu), p(job.ud),
                                                    ranks, Q, p(job.jval), p(job.jcnt),
                                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "job quantiles")

    gate = stream_gate.Gate(dev)
    gate.choose(1)
    kinds = dict(arrive=np.int64, req=np.int32, mips=np.int32, dl=np.int64, ul=np.int64, init=np.int64)
    decoys = dict({k: np.ascontiguousarray(decoy[k], dtype=kinds[k]) for k in names}, user_of=(who + 1) % 4,
                  user_ul=uu + 1000, user_dl=ud + 1000)
    job = gate.run("quantiles", f"quantiles-Q{Q}", Job, decoys, enqueue)
    got = (job.val, job.cnt, job.un, job.jval, job.jcnt)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)


# ---------------------------------------------------------------- the driver

@pytest.mark.parametrize("extra", [(), ("--assign", "rr")])
def test_driver_quantile_scalars(ctx, tmp_path, extra):
    """fognet_replay --sca f --quantiles 50,99,99.9 appends the job's quantiles: the file without the
    option is the same file minus those lines, and the lines parse back to fa.job_quantiles of the
    same job (regenerated through fognet_gen_trace_mqtt with the driver's seeds)."""
    from fognetsimpp_amd import formats
    from test_driver import INI, MS, SEC, drive
    a, b, trc = (str(tmp_path / n) for n in ("a.sca", "b.sca", "g.fogntrc"))
    args = ("-f", INI, "--users", "user[3]", "--reps", "8", *extra)
    drive(*args, "--sca", a, "--quantiles", "50,99,99.9", "--trace-out", trc)
    drive(*args, "--sca", b)
    plain, text = open(b).read(), open(a).read()
    lines = [ln for ln in text.splitlines(keepends=True) if re.search(r'"\w+:p[\d.]+"', ln)]
    assert "".join(ln for ln in text.splitlines(keepends=True) if ln not in lines) == plain and text.startswith(plain)
    tr = formats.load_trace(trc)
    tr = {k: tr[k] for k in ("arrive", "req", "mips", "dl", "ul", "init")}
    R, T = tr["arrive"].shape
    assert R == 8
    gens = [formats.gen_trace_mqtt(1 + r, [200 * MS] * 3, [1500 * MS] * 3, [MS] * 3, [MS] * 3, 300 * SEC) for r in range(R)]
    who = np.stack([g["user"] for g in gens]).astype(np.int32)
    links = np.full(3, MS, np.int64)  # --user-ul / --user-dl defaults
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    if extra:
        assign = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.arange(T, dtype=np.int32) % np.shape(tr["mips"])[-1], (R, T)))).to(dev)
        out = fa.run_assigned(ctx, d, assign)
    else:
        out = fa.run_batch(ctx, d)
    ppm = [500000, 990000, 999000]
    jv, jc = fa.job_quantiles(ctx, d, out, who, links, links, ppm, policy="REF_V3")
    want = []
    mods = ("fogNodes", "broker", "users", "users", "users")
    for s, sig in enumerate(("queueTime", "delay", "latency", "latencyH1", "taskTime")):
        if jc[s]:
            want += [f'scalar FogNet5.{mods[s]}.udpApp[0] \t"{sig}:p{pct}" \t{"%.14g" % (int(jv[s, q]) * 1e-12)}\n'
                     for q, pct in enumerate(("50", "99", "99.9"))]
    assert lines == want and int(jc[1]) == R * T and len(lines) >= 9
