"""Time-window statistics on the device (fognet_window_stats_dev, fognet_reduce_window_stats_dev)
against the restatement in Python integers (window_ref), byte for byte, in both accumulator
layouts (LDS; FOGNET_WINDOW_STATS=hbm), against the device's own signal vectors, node records
and user records on the same replay, and the job reduction against the host merge.  The oracle
cases come from test_window_stats.py, which checks the restatement without a GPU."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import node_stats_ref as ns
import per_user_ref as pu
import stream_gate
import tracegen as tg
import user_stats_ref as us
import window_ref as wr
from fognetsimpp_amd import _abi
from guarded import Arena
from test_per_user_stats import draw_links, draw_users, replay_oracle, trace_case
from test_user_stats import HIER_UP, hier_case
from test_window_stats import covering, oracle_case, parse_vec, random_records

pytestmark = pytest.mark.gpu

WINDOW, REP = _abi.WINDOW_STATS_DTYPE, _abi.REP_STATS_DTYPE
LDS_CAP = _abi.WINDOW_LDS_WINDOWS  # window_stats.hip kWinLdsMax: W = LDS_CAP + 1 is the first size above it
LAYOUTS = ("lds", "hbm")
I32_MAX = 2**31 - 1
_replays: dict = {}


def set_layout(monkeypatch, layout):
    if layout == "hbm":
        monkeypatch.setenv("FOGNET_WINDOW_STATS", "hbm")
    else:
        monkeypatch.delenv("FOGNET_WINDOW_STATS", raising=False)


def device_replay(ctx, key, tr, policy="REF_V3", **kw):
    """(device trace, replay outputs) of a trace, replayed once per key and left unchanged."""
    if key not in _replays:
        d = fa.as_device_trace(tr, torch.device("cuda", ctx.device))
        _replays[key] = (d, fa.run_batch(ctx, d, policy=policy, **kw))
    return _replays[key]


def records(buf, R, W) -> np.ndarray:
    return buf.cpu().numpy().view(WINDOW).reshape(R, W)


def both_layouts(ctx, monkeypatch, d, out, who, uu, ud, t0, window, W, **kw):
    """The pass in both layouts: byte-identical records and counts; returns the default layout's."""
    R = d["arrive"].shape[0]
    got = {}
    for layout in LAYOUTS:
        set_layout(monkeypatch, layout)
        buf, outside, un = fa.window_stats(ctx, d, out, who, uu, ud, t0, window, W, **kw)
        got[layout] = (records(buf, R, W).copy(), outside.cpu().numpy().copy(), un.cpu().numpy().copy())
    for a, b in zip(got["lds"], got["hbm"]):
        assert a.tobytes() == b.tobytes()
    return got["lds"]


def check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, t0, window, W, what="", flags=None, up=0, **kw):
    want, outside_want, un_want = wr.expected(tr, o, who, uu, ud, t0, window, W, flags=flags, up=up)
    g, outside, un = both_layouts(ctx, monkeypatch, d, out, who, uu, ud, t0, window, W, **kw)
    wr.assert_records_equal(g, want, what)
    np.testing.assert_array_equal(outside, outside_want, err_msg=what)
    np.testing.assert_array_equal(un, un_want, err_msg=what)
    return g, outside, un


def handmade(ctx, arrive, node, status, start, done, dl, ul):
    """A replay's outputs written by hand ([1, T] rows over len(dl) nodes): (trace, o, device trace, out)."""
    dev = torch.device("cuda", ctx.device)
    T, N = len(arrive), len(dl)
    tr = dict(arrive=np.array([arrive], np.int64), req=np.ones((1, T), np.int32), mips=np.ones(N, np.int32),
              dl=np.array(dl, np.int64), ul=np.array(ul, np.int64), init=np.array(ul, np.int64))
    stats = np.zeros(1, REP)
    stats["n_tasks"] = T
    o = dict(node=np.array([node], np.int32), status=np.array([status], np.uint8), start=np.array([start], np.int64),
             done=np.array([done], np.int64), stats=stats)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = fa.BatchResult(t(o["node"]), t(o["status"]), t(o["start"]), t(o["done"]), t(stats.view(np.uint8)))
    return tr, o, fa.as_device_trace(tr, dev), out


# ---------------------------------------------------------------- parity over the shapes

@pytest.mark.parametrize("N", [1, 5, 300])
def test_parity_over_shapes_both_layouts(ctx, monkeypatch, N):
    """T around a wavefront step and past one workgroup round, U = 1, 3 and none, W = 1, 2, around
    the LDS limit and past one round of the scan; a covering range, every tick its own window,
    and one window longer than the run."""
    i = 0
    for ti, T in enumerate((1, 63, 65, 257)):
        tr, o = trace_case(N, T)
        assert (o["stats"]["status"] == 0).all()
        d, out = device_replay(ctx, ("trace", N, T), tr)
        for wi, W in enumerate((1, 2, LDS_CAP - 1, LDS_CAP, LDS_CAP + 1, 257)):
            U = (1, 3, 0)[(wi + ti) % 3]  # (over the four T every W meets every U)
            i += 1
            if U:
                who, (uu, ud) = draw_users(100 * T + W, 3, T, U, "rr"), draw_links(100 * T + W + 1, 3, U, i % 2 == 0)
            else:
                who = uu = ud = None
            last = wr.latest_tick(tr, o, who, uu, ud)
            window, _ = covering(last, W)
            g, outside, un = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, 0, window, W, f"N{N} T{T} W{W} U{U}")
            assert (outside == 0).all() and (g["n_publish"].sum(axis=1) == T).all()
            assert list(un) == ([0, 0, 0] if U else [T, T, T])
            ticks = wr.event_ticks(tr, o, who, uu, ud)
            check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, ticks[len(ticks) // 2] - W // 2, 1, W, "window_tick 1")
        g, _, _ = check(ctx, monkeypatch, d, out, tr, o, None, None, None, 0, 4 * wr.latest_tick(tr, o, None, None, None) + 1, 1,
                        "one long window")
        assert (g["n_complete"][:, 0] == (o["done"] >= 0).sum(axis=1)).all()


def test_events_on_the_edges_of_the_range(ctx, monkeypatch):
    """Window edges put on the restatement's own event ticks: an event exactly at t0 and at
    t0 - 1, at the last tick of the range and at its end."""
    tr, o, who, uu, ud, _, _ = oracle_case("tracegen")
    d, out = device_replay(ctx, "tracegen", tr)
    ticks = wr.event_ticks(tr, o, who, uu, ud)
    a, b = ticks[len(ticks) // 4], ticks[3 * len(ticks) // 4]
    seen = set()
    for t0, end in ((a, b), (a + 1, b + 1), (a, b + 1), (a + 1, b)):
        for W in (1, 3):
            window = (end - t0) // W
            t1 = end - W * window  # the range ends exactly at `end`
            _, outside, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, t1, window, W, f"[{t1}, {end}) W{W}")
            seen.add(tuple(outside[0]))
    assert len(seen) >= 3  # moving an edge by one tick moved events across it


def test_intervals_handmade(ctx, monkeypatch):
    """An interval ending exactly on a window edge and on the range's end, a zero-service task, a
    task over more than 256 windows, t0 > 0 cutting intervals on the left."""
    tr, o, d, out = handmade(ctx, [100, 200, 200, 1000, 1000], [0, 0, 0, 0, 0], [5, 4, 4, 5, 4],
                             [110, 300, 400, 1010, 1010], [300, 400, 400, 1010, 5000], [10], [5])
    g, outside, _ = check(ctx, monkeypatch, d, out, tr, o, None, None, None, 100, 100, 4, "edges")
    assert [int(x) for x in g[0]["busy_lo"]] == [90, 100, 100, 0] and list(outside[0]) == [0, 5]
    g, _, _ = check(ctx, monkeypatch, d, out, tr, o, None, None, None, 101, 1, 299, "every tick a window")
    assert set(g[0]["busy_lo"][9:].tolist()) == {1}
    g, _, _ = check(ctx, monkeypatch, d, out, tr, o, None, None, None, 250, 10, 400, "a task over 399 windows")  # [250, 4250)
    assert (g[0]["busy_lo"][76:] == 10).all() and int(g[0]["busy_lo"][75]) == 0  # [1010, 5000) cut at the range's end
    g, _, _ = check(ctx, monkeypatch, d, out, tr, o, None, None, None, 1000, 4000, 1, "ends on the range's end")
    assert int(g[0, 0]["busy_lo"]) == 3990 and int(g[0, 0]["insys_lo"]) == 3990
    who, uu, ud = np.array([[0, 1, 0, 1, 0]], np.int32), np.array([3, 7], np.int64), np.array([2, 90], np.int64)
    for t0, window, W in ((100, 100, 4), (0, 7, 257), (395, 5, 2), (0, 6000, 1)):
        check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, t0, window, W, "with users")


def test_large_ticks_and_128_bit_sums(ctx, monkeypatch):
    """Ticks near 2^56 with windows of 2^40 ticks, and windows of 2^59 ticks that 40 tasks cover
    whole: cover * window_tick passes 2^64."""
    base, w40 = 2**56, 2**40
    T = 70
    arrive = [base + 3 * w40 * i // 7 for i in range(T)]
    start = [a + 5 for a in arrive]
    done = [s + (i % 9) * w40 + (i % 4) * 12345 for i, s in enumerate(start)]
    tr, o, d, out = handmade(ctx, arrive, [i % 3 for i in range(T)], [5] * T, start, done, [1, 2, 3], [4, 5, 6])
    who, uu, ud = np.array([[i % 2 for i in range(T)]], np.int32), np.array([2**30, 5], np.int64), np.array([7, 2**31], np.int64)
    for t0, W in ((base - w40, 50), (base + 5 * w40 + 17, LDS_CAP + 4)):
        g, _, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, t0, w40, W, "2^56 / 2^40")
        assert int(g[0]["busy_lo"].max()) > w40
    w59 = 2**59
    T = 40
    arrive = [1000 + i for i in range(T)]
    tr, o, d, out = handmade(ctx, arrive, [0] * T, [5] * T, [a + 1 for a in arrive], [4 * w59 - 1 - i for i in range(T)], [1], [1])
    g, _, _ = check(ctx, monkeypatch, d, out, tr, o, None, None, None, 0, w59, 4, "2^59")
    assert int(g[0, 1]["busy_hi"]) == 40 * w59 >> 64 > 0 and int(g[0, 1]["busy_lo"]) == 40 * w59 & (2**64 - 1)


# ---------------------------------------------------------------- the other policies and replays

@pytest.mark.parametrize("name", ["ext_lat", "down", "ties", "herded", "carry", "mqtt"])
def test_oracle_cases(ctx, monkeypatch, name):
    tr, o, who, uu, ud, _, _ = oracle_case(name)
    d, out = device_replay(ctx, name, tr, "EXT_LAT" if name == "ext_lat" else "REF_V3")
    np.testing.assert_array_equal(out.done_tick.cpu().numpy(), o["done"])
    if name == "down":
        assert (o["status"] == 9).any() and ((o["start"] == -1) | (o["done"] == -1)).any()
    last = wr.latest_tick(tr, o, who, uu, ud)
    ticks = wr.event_ticks(tr, o, who, uu, ud)
    lost = 0
    for t0, window, W in ((0, *covering(last, 9)), (ticks[len(ticks) // 3], max((last - ticks[len(ticks) // 3]) // 300, 1), 130)):
        g, _, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, t0, window, W, name)
        lost += sum(int(g[s]["overflow"].sum()) for s in wr.SIGNALS)
    if name in ("carry", "herded"):
        assert lost > 0  # lost emissions, in the window of their time


def test_ext_hier_with_the_replays_flags_and_refused_without(ctx, monkeypatch):
    tr, _, _, o, _ = hier_case(0)
    T = tr["arrive"].shape[1]
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_batch(ctx, d, policy="EXT_HIER", hier_threshold_s=0, hier_up_tick=HIER_UP, escalated=True)
    flags = out.escalated.cpu().numpy()
    assert 0 < int(flags.sum()) < T
    who, (uu, ud) = draw_users(0xE, 1, T, 4, "rr"), draw_links(0xF, 1, 4, False)
    window, W = covering(wr.latest_tick(tr, o, who, uu, ud, flags, HIER_UP), 40)
    g, outside, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, 0, window, W, "hier", flags=flags, up=HIER_UP)
    flat, _, _ = wr.expected(tr, o, who, uu, ud, 0, window, W)
    assert (outside == 0).all() and g.tobytes() != flat.tobytes()  # the hop shows
    bare = fa.BatchResult(out.node, out.status, out.start_tick, out.done_tick, out.stats)
    for layout in LAYOUTS:
        set_layout(monkeypatch, layout)
        res = torch.full((W * WINDOW.itemsize,), 0xA5, dtype=torch.uint8, device=dev)
        cnt = torch.full((1, 2), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        un = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        with pytest.raises(fa.FognetError) as e:
            fa.window_stats(ctx, d, bare, who, uu, ud, 0, window, W, policy="EXT_HIER", hier_up_tick=HIER_UP, res=res,
                            n_outside=cnt, n_unassigned=un)
        assert e.value.code == _abi.FOGNET_ERR_UNSUPPORTED and "escalated" in str(e.value)
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == 0xA5).all() and (cnt.cpu().numpy() == 0x5A5A5A5A).all() and int(un[0]) == 0x5A5A5A5A


def test_assigned_replay_outputs(ctx, monkeypatch):
    tr, _ = trace_case(5, 191)
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_assigned(ctx, d, fa.assign_random(3, 191, 5, 7, dev))
    o = dict(node=out.node.cpu().numpy(), status=out.status.cpu().numpy(), start=out.start_tick.cpu().numpy(),
             done=out.done_tick.cpu().numpy(), stats=out.rep_stats())
    assert (o["stats"]["status"] == 0).all() and (o["status"] == 4).any()
    who, (uu, ud) = draw_users(5, 3, 191, 6, "random"), draw_links(6, 3, 6, True)
    window, W = covering(wr.latest_tick(tr, o, who, uu, ud), 33)
    g, outside, _ = check(ctx, monkeypatch, d, out, tr, o, who, uu, ud, 0, window, W, "assigned", policy="REF_V3")
    assert (outside == 0).all() and (g["n_publish"].sum(axis=1) == 191).all()


def test_good_failed_aborted_good(ctx, monkeypatch):
    """[good, failed, REF_ABORTED, good]: the failed one gets empty records and zero counts and
    nothing of it is read; the aborted one keeps its records; the reduction takes the good ones."""
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
    for W in (7, LDS_CAP + 1):
        window, _ = covering(wr.latest_tick(tr, dict(o, stats=st), who, uu, ud), W)
        want, outside_want, un_want = wr.expected(tr, o, who, uu, ud, 0, window, W, statuses=statuses)
        g, outside, un = both_layouts(ctx, monkeypatch, d, out, who, uu, ud, 0, window, W)
        wr.assert_records_equal(g, want)
        assert g[1].tobytes() == wr.empty_records(W).tobytes() and (outside == 0).all() and list(un) == [0, 0, 0, 0]
        assert int(g[2]["n_publish"].sum()) == 129
        buf, _, _ = fa.window_stats(ctx, d, out, who, uu, ud, 0, window, W)
        red = fa.reduce_window_stats(ctx, buf.reshape(-1), out.stats, 4, W)
        wr.assert_records_equal(red, wr.to_records([wr.merged(want[[0, 3], w]) for w in range(W)]))


# ---------------------------------------------------------------- argument errors, empty shapes

def test_argument_errors_and_empty_shapes(ctx):
    dev = torch.device("cuda", ctx.device)
    tr, o = trace_case(5, 65)
    d, out = device_replay(ctx, ("trace", 5, 65), tr)
    who = torch.from_numpy(draw_users(1, 3, 65, 4, "rr")).to(dev)
    uu, ud = (torch.from_numpy(x).to(dev) for x in draw_links(2, 3, 4, False))
    so = fa.run_batch(ctx, d, out=fa.allocate_outputs(3, 65, dev, per_task=False))
    with pytest.raises(fa.FognetError) as e:
        fa.window_stats(ctx, d, so, who, uu, ud, 0, 10**12, 4)  # a statistics-only out
    assert e.value.code == _abi.FOGNET_ERR_ARG
    p = fa.engine._ptr
    bi = _abi.BatchIn(3, 65, 5, 1, 5, 0, *(p(d[k]) for k in ("arrive", "req", "mips", "dl", "ul", "init")))
    outs = dict(node=out.node, status=out.status, start_tick=out.start_tick, done_tick=out.done_tick, stats=out.stats)
    W = 4
    res = torch.full((3 * W * WINDOW.itemsize,), 0xA5, dtype=torch.uint8, device=dev)
    cnt = torch.full((3, 2), -7, dtype=torch.int64, device=dev)
    un = torch.full((3,), -7, dtype=torch.int64, device=dev)
    window = wr.latest_tick(tr, o, None, None, None) // W + 1

    def call(user_of=p(who), U=4, stride=0, ul=p(uu), dl=p(ud), t0=0, window=window, W=W, win=p(res), outside=p(cnt),
             unassigned=p(un), drop=None):
        bo = _abi.BatchOut(**{k: p(v) for k, v in outs.items() if k != drop})
        return ctx._lib.fognet_window_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), user_of, U, stride, ul, dl, t0, window, W,
                                                win, outside, unassigned, None)
    for bad in (dict(win=None), dict(user_of=None), dict(ul=None), dict(dl=None), dict(U=-1), dict(stride=3), dict(stride=5),
                dict(window=0), dict(window=-5), dict(t0=-1), dict(W=-1), dict(drop="start_tick"), dict(drop="node"),
                dict(t0=2**62 - W * window + 1), dict(window=2**62 // W + 1), dict(t0=2**62, window=1, W=1)):
        assert call(**bad) == _abi.FOGNET_ERR_ARG, bad
    assert call(W=2**20 + 1, window=1) == _abi.FOGNET_ERR_UNSUPPORTED and b"1048576" in ctx._lib.fognet_last_error(ctx.handle)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == 0xA5).all() and (cnt.cpu().numpy() == -7).all() and (un.cpu().numpy() == -7).all()
    assert call(t0=2**62 - W * window) == _abi.FOGNET_OK  # the range may end exactly at 2^62
    # U = 0 with NULL users: the node side alone, every decided publish unassigned
    assert call(user_of=None, U=0, ul=None, dl=None) == _abi.FOGNET_OK
    torch.cuda.synchronize()
    want, outside_want, _ = wr.expected(tr, o, None, None, None, 0, window, W)
    wr.assert_records_equal(records(res, 3, W), want)
    assert list(un.cpu().numpy()) == [65, 65, 65] and (cnt.cpu().numpy() == outside_want).all()
    # W = 0 writes only the counts; both are optional
    res.fill_(0xA5)
    assert call(W=0, win=None) == _abi.FOGNET_OK and call(outside=None, unassigned=None) == _abi.FOGNET_OK
    torch.cuda.synchronize()
    _, outside_want, un_want = wr.expected(tr, o, who.cpu().numpy(), uu.cpu().numpy(), ud.cpu().numpy(), 0, window, 0)
    assert (cnt.cpu().numpy() == outside_want).all() and (cnt.cpu().numpy()[:, 0] == 0).all() and (cnt.cpu().numpy()[:, 1] > 65).all()
    want, _, _ = wr.expected(tr, o, who.cpu().numpy(), uu.cpu().numpy(), ud.cpu().numpy(), 0, window, W)
    wr.assert_records_equal(records(res, 3, W), want)
    # T = 0: only empty records; R = 0: nothing
    t0 = {k: (v[:, :0] if k in ("arrive", "req") else v) for k, v in tr.items()}
    d0 = fa.as_device_trace(t0, dev)
    buf, outside, un0 = fa.window_stats(ctx, d0, fa.run_batch(ctx, d0), np.zeros((3, 0), np.int32), uu, ud, 0, 5, 3)
    assert records(buf, 3, 3).tobytes() == np.stack([wr.empty_records(3)] * 3).tobytes()
    assert not outside.cpu().numpy().any() and not un0.cpu().numpy().any()
    empty = fa.as_device_trace({k: v[:0] for k, v in tr.items()}, dev)
    buf, outside, un0 = fa.window_stats(ctx, empty, fa.allocate_outputs(0, 65, dev), np.zeros((0, 65), np.int32), uu, ud, 0, 5, 3)
    assert buf.numel() == 0 and outside.numel() == 0 and un0.numel() == 0


# ---------------------------------------------------------------- the device's own vectors and records

@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
def test_windows_hold_the_devices_own_vectors_and_records(ctx, monkeypatch, policy):
    """fognet_signal_vectors_dev's rows binned on the host give each window's count, extrema and
    sums; the merged windows of a covering range give fognet_node_stats_dev's queue and
    fognet_per_user_stats_dev's four signals, and 10^12 * busy_s."""
    tr, o = trace_case(5, 191, policy)
    d, out = device_replay(ctx, ("trace", 5, 191, policy), tr, policy)
    who, (uu, ud) = draw_users(21, 3, 191, 7, "random"), draw_links(22, 3, 7, True)
    N, U = 5, 7
    last = wr.latest_tick(tr, o, who, uu, ud)
    vec = fa.signal_vectors(ctx, d, out, who, uu, ud, policy=policy)
    nodes = fa.node_stats(ctx, d, out, policy=policy).cpu().numpy().view(_abi.NODE_STATS_DTYPE).reshape(3, N)
    users = fa.per_user_stats(ctx, d, out, who, uu, ud, policy=policy)[0].cpu().numpy().view(_abi.USER_STATS_DTYPE).reshape(3, U)
    for W in (11, LDS_CAP + 40):
        window, _ = covering(last, W)
        g, outside, _ = both_layouts(ctx, monkeypatch, d, out, who, uu, ud, 0, window, W, policy=policy)
        assert (outside == 0).all()
        for r in range(3):
            off = vec["offset"][r]
            rows = [[(None, int(vec["time"][r][p]), int(vec["value"][r][p]), int(vec["task"][r][p]), None)
                     for p in range(int(off[v]), int(off[v + 1]))] for v in range(N + 1 + 3 * U)]
            wr.assert_signals_match_rows(g[r], wr.binned(rows, N, U, 0, window, W))
            m = wr.merged(g[r])
            nm, um = ns.merged(nodes[r]), pu.merged(users[r])
            assert wr.to_records([m])[0]["queue"].tobytes() == ns.to_records([nm])[0]["queue"].tobytes()
            for s in us.SIGNALS:
                assert wr.to_records([m])[0][s].tobytes() == um[s].tobytes(), (r, s)
            assert m.busy == 10**12 * nm.busy and m.n_publish == nm.tasks and m.n_complete == nm.resp.n


# ---------------------------------------------------------------- reduction

@pytest.mark.parametrize("R", [0, 3, 130])
def test_reduction_equals_the_host_merge(ctx, R):
    W = 5
    rng = random.Random(1000 + R)
    recs = random_records(rng, R, W)
    stats = np.zeros(R, REP)
    stats["status"] = [rng.choice((0, 0, 0, _abi.FOGNET_REF_ABORTED, _abi.FOGNET_ERR_ARG)) for _ in range(R)]
    for r in (1, 127, 128, 129):
        if r < R:
            stats["status"][r] = (_abi.FOGNET_ERR_CAPACITY, _abi.FOGNET_REF_ABORTED, 0)[r % 3]
    dev = torch.device("cuda", ctx.device)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    got = fa.reduce_window_stats(ctx, to_dev(recs), to_dev(stats), R, W)
    ok = [r for r in range(R) if stats["status"][r] == 0]
    assert got.tobytes() == fa.merge_window_stats([wr.empty_records(W)] + [recs[r] for r in ok]).tobytes()
    wr.assert_records_equal(got, wr.to_records([wr.merged(recs[ok, w], wrap=True) for w in range(W)]))
    if R >= 2:  # the host merge of two shards
        half = [fa.reduce_window_stats(ctx, to_dev(recs[s]), to_dev(stats[s]), len(stats[s]), W)
                for s in (slice(0, R // 2), slice(R // 2, R))]
        assert fa.merge_window_stats(half).tobytes() == got.tobytes()


# ---------------------------------------------------------------- buffer contract, streams

def guarded_run(ctx, tr, who, uu, ud, window, W, poison, misalign):
    dev = torch.device("cuda", ctx.device)
    ain, aout = Arena(dev, poison), Arena(dev, poison)
    d = {k: ain.put(v, misalign, name=k) for k, v in tr.items()}
    g_who, g_uu, g_ud = ain.put(who, misalign, "user_of"), ain.put(uu, misalign, "user_ul"), ain.put(ud, misalign, "user_dl")
    R, T = d["arrive"].shape
    rec = lambda n, dt, name: aout.alloc(n * dt.itemsize // 8, torch.int64, misalign, name=name).view(torch.uint8)
    out = fa.BatchResult(node=aout.alloc((R, T), torch.int32, misalign, "node"), status=aout.alloc((R, T), torch.uint8, misalign, "status"),
                         start_tick=aout.alloc((R, T), torch.int64, misalign, "start"),
                         done_tick=aout.alloc((R, T), torch.int64, misalign, "done"), stats=rec(R, REP, "stats"))
    fa.run_batch(ctx, d, out=out)
    win, job = rec(R * W, WINDOW, "win"), rec(W, WINDOW, "job_windows")
    outside, un = aout.alloc((R, 2), torch.int64, misalign, "n_outside"), aout.alloc((R,), torch.int64, misalign, "n_unassigned")
    if misalign:
        assert g_who.data_ptr() % 8 == 4 and win.data_ptr() % 16 == 8  # natural alignment only
    fa.window_stats(ctx, d, out, g_who, g_uu, g_ud, 0, window, W, res=win, n_outside=outside, n_unassigned=un)
    red = fa.reduce_window_stats(ctx, win, out.stats, R, W, out=job)
    torch.cuda.synchronize()
    ain.check()
    aout.check()
    return records(win, R, W).copy(), outside.cpu().numpy().copy(), un.cpu().numpy().copy(), red.copy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T,W", [(65, 3), (191, LDS_CAP + 1)])
def test_buffer_contract(ctx, monkeypatch, layout, T, W):
    """Guard bands around every array, two poisons, and pointers at their natural alignment only."""
    set_layout(monkeypatch, layout)
    tr, o = trace_case(5, T)
    who = draw_users(T + W, 3, T, 4, "random")
    who[1, T // 2] = 4  # one past the last user
    uu, ud = draw_links(T + W + 1, 3, 4, True)
    window = (wr.latest_tick(tr, o, who, uu, ud) // 2) // W + 1  # the second half lies past the range
    want, outside_want, un_want = wr.expected(tr, o, who, uu, ud, 0, window, W)
    assert (outside_want[:, 1] > 0).all()
    runs = [guarded_run(ctx, tr, who, uu, ud, window, W, p, m) for p, m in ((0xA5, False), (0x5A, False), (0xA5, True))]
    for g, outside, un, red in runs:
        wr.assert_records_equal(g, want, layout)
        assert (outside == outside_want).all() and list(un) == list(un_want) == [0, 1, 0]
        wr.assert_records_equal(red, wr.to_records([wr.merged(want[:, w]) for w in range(W)]), "reduction")


@pytest.mark.parametrize("W", [9, LDS_CAP + 1])
def test_gated_on_a_side_stream(ctx, tmp_path, monkeypatch, W):
    """The pass and its reduction behind a gate on a side stream: only enqueued, and they read
    the inputs that the stream's own copies put there."""
    monkeypatch.setenv(stream_gate.REPORT_ENV, str(tmp_path / "gate.json"))
    dev = torch.device("cuda", ctx.device)
    tr, o = trace_case(5, 65)
    decoy = tg.make_batch(0xDEC0, 3, 5, 65, rho=0.9)
    who, (uu, ud) = draw_users(31, 3, 65, 4, "rr"), draw_links(32, 3, 4, True)
    window, _ = covering(wr.latest_tick(tr, o, who, uu, ud), W)
    want, outside_want, _ = wr.expected(tr, o, who, uu, ud, 0, window, W)
    names = ("arrive", "req", "mips", "dl", "ul", "init")
    fa.window_stats(ctx, fa.as_device_trace(tr, dev), fa.run_batch(ctx, fa.as_device_trace(tr, dev)), who, uu, ud, 0, window, W)
    torch.cuda.synchronize()  # (the workspace has grown)

    class Job:
        def __init__(self):
            self.d = fa.as_device_trace(tr, dev)
            self.who, self.uu, self.ud = (torch.from_numpy(x).to(dev) for x in (who, uu, ud))
            self.inputs = dict({k: self.d[k] for k in names}, user_of=self.who, user_ul=self.uu, user_dl=self.ud)
            self.out = fa.allocate_outputs(3, 65, dev)
            self.win = torch.empty(3 * W * WINDOW.itemsize, dtype=torch.uint8, device=dev)
            self.red = torch.empty(W * WINDOW.itemsize, dtype=torch.uint8, device=dev)
            self.outside = torch.empty((3, 2), dtype=torch.int64, device=dev)
            self.un = torch.empty(3, dtype=torch.int64, device=dev)

    def enqueue(job):
        fa.run_batch(ctx, job.d, out=job.out)
        fa.window_stats(ctx, job.d, job.out, job.who, job.uu, job.ud, 0, window, W, res=job.win, n_outside=job.outside,
                        n_unassigned=job.un)
        ctx.check(ctx._lib.fognet_reduce_window_stats_dev(ctx.handle, C.c_void_p(job.win.data_ptr()),
                                                          C.c_void_p(job.out.stats.data_ptr()), 3, W,
                                                          C.c_void_p(job.red.data_ptr()),
                                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "reduction")

    gate = stream_gate.Gate(dev)
    gate.choose(1)
    kinds = dict(arrive=np.int64, req=np.int32, mips=np.int32, dl=np.int64, ul=np.int64, init=np.int64)
    decoys = dict({k: np.ascontiguousarray(decoy[k], dtype=kinds[k]) for k in names}, user_of=(who + 1) % 4,
                  user_ul=uu + 1000, user_dl=ud + 1000)
    job = gate.run("windows", f"windows-W{W}", Job, decoys, enqueue)
    wr.assert_records_equal(records(job.win, 3, W), want, "gated")
    assert (job.outside.cpu().numpy() == outside_want).all() and not job.un.cpu().numpy().any()
    wr.assert_records_equal(job.red.cpu().numpy().view(WINDOW), wr.to_records([wr.merged(want[:, w]) for w in range(W)]))


# ---------------------------------------------------------------- the driver

@pytest.mark.parametrize("extra", [(), ("--vec-users",), ("--assign", "rr")])
def test_driver_windows_vectors(ctx, tmp_path, extra):
    """fognet_replay --vec f --windows DT appends the job's fourteen window vectors after whatever
    --vec / --vec-users wrote: the file parses, the ids follow on, and the counts sum to the job's
    (regenerated through fognet_gen_trace_mqtt with the driver's seeds and the oracle)."""
    from fognetsimpp_amd import formats
    from test_driver import INI, MS, SEC, drive
    a, b, trc = (str(tmp_path / n) for n in ("a.vec", "b.vec", "g.fogntrc"))
    args = ("-f", INI, "--users", "user[3]", "--reps", "4", *extra)
    p = drive(*args, "--vec", a, "--windows", "25s", "--trace-out", trc)
    drive(*args, "--vec", b)
    plain, text = open(b, "rb").read(), open(a, "rb").read()
    assert text.startswith(plain) and text.count(b"version 2") == 1 and b":window" not in plain
    decl, rows = parse_vec(text[len(plain):].decode())
    tr = formats.load_trace(trc)
    tr = {k: tr[k] for k in ("arrive", "req", "mips", "dl", "ul", "init")}
    N = np.shape(tr["mips"])[-1]
    first = N + 1 + (10 if "--vec-users" in extra else 0)  # after the decisions, the nodes and the user-side vectors
    assert sorted(decl) == list(range(first, first + 14))
    name = {v[1]: k for k, v in decl.items()}
    assert decl[first] == ("FogNet5.fogNodes.udpApp[0]", "utilisation:window")
    W = 12  # ceil(300 s / 25 s)
    assert "windows=12" in p.stdout and "events_before=0 events_after=" in p.stdout
    assert [t for t, _ in rows[name["publishes:window"]]] == [str(25 * (w + 1)) for w in range(W)]
    publishes = sum(int(x) for _, x in rows[name["publishes:window"]])
    after = int(p.stdout.split("events_after=")[1].split()[0])
    assert publishes == tr["arrive"].size  # every publish arrives before the stop time
    if "--assign" in extra:
        return
    gens = [formats.gen_trace_mqtt(1 + r, [200 * MS] * 3, [1500 * MS] * 3, [MS] * 3, [MS] * 3, 300 * SEC) for r in range(4)]
    who = np.stack([g["user"] for g in gens]).astype(np.int32)
    links = np.full(3, MS, np.int64)  # --user-ul / --user-dl defaults
    o = replay_oracle(tr)
    assert (o["stats"]["status"] == 0).all()
    want, outside, un = wr.expected(tr, o, who, links, links, 0, 25 * SEC, W)
    job = [wr.merged(want[:, w]) for w in range(W)]
    assert int(outside[:, 1].sum()) == after and not outside[:, 0].any() and not un.any()
    assert [int(x) for _, x in rows[name["publishes:window"]]] == [j.n_publish for j in job]
    assert [int(x) for _, x in rows[name["completions:window"]]] == [j.n_complete for j in job]
    for sig, vname in (("queue", "queueTime"), ("delay", "delay"), ("latency", "latency"), ("latencyH1", "latencyH1"),
                       ("taskTime", "taskTime")):
        assert [int(x) for _, x in rows[name[vname + ":window(count)"]]] == [j.sig[sig].n for j in job], sig
        means = [j.sig[sig].s / j.sig[sig].n * 1e-12 for j in job if j.sig[sig].n]
        assert [float(x) for _, x in rows[name[vname + ":window(mean)"]]] == pytest.approx(means, rel=1e-13)
    util = [float(x) for _, x in rows[name["utilisation:window"]]]
    # (the scenario's requirements lie below every node's MIPS: whole service seconds of 0, so both averages are 0)
    assert util == pytest.approx([j.busy / (N * 25 * SEC * 4) for j in job], rel=1e-13)
    insys = [float(x) for _, x in rows[name["tasksInSystem:window"]]]
    assert insys == pytest.approx([j.insys / (25 * SEC * 4) for j in job], rel=1e-13)
