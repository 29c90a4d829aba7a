"""Per-user signals on the device (fognet_per_user_stats_dev, fognet_reduce_user_stats_dev)
against records built in Python integers from the ORACLE's per-task outputs (per_user_ref),
in both accumulator layouts (LDS; FOGNET_USER_STATS=hbm), and the defining invariant
against the device's own fognet_user_stats_dev with per-task links.  The cases and their
references come from test_per_user_stats.py, which checks them against the oracle's
events without a GPU."""
from __future__ import annotations

import random

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import per_user_ref as pu
import tracegen as tg
import user_stats_ref as us
from fognetsimpp_amd import _abi, formats
from guarded import Arena
from test_per_user_stats import (carry_case, down_trace, draw_links, draw_users, grouping_trace, mqtt_case,
                                 random_records, replay_oracle, staircase_users, trace_case)
from test_user_stats import HIER_UP, abort_case, hier_case

pytestmark = pytest.mark.gpu

USER, REP = _abi.USER_STATS_DTYPE, _abi.REP_STATS_DTYPE
LDS_CAP = 128  # per_user_stats.hip kUserLdsMax: U = 129 is the first size above it
LAYOUTS = ("lds", "hbm")
I32_MAX = 2**31 - 1
_replays: dict = {}


def set_layout(monkeypatch, layout):
    if layout == "hbm":
        monkeypatch.setenv("FOGNET_USER_STATS", "hbm")
    else:
        monkeypatch.delenv("FOGNET_USER_STATS", raising=False)


def device_replay(ctx, key, tr, policy="REF_V3", **kw):
    """(device trace, replay outputs) of a trace, replayed once per key and left unchanged."""
    if key is None or key not in _replays:
        d = fa.as_device_trace(tr, torch.device("cuda", ctx.device))
        got = (d, fa.run_batch(ctx, d, policy=policy, **kw))
        if key is None:
            return got
        _replays[key] = got
    return _replays[key]


def records(buf, R, U) -> np.ndarray:
    return buf.cpu().numpy().view(USER).reshape(R, U)


def both_layouts(ctx, monkeypatch, d, out, who, uu, ud, **kw):
    """The pass in both layouts: byte-identical records and counts; returns the LDS ones."""
    R, U = d["arrive"].shape[0], np.shape(uu)[-1]
    got = {}
    for layout in LAYOUTS:
        set_layout(monkeypatch, layout)
        buf, un = fa.per_user_stats(ctx, d, out, who, uu, ud, **kw)
        got[layout] = (records(buf, R, U).copy(), un.cpu().numpy().copy())
    assert got["lds"][0].tobytes() == got["hbm"][0].tobytes() and (got["lds"][1] == got["hbm"][1]).all()
    return got["lds"]


def assert_merge_invariant(ctx, d, out, g, who, uu, ud, **kw):
    """Every OK replication's U records merge, bit for bit, to the device's own
    fognet_user_stats_dev(user_per_task = 1) record with the links expanded from user_of."""
    tu, td = pu.expand_links(who, uu, ud)
    whole = fa.user_stats(ctx, d, out, tu, td, **kw)
    st = out.rep_stats()["status"]
    for r in range(g.shape[0]):
        if int(st[r]) in us.OK_STATUSES:
            assert pu.merged(g[r]).tobytes() == whole[r].tobytes(), r


def check(ctx, monkeypatch, key, tr, o, who, uu, ud, policy="REF_V3", **kw):
    """Both layouts equal the helper's records on the oracle's outputs, and merge to the
    device's own whole-replication record."""
    d, out = device_replay(ctx, key, tr, policy, **kw)
    want, un_want = pu.expected(tr, o, who, uu, ud)
    g, un = both_layouts(ctx, monkeypatch, d, out, who, uu, ud)
    pu.assert_records_equal(g, want, str(key))
    np.testing.assert_array_equal(un, un_want)
    assert_merge_invariant(ctx, d, out, g, who, uu, ud)
    return g, want


# ---------------------------------------------------------------- parity, invariant

@pytest.mark.parametrize("N", [5, 300])  # register kernel / wide-kernel rows
@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
@pytest.mark.parametrize("U", [1, 2, 10, 64, 65, 128, LDS_CAP + 1])
def test_parity_with_oracle_both_layouts(ctx, monkeypatch, U, policy, N):
    for T in (1, 63, 64, 65, 129, 191):
        tr, o = trace_case(N, T, policy)
        assert (o["stats"]["status"] == 0).all()
        for per_rep in (False, True):
            for kind in ("random", "rr"):
                who = draw_users(1000 * U + T, 3, T, U, kind)
                uu, ud = draw_links(1000 * U + T + 1, 3, U, per_rep)
                g, want = check(ctx, monkeypatch, ("trace", N, T, policy), tr, o, who, uu, ud, policy)
                if U > 1 and kind == "random":  # the last user has no publish
                    assert all(us.is_empty(g[r, U - 1]) for r in range(3))
                assert (g["delay"]["count"].sum(axis=1) == T).all()


@pytest.mark.parametrize("U", [3, 10])
def test_reference_task_source_users(ctx, monkeypatch, U):
    tr, who, uu, ud = mqtt_case(U)
    o = replay_oracle(tr)
    check(ctx, monkeypatch, ("mqtt", U), tr, o, who, uu, ud)


# ---------------------------------------------------------------- grouping

def test_grouping_staircase_one_user_and_one_task_each(ctx, monkeypatch):
    """Group sizes 1 .. 10 in one 64-task step (any summing threshold up to 10 is crossed),
    all 192 tasks on one user of five (every step one summed group), and 64 users with one
    task each per step (no group)."""
    tr = grouping_trace(64)
    o = replay_oracle(tr)
    who = staircase_users()
    assert sorted(np.bincount(who[0]).tolist()) == sorted(list(range(1, 11)) + [9])
    check(ctx, monkeypatch, "stair", tr, o, who, *draw_links(5, 1, 11, False))
    tr = grouping_trace(192)
    o = replay_oracle(tr)
    g, _ = check(ctx, monkeypatch, "g192", tr, o, np.full((1, 192), 3, np.int32), *draw_links(6, 1, 5, False))
    assert [int(c) for c in g[0]["delay"]["count"]] == [0, 0, 0, 192, 0]
    who = np.stack([np.random.default_rng(c).permutation(64) for c in range(3)]).reshape(1, 192).astype(np.int32)
    g, _ = check(ctx, monkeypatch, "g192", tr, o, who, *draw_links(7, 1, 64, True))
    assert (g[0]["delay"]["count"] == 3).all()


# ---------------------------------------------------------------- carries and the emission rule

def test_carries_and_lost_emissions(ctx, monkeypatch):
    tr, who, uu, ud = carry_case()
    o = replay_oracle(tr)
    want, _ = pu.expected(tr, o, who, uu, ud)
    h1 = want[0, 0]["latencyH1"]
    assert int(h1["count"]) >= 8 and int(h1["min_raw"]) >= 2**62
    assert int(h1["sum_hi"]) != 0 and int(h1["sq_hi"]) != 0 and int(h1["sq_top"]) != 0
    assert sum(int(want[0, u][s]["overflow"]) for u in range(7) for s in us.SIGNALS) > 0
    assert int(want[0, 4]["latencyH1"]["overflow"]) > 0 and int(want[0, 6]["latencyH1"]["overflow"]) > 0
    check(ctx, monkeypatch, "carry", tr, o, who, uu, ud)


# ---------------------------------------------------------------- node-down

def test_node_down(ctx, monkeypatch):
    tr = down_trace()
    o = replay_oracle(tr)
    assert (o["status"] == 9).any() and ((o["status"] != 9) & (o["done"] == -1)).any()
    who = draw_users(0xD0, 3, 257, 10, "rr")
    uu, ud = draw_links(0xD1, 3, 10, True)
    g, want = check(ctx, monkeypatch, "down", tr, o, who, uu, ud)
    np.testing.assert_array_equal(g["taskTime"]["count"].sum(axis=1), (o["done"] >= 0).sum(axis=1))
    acks = (g["latency"]["count"] + g["latencyH1"]["count"]).sum(axis=1) - 257
    np.testing.assert_array_equal(acks, 257 - (o["status"] == 9).sum(axis=1))


# ---------------------------------------------------------------- failed, refused, aborted

def failed_trace():
    tr = {k: v.copy() for k, v in tg.make_batch(0xFA12, 5, 20, 191, rho=0.9).items()}
    tr["mips"][1, 0] = 0                                  # refused before its first decision
    tr["arrive"][3, 127] = tr["arrive"][3, 126] - 1       # fails in mid-trace
    return tr


@pytest.mark.parametrize("U", [10, LDS_CAP + 1])
def test_failed_replications_get_empty_rows_and_nothing_of_them_is_read(ctx, monkeypatch, U):
    """The oracle refuses replication 1 (MIPS 0) and replays replication 3's out-of-order
    publish as it comes; the library refuses that too (FOGNET_ERR_ARG), so both rows are
    expected empty.  Their user_of rows hold INT32_MAX and their link rows a poison."""
    tr = failed_trace()
    o = replay_oracle(tr)
    assert int(o["stats"]["status"][1]) not in us.OK_STATUSES and int(o["stats"]["n_tasks"][1]) == 0
    statuses = [0, int(o["stats"]["status"][1]), 0, _abi.FOGNET_ERR_ARG, 0]
    who = draw_users(9, 5, 191, U, "rr")
    uu, ud = draw_links(10, 5, U, True)
    who[[1, 3]] = I32_MAX
    uu[[1, 3]] = ud[[1, 3]] = 0x5A5A5A5A5A5A5A5A
    want, un_want = pu.expected(tr, o, who, uu, ud, statuses=statuses)
    d, out = device_replay(ctx, "failed", tr)
    st = out.rep_stats()
    assert [int(s) in us.OK_STATUSES for s in st["status"]] == [True, False, True, False, True]
    assert int(st["n_tasks"][1]) == 0 and 0 < int(st["n_tasks"][3]) < 191  # before its first decision; in mid-trace
    g, un = both_layouts(ctx, monkeypatch, d, out, who, uu, ud)
    pu.assert_records_equal(g, want)
    assert g[1].tobytes() == pu.empty_records(U).tobytes() == g[3].tobytes()
    assert list(un) == [0, 0, 0, 0, 0] == list(un_want)
    assert (g[[0, 2, 4]]["delay"]["count"].sum(axis=1) == 191).all()
    # the reduction leaves the failed ones out
    set_layout(monkeypatch, "lds")
    buf, _ = fa.per_user_stats(ctx, d, out, who, uu, ud)
    red = fa.reduce_user_stats(ctx, buf.reshape(-1), out.stats, 5, U)
    pu.assert_records_equal(red, np.array([pu.merged(want[[0, 2, 4], u]) for u in range(U)], USER))


def test_ref_aborted_replication_keeps_its_records_and_is_left_out_of_the_reduction(ctx, monkeypatch):
    tr, _, _, o, _ = abort_case()
    who = np.array([[0, 1, 2, 0, 1]], np.int32)
    uu, ud = draw_links(3, 1, 3, False)
    d, out = device_replay(ctx, None, tr, ref_abort=True)
    assert int(out.rep_stats()["status"][0]) == _abi.FOGNET_REF_ABORTED
    want, _ = pu.expected(tr, o, who, uu, ud)  # the oracle's full run
    g, un = both_layouts(ctx, monkeypatch, d, out, who, uu, ud)
    pu.assert_records_equal(g, want)
    assert int(g[0]["taskTime"]["overflow"].sum()) > 0 and int(un[0]) == 0
    assert_merge_invariant(ctx, d, out, g, who, uu, ud)
    buf, _ = fa.per_user_stats(ctx, d, out, who, uu, ud)
    red = fa.reduce_user_stats(ctx, buf.reshape(-1), out.stats, 1, 3)
    assert red.tobytes() == pu.empty_records(3).tobytes()


# ---------------------------------------------------------------- out-of-range users

@pytest.mark.parametrize("U", [4, LDS_CAP + 1])
def test_out_of_range_users_are_counted_and_left_out(ctx, monkeypatch, U):
    tr, o = trace_case(5, 65)
    who = draw_users(1, 3, 65, U, "rr")
    who[0, [3, 17, 64]] = (-1, U, I32_MAX)
    who[2, 0] = -(2**31)
    uu, ud = draw_links(2, 3, U, False)
    want, un_want = pu.expected(tr, o, who, uu, ud)
    assert list(un_want) == [3, 0, 1]
    d, out = device_replay(ctx, ("trace", 5, 65, "REF_V3"), tr)
    g, un = both_layouts(ctx, monkeypatch, d, out, who, uu, ud, allow_unassigned=True)
    pu.assert_records_equal(g, want)
    assert list(un) == [3, 0, 1] and [int(x) for x in g["delay"]["count"].sum(axis=1)] == [62, 65, 64]
    with pytest.raises(fa.FognetError) as e:
        fa.per_user_stats(ctx, d, out, who, uu, ud)
    assert e.value.code == _abi.FOGNET_ERR_ARG and "4 decided publishes" in str(e.value)


# ---------------------------------------------------------------- EXT_HIER

def test_ext_hier_with_the_replays_flags_and_refused_without(ctx, monkeypatch):
    tr, _, _, o, _ = hier_case(0)
    T = tr["arrive"].shape[1]
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_batch(ctx, d, policy="EXT_HIER", hier_threshold_s=0, hier_up_tick=HIER_UP, escalated=True)
    np.testing.assert_array_equal(out.node.cpu().numpy(), o["node"])
    flags = out.escalated.cpu().numpy()
    assert 0 < int(flags.sum()) < T  # some tasks escalate
    who = draw_users(0xE, 1, T, 4, "rr")
    uu, ud = draw_links(0xF, 1, 4, False)
    want, _ = pu.expected(tr, o, who, uu, ud, flags=flags, up=HIER_UP)
    flat, _ = pu.expected(tr, o, who, uu, ud)
    assert want.tobytes() != flat.tobytes()  # the hop shows
    g, un = both_layouts(ctx, monkeypatch, d, out, who, uu, ud)  # (policy and hop: what run_batch recorded)
    pu.assert_records_equal(g, want)
    assert_merge_invariant(ctx, d, out, g, who, uu, ud)
    bare = fa.BatchResult(out.node, out.status, out.start_tick, out.done_tick, out.stats)
    for layout in LAYOUTS:
        set_layout(monkeypatch, layout)
        res = torch.full((4 * USER.itemsize,), 0xA5, dtype=torch.uint8, device=dev)
        cnt = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        with pytest.raises(fa.FognetError) as e:
            fa.per_user_stats(ctx, d, bare, who, uu, ud, policy="EXT_HIER", hier_up_tick=HIER_UP, res=res, n_unassigned=cnt)
        assert e.value.code == _abi.FOGNET_ERR_UNSUPPORTED and "escalated" in str(e.value)
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == 0xA5).all() and int(cnt[0]) == 0x5A5A5A5A  # nothing written


# ---------------------------------------------------------------- argument errors, empty shapes

def test_argument_errors_and_empty_shapes(ctx):
    import ctypes as C
    dev = torch.device("cuda", ctx.device)
    tr, o = trace_case(5, 65)
    d, out = device_replay(ctx, ("trace", 5, 65, "REF_V3"), tr)
    who = torch.from_numpy(draw_users(1, 3, 65, 4, "rr")).to(dev)
    uu, ud = (torch.from_numpy(x).to(dev) for x in draw_links(2, 3, 4, False))
    so = fa.run_batch(ctx, d, out=fa.allocate_outputs(3, 65, dev, per_task=False))
    with pytest.raises(fa.FognetError) as e:
        fa.per_user_stats(ctx, d, so, who, uu, ud)  # a statistics-only out
    assert e.value.code == _abi.FOGNET_ERR_ARG
    p = fa.engine._ptr
    bi = _abi.BatchIn(3, 65, 5, 1, 5, 0, *(p(d[k]) for k in ("arrive", "req", "mips", "dl", "ul", "init")))
    bo = _abi.BatchOut(*(p(t) for t in (out.node, out.status, out.start_tick, out.done_tick, out.stats)))
    res = torch.full((3 * 4 * USER.itemsize,), 0xA5, dtype=torch.uint8, device=dev)
    un = torch.full((3,), -7, dtype=torch.int64, device=dev)

    def call(user_of=p(who), U=4, stride=0, ul=p(uu), dl=p(ud), per_user=p(res), cnt=p(un)):
        return ctx._lib.fognet_per_user_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), user_of, U, stride, ul, dl,
                                                  per_user, cnt, None)
    for bad in (dict(per_user=None), dict(user_of=None), dict(ul=None), dict(dl=None), dict(U=-1), dict(stride=3),
                dict(stride=5)):
        assert call(**bad) == _abi.FOGNET_ERR_ARG, bad
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == 0xA5).all() and (un.cpu().numpy() == -7).all()
    # U = 0 writes nothing but n_unassigned: every decided publish is unassigned
    assert call(U=0, ul=None, dl=None, per_user=None) == _abi.FOGNET_OK
    torch.cuda.synchronize()
    assert list(un.cpu().numpy()) == [65, 65, 65] and (res.cpu().numpy() == 0xA5).all()
    assert call(cnt=None) == _abi.FOGNET_OK  # n_unassigned is optional
    torch.cuda.synchronize()
    want, _ = pu.expected(tr, o, who.cpu().numpy(), uu.cpu().numpy(), ud.cpu().numpy())
    pu.assert_records_equal(records(res, 3, 4), want)
    # T = 0: only empty records; R = 0: nothing
    t0 = {k: (v[:, :0] if k in ("arrive", "req") else v) for k, v in tr.items()}
    d0 = fa.as_device_trace(t0, dev)
    buf, cnt = fa.per_user_stats(ctx, d0, fa.run_batch(ctx, d0), np.zeros((3, 0), np.int32), uu, ud)
    assert records(buf, 3, 4).tobytes() == pu.empty_records(3, 4).tobytes() and list(cnt.cpu().numpy()) == [0, 0, 0]
    empty = fa.as_device_trace({k: v[:0] for k, v in tr.items()}, dev)
    buf, cnt = fa.per_user_stats(ctx, empty, fa.allocate_outputs(0, 65, dev), np.zeros((0, 65), np.int32), uu, ud)
    assert buf.numel() == 0 and cnt.numel() == 0


# ---------------------------------------------------------------- reduction

@pytest.mark.parametrize("U", [1, 10, LDS_CAP + 1])
@pytest.mark.parametrize("R", [0, 1, 127, 128, 129, 300])
def test_reduction_of_random_records(ctx, R, U):
    rng = random.Random(1000 * R + U)
    recs = random_records(rng, R, U)
    stats = np.zeros(R, REP)
    stats["status"] = [rng.choice((0, 0, 0, _abi.FOGNET_REF_ABORTED, _abi.FOGNET_ERR_ARG)) for _ in range(R)]
    for r in (126, 127, 128, 129, 255, 256, 257, R - 1):  # both sides of the reduction's 128-thread stride edges
        if 0 < r < R:
            stats["status"][r] = (_abi.FOGNET_ERR_CAPACITY, _abi.FOGNET_REF_ABORTED, 0)[r % 3]
    dev = torch.device("cuda", ctx.device)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    got = fa.reduce_user_stats(ctx, to_dev(recs), to_dev(stats), R, U)
    ok = np.nonzero(stats["status"] == 0)[0]
    want = np.array([pu.merged(recs[ok, u], wrap=True) for u in range(U)], USER)
    pu.assert_records_equal(got, want)
    if R == 0:
        assert got.tobytes() == pu.empty_records(U).tobytes()
    if R >= 2:  # the host merge of two shards
        half = [fa.reduce_user_stats(ctx, to_dev(recs[s]), to_dev(stats[s]), len(stats[s]), U)
                for s in (slice(0, R // 2), slice(R // 2, R))]
        assert fa.merge_user_stats(half).tobytes() == got.tobytes()


def test_reduction_of_whole_replication_records(ctx):
    """U = 1: the [R] records of fognet_user_stats_dev, failed replications left out."""
    tr = failed_trace()
    d, out = device_replay(ctx, "failed", tr)
    uu, ud = draw_links(77, 5, 191, True)  # per-task links [R, T]
    dev = torch.device("cuda", ctx.device)
    res = torch.empty(5 * USER.itemsize, dtype=torch.uint8, device=dev)
    whole = fa.user_stats(ctx, d, out, uu, ud, res=res)
    red = fa.reduce_user_stats(ctx, res, out.stats, 5, 1)
    assert red.shape == (1,) and red[0].tobytes() == pu.merged(whole[[0, 2, 4]]).tobytes()
    assert int(red[0]["delay"]["count"]) == 3 * 191


# ---------------------------------------------------------------- buffer contract

def guarded_run(ctx, tr, who, uu, ud, poison, misalign):
    dev = torch.device("cuda", ctx.device)
    ain, aout = Arena(dev, poison), Arena(dev, poison)
    d = {k: ain.put(v, misalign, name=k) for k, v in tr.items()}
    g_who, g_uu, g_ud = ain.put(who, misalign, "user_of"), ain.put(uu, misalign, "user_ul"), ain.put(ud, misalign, "user_dl")
    R, T = d["arrive"].shape
    U = uu.shape[-1]
    rec = lambda n, dt, name: aout.alloc(n * dt.itemsize // 8, torch.int64, misalign, name=name).view(torch.uint8)
    out = fa.BatchResult(node=aout.alloc((R, T), torch.int32, misalign, "node"), status=aout.alloc((R, T), torch.uint8, misalign, "status"),
                         start_tick=aout.alloc((R, T), torch.int64, misalign, "start"),
                         done_tick=aout.alloc((R, T), torch.int64, misalign, "done"), stats=rec(R, REP, "stats"))
    fa.run_batch(ctx, d, out=out)
    users, job = rec(R * U, USER, "per_user"), rec(U, USER, "job_users")
    cnt = aout.alloc((R,), torch.int64, misalign, "n_unassigned")
    if misalign:
        assert g_who.data_ptr() % 8 == 4 and users.data_ptr() % 16 == 8  # natural alignment only
    fa.per_user_stats(ctx, d, out, g_who, g_uu, g_ud, res=users, n_unassigned=cnt, allow_unassigned=True)
    red = fa.reduce_user_stats(ctx, users, out.stats, R, U, out=job)
    torch.cuda.synchronize()
    ain.check()
    aout.check()
    return records(users, R, U).copy(), cnt.cpu().numpy().copy(), red.copy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T,U", [(65, 10), (191, LDS_CAP + 1), (191, 10), (65, LDS_CAP + 1)])
def test_buffer_contract(ctx, monkeypatch, layout, T, U):
    set_layout(monkeypatch, layout)
    tr, o = trace_case(5, T)
    who = draw_users(T + U, 3, T, U, "random")
    who[1, T // 2] = U  # one past the last record
    uu, ud = draw_links(T + U + 1, 3, U, True)
    want, un_want = pu.expected(tr, o, who, uu, ud)
    runs = [guarded_run(ctx, tr, who, uu, ud, p, m) for p, m in ((0xA5, False), (0x5A, False), (0xA5, True))]
    for g, un, red in runs:
        pu.assert_records_equal(g, want, layout)
        assert list(un) == list(un_want) == [0, 1, 0]
        pu.assert_records_equal(red, np.array([pu.merged(want[:, u]) for u in range(U)], USER), "reduction")
        assert g.tobytes() == runs[0][0].tobytes() and red.tobytes() == runs[0][2].tobytes()


# ---------------------------------------------------------------- the driver

def test_driver_user_stats_blocks(ctx, tmp_path):
    """fognet_replay --sca f --user-stats appends one block per user module plus the broker's
    delay; counts and sums equal the helper's on the same traces, regenerated through
    fognet_gen_trace_mqtt with the driver's seeds.  Without the flag the .sca is unchanged."""
    from fractions import Fraction
    from test_driver import INI, MS, SEC, drive
    from test_node_stats import blocks, want_fields
    a, b, trc = (str(tmp_path / n) for n in ("a.sca", "b.sca", "g.fogntrc"))
    args = ("-f", INI, "--users", "user[3]", "--reps", "4")
    drive(*args, "--sca", a, "--user-stats", "--trace-out", trc)
    drive(*args, "--sca", b)
    plain, text = open(b, "rb").read(), open(a, "rb").read()
    assert text.startswith(plain) and text.count(b"version 2") == 1 and b".user[" not in plain and b"delay:stats" not in plain
    tr = formats.load_trace(trc)
    tr = {k: tr[k] for k in ("arrive", "req", "mips", "dl", "ul", "init")}
    gens = [formats.gen_trace_mqtt(1 + r, [200 * MS] * 3, [1500 * MS] * 3, [MS] * 3, [MS] * 3, 300 * SEC) for r in range(4)]
    for r, g in enumerate(gens):
        np.testing.assert_array_equal(tr["arrive"][r], g["arrive"])
    who = np.stack([g["user"] for g in gens]).astype(np.int32)
    links = np.full(3, MS, np.int64)  # --user-ul / --user-dl defaults
    o = replay_oracle(tr)
    assert (o["stats"]["status"] == 0).all()
    want, un = pu.expected(tr, o, who, links, links)
    assert (un == 0).all()
    job = [pu.merged(want[:, u]) for u in range(3)]
    blk = blocks(text[len(plain):].decode())
    assert sorted(blk) == ["FogNet5.broker.udpApp[0]"] + [f"FogNet5.user[{u}].udpApp[0]" for u in range(3)]
    unit = Fraction(1, 10**12)
    for u in range(3):
        m = blk[f"FogNet5.user[{u}].udpApp[0]"]
        for sig in ("latency", "latencyH1", "taskTime"):
            w = want_fields(pu.load_mom(job[u][sig]), unit)
            for k in ("count", "sum", "sqrsum", "mean", "stddev"):
                assert m[sig + ":stats"][k] == w[k], (u, sig, k)
        # the broker's pubAck for every publish of the user, plus one ack per task a node queued
        queued = int(((o["status"] == 4) & (who == u)).sum())
        assert int(m["latencyH1:stats"]["count"]) == int((who == u).sum()) + queued and (who == u).any()
    w = want_fields(pu.load_mom(pu.merged(job)["delay"]), unit)
    d = blk["FogNet5.broker.udpApp[0]"]["delay:stats"]
    assert all(d[k] == w[k] for k in ("count", "sum", "sqrsum", "mean", "stddev")) and int(d["count"]) == who.size
