"""Queue-length statistics on the device (fognet_queue_stats_dev, fognet_reduce_queue_stats_dev),
byte for byte against the event-level restatement (queue_ref) of the device's own replay outputs,
in the LDS layout and with the workspace layout forced (FOGNET_QUEUE_STATS=hbm).  The restatement
also holds those outputs (status, start, done) to the node model on the way."""
from __future__ import annotations

import ctypes as C
import random
import re

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import golden_io
import node_stats_ref as ns
import queue_ref as qr
import stream_gate
import tracegen as tg
from fognetsimpp_amd import _abi
from guarded import Arena
from test_parity_gpu import with_crashes

pytestmark = pytest.mark.gpu

QUEUE, REP, NODE, WIN = _abi.QUEUE_STATS_DTYPE, _abi.REP_STATS_DTYPE, _abi.NODE_STATS_DTYPE, _abi.WINDOW_STATS_DTYPE
LAYOUTS = ("lds", "hbm")
RECORD_LDS_CAP, BUILD_LDS_CAP, COUNT_LDS_CAP = 256, 2048, 8192  # queue_stats.hip: kNodeLdsMax, kBuildLdsMax, kCountLdsMax
LEVELS = [1, 2, 3, 4, 8, 64, 256, 1000]
_cache: dict = {}


def set_layout(monkeypatch, layout):
    if layout == "hbm":
        monkeypatch.setenv("FOGNET_QUEUE_STATS", "hbm")
    else:
        monkeypatch.delenv("FOGNET_QUEUE_STATS", raising=False)


def dev_of(ctx):
    return torch.device("cuda", ctx.device)


def host_out(out) -> dict:
    torch.cuda.synchronize()
    return dict(node=out.node.cpu().numpy(), status=out.status.cpu().numpy(), start=out.start_tick.cpu().numpy(),
                done=out.done_tick.cpu().numpy(), stats=out.rep_stats().copy())


def covering(o) -> int:
    """One past the last completion of any replication (0 if there is none)."""
    ok = np.isin(o["stats"]["status"], qr.OK_STATUSES)
    last = o["stats"]["last_tick"][ok]
    return max(int(last.max()) + 1, 0) if last.size else 0


def replayed(ctx, key, make, policy="REF_V3", assign=None, **kw):
    """(host trace, device trace, device outputs, host copy of the outputs): replayed once per key."""
    if key not in _cache:
        tr = make()
        d = fa.as_device_trace(tr, dev_of(ctx))
        if assign is not None:
            out = fa.run_assigned(ctx, d, assign(tr, d))
        else:
            out = fa.run_batch(ctx, d, policy=policy, **kw)
        _cache[key] = (tr, d, out, host_out(out))
    return _cache[key]


def records(ctx, d, out, levels, t0, t1, policy="REF_V3") -> np.ndarray:
    R, N = d["arrive"].shape[0], d["mips"].shape[-1]
    buf = fa.queue_stats(ctx, d, out, levels, t0, t1, policy=policy)
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(QUEUE).reshape(R, N).copy()


def check(ctx, monkeypatch, case, levels=LEVELS, t0=0, t1=None, policy="REF_V3", what=""):
    """Both layouts equal the restatement and each other; returns the records and the expectation."""
    tr, d, out, o = case
    t1 = covering(o) if t1 is None else t1
    want = qr.expected(tr, o, levels, t0, t1)
    got = {}
    for layout in LAYOUTS:
        set_layout(monkeypatch, layout)
        got[layout] = records(ctx, d, out, levels, t0, t1, policy)
        qr.assert_records_equal(got[layout], want, len(levels), f"{what} [{layout}] range [{t0}, {t1})")
    assert got["lds"].tobytes() == got["hbm"].tobytes()
    return got["lds"], want


# ---------------------------------------------------------------- recordings and generated traces

def test_recorded_reference_traces(ctx, monkeypatch):
    cases = golden_io.ref_v3_replay_cases()
    assert len(cases) == 14
    seen_max = 0
    for name, tr, _, _, _ in cases:
        tr = {k: (np.atleast_2d(v) if k in ("arrive", "req") else v) for k, v in tr.items()}
        case = replayed(ctx, ("rec", name), lambda: tr)
        assert (case[3]["stats"]["status"] == 0).all(), name
        g, _ = check(ctx, monkeypatch, case, what=name)
        seen_max = max(seen_max, int(g["max_len"].max()))
    assert seen_max > 64  # the herded recordings: a queue longer than a tile


@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
@pytest.mark.parametrize("N", [1, 3, 64, 300])
def test_generated_traces(ctx, monkeypatch, N, policy):
    queued = 0
    for T in (1, 63, 64, 65, 129, 200):
        def make():
            return tg.make_batch(0x9E0 + 7 * N + T, 3, N, T, rho=3.0 if T in (129, 200) else 0.9)
        case = replayed(ctx, ("gen", N, T, policy), make, policy)
        assert (case[3]["stats"]["status"] == 0).all()
        g, _ = check(ctx, monkeypatch, case, policy=policy, what=f"N={N} T={T} {policy}")
        queued += int(g["n_enq"].sum())
        if N == 1 and T == 200:
            assert int(g["max_len"].max()) > 64  # more waiting tasks on one node than a tile of the build kernel
    assert queued > 0


def test_shared_node_rows_and_rounds(ctx, monkeypatch):
    """Node parameters shared by the replications, and the job cut into rounds of 2 replications."""
    def make():
        tr = tg.make_batch(0x9E1, 5, 7, 150, rho=2.0)
        return dict(tr, **{k: tr[k][0] for k in ("mips", "dl", "ul", "init")})
    case = replayed(ctx, "shared", make)
    g, want = check(ctx, monkeypatch, case, what="shared")
    for layout in LAYOUTS:
        set_layout(monkeypatch, layout)
        monkeypatch.setenv("FOGNET_QUEUE_ROUND", "2")
        r = records(ctx, case[1], case[2], LEVELS, 0, covering(case[3]))
        monkeypatch.delenv("FOGNET_QUEUE_ROUND")
        assert r.tobytes() == g.tobytes(), layout
    # per-replication node rows in rounds as well
    case = replayed(ctx, ("gen", 3, 200, "REF_V3"), lambda: tg.make_batch(0x9E0 + 21 + 200, 3, 3, 200, rho=3.0))
    g, _ = check(ctx, monkeypatch, case)
    monkeypatch.setenv("FOGNET_QUEUE_ROUND", "1")
    assert records(ctx, case[1], case[2], LEVELS, 0, covering(case[3])).tobytes() == g.tobytes()


# ---------------------------------------------------------------- the range

def tie_case(ctx):
    return replayed(ctx, "tie", lambda: qr.tie_heavy_trace(5, 4, 3, 150))


def test_ranges(ctx, monkeypatch):
    case = tie_case(ctx)
    tr, _, _, o = case
    assert (o["stats"]["status"] == 0).all()
    # a node with a tick that holds an enqueue alone, one with a dequeue alone and one with both
    both = only_enq = only_deq = None
    for r, k in np.ndindex(4, 3):
        idx = np.nonzero(o["node"][r] == k)[0]
        trail = qr.node_events(tr["arrive"][r][idx], tr["req"][r][idx], int(tr["mips"][r, k]), int(tr["dl"][r, k]))[3]
        enq = {t for t, _, kind in trail if kind == "enq"}
        deq = {t for t, _, kind in trail if kind == "deq"}
        if enq & deq and enq - deq and deq - enq:
            both, only_enq, only_deq = sorted(enq & deq), sorted(enq - deq), sorted(deq - enq)
            break
    assert both and only_enq and only_deq
    end = covering(o)
    lv = [1, 2, 3, 5]
    ticks = [only_enq[len(only_enq) // 2], only_deq[len(only_deq) // 2], both[len(both) // 2]]
    ranges = [(end // 3, 2 * end // 3), (0, end), (end // 2, end // 2), (0, 0), (end, end + 5)]
    for t in ticks:
        ranges += [(t, end), (0, t), (t, t + 1), (t, t), (t - 1, t)]
    for t0, t1 in ranges:
        g, _ = check(ctx, monkeypatch, case, lv, t0, t1, what="tie")
        assert (g["observed_lo"] == t1 - t0).all()
        if t1 == t0:
            assert not g["n_enq"].any() and not g["max_len"].any() and not g["area_lo"].any() and not g["time_ge"].any()


def test_levels_add_up_to_the_area_over_a_covering_range(ctx, monkeypatch):
    case = replayed(ctx, "light", lambda: tg.make_batch(0x9E2, 3, 5, 200, rho=0.2))
    lv = list(range(1, 9))
    g, _ = check(ctx, monkeypatch, case, lv, what="light")
    assert 1 <= int(g["max_len"].max()) <= 8
    ge = g["time_ge"][..., 0].astype(object)
    assert not g["time_ge"][..., 1].any() and not g["area_hi"].any()
    assert (ge.sum(axis=-1) == g["area_lo"].astype(object)).all()          # sum over levels 1 .. max of time_ge = area
    assert (ge[..., 1:] <= ge[..., :-1]).all()                             # nonincreasing in q
    assert (ge[..., 0] <= g["observed_lo"].astype(object)).all()           # never more than the observed time
    for r, k in np.ndindex(3, 5):  # no time at a length that was never reached
        assert not any(int(ge[r, k, q]) for q in range(int(g["max_len"][r, k]), 8))


# ---------------------------------------------------------------- agreement with the existing passes

@pytest.mark.parametrize("N", [5, 300])
def test_agreement_with_node_and_window_statistics(ctx, monkeypatch, N):
    case = replayed(ctx, ("agree", N), lambda: tg.make_batch(0x9E3 + N, 3, N, 200, rho=3.0))
    tr, d, out, o = case
    end = covering(o)
    g, _ = check(ctx, monkeypatch, case, what=f"agree N={N}")
    nodes = fa.node_stats(ctx, d, out).cpu().numpy().view(NODE).reshape(3, N)
    np.testing.assert_array_equal(g["n_enq"], nodes["n_queued"])
    assert int(g["n_enq"].sum()) > 0
    win = fa.window_stats(ctx, d, out, None, None, None, 0, end, 1)[0].cpu().numpy().view(WIN).reshape(3, 1)
    wide = lambda a, lo, hi: int(a[lo]) | (int(a[hi]) << 64)  # noqa: E731
    for r in range(3):
        waiting = wide(win[r, 0], "insys_lo", "insys_hi") - wide(win[r, 0], "busy_lo", "busy_hi")
        assert sum(wide(g[r, k], "area_lo", "area_hi") for k in range(N)) == waiting > 0


# ---------------------------------------------------------------- node-down

def test_crash_with_tasks_waiting(ctx, monkeypatch):
    def make():
        return with_crashes(qr.tie_heavy_trace(9, 4, 3, 150), seed=9, grid=10**11)
    case = replayed(ctx, "down-tie", make)
    o = case[3]
    assert (o["stats"]["status"] == 0).all()
    assert ((o["status"] == 4) & (o["start"] == -1)).any() and (o["status"] == 9).any()  # waiting at the crash; lost
    check(ctx, monkeypatch, case, [1, 2, 3, 5], what="down-tie")
    down = np.asarray(case[0]["down"])
    t = int(down[down != fa.NEVER].min())
    for t0, t1 in ((0, t), (t, covering(o) + 1), (t - 1, t + 1)):  # the range ends / starts at a crash tick
        check(ctx, monkeypatch, case, [1, 2, 3, 5], t0, t1, what="down-tie")
    case = replayed(ctx, "down-gen", lambda: with_crashes(tg.make_batch(0x9E4, 3, 40, 300, rho=4.0, lat_scale=10), seed=40),
                    "EXT_LAT")
    assert ((case[3]["status"] == 4) & (case[3]["start"] == -1)).any()
    check(ctx, monkeypatch, case, policy="EXT_LAT", what="down-gen")


# ---------------------------------------------------------------- the assigned replay's outputs

@pytest.mark.parametrize("rule", ["rr", "random"])
def test_assigned_replay_outputs(ctx, monkeypatch, rule):
    for N in (3, 40):
        def assign(tr, d):
            R, T = tr["arrive"].shape
            return fa.assign_round_robin(R, T, N, dev_of(ctx)) if rule == "rr" else fa.assign_random(R, T, N, 7, dev_of(ctx))
        case = replayed(ctx, ("asg", rule, N), lambda: tg.make_batch(0x9E5 + N, 3, N, 200, rho=6.0),
                        assign=assign)
        assert (case[3]["stats"]["status"] == 0).all()
        g, _ = check(ctx, monkeypatch, case, what=f"{rule} N={N}")
        assert int(g["n_enq"].sum()) > 0
    case = replayed(ctx, ("asg-down", rule), lambda: with_crashes(qr.tie_heavy_trace(12, 3, 4, 150), seed=12, grid=10**11),
                    assign=lambda tr, d: (fa.assign_round_robin(3, 150, 4, dev_of(ctx)) if rule == "rr"
                                          else fa.assign_random(3, 150, 4, 7, dev_of(ctx))))
    check(ctx, monkeypatch, case, [1, 2, 3, 5], what=f"{rule} down")


# ---------------------------------------------------------------- cursors past a tile, N past every LDS limit

def test_long_queue_on_one_node(ctx, monkeypatch):
    case = replayed(ctx, "herded", ns.herded_trace)
    g, _ = check(ctx, monkeypatch, case, [1, 64, 65, 128, 200, 256, 260, 261], what="herded")
    assert int(g["max_len"][0, 0]) > 4 * 64 and int(g["n_enq"][0, 0]) > 4 * 64


@pytest.mark.parametrize("N", [RECORD_LDS_CAP + 1, BUILD_LDS_CAP + 1, COUNT_LDS_CAP + 1])
def test_more_nodes_than_the_lds_layouts_hold(ctx, monkeypatch, N):
    case = replayed(ctx, ("big", N), lambda: tg.make_batch(0x9E6 + N, 2, N, 400, rho=16.0 / N),
                    assign=lambda tr, d: fa.assign_random(2, 400, 8, 3, dev_of(ctx)) * (N // 8) + (N % 8))
    g, _ = check(ctx, monkeypatch, case, what=f"big N={N}")
    assert int(g["n_enq"].sum()) > 0 and int((g["n_enq"].sum(axis=0) > 0).sum()) == 8  # (eight nodes, spread over [0, N))


# ---------------------------------------------------------------- failed and aborted replications

def failed_trace():
    tr = {k: v.copy() for k, v in tg.make_batch(0xFA12, 5, 100, 191, rho=3.0).items()}
    tr["mips"][2, 0] = 0                                  # refused before its first decision
    tr["arrive"][3, 127] = tr["arrive"][3, 126] - 1       # fails in mid-trace
    return tr


def guarded_run(ctx, tr, poison, misalign, levels):
    dev = dev_of(ctx)
    ain, aout = Arena(dev, poison), Arena(dev, poison)
    d = {k: ain.put(v, misalign, name=k) for k, v in tr.items()}
    R, T = d["arrive"].shape
    N = d["mips"].shape[-1]
    rec = lambda n, dt, name: aout.alloc(n * dt.itemsize // 8, torch.int64, misalign, name=name).view(torch.uint8)  # noqa: E731
    out = fa.BatchResult(node=aout.alloc((R, T), torch.int32, misalign, "node"), status=aout.alloc((R, T), torch.uint8, misalign, "status"),
                         start_tick=aout.alloc((R, T), torch.int64, misalign, "start"),
                         done_tick=aout.alloc((R, T), torch.int64, misalign, "done"), stats=rec(R, REP, "stats"))
    fa.run_batch(ctx, d, out=out)
    o = host_out(out)
    failed = [r for r in range(R) if int(o["stats"]["status"][r]) not in qr.OK_STATUSES]
    for r in failed:  # whatever the replay left in a failed replication's rows: poison again
        for t in (out.node, out.status, out.start_tick, out.done_tick):
            t[r].view(torch.uint8).fill_(poison)
    rows, job = rec(R * N, QUEUE, "queue_stats"), rec(N, QUEUE, "job_queue")
    fa.queue_stats(ctx, d, out, levels, 0, covering(o), res=rows)
    red = fa.reduce_queue_stats(ctx, rows, out.stats, R, N, out=job)
    torch.cuda.synchronize()
    ain.check()
    aout.check()
    return rows.cpu().numpy().view(QUEUE).reshape(R, N).copy(), red.copy(), o


@pytest.mark.parametrize("layout", LAYOUTS)
def test_failed_replications_get_empty_records_and_are_not_read(ctx, monkeypatch, layout):
    set_layout(monkeypatch, layout)
    tr = failed_trace()
    runs = [guarded_run(ctx, tr, p, m, LEVELS) for p, m in ((0xA5, False), (0x5A, False), (0xA5, True))]
    for g, red, o in runs:
        assert [int(s) in qr.OK_STATUSES for s in o["stats"]["status"]] == [True, True, False, False, True]
        assert int(o["stats"]["n_tasks"][2]) == 0 and 0 < int(o["stats"]["n_tasks"][3]) < 191
        want = qr.expected(tr, o, LEVELS, 0, covering(o))
        qr.assert_records_equal(g, want, 8, layout)
        assert g[2].tobytes() == bytes(100 * 176) == g[3].tobytes()  # between good ones: empty, and nothing of them read
        assert int(g[[0, 1, 4]]["n_enq"].sum()) > 0
        qr.assert_records_equal(red, np.array([qr.merged(want[[0, 1, 4], k], 8) for k in range(100)], QUEUE), 8, "reduction")
        assert g.tobytes() == runs[0][0].tobytes() and red.tobytes() == runs[0][1].tobytes()


def test_ref_aborted_replication_is_kept_by_the_pass_and_left_out_of_the_reduction(ctx, monkeypatch):
    def make():
        h, other = ns.herded_trace(), tg.make_batch(0x9E7, 1, 256, 320, rho=0.9, req_hi=4000)  # (short waits: no overflow)
        return dict(arrive=np.concatenate([h["arrive"], other["arrive"]]), req=np.concatenate([h["req"], other["req"]]),
                    mips=np.stack([h["mips"], other["mips"][0]]), dl=np.stack([h["dl"], other["dl"][0]]),
                    ul=np.stack([h["ul"], other["ul"][0]]), init=np.stack([h["init"], other["init"][0]]))
    case = replayed(ctx, "aborted", make, ref_abort=True)
    tr, d, out, o = case
    assert [int(s) for s in o["stats"]["status"]] == [_abi.FOGNET_REF_ABORTED, _abi.FOGNET_OK]
    g, want = check(ctx, monkeypatch, case, what="aborted")
    assert int(g["n_enq"][0].sum()) > 256 and int(g["n_enq"][1].sum()) > 0  # kept
    buf = fa.queue_stats(ctx, d, out, LEVELS, 0, covering(o))
    red = fa.reduce_queue_stats(ctx, buf.reshape(-1), out.stats, 2, 256)
    qr.assert_records_equal(red, want[1], 8, "reduction without the aborted replication")


# ---------------------------------------------------------------- the reduction

def test_reduction_at_130_replications_equals_the_host_merge(ctx):
    rng = random.Random(130)
    R, N = 130, 3
    recs = np.zeros((R, N), QUEUE)
    flat = recs.view(np.uint64).reshape(R, N, -1)
    flat[:] = np.frombuffer(rng.randbytes(flat.nbytes), np.uint64).reshape(flat.shape)
    recs["n_enq"] >>= 24  # counts that cannot overflow int64 when summed
    stats = np.zeros(R, REP)
    stats["status"] = [rng.choice((0, 0, 0, _abi.FOGNET_REF_ABORTED, _abi.FOGNET_ERR_ARG)) for _ in range(R)]
    stats["status"][[0, 127, 128, 129]] = (0, _abi.FOGNET_REF_ABORTED, 0, _abi.FOGNET_ERR_CAPACITY)  # the 128-thread stride's edges
    dev = dev_of(ctx)
    got = fa.reduce_queue_stats(ctx, torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev),
                                torch.from_numpy(stats.view(np.uint8).reshape(-1)).to(dev), R, N)
    ok = np.nonzero(stats["status"] == 0)[0]
    host = fa.merge_queue_stats([recs[r] for r in ok])
    assert got.tobytes() == host.tobytes()
    for lo, hi in (("observed_lo", "observed_hi"), ("area_lo", "area_hi")):  # (modulo 2^128, as the limbs wrap)
        total = sum(int(x[lo]) | (int(x[hi]) << 64) for x in recs[ok, 1]) % (1 << 128)
        assert int(got[1][lo]) | (int(got[1][hi]) << 64) == total
    total = sum(int(x["time_ge"][7][0]) | (int(x["time_ge"][7][1]) << 64) for x in recs[ok, 1]) % (1 << 128)
    assert int(got[1]["time_ge"][7][0]) | (int(got[1]["time_ge"][7][1]) << 64) == total
    assert int(got[1]["max_len"]) == int(recs[ok, 1]["max_len"].max()) and int(got[1]["n_enq"]) == int(recs[ok, 1]["n_enq"].sum())
    none = fa.reduce_queue_stats(ctx, torch.empty(0, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.uint8, device=dev), 0, 4)
    assert none.tobytes() == bytes(4 * 176)


# ---------------------------------------------------------------- refusals

def test_refusals_leave_the_output_untouched(ctx):
    dev = dev_of(ctx)
    tr = tg.make_batch(3, 2, 8, 65, rho=2.0)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_batch(ctx, d, escalated=True)
    res = torch.full((2 * 8 * 176,), 0xCD, dtype=torch.uint8, device=dev)
    ptr = fa.engine._ptr
    i64 = lambda *v: (C.c_int64 * len(v))(*v)  # noqa: E731

    def call(policy=1, bo=None, level=i64(1, 2), Q=2, t0=0, t1=10**15, qs=res, R=2, T=65):
        bi = fa.engine._batch_in(d, R, T, 8, 8, policy)
        bo = bo if bo is not None else fa.engine._batch_out(out)
        rc = ctx._lib.fognet_queue_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), level, Q, t0, t1, ptr(qs) if qs is not None else None,
                                             None)
        torch.cuda.synchronize()
        return rc

    hier = _abi.FOGNET_POLICY_EXT_HIER
    assert call(policy=hier) == _abi.FOGNET_ERR_UNSUPPORTED and "FIFO order" in ctx.last_error()
    assert call(policy=hier, bo=fa.engine._batch_out(out, escalated=True)) == _abi.FOGNET_ERR_UNSUPPORTED  # flags or not
    so = fa.run_batch(ctx, d, out=fa.allocate_outputs(2, 65, dev, per_task=False))
    no_start = fa.engine._batch_out(out)
    no_start.start_tick = None
    bad = [dict(bo=fa.engine._batch_out(so)), dict(bo=no_start), dict(Q=0), dict(Q=9, level=i64(*range(1, 10))),
           dict(level=i64(0, 1)), dict(level=i64(2, 2)), dict(level=i64(3, 2)), dict(t0=-1), dict(t0=5, t1=4),
           dict(t1=2**62 + 1), dict(level=None), dict(qs=None)]
    for kw in bad:
        assert call(**kw) == _abi.FOGNET_ERR_ARG, kw
    assert bytes(res.cpu().numpy()) == b"\xCD" * res.numel()  # nothing was written by any of them
    with pytest.raises(fa.FognetError) as e:
        fa.queue_stats(ctx, d, out, policy="EXT_HIER")
    assert e.value.code == _abi.FOGNET_ERR_UNSUPPORTED
    # R = 0, T = 0, t1 = t0 and t1 = 2^62 succeed
    assert call(R=0) == _abi.FOGNET_OK and bytes(res.cpu().numpy()) == b"\xCD" * res.numel()
    assert call(t0=7, t1=7) == _abi.FOGNET_OK
    g = res.cpu().numpy().view(QUEUE)
    assert not g["observed_lo"].any() and not g["n_enq"].any() and not g["area_lo"].any()
    assert call(t1=2**62) == _abi.FOGNET_OK
    t0d = {k: (v[:, :0] if k in ("arrive", "req") else v) for k, v in tr.items()}
    dd = fa.as_device_trace(t0d, dev)
    oo = fa.run_batch(ctx, dd)
    g = fa.queue_stats(ctx, dd, oo, [1], 0, 50).cpu().numpy().view(QUEUE).reshape(2, 8)
    assert (g["observed_lo"] == 50).all() and not g["n_enq"].any() and not g["time_ge"].any()


# ---------------------------------------------------------------- the driver

def test_driver_appends_the_queue_scalars(tmp_path):
    """fognet_replay --sca f --queue-stats appends the scalars to every fog node's block: the enqueues
    are the node block's queued tasks, the shares lie in [0, 1] and fall with the level; without the
    flag the .sca is unchanged; with --assign as well."""
    from test_driver import INI, drive
    from test_queue_stats import scalars
    a, b, c = (str(tmp_path / n) for n in ("a.sca", "b.sca", "c.sca"))
    args = ("-f", INI, "--users", "user[10]", "--reps", "4", "--node-stats")
    drive(*args, "--sca", a, "--queue-stats", "1,4,16")
    drive(*args, "--sca", b)
    plain, text = open(b).read(), open(a).read()
    assert text.startswith(plain) and "queueLength" not in plain and text.count("version 2") == 1
    blocks, node = scalars(text[len(plain):]), scalars(plain)
    queued = dict(re.findall(r'^scalar (\S+fogNode\[\d+\]\S+) \t"tasks queued" \t(\d+)$', plain, re.M))
    assert len(blocks) == len(queued) > 0 and sum(int(v) for v in queued.values()) > 0
    for mod, s in blocks.items():
        assert list(s) == ["queueLength:max", "queueLength:enqueued", "queueLength:timeavg", "queueLength:ge1",
                           "queueLength:ge4", "queueLength:ge16"], mod
        assert s["queueLength:enqueued"] == queued[mod] and (int(s["queueLength:max"]) > 0) == (int(queued[mod]) > 0)
        ge = [float(s[f"queueLength:ge{l}"]) for l in (1, 4, 16)]
        assert 1.0 >= ge[0] >= ge[1] >= ge[2] >= 0.0 and float(s["queueLength:timeavg"]) >= ge[0]
    assert node  # (the node blocks' unquoted scalars are still there)
    drive(*args, "--sca", c, "--queue-stats", "--assign", "random:7")
    tail = scalars(open(c).read())
    assert all("queueLength:ge128" in s for m, s in tail.items() if ".fogNode[" in m)


# ---------------------------------------------------------------- determinism

@pytest.mark.parametrize("layout", LAYOUTS)
def test_deterministic_and_independent_of_the_workspace(ctx, monkeypatch, layout):
    set_layout(monkeypatch, layout)
    tr, d, out, o = tie_case(ctx)
    end = covering(o)
    first = records(ctx, d, out, [1, 2, 3, 5], 0, end)
    again = records(ctx, d, out, [1, 2, 3, 5], 0, end)
    big = fa.as_device_trace(tg.make_batch(0xB16, 4, 300, 800, rho=3.0), dev_of(ctx))  # a larger job dirties the workspace
    fa.queue_stats(ctx, big, fa.run_batch(ctx, big), LEVELS, 0, 10**17)
    third = records(ctx, d, out, [1, 2, 3, 5], 0, end)
    assert first.tobytes() == again.tobytes() == third.tobytes()


# ---------------------------------------------------------------- a side stream

class StreamJob:
    """Plain device tensors of one replay + queue pass (stream_gate's job: ``inputs`` are the views the calls read)."""

    def __init__(self, ctx, tr):
        dev = dev_of(ctx)
        self.inputs = fa.as_device_trace(tr, dev)
        R, T = self.inputs["arrive"].shape
        self.N = self.inputs["mips"].shape[-1]
        self.out = fa.allocate_outputs(R, T, dev, N=self.N)
        self.rows = torch.empty(R * self.N * 176, dtype=torch.uint8, device=dev)
        self.red = torch.empty(self.N * 176, dtype=torch.uint8, device=dev)


def test_on_a_side_stream_behind_a_gate(ctx):
    gate = stream_gate.Gate(dev_of(ctx))
    try:
        gate.choose(1)
    except stream_gate.NoPower as e:
        pytest.skip(str(e))
    tr = tg.make_batch(0x9E8, 3, RECORD_LDS_CAP + 1, 129, rho=30.0)
    decoy = tg.make_batch(0x9E9, 3, RECORD_LDS_CAP + 1, 129, rho=30.0)
    t1 = 10**17  # (given, not read back from the records: the calls must only enqueue)

    def enqueue(j):
        dev = j.rows.device
        fa.run_batch(ctx, j.inputs, out=j.out)
        fa.queue_stats(ctx, j.inputs, j.out, LEVELS, 0, t1, res=j.rows)
        ctx.check(ctx._lib.fognet_reduce_queue_stats_dev(ctx.handle, fa.engine._ptr(j.rows), fa.engine._ptr(j.out.stats), 3, j.N,
                                                         fa.engine._ptr(j.red), fa.engine._stream_ptr(dev)), "reduction")

    plain = StreamJob(ctx, tr)
    enqueue(plain)
    o = host_out(plain.out)
    want = qr.expected(tr, o, LEVELS, 0, t1)
    g = plain.rows.cpu().numpy().view(QUEUE).reshape(3, -1)
    qr.assert_records_equal(g, want, 8, "plain")
    assert int(g["n_enq"].sum()) > 0
    job = gate.run("queuestats", "queuestats-N257", lambda: StreamJob(ctx, tr), dict(decoy), enqueue)
    assert job.rows.cpu().numpy().tobytes() == plain.rows.cpu().numpy().tobytes()
    assert job.red.cpu().numpy().tobytes() == plain.red.cpu().numpy().tobytes()
    gate.write()
