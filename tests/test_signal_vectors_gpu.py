"""Signal vectors on the device (fognet_signal_vectors_dev) against the restatement
(signal_vectors_ref), byte for byte -- offsets, times, values and tasks -- in the default
mode and with the HBM layouts forced on small segments too (FOGNET_VEC_SORT=hbm).  The cases and the
restatement come from test_signal_vectors.py, which holds them to the reference's recorded
runs and to the per-node and per-user records without a GPU."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import signal_vectors_ref as sv
import stream_gate
import tracegen as tg
from fognetsimpp_amd import _abi
from guarded import Arena
from test_per_user_stats import down_trace, draw_links, draw_users, mqtt_case, replay_oracle, trace_case
from test_signal_vectors import herded_case, level_counts, recording_cases, tie_case
from test_user_stats import HIER_UP, abort_case, hier_case

pytestmark = pytest.mark.gpu

REP = _abi.REP_STATS_DTYPE
SORT_LDS_CAP = 2048  # signal_vectors.hip kVecSortLdsMax: a longer segment is sorted in HBM
MODES = ("lds", "hbm")
I32_MAX = 2**31 - 1
_replays: dict = {}


def set_mode(monkeypatch, mode):
    if mode == "hbm":
        monkeypatch.setenv("FOGNET_VEC_SORT", "hbm")
    else:
        monkeypatch.delenv("FOGNET_VEC_SORT", raising=False)


def device_replay(ctx, key, tr, policy="REF_V3", **kw):
    """(device trace, replay outputs) of a trace, replayed once per key and left unchanged."""
    if key is None or key not in _replays:
        d = fa.as_device_trace(tr, torch.device("cuda", ctx.device))
        got = (d, fa.run_batch(ctx, d, policy=policy, **kw))
        if key is None:
            return got
        _replays[key] = got
    return _replays[key]


def both_modes(ctx, monkeypatch, d, out, who, uu, ud, want, what="", **kw):
    """The pass in both modes, each equal to ``want`` byte for byte; returns the default mode's."""
    got = {}
    for mode in MODES:
        set_mode(monkeypatch, mode)
        got[mode] = fa.signal_vectors(ctx, d, out, who, uu, ud, **kw)
        sv.assert_equal(got[mode], want, f"{what} {mode}")
    return got["lds"]


def check(ctx, monkeypatch, key, tr, o, who, uu, ud, policy="REF_V3", **kw):
    d, out = device_replay(ctx, key, tr, policy, **kw)
    want = sv.expected(tr, o, who, uu, ud)
    g = both_modes(ctx, monkeypatch, d, out, who, uu, ud, want, str(key))
    assert (g["n_unassigned"] == 0).all()
    return g, want


def host_outputs(out) -> dict:
    """A finished device replay as the restatement takes it."""
    return dict(node=out.node.cpu().numpy(), status=out.status.cpu().numpy(), start=out.start_tick.cpu().numpy(),
                done=out.done_tick.cpu().numpy(), stats=out.rep_stats())


# ---------------------------------------------------------------- the reference's recorded runs

def test_every_recording_replayed_on_the_device(ctx, monkeypatch):
    """The device's replay of every recorded trace, then its vectors: equal to the restatement on
    the device's own outputs, which are the recording's wherever the reference run completed."""
    cases = recording_cases()
    assert len(cases) == 14
    for name, tr, o_rec, who, uu, ud, rec in cases:
        d, out = device_replay(ctx, None, tr)
        o = host_outputs(out)
        assert int(o["stats"]["status"][0]) == 0, name
        if rec["abort"] is None:
            for k in ("node", "status", "start", "done"):
                np.testing.assert_array_equal(o[k].astype(np.int64), o_rec[k].astype(np.int64), err_msg=f"{name} {k}")
        want = sv.expected(tr, o, who, uu, ud)
        both_modes(ctx, monkeypatch, d, out, who, uu, ud, want, name)


# ---------------------------------------------------------------- oracle-checked traces

@pytest.mark.parametrize("N,U", [(1, 1), (5, 3), (64, 10), (300, 129)])  # N = 300: wide-kernel rows
@pytest.mark.parametrize("T", [1, 63, 65, 129, 300])
def test_parity_with_the_restatement_both_modes(ctx, monkeypatch, T, N, U):
    tr, o = trace_case(N, T)
    assert (o["stats"]["status"] == 0).all()
    for per_rep, kind in ((False, "random"), (True, "rr")):
        who = draw_users(1000 * U + T, 3, T, U, kind)
        uu, ud = draw_links(1000 * U + T + 1, 3, U, per_rep)
        g, want = check(ctx, monkeypatch, ("trace", N, T), tr, o, who, uu, ud)
        V = N + 1 + 3 * U
        assert g["offset"].shape == (3, V + 1) and (g["offset"][:, N + 1] - g["offset"][:, N] == T).all()  # delay


def test_ext_lat(ctx, monkeypatch):
    tr, o = trace_case(5, 129, "EXT_LAT")
    who = draw_users(3, 3, 129, 3, "rr")
    check(ctx, monkeypatch, ("trace", 5, 129, "EXT_LAT"), tr, o, who, *draw_links(4, 3, 3, False), policy="EXT_LAT")


def test_reference_task_source_users(ctx, monkeypatch):
    tr, who, uu, ud = mqtt_case(3)
    check(ctx, monkeypatch, ("mqtt", 3), tr, replay_oracle(tr), who, uu, ud)


@pytest.mark.parametrize("N", [1, 3, 5])
def test_tie_heavy_traces(ctx, monkeypatch, N):
    """A 100-ms grid, some dl = 0, zero-service tasks: every level of the key decides somewhere."""
    tr, o, who, uu, ud = tie_case(N)
    n = level_counts(sv.expected(tr, o, who, uu, ud, with_rows=True), N, len(uu))
    assert all(c > 0 for lv, c in zip(sv.LEVELS, n) if N > 1 or lv != "send tick"), dict(zip(sv.LEVELS, n))
    check(ctx, monkeypatch, ("tie", N), tr, o, who, uu, ud)


def test_herded_trace_most_rows_on_one_node(ctx, monkeypatch):
    tr, o, who, uu, ud = herded_case()
    g, want = check(ctx, monkeypatch, "herd", tr, o, who, uu, ud)
    assert int(g["offset"][0][1]) > 100 and int(o["stats"]["n_qtime_overflow"][0]) > 0


def test_one_user_segment_above_the_lds_capacity(ctx):
    """U = 1, T = 20,000: latencyH1 holds every pubAck and every "task queued" ack, far above
    the LDS sort's capacity, so the default mode sorts it in HBM."""
    T = 20000
    tr = tg.make_batch(0x20000, 1, 5, T, rho=0.9)
    o = replay_oracle(tr)
    who = np.zeros((1, T), np.int32)
    uu, ud = np.array([3 * 10**9], np.int64), np.array([2 * 10**9], np.int64)
    want = sv.expected(tr, o, who, uu, ud)
    h1 = int(want["offset"][0][5 + 1 + 2] - want["offset"][0][5 + 1 + 1])
    assert T < h1 <= 2 * T and h1 > SORT_LDS_CAP
    d, out = device_replay(ctx, None, tr)
    sv.assert_equal(fa.signal_vectors(ctx, d, out, who, uu, ud), want, "T = 20,000")


# ---------------------------------------------------------------- failed, aborted, down, unassigned, ranges

def mixed_batch():
    """[good, refused before its first decision (MIPS 0), REF_ABORTED, good]: abort_case's shape."""
    base = abort_case()[0]
    tr = {k: np.repeat(np.atleast_2d(v), 4, axis=0).copy() for k, v in base.items()}
    tr["req"][[0, 3]] = [[3, 1, 2, 1, 1], [1, 2, 1, 3, 1]]
    tr["mips"][1, 0] = 0
    return tr


def test_failed_and_ref_aborted_replications_between_good_ones(ctx, monkeypatch):
    tr = mixed_batch()
    o = replay_oracle(tr)  # the oracle's full run of the aborted replication: the engine replays on as well
    who = np.array([[0, 1, 2, 0, 1]] * 4, np.int32)
    uu, ud = draw_links(3, 4, 3, True)
    who[1] = I32_MAX  # nothing of a failed replication is read
    uu[1] = ud[1] = 0x5A5A5A5A5A5A5A5A
    d, out = device_replay(ctx, None, tr, ref_abort=True)
    st = [int(s) for s in out.rep_stats()["status"]]
    assert st[0] == st[3] == 0 and st[2] == _abi.FOGNET_REF_ABORTED and st[1] not in sv.OK_STATUSES
    want = sv.expected(tr, o, who, uu, ud, statuses=st)
    g = both_modes(ctx, monkeypatch, d, out, who, uu, ud, want)
    assert (g["offset"][1] == 0).all() and list(g["n_unassigned"]) == [0, 0, 0, 0]
    assert g["offset"][2][-1] > 0 and g["offset"][0][-1] > 0


def test_node_down(ctx, monkeypatch):
    tr = down_trace()
    o = replay_oracle(tr)
    assert (o["status"] == 9).any() and ((o["status"] != 9) & (o["done"] == -1)).any()
    check(ctx, monkeypatch, "down", tr, o, draw_users(0xD0, 3, 257, 10, "rr"), *draw_links(0xD1, 3, 10, True))


def test_out_of_range_users_are_counted_and_give_no_user_side_row(ctx, monkeypatch):
    tr, o = trace_case(5, 65)
    who = draw_users(1, 3, 65, 4, "rr")
    who[0, [3, 17, 64]] = (-1, 4, I32_MAX)
    who[2, 0] = -(2**31)
    uu, ud = draw_links(2, 3, 4, False)
    want = sv.expected(tr, o, who, uu, ud)
    d, out = device_replay(ctx, ("trace", 5, 65), tr)
    g = both_modes(ctx, monkeypatch, d, out, who, uu, ud, want, allow_unassigned=True)
    assert list(g["n_unassigned"]) == [3, 0, 1]
    assert [int(x) for x in g["offset"][:, 6] - g["offset"][:, 5]] == [62, 65, 64]  # delay rows
    with pytest.raises(fa.FognetError) as e:
        fa.signal_vectors(ctx, d, out, who, uu, ud)
    assert e.value.code == _abi.FOGNET_ERR_ARG and "4 decided publishes" in str(e.value)


def test_a_range_of_replications(ctx, monkeypatch):
    tr, o = trace_case(5, 129)
    who = draw_users(5, 3, 129, 3, "random")
    who[1, 7] = 3  # counted at the range's own index
    uu, ud = draw_links(6, 3, 3, True)
    d, out = device_replay(ctx, ("trace", 5, 129), tr)
    for r0, Rv in ((1, 1), (1, 2), (0, 2), (2, 1), (3, 0)):
        want = sv.expected(tr, o, who, uu, ud, r0=r0, Rv=Rv)
        g = both_modes(ctx, monkeypatch, d, out, who, uu, ud, want, f"r0={r0} Rv={Rv}", r0=r0, Rv=Rv, allow_unassigned=True)
        assert list(g["n_unassigned"]) == [int(r0 + q == 1) for q in range(Rv)]
    with pytest.raises(fa.FognetError) as e:
        fa.signal_vectors(ctx, d, out, who, uu, ud, r0=2, Rv=2)
    assert e.value.code == _abi.FOGNET_ERR_ARG


# ---------------------------------------------------------------- refusals

def poisoned_bufs(dev, Rv, V, T):
    return dict(offset=torch.full((Rv, V + 1), 0x5A5A5A5A, dtype=torch.int64, device=dev),
                time=torch.full((Rv, 6 * T), -7, dtype=torch.int64, device=dev),
                value=torch.full((Rv, 6 * T), -7, dtype=torch.int64, device=dev),
                task=torch.full((Rv, 6 * T), -7, dtype=torch.int32, device=dev),
                n_unassigned=torch.full((Rv,), -7, dtype=torch.int64, device=dev))


def untouched(bufs) -> bool:
    torch.cuda.synchronize()
    return bool((bufs["offset"] == 0x5A5A5A5A).all()) and all(bool((bufs[k] == -7).all())
                                                             for k in ("time", "value", "task", "n_unassigned"))


def test_ext_hier_is_refused_with_nothing_written(ctx, monkeypatch):
    tr = hier_case(0)[0]
    T = tr["arrive"].shape[1]
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_batch(ctx, d, policy="EXT_HIER", hier_threshold_s=0, hier_up_tick=HIER_UP, escalated=True)
    who = draw_users(0xE, 1, T, 4, "rr")
    uu, ud = draw_links(0xF, 1, 4, False)
    for mode in MODES:
        set_mode(monkeypatch, mode)
        bufs = poisoned_bufs(dev, 1, 2 + 1 + 12, T)
        with pytest.raises(fa.FognetError) as e:
            fa.signal_vectors(ctx, d, out, who, uu, ud, bufs=bufs)  # (the policy run_batch recorded)
        assert e.value.code == _abi.FOGNET_ERR_UNSUPPORTED and "EXT_HIER" in str(e.value)
        assert untouched(bufs)


def test_argument_errors_and_empty_shapes(ctx):
    import ctypes as C
    dev = torch.device("cuda", ctx.device)
    tr, o = trace_case(5, 65)
    d, out = device_replay(ctx, ("trace", 5, 65), tr)
    who = torch.from_numpy(draw_users(1, 3, 65, 4, "rr")).to(dev)
    uu, ud = (torch.from_numpy(x).to(dev) for x in draw_links(2, 3, 4, False))
    V, T = 5 + 1 + 12, 65
    bufs = poisoned_bufs(dev, 3, V, T)
    p = fa.engine._ptr
    bi = _abi.BatchIn(3, T, 5, 1, 5, 0, *(p(d[k]) for k in ("arrive", "req", "mips", "dl", "ul", "init")))

    def call(user_of=p(who), U=4, stride=0, ul=p(uu), dl=p(ud), r0=0, Rv=3, cap=6 * T, offset=p(bufs["offset"]),
             time=p(bufs["time"]), start=p(out.start_tick), null_vec=False):
        bo = _abi.BatchOut(p(out.node), p(out.status), start, p(out.done_tick), p(out.stats))
        vec = _abi.SignalVectors(cap, offset, time, p(bufs["value"]), p(bufs["task"]))
        return ctx._lib.fognet_signal_vectors_dev(ctx.handle, C.byref(bi), C.byref(bo), user_of, U, stride, ul, dl, r0, Rv,
                                                  None if null_vec else C.byref(vec), p(bufs["n_unassigned"]), None)
    for bad in (dict(start=None), dict(user_of=None), dict(ul=None), dict(dl=None), dict(U=-1), dict(stride=3),
                dict(cap=6 * T - 1), dict(offset=None), dict(time=None), dict(null_vec=True), dict(r0=-1), dict(Rv=-1),
                dict(r0=1, Rv=3)):
        assert call(**bad) == _abi.FOGNET_ERR_ARG, bad
    so = fa.run_batch(ctx, d, out=fa.allocate_outputs(3, 65, dev, per_task=False))
    with pytest.raises(fa.FognetError) as e:
        fa.signal_vectors(ctx, d, so, who, uu, ud, bufs=bufs)  # a statistics-only out
    assert e.value.code == _abi.FOGNET_ERR_ARG
    assert untouched(bufs)
    assert call() == _abi.FOGNET_OK  # a larger capacity than 6 T is fine as well
    want = sv.expected(tr, o, who.cpu().numpy(), uu.cpu().numpy(), ud.cpu().numpy())
    sv.assert_equal({k: v.cpu().numpy() for k, v in bufs.items()}, want)
    # U = 0: the nodes' vectors alone, every decided publish unassigned
    g = fa.signal_vectors(ctx, d, out, who, np.zeros(0, np.int64), np.zeros(0, np.int64), allow_unassigned=True)
    assert list(g["n_unassigned"]) == [65, 65, 65] and g["offset"].shape == (3, 7)
    np.testing.assert_array_equal(g["offset"][:, :6], want["offset"][:, :6])
    assert (g["offset"][:, 6] == g["offset"][:, 5]).all()
    # T = 0: all-zero offsets; Rv = 0: nothing
    t0 = {k: (v[:, :0] if k in ("arrive", "req") else v) for k, v in tr.items()}
    d0 = fa.as_device_trace(t0, dev)
    g = fa.signal_vectors(ctx, d0, fa.run_batch(ctx, d0), np.zeros((3, 0), np.int32), uu, ud)
    assert g["offset"].shape == (3, V + 1) and (g["offset"] == 0).all() and g["time"].shape == (3, 0)
    g = fa.signal_vectors(ctx, d, out, who, uu, ud, r0=3, Rv=0)
    assert g["offset"].shape == (0, V + 1)


# ---------------------------------------------------------------- buffer contract

def guarded_run(ctx, tr, who, uu, ud, poison, misalign):
    dev = torch.device("cuda", ctx.device)
    ain, aout = Arena(dev, poison), Arena(dev, poison)
    d = {k: ain.put(v, misalign, name=k) for k, v in tr.items()}
    g_who, g_uu, g_ud = ain.put(who, misalign, "user_of"), ain.put(uu, misalign, "user_ul"), ain.put(ud, misalign, "user_dl")
    R, T = d["arrive"].shape
    V = d["mips"].shape[-1] + 1 + 3 * uu.shape[-1]
    out = fa.BatchResult(node=aout.alloc((R, T), torch.int32, misalign, "node"), status=aout.alloc((R, T), torch.uint8, misalign, "status"),
                         start_tick=aout.alloc((R, T), torch.int64, misalign, "start"),
                         done_tick=aout.alloc((R, T), torch.int64, misalign, "done"),
                         stats=aout.alloc(R * REP.itemsize // 8, torch.int64, misalign, "stats").view(torch.uint8))
    fa.run_batch(ctx, d, out=out)
    bufs = dict(offset=aout.alloc((R, V + 1), torch.int64, misalign, "offset"), time=aout.alloc((R, 6 * T), torch.int64, misalign, "time"),
                value=aout.alloc((R, 6 * T), torch.int64, misalign, "value"), task=aout.alloc((R, 6 * T), torch.int32, misalign, "task"),
                n_unassigned=aout.alloc((R,), torch.int64, misalign, "n_unassigned"))
    if misalign:
        assert g_who.data_ptr() % 8 == 4 and bufs["task"].data_ptr() % 8 == 4 and bufs["offset"].data_ptr() % 16 == 8
    g = fa.signal_vectors(ctx, d, out, g_who, g_uu, g_ud, bufs=bufs, allow_unassigned=True)
    torch.cuda.synchronize()
    ain.check()
    aout.check()
    return g


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,N,U", [(65, 5, 10), (191, 5, 3), (191, 64, 129)])
def test_buffer_contract(ctx, monkeypatch, mode, T, N, U):
    set_mode(monkeypatch, mode)
    tr, o = trace_case(N, T)
    who = draw_users(T + U, 3, T, U, "random")
    who[1, T // 2] = U  # one past the last user
    uu, ud = draw_links(T + U + 1, 3, U, True)
    want = sv.expected(tr, o, who, uu, ud)
    runs = [(guarded_run(ctx, tr, who, uu, ud, p, m), p) for p, m in ((0xA5, False), (0x5A, False), (0xA5, True))]
    for g, poison in runs:
        sv.assert_equal(g, want, mode)
        assert list(g["n_unassigned"]) == [0, 1, 0]
        for q in range(3):  # rows at and past offset[V] still hold the poison
            n = int(want["offset"][q, -1])
            assert n < 6 * T
            for k in ("time", "value", "task"):
                assert (g[k][q][n:].view(np.uint8) == poison).all(), (k, q)
    for g, _ in runs[1:]:  # two poisons, and natural alignment: identical bytes
        for q in range(3):
            n = int(want["offset"][q, -1])
            for k in ("time", "value", "task"):
                assert g[k][q][:n].tobytes() == runs[0][0][k][q][:n].tobytes()
        assert g["offset"].tobytes() == runs[0][0]["offset"].tobytes()


def test_dirty_scratch_a_larger_job_first_then_a_smaller_one(monkeypatch):
    """The cursors in the workspace (HBM mode) are set by the pass itself: a smaller job after a
    larger one, and a rerun, do not depend on what the workspace held."""
    set_mode(monkeypatch, "hbm")
    c = fa.Context(0)
    try:
        dev = torch.device("cuda", c.device)
        jobs = []
        for N, T, U in ((64, 300, 10), (5, 65, 3), (64, 300, 10), (5, 65, 3)):
            tr, o = trace_case(N, T)
            who = draw_users(T + U, 3, T, U, "random")
            uu, ud = draw_links(T + U + 1, 3, U, True)
            d = fa.as_device_trace(tr, dev)
            out = fa.run_batch(c, d)
            g = fa.signal_vectors(c, d, out, who, uu, ud)
            sv.assert_equal(g, sv.expected(tr, o, who, uu, ud), f"N={N} T={T}")
            jobs.append(g)
        for a, b in ((0, 2), (1, 3)):
            sv.assert_equal(jobs[a], jobs[b], "rerun")
    finally:
        c.close()


# ---------------------------------------------------------------- streams

@pytest.fixture(scope="module")
def gate(ctx):
    g = stream_gate.Gate(torch.device("cuda", ctx.device))
    try:
        g.choose()
    except stream_gate.NoPower as e:
        pytest.skip(str(e))
    yield g
    g.write()


def stream_arrays(decoy: bool) -> dict:
    ds = 100 if decoy else 0
    N, T, U = 5, 129, 3
    tr = tg.make_batch(0x9E5 + 7 * N + T + ds, 3, N, T, rho=0.9) if decoy else trace_case(N, T)[0]
    uu, ud = draw_links(T + U + 1 + ds, 3, U, True)
    return dict(tr, user_of=draw_users(T + U + ds, 3, T, U, "rr" if decoy else "random"), user_ul=uu, user_dl=ud)


class StreamJob:
    def __init__(self, ctx, arrays):
        dev = torch.device("cuda", ctx.device)
        self.inputs = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in arrays.items()}
        R, T = self.inputs["arrive"].shape
        V = self.inputs["mips"].shape[-1] + 1 + 3 * self.inputs["user_ul"].shape[-1]
        self.out = fa.allocate_outputs(R, T, dev)
        self.bufs = dict(offset=torch.empty((R, V + 1), dtype=torch.int64, device=dev),
                         time=torch.empty((R, 6 * T), dtype=torch.int64, device=dev),
                         value=torch.empty((R, 6 * T), dtype=torch.int64, device=dev),
                         task=torch.empty((R, 6 * T), dtype=torch.int32, device=dev),
                         n_unassigned=torch.empty((R,), dtype=torch.int64, device=dev))


def stream_call(ctx, j: StreamJob):
    """The replay and the vectors, chained on the current stream; nothing is read back."""
    d = j.inputs
    fa.run_batch(ctx, d, out=j.out)
    fa.signal_vectors(ctx, d, j.out, d["user_of"], d["user_ul"], d["user_dl"], bufs=j.bufs, to_host=False)


@pytest.mark.parametrize("mode", MODES)
def test_gated_on_a_side_stream(ctx, gate, monkeypatch, mode):
    """Every kernel of the pass goes to the caller's stream, and the call only enqueues: behind a
    gate on a side stream it computes from the real inputs, byte-identical to the plain run."""
    set_mode(monkeypatch, mode)
    a = stream_arrays(False)
    tr, o = trace_case(5, 129)
    want = sv.expected(tr, o, a["user_of"], a["user_ul"], a["user_dl"])
    j = StreamJob(ctx, a)
    stream_call(ctx, j)
    torch.cuda.synchronize()
    plain = {k: v.cpu().numpy() for k, v in j.bufs.items()}
    sv.assert_equal(plain, want, "plain")
    job = gate.run("vectors", f"vectors-{mode}", lambda: StreamJob(ctx, stream_arrays(False)), stream_arrays(True),
                   lambda jb: stream_call(ctx, jb))
    got = {k: v.cpu().numpy() for k, v in job.bufs.items()}
    sv.assert_equal(got, want, "gated")
    sv.assert_equal(got, plain, "gated against plain")
    assert (got["n_unassigned"] == 0).all()


# ---------------------------------------------------------------- the driver

def test_driver_vec_users(ctx, tmp_path):
    """fognet_replay --vec f --vec-users appends replication 0's delay vector and three vectors per
    user module, in emission order; the times equal the restatement's on the same trace, regenerated
    through fognet_gen_trace_mqtt with the driver's seed.  Without the flag the .vec is unchanged."""
    from decimal import Decimal
    from fognetsimpp_amd import formats
    from test_driver import INI, MS, SEC, drive
    a, b, trc = (str(tmp_path / n) for n in ("a.vec", "b.vec", "g.fogntrc"))
    args = ("-f", INI, "--users", "user[3]", "--reps", "2")
    drive(*args, "--vec", a, "--vec-users", "--trace-out", trc)
    drive(*args, "--vec", b)
    plain, text = open(b, "rb").read(), open(a, "rb").read()
    assert text.startswith(plain) and text.count(b"version 2") == 1 and b".user[" not in plain and b"delay:vector" not in plain
    tr = formats.load_trace(trc)
    tr = {k: tr[k] for k in ("arrive", "req", "mips", "dl", "ul", "init")}
    gens = [formats.gen_trace_mqtt(1 + r, [200 * MS] * 3, [1500 * MS] * 3, [MS] * 3, [MS] * 3, 300 * SEC) for r in range(2)]
    np.testing.assert_array_equal(tr["arrive"][0], gens[0]["arrive"])
    who = np.stack([g["user"] for g in gens]).astype(np.int32)
    links = np.full(3, MS, np.int64)  # --user-ul / --user-dl defaults
    o = replay_oracle(tr)
    assert (o["stats"]["status"] == 0).all()
    N, U = tr["mips"].shape[-1], 3
    want = sv.expected(tr, o, who, links, links, r0=0, Rv=1)
    lines = text[len(plain):].decode().splitlines()
    decl = {int(ln.split()[1]): (ln.split()[2], ln.split()[3]) for ln in lines if ln.startswith("vector ")}
    assert decl[N + 1] == ("FogNet5.broker.udpApp[0]", "delay:vector")
    for u in range(U):
        for s, name in enumerate(("latency", "latencyH1", "taskTime")):
            assert decl[N + 2 + 3 * u + s] == (f"FogNet5.user[{u}].udpApp[0]", f"{name}:vector"), (u, name)
    assert len(decl) == 1 + 3 * U
    rows = {i: [] for i in decl}
    for ln in lines:
        if ln[:1].isdigit():
            i, t, _ = ln.split("\t")
            rows[int(i)].append(int(Decimal(t) * 10**12))
    off, time = want["offset"][0], want["time"][0]
    for i in decl:
        v = N if i == N + 1 else N + 1 + ((i - N - 2) % 3) * U + (i - N - 2) // 3
        assert rows[i] == [int(x) for x in time[off[v]:off[v + 1]]], decl[i]
        assert rows[i] == sorted(rows[i])
    assert all(rows[N + 2 + 3 * u + 1] for u in range(U))  # every user has latencyH1 rows: its pubAcks
