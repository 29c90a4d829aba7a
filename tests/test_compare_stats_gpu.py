"""Paired comparison on the device (fognet_compare_dev, fognet_reduce_compare_dev), byte for byte
against the plain-integer reference (compare_ref).  The pass takes any device arrays, so most
cases fabricate the two outputs with numpy; the real replays add the identities that tie the
record to the two runs' own statistics."""
from __future__ import annotations

import ctypes as C
import random
import re

import numpy as np
import pytest
import torch

import compare_ref as cr
import fognetsimpp_amd as fa
import stream_gate
import tracegen as tg
from fognetsimpp_amd import _abi
from guarded import Arena
from test_parity_gpu import with_crashes

pytestmark = pytest.mark.gpu

CMP, REP = _abi.COMPARE_STATS_DTYPE, _abi.REP_STATS_DTYPE
BINS = _abi.HIST_BINS
TASK_KEYS = (("node", "node"), ("status", "status"), ("start", "start_tick"), ("done", "done_tick"))


def dev_of(ctx):
    return torch.device("cuda", ctx.device)


def fabricate(seed: int, R: int, T: int, like: dict | None = None) -> dict:
    """Host arrays of one replay's outputs: random nodes, statuses in {4, 5, 9}, start and done with
    -1 sprinkled in.  like: another output, of which about a third of the tasks keep node / ticks."""
    rng = np.random.default_rng(seed)
    node = rng.integers(0, 7, (R, T)).astype(np.int32)
    status = rng.choice(np.array([4, 5, 9], np.uint8), (R, T))
    start = rng.integers(0, 10**15, (R, T)).astype(np.int64)
    # service times from under a millisecond to 10^5 s, so that the differences reach many histogram bins
    done = start + (10.0 ** rng.uniform(6, 17, (R, T))).astype(np.int64)
    if like is not None:
        same = rng.random((R, T)) < 0.33
        node, done = np.where(same, like["node"], node), np.where(same, like["done"], done)
    start[rng.random((R, T)) < 0.1] = -1
    done[rng.random((R, T)) < 0.15] = -1
    stats = np.zeros(R, REP)
    stats["n_tasks"] = T
    return dict(node=node, status=status, start=start, done=done, stats=stats)


def to_result(host: dict, dev, put=None) -> fa.BatchResult:
    """A BatchResult over device copies (put: where each array goes, e.g. an Arena's put)."""
    put = put or (lambda a, name: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    arrays = {attr: put(host[k], attr) for k, attr in TASK_KEYS}
    return fa.BatchResult(stats=put(host["stats"].view(np.uint8).reshape(-1), "stats"), **arrays)


def host_of(out: fa.BatchResult) -> dict:
    torch.cuda.synchronize()
    d = {k: getattr(out, attr).cpu().numpy() for k, attr in TASK_KEYS}
    d["stats"] = out.rep_stats().copy()
    return d


def device_compare(ctx, ra, rb, R):
    """(records [R], job record, hist [2][BINS]) of the device pass and its reduction."""
    h = torch.zeros((2, BINS), dtype=torch.int64, device=dev_of(ctx))
    buf = fa.compare(ctx, ra, rb, hist=h)
    job = fa.reduce_compare(ctx, buf, R)[0]
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(CMP).copy(), job, h.cpu().numpy()


def check(ctx, a: dict, b: dict, what: str):
    """Device records, job and histogram of (a, b) equal the reference; returns (records, job, hist, reference dicts)."""
    R = len(a["stats"])
    dev = dev_of(ctx)
    got, job, hist = device_compare(ctx, to_result(a, dev), to_result(b, dev), R)
    recs, want_job, want_hist = cr.compare(a, b)
    cr.assert_equal(got, cr.to_records(recs), what)
    cr.assert_equal(job, cr.to_record(want_job), what + " (job)")
    assert hist.tolist() == want_hist, what
    return got, job, hist, recs


# ---------------------------------------------------------------- shapes

@pytest.mark.parametrize("T", [1, 63, 64, 65, 257, 1000])
def test_fabricated_outputs_equal_the_reference(ctx, T):
    """T = 257 puts a wavefront into a second step of the row loop (4 wavefronts x 64 tasks a step)."""
    seen = 0
    for R in (1, 3, 5):
        a = fabricate(100 * T + R, R, T)
        b = fabricate(100 * T + R + 50, R, T, like=a)
        if R >= 3:  # the decided counts differ, and are clamped to [0, T]
            a["stats"]["n_tasks"][1], b["stats"]["n_tasks"][1] = T + 5, max(T - 3, 0)
            a["stats"]["n_tasks"][2], b["stats"]["n_tasks"][2] = T // 2, T + 1
        if R == 5:
            b["stats"]["n_tasks"][4] = -3
        got, job, hist, _ = check(ctx, a, b, f"T={T} R={R}")
        if R == 5:
            assert got["n_pairs"].tolist() == [T, max(T - 3, 0), T // 2, T, 0]
        assert int(job["n_reps"]) == R and hist.sum(axis=1).tolist() == [int(job["n_better"]), int(job["n_worse"])]
        seen += int(job["n_done_both"])
    assert seen > 0 or T == 1


# ---------------------------------------------------------------- carries

@pytest.mark.parametrize("T", [65, 257])
def test_limb_carries_negative_sums_and_a_foreign_status_byte(ctx, T):
    """Differences of +-(2^62 - 1): |sum| passes 2^64 and the sum is negative, each square is about
    2^124 so T of them carry through all three limbs of the square sum."""
    big = 2**62 - 1
    i = np.arange(T)
    pos = i % 3 == 0  # a third later, two thirds earlier: the signed sums are negative
    a = dict(node=np.zeros((1, T), np.int32), status=np.full((1, T), 5, np.uint8), stats=np.zeros(1, REP),
             start=np.where(pos, big, 0).astype(np.int64)[None], done=np.where(pos, 0, big).astype(np.int64)[None])
    b = dict(node=np.ones((1, T), np.int32), status=np.full((1, T), 4, np.uint8), stats=np.zeros(1, REP),
             start=np.where(pos, 0, big).astype(np.int64)[None], done=np.where(pos, big, 0).astype(np.int64)[None])
    a["stats"]["n_tasks"] = b["stats"]["n_tasks"] = T
    got, job, hist, recs = check(ctx, a, b, f"carries T={T}")
    d = recs[0]
    npos = int(pos.sum())
    assert d["d_resp"]["sum"] == (2 * npos - T) * big < -(2**64) and d["d_resp"]["sq"] == T * big * big >= 2**128
    assert d["d_start"]["sum"] == (T - 2 * npos) * big and d["d_service"]["sum"] == 2 * (2 * npos - T) * big
    assert d["d_service"]["min"] == -2 * big and d["d_service"]["max"] == 2 * big
    g = got[0]
    assert int(g["d_resp"]["sum_hi"]) >> 63 == 1 and int(g["d_resp"]["sq_top"]) > 0 and int(g["rep_better"]) == 1
    assert int(g["n_moved"]) == T and g["trans"].tolist() == [[0, T, 0], [0, 0, 0], [0, 0, 0]]
    # a status byte outside {4, 5, 9}: in no cell of trans, nothing else disturbed
    a2 = dict(a, status=a["status"].copy())
    a2["status"][0, 10] = 0xA5
    got2, _, hist2, _ = check(ctx, a2, b, f"foreign status T={T}")
    assert int(got2[0]["trans"].sum()) == int(got2[0]["n_pairs"]) - 1 == T - 1
    assert all(got2[k].tobytes() == got[k].tobytes() for k in CMP.names if k != "trans") and hist2.tolist() == hist.tolist()


# ---------------------------------------------------------------- real replays

_replays: dict = {}


def replays(ctx, N: int) -> dict:
    """One trace of 3 x 300 tasks on N nodes (5: the register kernel; 300: the wide kernel) under every
    rule the tests compare, replayed once."""
    if N not in _replays:
        dev = dev_of(ctx)
        tr = tg.make_batch(0xC0 + N, 3, N, 300, rho=1.5 if N == 5 else 0.05, lat_scale=1 if N == 5 else 10)
        d = fa.as_device_trace(tr, dev)
        outs = {"REF_V3": fa.run_batch(ctx, d), "EXT_LAT": fa.run_batch(ctx, d, policy="EXT_LAT"),
                "rr": fa.run_assigned(ctx, d, fa.assign_round_robin(3, 300, N, dev))}
        dd = fa.as_device_trace(with_crashes(tr, 7), dev)
        outs["REF_V3/down"] = fa.run_batch(ctx, dd)
        outs["rr/down"] = fa.run_assigned(ctx, dd, fa.assign_round_robin(3, 300, N, dev))
        dh = fa.as_device_trace(dict(tr, region=fa.mobility_regions(tr["arrive"], N, users=37)), dev)
        outs["EXT_HIER"] = fa.run_batch(ctx, dh, policy="EXT_HIER", hier_threshold_s=1)  # (no escalation flags kept)
        _replays[N] = {k: (o, host_of(o)) for k, o in outs.items()}
        for k, (_, h) in _replays[N].items():
            assert (h["stats"]["status"] == 0).all(), k
    return _replays[N]


def u128(s, lo, hi) -> int:
    return int(s[lo]) | (int(s[hi]) << 64)


@pytest.mark.parametrize("pair", [("REF_V3", "EXT_LAT"), ("REF_V3", "rr"), ("REF_V3/down", "rr/down"), ("EXT_HIER", "REF_V3")],
                         ids=lambda p: "-".join(p).replace("/", "_"))
@pytest.mark.parametrize("N", [5, 300])
def test_real_replays_and_their_identities(ctx, N, pair):
    rp = replays(ctx, N)
    (ra, a), (rb, b) = rp[pair[0]], rp[pair[1]]
    got, job, hist = device_compare(ctx, ra, rb, 3)
    recs, want_job, want_hist = cr.compare(a, b)
    cr.assert_equal(got, cr.to_records(recs), str(pair))
    cr.assert_equal(job, cr.to_record(want_job), str(pair) + " (job)")
    assert hist.tolist() == want_hist
    for r, d in enumerate(recs):
        sa, sb = a["stats"][r], b["stats"][r]
        assert d["n_pairs"] == 300 and d["d_start"]["sum"] + d["d_service"]["sum"] == d["d_resp"]["sum"]
        assert [sum(row) for row in d["trans"]][:2] == [int(sa["n_started"]), int(sa["n_queued"])]
        assert [sum(d["trans"][i][j] for i in range(3)) for j in range(2)] == [int(sb["n_started"]), int(sb["n_queued"])]
        if d["n_done_both"] == 300:  # every task completes in both
            assert d["d_resp"]["sum"] == u128(sb, "resp_sum_lo", "resp_sum_hi") - u128(sa, "resp_sum_lo", "resp_sum_hi")
            assert d["d_service"]["sum"] == (int(sb["busy_s"]) - int(sa["busy_s"])) * 10**12
    done_all = sum(d["n_done_both"] == 300 for d in recs)
    if "down" in pair[0]:
        assert sum(d["n_done_both"] for d in recs) < 900 and sum(sum(d["trans"][2]) + d["trans"][0][2] + d["trans"][1][2] for d in recs) > 0
    else:
        assert done_all == 3
    if pair[0] != "EXT_HIER":  # (one region at these N: the hierarchy may well decide as REF_V3 does)
        assert int(job["n_moved"]) > 0


def test_self_and_swap(ctx):
    rp = replays(ctx, 5)
    (ra, a), (rb, b) = rp["REF_V3/down"], rp["rr/down"]
    same, job, hist = device_compare(ctx, ra, ra, 3)
    for g in same:
        assert int(g["n_moved"]) == 0 and int(g["n_equal"]) == int(g["n_done_both"]) > 0 and int(g["rep_equal"]) == 1
        assert not (g["trans"] - np.diag(np.diag(g["trans"]))).any()
        for s in cr.SIGNALS:
            assert int(g[s]["min_raw"]) == int(g[s]["max_raw"]) == 0 and not int(g[s]["sum_lo"]) and not int(g[s]["sq_lo"])
    assert not hist.any()
    ab, jab, hab = device_compare(ctx, ra, rb, 3)
    ba, jba, hba = device_compare(ctx, rb, ra, 3)
    assert hba.tolist() == hab[::-1].tolist() and hab.any()
    for x, y in list(zip(ab, ba)) + [(jab, jba)]:
        dx, dy = cr.from_record(x), cr.from_record(y)
        assert dy["trans"] == [list(col) for col in zip(*dx["trans"])] and dy["n_moved"] == dx["n_moved"]
        assert (dy["n_better"], dy["n_equal"], dy["n_worse"]) == (dx["n_worse"], dx["n_equal"], dx["n_better"])
        assert (dy["rep_better"], dy["rep_equal"], dy["rep_worse"]) == (dx["rep_worse"], dx["rep_equal"], dx["rep_better"])
        assert (dy["n_done_only_a"], dy["n_done_only_b"], dy["n_done_both"]) == (dx["n_done_only_b"], dx["n_done_only_a"], dx["n_done_both"])
        for s in cr.SIGNALS:
            assert dy[s]["sum"] == -dx[s]["sum"] and dy[s]["sq"] == dx[s]["sq"] and dy[s]["count"] == dx[s]["count"]
            assert (dy[s]["min"], dy[s]["max"]) == (-dx[s]["max"], -dx[s]["min"])


# ---------------------------------------------------------------- a failed replication

@pytest.mark.parametrize("where", ["a", "b", "both"])
def test_a_failed_replication_gets_the_empty_record_and_is_not_read(ctx, where):
    R, T = 4, 257
    a = fabricate(900, R, T)
    b = fabricate(901, R, T, like=a)
    a["stats"]["status"][3] = _abi.FOGNET_REF_ABORTED  # keeps its record; out of hist and of the job
    clean_got, clean_job, clean_hist, _ = check(ctx, a, b, "before the failure")
    bad = 1
    for side, o in (("a", a), ("b", b)):
        if where in (side, "both"):
            o["stats"]["status"][bad] = _abi.FOGNET_ERR_ARG
            o["stats"]["n_tasks"][bad] = 2**40  # its rows and its record are poison
            o["node"][bad], o["status"][bad] = 0x5A5A5A5A, 0x5A
            o["start"][bad] = o["done"][bad] = 0x5A5A5A5A5A5A5A5A
    got, job, hist, _ = check(ctx, a, b, f"failed in {where}")
    want = cr.to_record(cr.empty(a["stats"]["status"][bad], b["stats"]["status"][bad]))
    assert got[bad].tobytes() == want.tobytes() and int(got[bad]["n_reps"]) == 0
    assert {int(got[bad]["status_a"]), int(got[bad]["status_b"])} == ({_abi.FOGNET_ERR_ARG} if where == "both" else {0, _abi.FOGNET_ERR_ARG})
    keep = [0, 2, 3]
    assert got[keep].tobytes() == clean_got[keep].tobytes()  # the neighbours: as in the run without the failure
    # the job and the histogram lose exactly replication 1; the aborted one was never in them
    assert int(clean_job["n_reps"]) == 3 and int(job["n_reps"]) == 2 and int(got[3]["n_reps"]) == 1 and int(got[3]["n_pairs"]) == T
    lost = cr.new_hist()
    cr.replication({k: v for k, v in fabricate(900, R, T).items()}, fabricate(901, R, T, like=fabricate(900, R, T)), bad, lost)
    assert (clean_hist - hist).tolist() == lost and hist.sum() == int(job["n_better"]) + int(job["n_worse"])


# ---------------------------------------------------------------- the buffer contract

@pytest.mark.parametrize("poison", [0xA5, 0x5A])
def test_guard_bands_poisoned_records_and_odd_offsets(ctx, poison):
    """cmp and hist between guard bands, cmp prefilled with poison (the arena's), hist added to, the inputs
    at odd element offsets: the records equal the reference and nothing outside cmp [R] and hist changes."""
    R, T = 3, 130
    a = fabricate(77, R, T)
    b = fabricate(78, R, T, like=a)
    arena = Arena(dev_of(ctx), poison, 1 << 20)
    put = lambda arr, name: arena.put(arr, misalign=arr.dtype != np.uint8 or name != "stats", name=name)  # noqa: E731
    ra, rb = to_result(a, arena.device, put), to_result(b, arena.device, put)
    cmp_buf = arena.alloc(R * CMP.itemsize, torch.uint8, misalign=False, name="cmp")
    hist = arena.alloc((2, BINS), torch.int64, misalign=True, name="hist")
    hist.zero_()
    recs, _, want_hist = cr.compare(a, b)
    for calls in (1, 2):
        fa.compare(ctx, ra, rb, res=cmp_buf, hist=hist)
        torch.cuda.synchronize()
        cr.assert_equal(cmp_buf.cpu().numpy().view(CMP), cr.to_records(recs), f"call {calls}")
        assert hist.cpu().numpy().tolist() == (np.array(want_hist) * calls).tolist()  # added to: two calls double it
        arena.check()
    assert np.array(want_hist).sum() > 0
    for o, h in ((ra, a), (rb, b)):  # the inputs are unchanged
        assert host_of(o)["done"].tobytes() == h["done"].tobytes() and o.rep_stats().tobytes() == h["stats"].tobytes()


# ---------------------------------------------------------------- a side stream

class StreamJob:
    """Plain device tensors of one comparison (stream_gate's job: ``inputs`` are the views the calls read)."""

    def __init__(self, ctx, a, b):
        dev = dev_of(ctx)
        self.a, self.b = to_result(a, dev), to_result(b, dev)
        self.inputs = {"a_done": self.a.done_tick, "b_node": self.b.node, "b_stats": self.b.stats}
        self.R = len(a["stats"])
        self.cmp = torch.empty(self.R * CMP.itemsize, dtype=torch.uint8, device=dev)
        self.job = torch.empty(CMP.itemsize, dtype=torch.uint8, device=dev)
        self.hist = torch.zeros((2, BINS), dtype=torch.int64, device=dev)


STREAM_POOL = 32  # side streams torch keeps per device and priority


def finish_the_rotation(gate, dev):
    """torch.cuda.Stream() hands out the streams of a fixed pool in rotation, and the hardware queue of a pool
    stream does not change.  Which streams a later module's gate is offered therefore depends on how many were
    taken before it; test_streams_gpu.py's host-pointer case needs a side stream off the context's own queue and
    is sensitive to that.  Take the rest of one rotation, so that the pool stands where this test found it."""
    took = len(gate.report["candidates"])
    rest = [torch.cuda.Stream(dev).cuda_stream for _ in range(-took % STREAM_POOL)]
    assert len(set(rest)) == len(rest), "the pool is smaller than STREAM_POOL"


def test_on_a_side_stream_behind_a_gate(ctx, monkeypatch, tmp_path):
    """The pass and the reduction run on the caller's stream and on no other: behind a gate their inputs
    still hold a decoy, so a launch on another stream computes other records."""
    monkeypatch.setenv(stream_gate.REPORT_ENV, str(tmp_path / "gate.json"))
    gate = stream_gate.Gate(dev_of(ctx))
    try:
        gate.choose(1)
    except stream_gate.NoPower as e:
        pytest.skip(str(e))
    finally:
        finish_the_rotation(gate, dev_of(ctx))
    R, T = 3, 257
    a = fabricate(31, R, T)
    b = fabricate(32, R, T, like=a)
    other = fabricate(33, R, T)
    other["stats"]["n_tasks"] = T - 1
    decoy = {"a_done": other["done"], "b_node": other["node"], "b_stats": other["stats"].view(np.uint8).reshape(-1)}

    def enqueue(j):
        fa.compare(ctx, j.a, j.b, res=j.cmp, hist=j.hist)
        ctx.check(ctx._lib.fognet_reduce_compare_dev(ctx.handle, fa.engine._ptr(j.cmp), j.R, fa.engine._ptr(j.job),
                                                     fa.engine._stream_ptr(j.cmp.device)), "reduction")

    recs, want_job, want_hist = cr.compare(a, b)
    job = gate.run("compare", "compare-T257", lambda: StreamJob(ctx, a, b), decoy, enqueue)
    cr.assert_equal(job.cmp.cpu().numpy().view(CMP), cr.to_records(recs), "gated")
    cr.assert_equal(job.job.cpu().numpy().view(CMP), cr.to_record(want_job), "gated (job)")
    assert job.hist.cpu().numpy().tolist() == want_hist
    decoyed = cr.compare(dict(a, done=other["done"]), dict(b, node=other["node"], stats=other["stats"]))[0]
    assert cr.to_records(decoyed).tobytes() != cr.to_records(recs).tobytes()  # (the decoy would have shown)


# ---------------------------------------------------------------- the reduction

@pytest.mark.parametrize("R", [0, 1, 4096, 4097])
def test_reduction_equals_the_host_merge_of_the_included_records(ctx, R):
    rng = random.Random(R)
    recs = np.zeros(R, CMP)
    flat = recs.view(np.uint64).reshape(R, CMP.itemsize // 8)
    flat[:] = np.frombuffer(rng.randbytes(flat.nbytes), np.uint64).reshape(flat.shape)
    for k in cr.COUNTS:
        recs[k] >>= 16  # counts that cannot overflow int64 when summed
    recs["trans"] >>= 16
    for s in cr.SIGNALS:
        recs[s]["count"] >>= 16
        recs[s]["overflow"] = 0
    recs["n_reps"] = 1
    pairs = [(0, 0), (0, 0), (0, 0), (0, _abi.FOGNET_REF_ABORTED), (_abi.FOGNET_REF_ABORTED, 0), (_abi.FOGNET_ERR_ARG, 0),
             (0, _abi.FOGNET_ERR_CAPACITY), (_abi.FOGNET_ERR_ARG, _abi.FOGNET_ERR_ARG)]
    st = [rng.choice(pairs) for _ in range(R)]
    if R >= 4096:  # the 128-thread stride's last rounds
        st[4095] = (0, 0)
        st[-1] = (0, 0) if R == 4097 else st[-1]
        st[4094] = (0, _abi.FOGNET_ERR_ARG)
    recs["status_a"], recs["status_b"] = [s[0] for s in st], [s[1] for s in st]
    dev = dev_of(ctx)
    buf = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev) if R else torch.empty(0, dtype=torch.uint8, device=dev)
    got = fa.reduce_compare(ctx, buf, R)[0]
    keep = np.array([r for r in range(R) if st[r] == (0, 0)], np.int64)
    host = fa.merge_compare(recs[keep])
    assert got.tobytes() == host.tobytes()
    assert int(got["n_reps"]) == len(keep) and int(got["status_a"]) == int(got["status_b"]) == 0
    if R == 0:
        assert got.tobytes() == cr.to_record(cr.empty()).tobytes()
    else:
        total = sum(u128(x["d_resp"], "sum_lo", "sum_hi") for x in recs[keep]) % 2**128  # (modulo 2^128, as the limbs wrap)
        assert u128(got["d_resp"], "sum_lo", "sum_hi") == total
        assert int(got["n_moved"]) == int(recs[keep]["n_moved"].sum())


# ---------------------------------------------------------------- refused calls

def test_refusals_leave_the_outputs_untouched(ctx):
    dev = dev_of(ctx)
    R, T = 2, 65
    a, b = fabricate(5, R, T), fabricate(6, R, T)
    ra, rb = to_result(a, dev), to_result(b, dev)
    res = torch.full((R * CMP.itemsize,), 0xCD, dtype=torch.uint8, device=dev)
    hist = torch.full((2, BINS), 0x0123456789ABCDEF, dtype=torch.int64, device=dev)
    ptr = fa.engine._ptr

    def call(oa=ra, ob=rb, cmp=res, R=R, T=T, drop_a=None, drop_b=None, null=None):
        bi = fa.engine._batch_in_dims(R, T)
        ba, bb = fa.engine._batch_out(oa), fa.engine._batch_out(ob)
        for bo, drop in ((ba, drop_a), (bb, drop_b)):
            if drop:
                setattr(bo, drop, None)
        args = [ctx.handle, C.byref(bi), C.byref(ba), C.byref(bb), ptr(cmp) if cmp is not None else None, ptr(hist), None]
        if null is not None:
            args[null] = None
        rc = ctx._lib.fognet_compare_dev(*args)
        torch.cuda.synchronize()
        return rc

    stats_only = fa.BatchResult(node=None, status=None, start_tick=None, done_tick=None, stats=ra.stats)
    bad = [dict(oa=stats_only), dict(ob=stats_only), dict(drop_a="start_tick"), dict(drop_b="done_tick"), dict(drop_a="node"),
           dict(drop_b="status"), dict(drop_a="stats"), dict(drop_b="stats"), dict(cmp=None), dict(R=-1), dict(T=-1),
           dict(null=1), dict(null=2), dict(null=3)]
    for kw in bad:
        assert call(**kw) == _abi.FOGNET_ERR_ARG, kw
    assert "per-task outputs" in (call(oa=stats_only) and ctx.last_error())
    untouched = lambda: (bytes(res.cpu().numpy()) == b"\xCD" * res.numel()  # noqa: E731
                         and bool((hist == 0x0123456789ABCDEF).all()))
    assert untouched()  # nothing was written by any of them
    with pytest.raises(fa.FognetError) as e:
        fa.compare(ctx, stats_only, stats_only)
    assert e.value.code == _abi.FOGNET_ERR_ARG
    job = torch.full((CMP.itemsize,), 0xCD, dtype=torch.uint8, device=dev)
    lib = ctx._lib
    assert lib.fognet_reduce_compare_dev(ctx.handle, ptr(res), -1, ptr(job), None) == _abi.FOGNET_ERR_ARG
    assert lib.fognet_reduce_compare_dev(ctx.handle, None, 2, ptr(job), None) == _abi.FOGNET_ERR_ARG
    assert lib.fognet_reduce_compare_dev(ctx.handle, ptr(res), 2, None, None) == _abi.FOGNET_ERR_ARG
    torch.cuda.synchronize()
    assert bytes(job.cpu().numpy()) == b"\xCD" * job.numel()
    # R = 0 succeeds and writes nothing, statistics-only outputs and NULL cmp included; T = 0 gives R records without pairs
    assert call(R=0) == call(R=0, oa=stats_only, ob=stats_only, cmp=None) == _abi.FOGNET_OK and untouched()
    assert call(T=0, oa=stats_only, ob=stats_only) == _abi.FOGNET_OK
    g = res.cpu().numpy().view(CMP)
    assert g["n_reps"].tolist() == [1, 1] and g["rep_equal"].tolist() == [1, 1] and not g["n_pairs"].any()
    assert bool((hist == 0x0123456789ABCDEF).all())
    want = cr.to_record(dict(cr.empty(), n_reps=1, rep_equal=1))
    assert g[0].tobytes() == want.tobytes()


# ---------------------------------------------------------------- the driver

def test_driver_appends_the_block_of_the_two_replays(ctx, tmp_path):
    """fognet_replay --compare random:7: the appended block parses, counts 3 x T pairs and equals the
    reference applied to the two replays run through the binding on the driver's own trace."""
    from fognetsimpp_amd import formats
    from test_assigned_driver import Mt19937_64
    from test_compare_stats import check_block, parse
    from test_driver import INI, drive
    sca, plain, trc = (str(tmp_path / n) for n in ("a.sca", "b.sca", "a.fogntrc"))
    R = 3
    args = ("-f", INI, "--users", "user[6]", "--reps", str(R))
    out = drive(*args, "--sca", sca, "--trace-out", trc, "--compare", "random:7").stdout
    drive(*args, "--sca", plain)
    text, before = open(sca).read(), open(plain).read()
    assert text.startswith(before) and "compare:" not in before and text.count("version 2") == 1
    tr = formats.load_trace(trc)
    T, N = tr["arrive"].shape[1], len(tr["mips"])
    dev = dev_of(ctx)
    d = fa.as_device_trace(tr, dev)
    gens = [Mt19937_64(7 + r) for r in range(R)]
    assign = torch.tensor([[g() % N for _ in range(T)] for g in gens], dtype=torch.int32, device=dev)
    a, b = host_of(fa.run_batch(ctx, d)), host_of(fa.run_assigned(ctx, d, assign))
    _, job, hist = cr.compare(a, b)
    scal, stats = parse(text[len(before):])
    mod = re.search(r"^attr network (\S+)$", text, re.M).group(1) + ".compare"  # the ini's network
    assert list(scal) == [mod] and int(scal[mod]["compare:pairs"]) == R * T
    check_block(scal, stats, mod, job, hist)
    mean = job["d_resp"]["sum"] / job["d_resp"]["count"] / 1e9
    line = next(ln for ln in out.splitlines() if ln.startswith("compare "))
    assert f"A=REF_V3 B=assign:random:7 reps={R} pairs={R * T} moved={job['n_moved']} better={job['n_better']} " \
           f"equal={job['n_equal']} worse={job['n_worse']} mean_response_diff_ms=" in line
    assert abs(float(line.rsplit("=", 1)[1]) - mean) <= 1e-8 * abs(mean)
    assert "compare " not in drive(*args, "--sca", sca, "--compare", "EXT_LAT", "--quiet").stdout
