"""Per-node statistics on the device (fognet_node_stats_dev, fognet_reduce_node_stats_dev)
against records built in Python integers from the ORACLE's per-task outputs
(node_stats_ref), in both accumulator layouts (LDS; FOGNET_NODE_STATS=hbm), and the
defining invariant against the device's own fognet_rep_stats."""
from __future__ import annotations

import random

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import node_stats_ref as ns
import oracle_lib as ol
import tracegen as tg
from fognetsimpp_amd import _abi
from guarded import Arena
from test_parity_gpu import with_crashes

pytestmark = pytest.mark.gpu

NODE, REP = _abi.NODE_STATS_DTYPE, _abi.REP_STATS_DTYPE
LDS_CAP = 256  # node_stats.hip kNodeLdsMax: N = 257 is the first size above it
LAYOUTS = ("lds", "hbm")
_oracle: dict = {}


def oracle(key, make, policy="REF_V3"):
    """(trace, oracle result, expected records), computed once per key and left unchanged."""
    if key not in _oracle:
        tr = make()
        o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=4,
                         policy=ol.POLICIES[policy], down=tr.get("down"))
        _oracle[key] = (tr, o, ns.expected(tr, o))
    return _oracle[key]


def set_layout(monkeypatch, layout):
    if layout == "hbm":
        monkeypatch.setenv("FOGNET_NODE_STATS", "hbm")
    else:
        monkeypatch.delenv("FOGNET_NODE_STATS", raising=False)


def device_records(ctx, tr, policy="REF_V3", **kw):
    """Replay on the device, then the node pass: ([R, N] records, rep records, device buffers)."""
    d = fa.as_device_trace(tr, torch.device("cuda", ctx.device))
    out = fa.run_batch(ctx, d, policy=policy, **kw)
    buf = fa.node_stats(ctx, d, out, policy=policy)
    torch.cuda.synchronize()
    R, N = d["arrive"].shape[0], d["mips"].shape[-1]
    return buf.cpu().numpy().view(NODE).reshape(R, N), out.rep_stats(), (d, out, buf)


def check(ctx, monkeypatch, tr, o, want, policy="REF_V3", **kw):
    """Both layouts equal the oracle's records, and merge to the device's own rep records."""
    got = {}
    for layout in LAYOUTS:
        set_layout(monkeypatch, layout)
        g, st, _ = device_records(ctx, tr, policy, **kw)
        np.testing.assert_array_equal(np.isin(st["status"], ns.OK_STATUSES), np.isin(o["stats"]["status"], ns.OK_STATUSES))
        ns.assert_records_equal(g, want, layout)
        for r in range(g.shape[0]):
            if int(st["status"][r]) in ns.OK_STATUSES:
                ns.assert_merge_is_rep_record(g[r], st[r])
        got[layout] = g
    assert got["lds"].tobytes() == got["hbm"].tobytes()
    return got["lds"]


# ---------------------------------------------------------------- 1 + 5: parity, invariant

@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
@pytest.mark.parametrize("N", [1, 5, 64, 65, 256, LDS_CAP + 1])
def test_parity_with_oracle_both_layouts(ctx, monkeypatch, N, policy):
    for T in (1, 63, 64, 65, 129, 191):
        for shared in (False, True):
            def make():
                tr = tg.make_batch(0x0D5 + 7 * N + T, 3, N, T, rho=0.9)
                return dict(tr, **{k: tr[k][0] for k in ("mips", "dl", "ul", "init")}) if shared else tr
            tr, o, want = oracle((N, T, shared, policy), make, policy)
            check(ctx, monkeypatch, tr, o, want, policy)


@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
def test_parity_ten_thousand_nodes(ctx, monkeypatch, policy):
    tr, o, want = oracle(("10k", policy), lambda: tg.make_batch(0x10000, 3, 10000, 2000, rho=0.9), policy)
    g = check(ctx, monkeypatch, tr, o, want, policy)
    assert (g["n_tasks"] == 0).any() and (g["n_tasks"].sum(axis=1) == 2000).all()  # nodes without a task too


# ---------------------------------------------------------------- 2: herded

def test_herded_node_carries_overflows_and_negative_queue_time(ctx, monkeypatch):
    tr, o, want = oracle("herded", ns.herded_trace)
    node, status, start = o["node"][0], o["status"][0], o["start"][0]
    on0 = node == 0
    assert on0.sum() > 200 and on0[:64].all() and on0[64:128].all()  # whole 64-task steps on one node
    raws = [ol.qtime_raw(int(start[i]), int(tr["arrive"][0, i]) + int(tr["dl"][0]))
            for i in np.nonzero(on0 & (status == 4) & (start >= 0))[0]]
    vals = [v for v in raws if v is not None]
    assert sum(vals) >> 64 > 0                      # carries out of sum_lo
    q = sum(v * v for v in vals)
    assert q >> 128 > 0                             # carries out of sq_lo and sq_hi, into sq_top
    assert raws.count(None) > 0 and min(vals) < 0   # an overflowing emission; a same-tick pop's negative value
    rec = want[0, 0]
    assert int(rec["queue"]["overflow"]) == raws.count(None) and int(rec["queue"]["sq_top"]) == q >> 128
    assert int(rec["queue"]["min_raw"]) == min(vals) < 0 and int(rec["queue"]["sum_hi"]) == sum(vals) >> 64
    check(ctx, monkeypatch, tr, o, want)
    check(ctx, monkeypatch, tr, o, want, ref_abort=True)  # FOGNET_REF_ABORTED: outputs written in full, still counted


# ---------------------------------------------------------------- 3: spread

def spread_trace(N):
    """A light load that spreads: under EXT_LAT node j costs dl_j + (req / mips_j) s; with
    dl_j = j s and mips_j = 1000 (j + 1) a publish of 1000 J^2 MIPS is cheapest near node
    J - 1, and the publishes are 600 s apart, so every node is idle again (advertised busy
    0) at each decision.  J walks through a permutation of the nodes."""
    S = 10**12
    j = np.arange(N, dtype=np.int64)
    mips, dl = (1000 * (j + 1)).astype(np.int32), j * S
    ul = np.full(N, 10**9, np.int64)
    J = 1 + (37 * np.arange(320, dtype=np.int64)) % N
    arrive = 10 * S + 600 * S * np.arange(320, dtype=np.int64)
    return dict(arrive=arrive[None], req=(1000 * J * J).astype(np.int32)[None], mips=mips, dl=dl, ul=ul, init=ul.copy())


@pytest.mark.parametrize("N", [64, 256])
def test_spread_case(ctx, monkeypatch, N):
    tr, o, want = oracle(("spread", N), lambda: spread_trace(N), "EXT_LAT")
    assert (o["stats"]["status"] == 0).all()
    most = max(len(set(o["node"][0, c:c + 64].tolist())) for c in range(0, 320, 64))
    assert most >= 48, most
    check(ctx, monkeypatch, tr, o, want, "EXT_LAT")


# ---------------------------------------------------------------- 4: node-down

def down_trace(kind):
    """A crash of node 0 mid-run, exactly at one of its completion ticks, or exactly at
    the tick a task reaches it (found from a crash-free oracle run of the same trace)."""
    tr = tg.make_batch(0xD0D0, 3, 5, 300, rho=1.5, lat_scale=10)
    tr = dict(tr, down=np.full(tr["mips"].shape, fa.NEVER, np.int64))
    o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=3)
    for r in range(3):
        i = int(np.nonzero(o["node"][r] == 0)[0][20])  # node 0's 21st task
        tr["down"][r, 0] = {"mid": int(o["done"][r, i]) - 12345, "completion": int(o["done"][r, i]),
                            "arrival": int(tr["arrive"][r, i]) + int(tr["dl"][r, 0])}[kind]
        tr["down"][r, 3] = int(tr["arrive"][r, 150])
    return tr


@pytest.mark.parametrize("kind", ["mid", "completion", "arrival"])
def test_node_down(ctx, monkeypatch, kind):
    tr, o, want = oracle(("down", kind), lambda: down_trace(kind))
    assert (o["stats"]["status"] == 0).all()
    assert (o["status"] == 9).any() and (want["n_lost"] > 0).any()                 # lost tasks
    assert ((o["status"] != 9) & (o["done"] == -1)).any()                           # accepted, never completed
    assert ((o["status"] == 4) & (o["start"] >= 0) & (o["done"] == -1)).any()       # queued, started, never completed
    check(ctx, monkeypatch, tr, o, want)


def test_node_down_random_crashes_ext_lat(ctx, monkeypatch):
    tr, o, want = oracle("down-extlat", lambda: with_crashes(tg.make_batch(0xD1, 3, 40, 400, rho=0.9, lat_scale=10), seed=40),
                         "EXT_LAT")
    assert ((o["status"] == 9) | (o["done"] == -1)).any()
    check(ctx, monkeypatch, tr, o, want, "EXT_LAT")


# ---------------------------------------------------------------- 5: a C4-shaped job

def test_invariant_c4_shape(ctx, monkeypatch):
    tr, o, want = oracle("c4", lambda: tg.make_batch(0xC4, 64, 256, 300, sweep=True))
    check(ctx, monkeypatch, tr, o, want)


# ---------------------------------------------------------------- 6: failed and refused

def failed_trace():
    tr = {k: v.copy() for k, v in tg.make_batch(0xFA11, 5, 100, 191, rho=0.9).items()}
    tr["mips"][2, 0] = 0                                  # refused before its first decision
    tr["arrive"][3, 127] = tr["arrive"][3, 126] - 1       # fails in mid-trace
    return tr


def failed_case():
    """The oracle refuses replication 2 (MIPS 0) but replays replication 3's out-of-order
    publish as it comes; the library refuses that precondition (FOGNET_ERR_ARG, as in
    test_buffer_contract_gpu's "unsorted" cases), so the expected rows of both are empty."""
    if "failed" not in _oracle:
        tr, o, _ = oracle("failed-raw", failed_trace)
        assert int(o["stats"]["status"][2]) not in ns.OK_STATUSES and int(o["stats"]["n_tasks"][2]) == 0
        st = o["stats"].copy()
        st["status"][3] = _abi.FOGNET_ERR_ARG
        o = dict(o, stats=st)
        _oracle["failed"] = (tr, o, ns.expected(tr, o))
    return _oracle["failed"]


def test_failed_replications_get_empty_rows(ctx, monkeypatch):
    tr, o, want = failed_case()
    assert [int(s) in ns.OK_STATUSES for s in o["stats"]["status"]] == [True, True, False, False, True]
    g = check(ctx, monkeypatch, tr, o, want)
    empty = ns.empty_records(100)
    assert g[2].tobytes() == empty.tobytes() == g[3].tobytes()
    _, st, _ = device_records(ctx, tr)
    assert int(st["n_tasks"][2]) == 0 and 0 < int(st["n_tasks"][3]) < 191  # before its first decision; in mid-trace
    assert (g[[0, 1, 4]]["n_tasks"].sum(axis=1) == 191).all()


def test_refusals_and_empty_shapes(ctx):
    dev = torch.device("cuda", ctx.device)
    tr = tg.make_batch(3, 2, 8, 65)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_batch(ctx, d)
    with pytest.raises(fa.FognetError) as e:
        fa.node_stats(ctx, d, out, policy="EXT_HIER")
    assert e.value.code == _abi.FOGNET_ERR_UNSUPPORTED and "escalated" in str(e.value)
    so = fa.run_batch(ctx, d, out=fa.allocate_outputs(2, 65, dev, per_task=False))
    with pytest.raises(fa.FognetError) as e:
        fa.node_stats(ctx, d, so)
    assert e.value.code == _abi.FOGNET_ERR_ARG
    bi = _abi.BatchIn(2, 65, 8, 1, 8, 0, *(fa.engine._ptr(d[k]) for k in ("arrive", "req", "mips", "dl", "ul", "init")))
    bo = _abi.BatchOut(*(fa.engine._ptr(t) for t in (out.node, out.status, out.start_tick, out.done_tick, out.stats)))
    import ctypes as C
    rc = ctx._lib.fognet_node_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), None, None)
    assert rc == _abi.FOGNET_ERR_ARG
    # T = 0: only empty records; R = 0: nothing
    t0 = {k: (v[:, :0] if k in ("arrive", "req") else v) for k, v in tr.items()}
    g, st, _ = device_records(ctx, t0)
    assert g.tobytes() == np.stack([ns.empty_records(8)] * 2).tobytes()
    empty = fa.as_device_trace({k: v[:0] for k, v in tr.items()}, dev)
    assert fa.node_stats(ctx, empty, fa.allocate_outputs(0, 65, dev)).numel() == 0
    red = fa.reduce_node_stats(ctx, torch.empty(0, dtype=torch.uint8, device=dev),
                               torch.empty(0, dtype=torch.uint8, device=dev), 0, 8)
    assert red.tobytes() == ns.empty_records(8).tobytes()


# ---------------------------------------------------------------- 7: buffer contract

def guarded_run(ctx, tr, poison, misalign):
    dev = torch.device("cuda", ctx.device)
    ain, aout = Arena(dev, poison), Arena(dev, poison)
    d = {k: ain.put(v, misalign, name=k) for k, v in tr.items()}
    R, T = d["arrive"].shape
    N = d["mips"].shape[-1]
    rec = lambda n, dt, name: aout.alloc(n * dt.itemsize // 8, torch.int64, misalign, name=name).view(torch.uint8)
    out = fa.BatchResult(node=aout.alloc((R, T), torch.int32, misalign, "node"), status=aout.alloc((R, T), torch.uint8, misalign, "status"),
                         start_tick=aout.alloc((R, T), torch.int64, misalign, "start"),
                         done_tick=aout.alloc((R, T), torch.int64, misalign, "done"), stats=rec(R, REP, "stats"))
    fa.run_batch(ctx, d, out=out)
    nodes, job = rec(R * N, NODE, "node_stats"), rec(N, NODE, "job_nodes")
    fa.node_stats(ctx, d, out, res=nodes)
    red = fa.reduce_node_stats(ctx, nodes, out.stats, R, N, out=job)
    torch.cuda.synchronize()
    ain.check()
    aout.check()
    return nodes.cpu().numpy().view(NODE).reshape(R, N).copy(), red.copy()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_buffer_contract(ctx, monkeypatch, layout):
    set_layout(monkeypatch, layout)
    tr, o, want = failed_case()
    runs = [guarded_run(ctx, tr, p, m) for p, m in ((0xA5, False), (0x5A, False), (0xA5, True))]
    for g, red in runs:
        ns.assert_records_equal(g, want, layout)
        ok = [r for r in range(5) if int(o["stats"]["status"][r]) == 0]
        ns.assert_records_equal(red, ns.to_records([ns.merged(want[ok, j]) for j in range(100)]), "reduction")
        assert g.tobytes() == runs[0][0].tobytes() and red.tobytes() == runs[0][1].tobytes()


# ---------------------------------------------------------------- 8: determinism

@pytest.mark.parametrize("layout", LAYOUTS)
def test_deterministic_and_independent_of_the_workspace(ctx, monkeypatch, layout):
    set_layout(monkeypatch, layout)
    tr, o, want = oracle("herded", ns.herded_trace)
    _, _, (d, out, buf) = device_records(ctx, tr)
    first = buf.cpu().numpy().copy()
    again = fa.node_stats(ctx, d, out).cpu().numpy()
    big = tg.make_batch(0xB16, 8, 300, 1500, rho=0.9)  # a larger job dirties the context's workspace
    device_records(ctx, big)
    third = fa.node_stats(ctx, d, out).cpu().numpy()
    assert first.tobytes() == again.tobytes() == third.tobytes()
    ns.assert_records_equal(first.view(NODE).reshape(1, -1), want)


# ---------------------------------------------------------------- 9: reduction

def random_records(rng, R, N) -> np.ndarray:
    recs = np.zeros((R, N), NODE)
    flat = recs.view(np.uint64).reshape(R, N, -1)
    flat[:] = np.frombuffer(rng.randbytes(flat.nbytes), np.uint64).reshape(flat.shape)
    for k in ("n_tasks", "n_queued", "n_started", "n_lost", "busy_s"):
        recs[k] >>= 24  # counts that cannot overflow int64 when summed
    for m in ("queue", "resp"):
        recs[m]["count"] >>= 24
        recs[m]["overflow"] >>= 24
        recs[m]["sq_top"] >>= np.uint64(16)
    return recs


@pytest.mark.parametrize("R,N", [(1, 3), (2, 3), (4097, 3), (70, 1000)])
def test_reduction_of_random_records(ctx, R, N):
    rng = random.Random(1000 * R + N)
    recs = random_records(rng, R, N)
    stats = np.zeros(R, REP)
    stats["status"] = [rng.choice((0, 0, 0, _abi.FOGNET_REF_ABORTED, _abi.FOGNET_ERR_ARG)) for _ in range(R)]
    for r in (0, 127, 128, R - 1):  # the edges of the reduction's 128-thread stride
        if r < R:
            stats["status"][r] = (_abi.FOGNET_ERR_CAPACITY, _abi.FOGNET_REF_ABORTED)[r & 1] if r else 0
    dev = torch.device("cuda", ctx.device)
    got = fa.reduce_node_stats(ctx, torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev),
                               torch.from_numpy(stats.view(np.uint8).reshape(-1)).to(dev), R, N)
    ok = np.nonzero(stats["status"] == 0)[0]
    want = []
    for j in range(N):
        m = ns.merged(recs[ok, j])
        m.queue.q %= 1 << 192
        m.resp.q %= 1 << 192
        want.append(m)
    ns.assert_records_equal(got, ns.to_records(want))
    half = [fa.reduce_node_stats(ctx, torch.from_numpy(recs[s].copy().view(np.uint8).reshape(-1)).to(dev),
                                 torch.from_numpy(stats[s].copy().view(np.uint8).reshape(-1)).to(dev), len(stats[s]), N)
            for s in (slice(0, R // 2), slice(R // 2, R))]
    assert fa.merge_node_stats(half).tobytes() == got.tobytes()  # the host merge of two shards


def test_reduction_of_a_real_job_matches_the_job_record(ctx):
    tr, o, want = oracle("c4", lambda: tg.make_batch(0xC4, 64, 256, 300, sweep=True))
    _, st, (d, out, buf) = device_records(ctx, tr)
    red = fa.reduce_node_stats(ctx, buf, out.stats, 64, 256)
    job = fa.reduce_stats(ctx, out.stats, 64)
    m = ns.merged(red)
    u192 = lambda a: int(a[0]) | (int(a[1]) << 64) | (int(a[2]) << 128)
    assert (m.tasks, m.queued, m.started, m.busy, m.last) == tuple(int(job[k]) for k in ("n_tasks", "n_queued", "n_started", "busy_s", "last_tick"))
    assert (m.queue.n, m.queue.ovf, m.queue.mn, m.queue.mx) == tuple(int(job[k]) for k in ("n_qtime", "n_qtime_overflow", "queue_min_raw", "queue_max_raw"))
    assert m.queue.s % (1 << 192) == u192(job["queue_sum"]) and m.queue.q == u192(job["queue_sq"])
    assert m.resp.s == u192(job["resp_sum"]) and m.resp.q == u192(job["resp_sq"])
    assert (m.resp.mn, m.resp.mx) == (int(job["resp_min_ticks"]), int(job["resp_max_ticks"]))
    ns.assert_records_equal(red, ns.to_records([ns.merged(want[:, j]) for j in range(256)]))


# ---------------------------------------------------------------- 10: the driver

def test_driver_node_stats_blocks(ctx, tmp_path):
    """fognet_replay --sca f --node-stats appends one block per fog node whose task
    counts are the tasks_per_node= line; without the flag the .sca is unchanged."""
    import re
    from test_driver import INI, drive
    from test_node_stats import blocks
    a, b, c = (str(tmp_path / n) for n in ("a.sca", "b.sca", "c.sca"))
    args = ("-f", INI, "--users", "user[10]", "--reps", "4")
    out = drive(*args, "--sca", a, "--node-stats").stdout
    drive(*args, "--sca", b)
    drive(*args, "--sca", c)
    plain = open(b, "rb").read()
    assert plain == open(c, "rb").read() and b"fogNode[" not in plain
    text = open(a, "rb").read()
    assert text.startswith(plain) and text.count(b"version 2") == 1
    per = [int(x) for x in re.search(r"tasks_per_node=([\d,]+)", out).group(1).split(",")]
    blk = blocks(text[len(plain):].decode())
    mods = [m for m in blk if ".fogNode[" in m]
    assert len(mods) == len(per) and sum(per) > 0
    for m in mods:
        j = int(re.search(r"fogNode\[(\d+)\]", m).group(1))
        assert int(blk[m]["scalars"]["tasks"]) == per[j]
        assert int(blk[m]["response:stats"]["count"]) == per[j]
