"""Every device entry point on a caller's side stream (include/fognet_hip.h, "Streams").

All other tests run on the null stream, where work that the library enqueued on another
stream than the caller's is still ordered and a host-side wait inside an enqueue-only
call cannot be seen.  Here every call runs on a non-blocking side stream behind a gate
(tests/stream_gate.py): its inputs hold a decoy until the gate opens, so a kernel, a
clear or a copy that went to the null stream or to the context's private stream runs
early, on the decoy or under the work that was meant to follow it, and the outputs differ
from the plain run's; a call that waits for the device is seen by the stream still being
gated when it returns.

(a) every case of the buffer-contract table (and the keyed passes with their reductions),
    gated, after a dirtying job on the same context: byte-identical to the plain run;
(b) one context on two streams ordered by an event;
(c) two contexts on two streams at once;
(d) the host-pointer calls while a gated device job of the same context waits;
(e) the EXT_HIER path choice belongs to the stream that measured it.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import node_stats_ref as ns
import oracle_lib as ol
import per_user_ref as pu
import stream_gate
import tracegen as tg
from fognetsimpp_amd import _abi
from test_buffer_contract_gpu import (CASES, JOB, REP, USER, Job, assert_user_parity, batch_inputs, build_guarded,
                                      call_guarded, check_against_oracle, collect_guarded,
                                      enqueue_user_stats, host, input_arrays, run_guarded, same_bytes, user_inputs)
from test_node_stats_gpu import LDS_CAP as NODE_LDS_CAP
from test_node_stats_gpu import oracle as node_oracle
from test_parity_gpu import assert_parity
from test_per_user_stats import draw_links, draw_users, trace_case
from test_per_user_stats_gpu import LDS_CAP as USER_LDS_CAP

pytestmark = pytest.mark.gpu

NODE = _abi.NODE_STATS_DTYPE
BY_ID = {c["id"]: c for c in CASES}
KEYED = [dict(id=f"nodestats-N{N}", kind="nodestats", N=N, T=65) for N in (5, NODE_LDS_CAP + 1)] + \
        [dict(id=f"peruser-U{U}", kind="peruser", U=U, T=65) for U in (10, USER_LDS_CAP + 1)]


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def cur(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---------------------------------------------------------------- the gate, the dirtying job

@pytest.fixture(scope="module")
def gate(ctx):
    g = stream_gate.Gate(torch.device("cuda", ctx.device))
    try:
        g.choose()
    except stream_gate.NoPower as e:
        pytest.skip(str(e))
    yield g
    g.write()


def make_dirty(c):
    """The hand-over case with ring 4 on plain tensors, run once so that it grows nothing later: it
    leaves a non-zero hand-over count, a used progress board and used rings in the workspace."""
    tr, kw, _ = batch_inputs(BY_ID["handover-3x4x191"])
    d = fa.as_device_trace(tr, torch.device("cuda", c.device))
    out = fa.allocate_outputs(3, 191, d["arrive"].device, N=4, energy="p_busy" in tr)
    run = lambda: fa.run_batch(c, d, out=out, **kw)
    run()
    torch.cuda.synchronize()
    assert out.rep_stats()["max_pending"][1] > 4  # it does hand over
    return run


@pytest.fixture(scope="module")
def dirty(ctx):
    return make_dirty(ctx)


# ---------------------------------------------------------------- the keyed passes and their reductions

def keyed_arrays(case, decoy=False):
    ds = 100 if decoy else 0
    if case["kind"] == "nodestats":
        N, T = case["N"], case["T"]
        if decoy:
            return dict(tg.make_batch(0x0D5 + 7 * N + T + ds, 3, N, T, rho=0.9))
        return dict(node_oracle((N, T, False, "REF_V3"), lambda: tg.make_batch(0x0D5 + 7 * N + T, 3, N, T, rho=0.9))[0])
    U, T = case["U"], case["T"]
    tr = tg.make_batch(0x9E5 + 7 * 5 + T + ds, 3, 5, T, rho=0.9) if decoy else trace_case(5, T)[0]
    who = draw_users(T + U + ds, 3, T, U, "rr" if decoy else "random")
    uu, ud = draw_links(T + U + 1 + ds, 3, U, True)
    return dict(tr, user_of=who, user_ul=uu, user_dl=ud)


def keyed_build(ctx, case, poison=0xA5, misalign=False) -> Job:
    j = Job(ctx, case, poison, misalign, arrays=keyed_arrays(case))
    R, T = j.inputs["arrive"].shape
    j.out = fa.BatchResult(j.new((R, T), torch.int32, "node"), j.new((R, T), torch.uint8, "status"),
                           j.new((R, T), torch.int64, "start_tick"), j.new((R, T), torch.int64, "done_tick"),
                           stats=j.records(R, REP, "stats"))
    if case["kind"] == "nodestats":
        N = case["N"]
        j.rows, j.red = j.records(R * N, NODE, "node_stats"), j.records(N, NODE, "job_nodes")
    else:
        U = case["U"]
        j.rows, j.red = j.records(R * U, USER, "per_user"), j.records(U, USER, "job_users")
        j.cnt = j.new((R,), torch.int64, "n_unassigned")
    return j


def keyed_call(ctx, j: Job):
    """The replay, the keyed pass and its job reduction, chained on the current stream; the
    reductions through the entry points themselves (their wrappers read the result back)."""
    case, d, out = j.case, j.inputs, j.out
    R = d["arrive"].shape[0]
    fa.run_batch(ctx, d, out=out)
    if case["kind"] == "nodestats":
        fa.node_stats(ctx, d, out, res=j.rows)
        rc = ctx._lib.fognet_reduce_node_stats_dev(ctx.handle, ptr(j.rows), ptr(out.stats), R, case["N"], ptr(j.red),
                                                   cur(j.rows.device))
    else:
        fa.per_user_stats(ctx, d, out, d["user_of"], d["user_ul"], d["user_dl"], res=j.rows, n_unassigned=j.cnt,
                          allow_unassigned=True)
        rc = ctx._lib.fognet_reduce_user_stats_dev(ctx.handle, ptr(j.rows), ptr(out.stats), R, case["U"], ptr(j.red),
                                                   cur(j.rows.device))
    ctx.check(rc, "reduction")


def keyed_collect(j: Job) -> dict:
    g = dict(rows=host(j.rows), red=host(j.red), stats=host(j.out.stats))
    if j.case["kind"] == "peruser":
        g["cnt"] = host(j.cnt)
    return g


def keyed_check(case, g):
    if case["kind"] == "nodestats":
        N, T = case["N"], case["T"]
        _, o, want = node_oracle((N, T, False, "REF_V3"), None)
        assert (o["stats"]["status"] == 0).all() and g["stats"].tobytes() == o["stats"].tobytes()
        ns.assert_records_equal(g["rows"].view(NODE).reshape(3, N), want, case["id"])
        ns.assert_records_equal(g["red"].view(NODE), ns.to_records([ns.merged(want[:, j]) for j in range(N)]), "reduction")
    else:
        U, T = case["U"], case["T"]
        tr, o = trace_case(5, T)
        a = keyed_arrays(case)
        want, un_want = pu.expected(tr, o, a["user_of"], a["user_ul"], a["user_dl"])
        assert g["stats"].tobytes() == o["stats"].tobytes()
        pu.assert_records_equal(g["rows"].view(USER).reshape(3, U), want, case["id"])
        assert list(g["cnt"]) == list(un_want) == [0, 0, 0]
        pu.assert_records_equal(g["red"].view(USER), np.array([pu.merged(want[:, u]) for u in range(U)], USER), "reduction")


def undamaged(j: Job, what: str):
    for a, name in zip(j.arenas, ("inputs", "outputs")):
        msg = a.damage()
        assert msg is None, f"{what}, {name} arena: {msg}"


# ---------------------------------------------------------------- (a)

@pytest.mark.parametrize("case", CASES + KEYED, ids=lambda c: c["id"])
def test_gated_on_a_side_stream(ctx, gate, dirty, monkeypatch, case):
    """Plainly on the default stream against the oracle (which also grows the workspace), then
    gated on the side stream: only enqueued, byte-identical, no arena damaged."""
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    keyed = case["kind"] in ("nodestats", "peruser")
    if keyed:
        j = keyed_build(ctx, case)
        keyed_call(ctx, j)
        torch.cuda.synchronize()
        plain = keyed_collect(j)
        undamaged(j, "plain")
        keyed_check(case, plain)
        job = gate.run(case["kind"], case["id"], lambda: keyed_build(ctx, case), keyed_arrays(case, decoy=True),
                       lambda jb: keyed_call(ctx, jb), dirty=dirty)
        got = keyed_collect(job)
    else:
        plain, arenas = run_guarded(ctx, case, 0xA5, False)
        for a in arenas:
            assert a.damage() is None
        check_against_oracle(ctx, case, plain)
        job = gate.run(case["kind"], case["id"], lambda: build_guarded(ctx, case, 0xA5, False),
                       input_arrays(ctx, case, decoy=True), lambda jb: call_guarded(ctx, jb, enqueue_only=True),
                       dirty=dirty if case["kind"] == "batch" else None)
        got = collect_guarded(ctx, job)
    undamaged(job, "gated")
    same_bytes(plain, got, "plain on the default stream against gated on the side stream")
    if not keyed:
        check_against_oracle(ctx, case, got)  # (the path counters of the EXT_HIER cases among it)


# ---------------------------------------------------------------- (b)

def chain_job(ctx, tr, uu, ud):
    """Plain tensors for a replay followed by the user signals, the node statistics and the job reduction."""
    dev = torch.device("cuda", ctx.device)
    inputs = fa.as_device_trace(tr, dev)
    inputs["user_ul"], inputs["user_dl"] = torch.from_numpy(uu).to(dev), torch.from_numpy(ud).to(dev)
    R, T = tr["arrive"].shape
    N = tr["mips"].shape[-1]
    new = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    out = fa.allocate_outputs(R, T, dev)
    out.stats.fill_(0xA5)
    return SimpleNamespace(inputs=inputs, out=out, user=new(R * USER.itemsize), nodes=new(R * N * NODE.itemsize),
                           job=new(JOB.itemsize), R=R, N=N)


def chain_enqueue(ctx, j, second=None):
    """The replay on the current stream; the three passes on ``second``, ordered after it by an event
    (None: on the current stream as well)."""
    d = j.inputs
    fa.run_batch(ctx, d, out=j.out)
    first = torch.cuda.current_stream(j.user.device)
    if second is not None:
        second.wait_stream(first)
    with torch.cuda.stream(second if second is not None else first):
        enqueue_user_stats(ctx, d, j.out, d["user_ul"], d["user_dl"], j.user)
        fa.node_stats(ctx, d, j.out, res=j.nodes)
        ctx.check(ctx._lib.fognet_reduce_stats_dev(ctx.handle, ptr(j.out.stats), j.R, ptr(j.job), cur(j.job.device)),
                  "reduce_stats")


def chain_collect(j):
    return dict(node=host(j.out.node), status=host(j.out.status), start=host(j.out.start_tick),
                done=host(j.out.done_tick), stats=host(j.out.stats), user=host(j.user), nodes=host(j.nodes), job=host(j.job))


def test_one_context_two_streams_ordered_by_an_event(ctx, gate):
    case = BY_ID["user-per-task"]
    tr, uu, ud, o = user_inputs(case)
    dtr, duu, dud, _ = user_inputs(case, decoy=True)
    decoys = dict(dtr, user_ul=duu, user_dl=dud)
    single = chain_job(ctx, tr, uu, ud)
    chain_enqueue(ctx, single)
    torch.cuda.synchronize()
    want = chain_collect(single)
    s2 = torch.cuda.Stream(torch.device("cuda", ctx.device))
    job = gate.run("chain", "replay-S1-then-passes-S2", lambda: chain_job(ctx, tr, uu, ud), decoys,
                   lambda jb: chain_enqueue(ctx, jb, s2), also=(s2,))
    got = chain_collect(job)
    same_bytes(want, got, "one stream against two streams ordered by an event")
    st = got["stats"].view(REP)
    assert_parity(None, dict(got, stats=st), o)
    assert st.tobytes() == o["stats"].tobytes()
    assert_user_parity(got["user"].view(USER), o["user"])
    ns.assert_records_equal(got["nodes"].view(NODE).reshape(job.R, job.N), ns.expected(tr, o), "node statistics")
    host_job = fa.job_from_reps(o["stats"])  # the library's host twin on the oracle's records
    for f in JOB.names:
        if f != "energy_j":
            np.testing.assert_array_equal(got["job"].view(JOB)[0][f], host_job[f], err_msg=f)


# ---------------------------------------------------------------- (c)

def test_two_contexts_two_streams_at_once(gate):
    """Nothing is shared between contexts: each behind its own gate, both released, each equal to its oracle."""
    cases = [BY_ID["reg-2x256x129"], BY_ID["wide-2x257x191"]]
    ctxs = [fa.Context(0), fa.Context(0)]
    try:
        plain = []
        for c, case in zip(ctxs, cases):  # (grows each context's workspace)
            g, _ = run_guarded(c, case, 0xA5, False)
            check_against_oracle(c, case, g)
            plain.append(g)
        assert len(gate.streams) == 2, ("only one of the candidate side streams let default-stream work run ahead of "
                                        "its gate (the runtime maps streams to hardware queues): two are needed here")
        streams = gate.streams
        lanes = [stream_gate.Lane(s, (lambda c=c, case=case: build_guarded(c, case, 0xA5, False)),
                                  input_arrays(c, case, decoy=True),
                                  (lambda jb, c=c: call_guarded(c, jb, enqueue_only=True)))
                 for s, c, case in zip(streams, ctxs, cases)]
        jobs = gate.run_lanes("two-contexts", "reg-2x256x129+wide-2x257x191", lanes)
        for c, case, job, p in zip(ctxs, cases, jobs, plain):
            got = collect_guarded(c, job)
            undamaged(job, case["id"])
            check_against_oracle(c, case, got)
            same_bytes(p, got, case["id"])
    finally:
        torch.cuda.synchronize()
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------- (d)

def host_calls(ctx):
    """fognet_decide (argument path and mapped-memory path), fognet_decide_window, fognet_decide_v2 and
    fognet_run_batch with host pointers: two lists of callables, each returning None or raising."""
    rng = np.random.default_rng(0xD)
    b3, b2 = fa.BrokerBaseApp3(ctx), fa.BrokerBaseApp2(ctx)
    quick = []
    for n in (5, 257):
        busy = rng.integers(0, 6, size=n).astype(np.float64) + rng.choice([0.0, 0.5], size=n)
        mips = rng.integers(1, 3000, size=n).astype(np.int32)
        reqs = rng.integers(0, 70000, size=7).astype(np.int32)
        want = [ol.decide_v3(busy, mips, int(q)) for q in reqs]
        assert all(rc == 0 for rc, _ in want)

        def decide(busy=busy, mips=mips, reqs=reqs, want=want):
            assert b3.sendPubAck(busy, mips, int(reqs[0])) == want[0][1]

        def window(busy=busy, mips=mips, reqs=reqs, want=want):
            assert b3.sendPubAck_window(busy, mips, reqs).tolist() == [k for _, k in want]
        quick += [decide, window]
    mips2 = rng.choice([0, 500, 999, 1000, 1001, 2000, 4000], size=65).astype(np.int32)

    def decide_v2():
        for local, req in ((1500, 1000), (100, 3000), (100, 4400)):
            assert b2.sendPubAck(mips2, local, req) == ol.decide_v2(mips2, local, req)
    quick.append(decide_v2)

    case = BY_ID["reg-3x5x63"]
    tr, _, o = batch_inputs(case)
    R, T, N = case["R"], case["T"], case["N"]

    def run_batch():
        hp = lambda a: C.c_void_p(a.ctypes.data)
        node, status = np.empty((R, T), np.int32), np.empty((R, T), np.uint8)
        start, done = np.empty((R, T), np.int64), np.empty((R, T), np.int64)
        stats, energy = np.zeros(R, REP), np.zeros((R, N), np.float64)
        hist = np.zeros((_abi.HIST_METRICS, _abi.HIST_BINS), np.int64)
        bi = _abi.BatchIn(R, T, N, _abi.FOGNET_POLICY_REF_V3, N, 0, *(hp(tr[k]) for k in
                          ("arrive", "req", "mips", "dl", "ul", "init", "p_busy", "p_idle")), None, None, 0, 0, 0)
        bo = _abi.BatchOut(hp(node), hp(status), hp(start), hp(done), hp(stats), hp(energy), hp(hist), None)
        assert ctx._lib.fognet_run_batch(ctx.handle, C.byref(bi), C.byref(bo)) == _abi.FOGNET_OK, ctx.last_error()
        assert_parity(None, dict(node=node, status=status, start=start, done=done, stats=stats), o)
        assert stats.tobytes() == o["stats"].tobytes()
        np.testing.assert_array_equal(hist, o["hist"].sum(axis=0))
        np.testing.assert_array_equal(energy, o["node_energy"])
    return quick, run_batch


def test_host_pointer_calls_while_a_gated_job_waits(ctx, gate):
    """The host-pointer calls run on the context's own stream: they return the oracle's answers while
    a device job of the same context waits behind the gate, and that job, released over the workspace
    they used, still equals its oracle.  fognet_decide* must leave the gate closed; fognet_run_batch
    frees its staging buffers, which waits for the device, so it comes last and is not asked to."""
    case = BY_ID["reg-2x256x129"]
    plain, _ = run_guarded(ctx, case, 0xA5, False)  # (the larger job: the workspace does not grow below)
    check_against_oracle(ctx, case, plain)
    quick, run_batch = host_calls(ctx)
    for f in quick + [run_batch]:  # (grows the decision scratch and the mapped stage)
        f()

    def during(check):
        for f in quick:
            f()
            check()
        run_batch()
        gate.report["fognet_run_batch_left_the_gate_closed"] = not gate.stream.query()
    job = gate.run("host-calls", "host-calls-over-reg-2x256x129", lambda: build_guarded(ctx, case, 0xA5, False),
                   input_arrays(ctx, case, decoy=True), lambda jb: call_guarded(ctx, jb, enqueue_only=True),
                   during=during, final_check=False)
    got = collect_guarded(ctx, job)
    undamaged(job, "the waiting job")
    check_against_oracle(ctx, case, got)
    same_bytes(plain, got, "the waiting job")


# ---------------------------------------------------------------- (e)

def test_hier_path_choice_is_per_stream(monkeypatch):
    """FOGNET_HIER_RESUME=0 with FOGNET_HIER_REGIONS unset: a region pass that handed most replications
    over sends the next launches of that shape *and stream* straight to the sequential replay."""
    monkeypatch.setenv("FOGNET_HIER_RESUME", "0")
    monkeypatch.delenv("FOGNET_HIER_REGIONS", raising=False)
    case = BY_ID["hier-escalating-3x2054x191"]
    tr, kw, o = batch_inputs(case)
    row = {k: (v[1:2] if v.ndim == 2 else v) for k, v in tr.items()}  # the escalating replication alone
    want = dict({k: o[k][1:2] for k in ("node", "status", "start", "done")}, stats=o["stats"][1:2])
    c = fa.Context(0)
    try:
        dev = torch.device("cuda", c.device)
        d = fa.as_device_trace(row, dev)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        for s, paths in ((s1, (1, 0)), (s1, (1, 1)), (s2, (2, 1))):
            with torch.cuda.stream(s):
                out = fa.run_batch(c, d, hist=True, **kw)
            assert c.hier_path_stats() == paths
            s.synchronize()
            g = dict(node=host(out.node), status=host(out.status), start=host(out.start_tick),
                     done=host(out.done_tick), stats=out.rep_stats())
            assert_parity(None, g, want)
            assert g["stats"].tobytes() == want["stats"].tobytes(), paths
            np.testing.assert_array_equal(host(out.hist), o["hist"][1], err_msg=str(paths))
            np.testing.assert_array_equal(host(out.node_energy), o["node_energy"][1:2], err_msg=str(paths))
    finally:
        torch.cuda.synchronize()
        c.close()
