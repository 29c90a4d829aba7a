"""replay_kernel's chunk flush takes the replication's output rows from LDS (formed once, not
re-read from the argument block per chunk), and its packed statistics pass is instantiated per
(histogram, write-back) pair, reads a block's downlinks ahead of its arithmetic, converts the
queueStartTime round trip without a range test, bins the queueTime from the double at hand and
counts in 32 bits per lane (replay_common.h stats_accumulate_packed).  None of it may change a
byte: stage="all" must equal the oracle in node, status, start, done, the statistics record, the
histograms and the energy, and the replay-only launch followed by the statistics stage.

Every shape runs with the histograms on and off, the power model on and off, and into the
caller's outputs or the internal scratch outputs of a statistics-only run (the pass stores the
clean node back only into the former), which reaches each instantiation of the pass.

The resume cases are about a run that continues from one 64-publish chunk into the next on the
same node (replay.hip `resume`): each case asserts from the oracle's outputs that its trace is
shaped as meant.  The trace generators are those of tests/test_epilogue_counts_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
from fognetsimpp_amd import _abi
import golden_io
import oracle_lib as ol
import tracegen as tg
import test_epilogue_counts_gpu as ec

pytestmark = pytest.mark.gpu
TPS = 10**12
MS = 10**9
ARRAYS = ("node", "status", "start", "done")
POISON = dict(node=0x7A7A7A7A, status=0xEE, start=-0x0123456789ABCDEF, done=-0x0FEDCBA987654321)


# ------------------------------------------------------------------ running a trace every way

def without_power(tr):
    return {k: v for k, v in tr.items() if k not in ("p_busy", "p_idle")}


def oracle(tr, power=True):
    pw = dict(p_busy=tr["p_busy"], p_idle=tr["p_idle"]) if power else {}
    return ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=6, hist=True, **pw)


def run_gpu(ctx, tr, hist=True, power=True, per_task=True, separate=False):
    """stage="all" into poisoned buffers, or stage="replay" then stage="stats"."""
    dev = torch.device("cuda", ctx.device)
    R, T = tr["arrive"].shape
    out = fa.allocate_outputs(R, T, dev, N=tr["mips"].shape[-1], energy=power, hist=hist, per_task=per_task)
    if per_task:
        out.node.fill_(POISON["node"])
        out.status.fill_(POISON["status"])
        out.start_tick.fill_(POISON["start"])
        out.done_tick.fill_(POISON["done"])
    d = fa.as_device_trace(tr if power else without_power(tr), dev)
    if separate:
        fa.run_batch(ctx, d, out=out, stage="replay")
        fa.run_batch(ctx, d, out=out, stage="stats")
    else:
        fa.run_batch(ctx, d, out=out)
    torch.cuda.synchronize()
    g = dict(stats=out.rep_stats(), hist=None if out.hist is None else out.hist.cpu().numpy(),
             energy=None if out.node_energy is None else out.node_energy.cpu().numpy())
    if per_task:
        g.update(node=out.node.cpu().numpy(), status=out.status.cpu().numpy(), start=out.start_tick.cpu().numpy(),
                 done=out.done_tick.cpu().numpy())
    return g


def assert_equals_oracle(g, o, what):
    if "node" in g:
        for k in ARRAYS:
            np.testing.assert_array_equal(g[k], o[k], err_msg=f"{k} {what}")
        assert (g["node"] >> 8 == 0).all(), what  # no packed field left behind
    assert g["stats"].tobytes() == o["stats"].tobytes(), what
    if g["hist"] is not None:
        np.testing.assert_array_equal(g["hist"], o["hist"].sum(axis=0), err_msg=what)
    if g["energy"] is not None:
        np.testing.assert_array_equal(g["energy"], o["node_energy"], err_msg=what)


# (histograms, power model, caller's per-task outputs): every flag on, each one off, all off
WAYS = [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False),
        (False, True, False)]


def check_every_way(ctx, tr, o_power, o_plain):
    for hist, power, per_task in WAYS:
        o = o_power if power else o_plain
        g = run_gpu(ctx, tr, hist=hist, power=power, per_task=per_task)
        assert (g["hist"] is not None) == hist and (g["energy"] is not None) == power
        assert_equals_oracle(g, o, f"hist={hist} power={power} per_task={per_task}")
    for hist in (True, False):
        s = run_gpu(ctx, tr, hist=hist, separate=True)
        assert_equals_oracle(s, o_power, f"separate stages, hist={hist}")


def check_case(ctx, tr):
    check_every_way(ctx, tr, oracle(tr), oracle(tr, power=False))


# ------------------------------------------------------------------ resume path

def one_node_batch(arrive, req_s, ul_ms=1):
    """R replications on one node of 1,000 MIPS each (1 ms downlink); arrive, req_s: [R, T]."""
    arrive = np.asarray(arrive, np.int64)
    R = arrive.shape[0]
    one = np.full((R, 1), MS, np.int64)
    return ec.with_power(dict(arrive=arrive, req=(1000 * np.asarray(req_s, np.int64)).astype(np.int32),
                              mips=np.full((R, 1), 1000, np.int32), dl=one.copy(), ul=ul_ms * one, init=ul_ms * one))


def four_nodes(arrive, req_s, ul_ms=1):
    """R replications on four equal nodes (1,000 MIPS, 1 ms downlink)."""
    arrive = np.asarray(arrive, np.int64)
    R = arrive.shape[0]
    one = np.full((R, 4), MS, np.int64)
    return ec.with_power(dict(arrive=arrive, req=(1000 * np.asarray(req_s, np.int64)).astype(np.int32),
                              mips=np.full((R, 4), 1000, np.int32), dl=one.copy(), ul=ul_ms * one, init=ul_ms * one))


@functools.lru_cache(maxsize=None)
def single_node_case(T):
    """Replication r publishes T tasks of r + 1 seconds, r + 1 ms apart: all of them precede the first
    completion advert, so each chunk is one run and every chunk after the first resumes it."""
    gaps = np.array([1, 2, 3], np.int64)[:, None] * MS
    arrive = 10 * MS + gaps * np.arange(T, dtype=np.int64)[None]
    tr = one_node_batch(arrive, np.repeat(np.array([[1], [2], [3]], np.int64), T, axis=1))
    return tr, oracle(tr), oracle(tr, power=False)


@pytest.mark.parametrize("T", [64, 65, 128, 129, 193])
def test_resume_single_node(ctx, T):
    tr, o, o_plain = single_node_case(T)
    assert ec.stays_in_register_kernel(tr, o)
    first_advert = o["done"][:, 0] + tr["ul"][:, 0]
    assert (tr["arrive"][:, -1] <= first_advert).all()  # no advert reaches the broker inside the trace
    assert (o["status"][:, 0] == 5).all() and (o["status"][:, 1:] == 4).all()
    check_every_way(ctx, tr, o, o_plain)


def herd_trace(tick_64):
    """Four nodes.  Replication r: 64 publishes 1 ms apart herd onto node 0 (the stale view), the first
    of r + 1 seconds; its advert reaches the broker at X = 10 ms + 1 ms + (r + 1) s + 1 ms and carries the
    63 queued seconds, which moves the argmin to node 1.  The run covers the whole first chunk with the
    horizon X.  tick_64(X): the tick of publish 64; 40 more publishes follow 1 ms apart."""
    R, T = 3, 105
    arrive = np.empty((R, T), np.int64)
    req_s = np.ones((R, T), np.int64)
    for r in range(R):
        req_s[r, 0] = r + 1
        X = 10 * MS + MS + (r + 1) * TPS + MS
        arrive[r, :64] = 10 * MS + MS * np.arange(64, dtype=np.int64)
        arrive[r, 64:] = tick_64(X) + MS * np.arange(T - 64, dtype=np.int64)
    return four_nodes(arrive, req_s)


def test_run_ends_on_the_chunks_last_publish_and_resumes_at_the_horizon(ctx):
    """Publish 64 is at the horizon itself: an advert applies only strictly before a publish's tick, so
    the run resumes for this one publish and ends there."""
    tr = herd_trace(lambda X: X)
    o = oracle(tr)
    assert ec.stays_in_register_kernel(tr, o)
    assert (o["node"][:, :65] == 0).all() and (o["node"][:, 65] == 1).all()
    check_every_way(ctx, tr, o, oracle(tr, power=False))


def test_next_chunk_starts_past_the_carried_horizon(ctx):
    """Publish 64 is one tick past the horizon: the run that filled chunk 0 does not resume."""
    tr = herd_trace(lambda X: X + 1)
    o = oracle(tr)
    assert ec.stays_in_register_kernel(tr, o)
    assert (o["node"][:, :64] == 0).all() and (o["node"][:, 64] == 1).all()
    check_every_way(ctx, tr, o, oracle(tr, power=False))


def test_resumed_run_is_the_nodes_first_idle_to_busy_transition(ctx):
    """Chunk 0: 64 publishes of 0 s (each completes at its arrival: the node never gets busy) with
    uplinks of 10 s, so the first advert is far off and the run's horizon with it; chunk 1, 5 s later,
    brings tasks of r + 1 seconds: the resumed run's first task finds node 0 idle (status 5) and makes
    it busy for the first time, the others queue behind it."""
    R, T = 3, 100
    arrive = np.empty((R, T), np.int64)
    req_s = np.zeros((R, T), np.int64)
    for r in range(R):
        arrive[r, :64] = 10 * TPS + MS + MS * np.arange(64, dtype=np.int64)
        arrive[r, 64:] = 15 * TPS + MS * np.arange(T - 64, dtype=np.int64)
        req_s[r, 64:] = r + 1
    tr = four_nodes(arrive, req_s, ul_ms=10_000)
    o = oracle(tr)
    assert ec.stays_in_register_kernel(tr, o)
    assert (o["node"] == 0).all()  # one run per chunk, the second resumed
    assert (tr["arrive"][:, -1] < o["done"][:, 0] + tr["ul"][:, 0]).all()
    assert (o["status"][:, :65] == 5).all() and (o["status"][:, 65:] == 4).all()
    assert ((o["done"] - o["start"])[:, :64] == 0).all()
    check_every_way(ctx, tr, o, oracle(tr, power=False))


# ------------------------------------------------------------------ pass shapes

@functools.lru_cache(maxsize=None)
def sweep_case(T, N):
    tr = ec.with_power(tg.make_batch(0x5EED0900 + 1000 * N + T, 6, N, T, sweep=True))
    return tr, oracle(tr), oracle(tr, power=False)


@pytest.mark.parametrize("N", [1, 65, 256])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 513])
def test_row_and_block_edges_every_way(ctx, T, N):
    """One task, the 64-task row, the 4 x 64-row block of the pass, and one past each."""
    tr, o, o_plain = sweep_case(T, N)
    assert ec.stays_in_register_kernel(tr, o)
    assert (o["status"] == 5).any() and (T == 1 or (o["status"] == 4).any())
    check_every_way(ctx, tr, o, o_plain)


@pytest.mark.parametrize("T", [100, 321])
def test_no_task_queues(ctx, T):
    """Tasks of 1 s, 5 s apart: every one finds the node idle (n_queued = 0, no queueTime emission)."""
    tr = ec.one_node(10 * MS + 5 * TPS * np.arange(T, dtype=np.int64), np.ones(T, np.int64))
    o = oracle(tr)
    assert (o["status"] == 5).all() and int(o["stats"]["n_queued"][0]) == 0 and int(o["stats"]["n_qtime"][0]) == 0
    check_every_way(ctx, tr, o, oracle(tr, power=False))


@pytest.mark.parametrize("T", [65, 321])
def test_every_task_queues(ctx, T):
    """A node's first task always finds it idle, so "every task queued" means every task but task 0:
    one-second tasks 1 ms apart on one node.  Rows 1 and up hold only queued tasks, and the waits pass
    9.1 s, where the raw queueTime (ticks x 1000) reaches 2^53 and more: the bin from the double at
    hand must equal the bin of the converted integer."""
    tr, o = ec.queue_case(T)
    assert ec.stays_in_register_kernel(tr, o)
    assert o["status"][0, 0] == 5 and (o["status"][0, 1:] == 4).all()
    assert int(o["stats"]["n_queued"][0]) == T - 1 == int(o["stats"]["n_qtime"][0])
    raws = [x for x in ec.qtime_raws(tr, o) if x != "idle"]
    assert None not in raws and max(abs(x) for x in raws) >= 2**53
    check_every_way(ctx, tr, o, oracle(tr, power=False))


def test_negative_qtime_every_way(ctx):
    """tests/golden/kat_qtime.json same_tick: a pop at the tick of the push emits a negative value."""
    name, tr, exp = next(c for c in golden_io.qtime_cases() if c[0] == "same_tick")
    tr = ec.with_power({k: (v if k in ("arrive", "req") else v[None]) for k, v in tr.items()})
    o = oracle(tr)
    assert int(o["stats"]["queue_min_raw"][0]) < 0 and ec.stays_in_register_kernel(tr, o)
    golden_io.check_qtime_record(o["stats"][0], exp)
    check_every_way(ctx, tr, o, oracle(tr, power=False))


@pytest.mark.parametrize("T", [64, 100])
def test_overflowing_emissions_every_way(ctx, T):
    """255-second tasks published at one tick: the later emissions overflow the reference's simtime_t
    (n_qtime_overflow > 0, n_qtime = n_queued - n_qtime_overflow) and the abort point is set."""
    tr, o = ec.overflow_case(T)
    st = o["stats"][0]
    assert ec.stays_in_register_kernel(tr, o)
    assert int(st["n_qtime_overflow"]) > 0 and int(st["n_qtime"]) > 0
    assert int(st["n_qtime"]) + int(st["n_qtime_overflow"]) == int(st["n_queued"]) == T - 1
    assert int(st["abort_task"]) >= 0 and int(st["abort_tick"]) == int(o["start"][0, int(st["abort_task"])])
    check_every_way(ctx, tr, o, oracle(tr, power=False))


def test_large_ticks_every_way(ctx):
    """Arrivals just below the register kernel's 2^56-tick bound: the queueStartTime round trip
    a -> a * 1e-12 -> * 1e12 at its largest values here, and large high halves in the sums."""
    tr, o = ec.carries_case(True)
    assert ec.stays_in_register_kernel(tr, o) and (o["status"] == 4).any()
    check_every_way(ctx, tr, o, oracle(tr, power=False))


# ------------------------------------------------------------------ precondition error inside a chunk

@pytest.mark.parametrize("p", [70, 100, 129, 200])
@pytest.mark.parametrize("fault", ["order", "range"])
def test_precondition_error_mid_chunk(ctx, fault, p):
    """Replication 1 breaks a precondition at index p, inside a chunk, and ends with FOGNET_ERR_ARG after
    n_tasks <= p tasks.  "order": the tick is lower than its predecessor's, which the chunk's own check
    finds before any of its publishes is pushed (n_tasks = the chunks before it).  "range": the ticks
    from p on are 2^61 - 1, a valid tick whose arrival at a node is past the range: the run that starts
    at p is refused after the chunk's earlier runs were pushed, so n_tasks = p and the chunk is flushed
    in part.  The epilogue runs over exactly those tasks (its counters add up to n_tasks and equal the
    separate statistics stage's over the same outputs), their outputs equal the oracle's of the
    faultless trace, and every entry past them keeps the caller's bytes."""
    good = ec.with_power(tg.make_batch(0x5EED0933, 2, 16, 300, rho=0.9))
    o = oracle(good)
    tr = {k: v.copy() for k, v in good.items()}
    if fault == "order":
        tr["arrive"][1, p] = tr["arrive"][1, p - 1] - 1
    else:
        tr["arrive"][1, p:] = 2**61 - 1
    for hist in (True, False):
        g = run_gpu(ctx, tr, hist=hist)
        s = run_gpu(ctx, tr, hist=hist, separate=True)
        assert g["stats"]["status"][0] == 0 and g["stats"]["status"][1] == _abi.FOGNET_ERR_ARG
        n = int(g["stats"]["n_tasks"][1])
        assert n == (64 * (p // 64) if fault == "order" else p)
        assert int(g["stats"]["n_queued"][1]) + int(g["stats"]["n_started"][1]) == n
        assert int(g["stats"]["n_queued"][1]) == int((o["status"][1, :n] == 4).sum())
        for k in ARRAYS:
            np.testing.assert_array_equal(g[k][0], o[k][0], err_msg=k)
            np.testing.assert_array_equal(g[k][1, :n], o[k][1, :n], err_msg=k)
            assert (g[k][1, n:] == np.array(POISON[k]).astype(g[k].dtype)).all(), k
            np.testing.assert_array_equal(g[k], s[k], err_msg=k)
        assert g["stats"][:1].tobytes() == o["stats"][:1].tobytes()
        assert g["stats"].tobytes() == s["stats"].tobytes()
        if hist:
            np.testing.assert_array_equal(g["hist"], s["hist"])
        np.testing.assert_array_equal(g["energy"], s["energy"])
    # the statistics-only run of the same trace: the same records
    so = run_gpu(ctx, tr, per_task=False)
    assert so["stats"].tobytes() == g["stats"].tobytes()
