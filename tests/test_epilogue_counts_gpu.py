"""The packed statistics pass of replay_kernel's fused epilogue keeps each sum
of squares as three running partial sums with wrap counters, folded once after
the loop, and counts its two histograms per 64-task row.  Both are reorderings
of exact integer sums and counts, so whatever a row looks like -- one bin or
several, the leading bin in the minority, no queued task or only queued ones,
a leading bin that changes from row to row, a partial last row, overflowing
or negative queueTime values, partial sums that wrap -- the record bytes, the
histograms, the per-node energy and the four per-task arrays must equal the
oracle's and those of the separate replay + statistics stages.  (The row
cases were written for a per-wavefront histogram count, measured and not kept,
DESIGN.md §4.4: they hold for any way of counting a row.)

Every case first asserts, from the oracle's outputs alone, that its trace hits
what it is meant to hit (rows are those of the pass: task i sits in row i // 64,
lane i % 64 of its replication)."""
import functools

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import golden_io
import oracle_lib as ol
import tracegen as tg

pytestmark = pytest.mark.gpu
TPS = 10**12
MS = 10**9
BINS = 64
I64_MAX = np.iinfo(np.int64).max
ARRAYS = ("node", "status", "start", "done")
DEFAULT_RING = 2048  # (capi.hip kDefaultRing)


# ------------------------------------------------------------------ running the three ways

def with_power(tr):
    pb, pi = fa.power_model(tr["mips"])
    return dict(tr, p_busy=pb, p_idle=pi)


def run_oracle(tr):
    return ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=6,
                        p_busy=tr["p_busy"], p_idle=tr["p_idle"], hist=True)


def to_host(out):
    torch.cuda.synchronize()
    return dict(stats=out.rep_stats(), hist=None if out.hist is None else out.hist.cpu().numpy(),
                energy=out.node_energy.cpu().numpy(), node=out.node.cpu().numpy(), status=out.status.cpu().numpy(),
                start=out.start_tick.cpu().numpy(), done=out.done_tick.cpu().numpy())


def run_gpu(ctx, tr, separate=False, hist=True, prefill=None):
    """stage="all" (the fused epilogue), or stage="replay" then stage="stats" (rep_stats_kernel).
    prefill: [2, 64] counts the caller's histogram holds before the run."""
    dev = torch.device("cuda", ctx.device)
    R, T = tr["arrive"].shape
    out = fa.allocate_outputs(R, T, dev, N=tr["mips"].shape[-1], energy=True, hist=hist)
    if prefill is not None:
        out.hist.copy_(torch.from_numpy(prefill).to(dev).reshape(out.hist.shape))
    d = fa.as_device_trace(tr, dev)
    if separate:
        fa.run_batch(ctx, d, out=out, stage="replay")
        fa.run_batch(ctx, d, out=out, stage="stats")
    else:
        fa.run_batch(ctx, d, out=out)
    return to_host(out)


def check(ctx, tr, o, base=None):
    """Fused and separate runs against the oracle (histograms: base + the oracle's)."""
    want_hist = o["hist"].sum(axis=0) + (0 if base is None else base)
    for separate in (False, True):
        g = run_gpu(ctx, tr, separate=separate, prefill=base)
        for k in ARRAYS:
            np.testing.assert_array_equal(g[k], o[k], err_msg=f"{k} separate={separate}")
        assert g["stats"].tobytes() == o["stats"].tobytes(), f"separate={separate}"
        np.testing.assert_array_equal(g["hist"], want_hist, err_msg=f"separate={separate}")
        np.testing.assert_array_equal(g["energy"], o["node_energy"])


# ------------------------------------------------------------------ what the rows of a trace look like

def resp_bin(ticks):
    """internal.h hist_bin: bin of a response time (whole milliseconds, log2)."""
    ticks = int(ticks)
    if ticks < MS:
        return 0
    j = ticks.bit_length() - 30
    return min(j + (1 if ticks >= (MS << j) else 0), BINS - 1)


def qtime_bin(raw):
    """replay_common.h hist_bin_raw: bin of a raw queueTime (the recorded double's whole part)."""
    v = float(raw) * 1e-12
    return 0 if not v >= 1.0 else min(int(np.frexp(v)[1]), BINS - 1)


def qtime_raws(tr, o, r=0):
    """Per task of replication r: the raw queueTime of a status-4 task (None: the emission overflows),
    else the string "idle"."""
    dl = np.broadcast_to(tr["dl"], (tr["arrive"].shape[0], tr["dl"].shape[-1]))[r]
    return [ol.qtime_raw(int(o["start"][r, i]), int(tr["arrive"][r, i]) + int(dl[o["node"][r, i]]))
            if o["status"][r, i] == 4 else "idle" for i in range(tr["arrive"].shape[1])]


def rows_of(tr, o, r=0):
    """(response bins, statuses) of each 64-task row of replication r; the bins are checked against
    the oracle's own histogram, so the row asserts rest on the oracle and not on resp_bin."""
    resp = o["done"][r] - tr["arrive"][r]
    bins = np.array([resp_bin(x) for x in resp])
    np.testing.assert_array_equal(np.bincount(bins, minlength=BINS), o["hist"][r, 1])
    T = len(bins)
    return [(bins[i:i + 64], o["status"][r, i:i + 64]) for i in range(0, T, 64)]


def leading_bins_change(rows):
    lead = [int(b[0]) for b, _ in rows]
    return any(a != b for a, b in zip(lead, lead[1:]))


def stays_in_register_kernel(tr, o, ring=DEFAULT_RING):
    """None of replay_kernel's hand-over conditions (replay.hip: a service past 255 s, an arrival at
    the node past the ring entry's 2^56 ticks, more pending tasks than the ring holds) is met."""
    svc = (o["done"] - o["start"]) // TPS
    return bool((o["stats"]["status"] == 0).all() and svc.max() <= 255 and o["stats"]["max_pending"].max() <= ring
                and int(tr["arrive"].max()) + int(tr["dl"].max()) < 2**56)


def one_node(arrive, req_s):
    """One node of 1,000 MIPS behind 1 ms links; task i needs req_s[i] seconds."""
    one = np.array([[MS]], np.int64)
    return with_power(dict(arrive=np.asarray(arrive, np.int64)[None],
                           req=(1000 * np.asarray(req_s, np.int64)).astype(np.int32)[None],
                           mips=np.array([[1000]], np.int32), dl=one.copy(), ul=one.copy(), init=one.copy()))


def queue_trace(T):
    """T one-second tasks published 1 ms apart onto one node: task i waits about i seconds, so the
    response and queueTime bins climb through the powers of two inside and across the rows."""
    return one_node(10 * MS + MS * np.arange(T, dtype=np.int64), np.ones(T, np.int64))


# ------------------------------------------------------------------ 1: row and block edges

@functools.lru_cache(maxsize=None)
def sweep_case(T, N):
    tr = with_power(tg.make_batch(0x5EED0800 + 1000 * N + T, 6, N, T, sweep=True))
    return tr, run_oracle(tr)


@pytest.mark.parametrize("N", [3, 256])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 513])
def test_row_and_block_edges(ctx, T, N):
    """One task, the 64-task row, the 4 x 64-row block of the pass, and one past each."""
    tr, o = sweep_case(T, N)
    assert stays_in_register_kernel(tr, o)
    assert T == 1 or (o["status"] == 4).any()
    assert len(rows_of(tr, o)) == -(-T // 64)
    check(ctx, tr, o)


# ------------------------------------------------------------------ 2: mixed rows

@functools.lru_cache(maxsize=None)
def mixed_rows_case():
    """Row 0: 63 one-second tasks 5 s apart (each finds the node idle, one response bin) and the first
    task of a burst; rows 1 and 2: the burst's 1 ms-apart tasks, all queued, the response growing by a
    second per task; then tasks 400 s apart again (a partial last row, both statuses in row 2)."""
    spaced = 10 * MS + 5 * TPS * np.arange(63, dtype=np.int64)
    burst = spaced[-1] + 5 * TPS + MS * np.arange(100, dtype=np.int64)
    late = burst[-1] + 400 * TPS * (1 + np.arange(37, dtype=np.int64))
    tr = one_node(np.concatenate([spaced, burst, late]), np.ones(200, np.int64))
    return tr, run_oracle(tr)


def test_mixed_rows(ctx):
    tr, o = mixed_rows_case()
    assert tr["arrive"].shape[1] <= 512 and stays_in_register_kernel(tr, o)
    rows = rows_of(tr, o)
    assert any(len(set(b.tolist())) == 1 for b, _ in rows)  # all response bins equal
    # two or more bins, the first task's in the minority
    assert any(len(set(b.tolist())) >= 2 and 2 * int((b == b[0]).sum()) < len(b) for b, _ in rows)
    assert any((s != 4).all() for _, s in rows)  # no queued task
    assert any((s == 4).all() for _, s in rows)  # only queued tasks
    assert any((s == 4).any() and (s == 5).any() for _, s in rows)
    check(ctx, tr, o)


# ------------------------------------------------------------------ 3: the carried count's flushes

@functools.lru_cache(maxsize=None)
def queue_case(T):
    tr = queue_trace(T)
    return tr, run_oracle(tr)


@pytest.mark.parametrize("T", [130, 321])
def test_leading_bin_changes_and_partial_last_row(ctx, T):
    tr, o = queue_case(T)
    assert stays_in_register_kernel(tr, o)
    rows = rows_of(tr, o)
    assert leading_bins_change(rows) and 0 < len(rows[-1][0]) < 64
    # the queueTime bins too: leading emission of consecutive rows
    raws = qtime_raws(tr, o)
    lead = [next(qtime_bin(x) for x in raws[i:i + 64] if x != "idle" and x is not None)
            for i in range(0, T, 64)]
    assert any(a != b for a, b in zip(lead, lead[1:]))
    check(ctx, tr, o)


# ------------------------------------------------------------------ 4, 5: the caller's histogram

def test_histogram_is_added_to_the_callers(ctx):
    tr, o = queue_case(321)
    base = (1 + 3 * np.arange(2 * BINS, dtype=np.int64)).reshape(2, BINS)
    assert o["hist"].sum() > 0
    check(ctx, tr, o, base=base)


def test_no_histogram(ctx):
    tr, o = mixed_rows_case()
    for separate in (False, True):
        g = run_gpu(ctx, tr, separate=separate, hist=False)
        assert g["hist"] is None
        assert g["stats"].tobytes() == o["stats"].tobytes()
        for k in ARRAYS:
            np.testing.assert_array_equal(g[k], o[k], err_msg=k)
        np.testing.assert_array_equal(g["energy"], o["node_energy"])


# ------------------------------------------------------------------ 6: queueTime overflow

@functools.lru_cache(maxsize=None)
def overflow_case(T):
    tr = one_node(np.full(T, 10 * MS, np.int64), np.full(T, 255, np.int64))
    return tr, run_oracle(tr)


@pytest.mark.parametrize("T", [64, 100])
def test_qtime_overflow_in_register_kernel(ctx, T):
    """255-second tasks published at one tick: the wait passes 9,223 s (the simtime_t range of the
    reference's millisecond product) after about 37 tasks."""
    tr, o = overflow_case(T)
    assert stays_in_register_kernel(tr, o)
    st = o["stats"][0]
    raws = qtime_raws(tr, o)
    lost = [i for i, x in enumerate(raws) if x is None]
    kept = [x for x in raws if x is not None and x != "idle"]
    assert int(st["n_qtime_overflow"]) == len(lost) > 0 and int(st["n_qtime"]) == len(kept) > 0
    # the overflowing emissions are in no bin
    assert int(o["hist"][0, 0].sum()) == len(kept)
    np.testing.assert_array_equal(np.bincount([qtime_bin(x) for x in kept], minlength=BINS), o["hist"][0, 0])
    assert int(st["abort_task"]) == lost[0] and int(st["abort_tick"]) == int(o["start"][0, lost[0]])
    assert int((o["done"][0] - tr["arrive"][0]).max()) >= 2**52  # a large high half in the square sums
    for separate in (False, True):
        g = run_gpu(ctx, tr, separate=separate)
        assert int(g["stats"]["abort_tick"][0]) == int(st["abort_tick"])
        assert int(g["stats"]["abort_task"][0]) == int(st["abort_task"])
    check(ctx, tr, o)


# ------------------------------------------------------------------ 7: partial-sum carries

@functools.lru_cache(maxsize=None)
def carries_case(late):
    tr = tg.make_batch(0x5EED0877, 3, 4, 1000, rho=0.9)
    if late:  # the last arrival at a node lands just below the ring entry's 2^56 ticks
        tr["arrive"] = tr["arrive"] + (2**56 - 1 - int(tr["arrive"].max()) - int(tr["dl"].max()))
    tr = with_power(tr)
    return tr, run_oracle(tr)


def test_partial_sums_wrap(ctx):
    """With v = h 2^32 + l the pass keeps sum l^2, sum h l and sum h^2 per lane in 64 bits each plus a
    wrap count: here some lane's sum l^2 passes 2^64 and the high halves are not zero."""
    tr, o = carries_case(False)
    assert stays_in_register_kernel(tr, o)
    resp = [int(x) for x in (o["done"][0] - tr["arrive"][0])]
    lanes = [resp[l::64] for l in range(64)]
    assert max(sum((v & 0xFFFFFFFF) ** 2 for v in lane) for lane in lanes) >= 2**64
    assert max(sum((v >> 32) ** 2 for v in lane) for lane in lanes) > 0
    raws = [abs(x) for x in qtime_raws(tr, o) if x != "idle" and x is not None]
    assert sum((v & 0xFFFFFFFF) ** 2 for v in raws) >= 2**64 and max(raws) >= 2**32
    check(ctx, tr, o)


def test_arrivals_just_below_the_register_kernels_bound(ctx):
    tr, o = carries_case(True)
    assert int(tr["arrive"].max()) + int(tr["dl"].max()) == 2**56 - 1 and int(tr["arrive"].min()) > 2**55
    assert stays_in_register_kernel(tr, o)  # no replication handed over
    assert (o["status"] == 4).any()
    check(ctx, tr, o)


# ------------------------------------------------------------------ 8: negative queueTime

def test_negative_qtime(ctx):
    """tests/golden/kat_qtime.json same_tick: a pop at the tick of the push emits a negative value (the
    queueStartTime double round trip); the signed sum and the 192-bit sum of squares."""
    name, tr, exp = next(c for c in golden_io.qtime_cases() if c[0] == "same_tick")
    tr = with_power({k: (v if k in ("arrive", "req") else v[None]) for k, v in tr.items()})
    o = run_oracle(tr)
    st = o["stats"][0]
    assert int(st["queue_min_raw"]) < 0 and stays_in_register_kernel(tr, o)
    golden_io.check_qtime_record(st, exp)
    check(ctx, tr, o)
    g = run_gpu(ctx, tr)
    golden_io.check_qtime_record(g["stats"][0], exp)
