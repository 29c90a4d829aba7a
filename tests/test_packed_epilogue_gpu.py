"""replay_kernel's fused statistics epilogue reads one packed word per task
(node | service seconds << 8 | status << 16, stored into out_node by the chunk
flush) and stores the clean node back.  Whatever path a replication takes --
the epilogue, a hand-over to the wide kernel, a precondition error in the
middle of the trace, a replay without the epilogue -- the four per-task arrays,
the record bytes, the histograms and the per-node energy must equal the
oracle's and those of the separate replay + statistics stages, and entries the
replay never reached must stay untouched."""
import functools

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import oracle_lib as ol
import tracegen as tg
from fognetsimpp_amd import _abi

pytestmark = pytest.mark.gpu
TPS = 10**12
MS = 10**9
POISON = {"node": 0x7A7A7A7A, "status": 0xEE, "start": -0x0123456789ABCDEF, "done": -0x0FEDCBA987654321}
ARRAYS = ("node", "status", "start", "done")


def poisoned_outputs(R, T, N, dev, per_task=True):
    out = fa.allocate_outputs(R, T, dev, N=N, energy=True, hist=True, per_task=per_task)
    if per_task:
        out.node.fill_(POISON["node"])
        out.status.fill_(POISON["status"])
        out.start_tick.fill_(POISON["start"])
        out.done_tick.fill_(POISON["done"])
    return out


def to_host(out):
    torch.cuda.synchronize()
    d = dict(stats=out.rep_stats(), hist=out.hist.cpu().numpy(), energy=out.node_energy.cpu().numpy())
    if out.node is not None:
        d.update(node=out.node.cpu().numpy(), status=out.status.cpu().numpy(), start=out.start_tick.cpu().numpy(),
                 done=out.done_tick.cpu().numpy())
    return d


def with_power(tr):
    pb, pi = fa.power_model(tr["mips"])
    return dict(tr, p_busy=pb, p_idle=pi)


def run_all(ctx, tr, ring=0, per_task=True):
    """stage="all" (the fused epilogue) into poisoned buffers."""
    dev = torch.device("cuda", ctx.device)
    R, T = tr["arrive"].shape
    out = poisoned_outputs(R, T, tr["mips"].shape[-1], dev, per_task)
    fa.run_batch(ctx, fa.as_device_trace(tr, dev), out=out, ring_capacity=ring)
    return to_host(out)


def run_separate(ctx, tr, ring=0):
    """stage="replay" (no epilogue: the flush stores the plain node), then stage="stats"."""
    dev = torch.device("cuda", ctx.device)
    R, T = tr["arrive"].shape
    out = poisoned_outputs(R, T, tr["mips"].shape[-1], dev)
    d = fa.as_device_trace(tr, dev)
    fa.run_batch(ctx, d, out=out, ring_capacity=ring, stage="replay")
    fa.run_batch(ctx, d, out=out, ring_capacity=ring, stage="stats")
    return to_host(out)


def run_oracle(tr):
    return ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=6,
                        p_busy=tr["p_busy"], p_idle=tr["p_idle"], hist=True)


def assert_same_as_oracle(g, o):
    for k in ARRAYS:
        np.testing.assert_array_equal(g[k], o[k], err_msg=k)
    assert (g["node"] >> 8 == 0).all()  # no packed field left behind
    assert g["stats"].tobytes() == o["stats"].tobytes()
    np.testing.assert_array_equal(g["hist"], o["hist"].sum(axis=0))
    np.testing.assert_array_equal(g["energy"], o["node_energy"])


def assert_same_runs(a, b):
    for k in ARRAYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["stats"].tobytes() == b["stats"].tobytes()
    np.testing.assert_array_equal(a["hist"], b["hist"])
    np.testing.assert_array_equal(a["energy"], b["energy"])


@functools.lru_cache(maxsize=None)
def sweep_case(T, N):
    """R = 6 covers the sweep's three rho classes and two of its latency scales."""
    tr = with_power(tg.make_batch(0x5EED0700 + 1000 * N + T, 6, N, T, sweep=True))
    return tr, run_oracle(tr)


# T: one task, the 64-publish chunk boundary, the epilogue's 4 x 64 = 256-row block boundary, and its
# pipeline's prologue and drain (one, two, three and four blocks)
@pytest.mark.parametrize("N", [1, 3, 64, 65, 256])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 513, 1000])
def test_packed_epilogue_matches_oracle_and_separate_stages(ctx, T, N):
    tr, o = sweep_case(T, N)
    assert (o["stats"]["status"] == 0).all()
    # both statuses: a replication's first task always finds its node idle (5); a queued one (4) needs a
    # second task, so a one-task trace cannot hold it
    assert (o["status"] == 5).any()
    assert T == 1 or (o["status"] == 4).any()
    g = run_all(ctx, tr)
    assert_same_as_oracle(g, o)
    assert_same_runs(g, run_separate(ctx, tr))


def node_255_trace(giant_s=255):
    """256 nodes at 1,000 MIPS, 1 ms links.  Burst j (two publishes at one tick, 5 ms after burst j - 1):
    a task of 0 s, which completes at its arrival, and one of giant_s seconds, which reaches the node at
    the same tick and so before that completion: the advert then carries giant_s busy seconds, and burst
    j + 1 goes to node j + 1 -- burst 255 to node 255.  Tasks of 1 s follow."""
    N = 256
    mips = np.full(N, 1000, np.int32)
    dl = np.full(N, MS, np.int64)
    ul = np.full(N, MS, np.int64)
    t = 10 * MS + 5 * MS * np.repeat(np.arange(N, dtype=np.int64), 2)
    req = np.tile(np.array([500, giant_s * 1000], np.int32), N)
    tail_t = t[-1] + 5 * MS * (1 + np.arange(40, dtype=np.int64))
    arrive = np.concatenate([t, tail_t])
    req = np.concatenate([req, np.full(40, 1000, np.int32)])
    return with_power(dict(arrive=arrive[None], req=req[None], mips=mips[None], dl=dl[None], ul=ul[None],
                           init=ul[None].copy()))


def test_node_255_and_service_0_1_255(ctx):
    """The word's node field is full at node 255 and its service field at 255 s; 0 s and 1 s beside them."""
    tr = node_255_trace()
    o = run_oracle(tr)
    assert o["stats"]["status"][0] == 0
    assert (o["node"] == 255).sum() >= 2 and o["node"].max() == 255
    svc = (o["done"] - o["start"]) // TPS
    assert {0, 1, 255} <= set(np.unique(svc).tolist())
    assert (o["status"] == 4).any() and (o["status"] == 5).any()
    g = run_all(ctx, tr)
    assert_same_as_oracle(g, o)
    assert (g["node"][0, :int(g["stats"]["n_tasks"][0])] >> 8 == 0).all()
    assert_same_runs(g, run_separate(ctx, tr))


def test_service_256_hands_over(ctx):
    """256 s does not fit the word (nor the ring entry): the replication goes to the wide kernel, which
    rewrites every output from the start."""
    tr = node_255_trace(giant_s=256)
    o = run_oracle(tr)
    assert o["stats"]["status"][0] == 0 and ((o["done"] - o["start"]) // TPS).max() == 256
    g = run_all(ctx, tr)
    assert_same_as_oracle(g, o)
    assert_same_runs(g, run_separate(ctx, tr))


def test_ring_hand_over_leaves_clean_outputs(ctx):
    """ring_capacity=4: the overloaded replications leave the register kernel after it flushed packed
    words; the wide kernel's outputs replace them."""
    over = tg.make_batch(711, 2, 4, 700, rho=3.0)
    light = tg.make_batch(712, 3, 4, 700, rho=0.3)
    tr = with_power({k: np.concatenate([light[k][:1], over[k], light[k][1:]]) for k in over})
    o = run_oracle(tr)
    g = run_all(ctx, tr, ring=4)
    assert (g["stats"]["status"] == 0).all() and g["stats"]["max_pending"].max() > 4
    assert_same_as_oracle(g, o)
    assert_same_runs(g, run_separate(ctx, tr, ring=4))


@pytest.mark.parametrize("p", [0, 1, 64, 65, 200])
def test_precondition_error_mid_trace(ctx, p):
    """The tick at index p is lower than what precedes it: the previous publish, or for p = 0 the nodes'
    first adverts (which the first publish must follow).  The replication ends with FOGNET_ERR_ARG after
    n_tasks <= p tasks: outputs below n_tasks equal the oracle's (of the trace without the fault: a
    task's outcome depends on no later publish), entries past them keep the poison."""
    good = with_power(tg.make_batch(0x5EED0733, 2, 16, 300, rho=0.9))
    o = run_oracle(good)
    tr = {k: v.copy() for k, v in good.items()}
    if p == 0:
        tr["arrive"][1, 0] = tr["init"][1].max()
    else:
        tr["arrive"][1, p] = tr["arrive"][1, p - 1] - 1
    g = run_all(ctx, tr)
    s = run_separate(ctx, tr)
    assert g["stats"]["status"][0] == 0 and g["stats"]["status"][1] == _abi.FOGNET_ERR_ARG
    n = int(g["stats"]["n_tasks"][1])
    assert 0 <= n <= p
    for k in ARRAYS:
        np.testing.assert_array_equal(g[k][0], o[k][0], err_msg=k)
        np.testing.assert_array_equal(g[k][1, :n], o[k][1, :n], err_msg=k)
        assert (g[k][1, n:] == np.array(POISON[k]).astype(g[k].dtype)).all(), k
        np.testing.assert_array_equal(g[k], s[k], err_msg=k)
    assert (g["node"][1, :n] >> 8 == 0).all()
    assert g["stats"][:1].tobytes() == o["stats"][:1].tobytes()
    assert g["stats"].tobytes() == s["stats"].tobytes()
    np.testing.assert_array_equal(g["hist"], s["hist"])
    np.testing.assert_array_equal(g["energy"], s["energy"])


@pytest.mark.parametrize("T,N", [(257, 256), (1000, 65)])
def test_statistics_only_equals_full_run(ctx, T, N):
    """Per-task outputs null: the epilogue reads the words from the internal scratch and writes nothing
    back; same record, histogram and energy as the full run."""
    tr, o = sweep_case(T, N)
    so = run_all(ctx, tr, per_task=False)
    assert so["stats"].tobytes() == o["stats"].tobytes()
    np.testing.assert_array_equal(so["hist"], o["hist"].sum(axis=0))
    np.testing.assert_array_equal(so["energy"], o["node_energy"])
    full = run_all(ctx, tr)
    assert so["stats"].tobytes() == full["stats"].tobytes()
