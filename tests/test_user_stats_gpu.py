"""User-side signals on the device (fognet_user_stats_dev) at the edges of its block
reduction, its emission rule, every policy and replay kernel that can feed it, an
aborted and a failed replication, and its refusal of EXT_HIER.

Every comparison is exact equality of all nine fognet_moments fields of all four
signals: against the oracle's event-level records and against the independent Python
restatement (user_stats_ref).  The cases and their references come from
test_user_stats.py, which checks them against each other without a GPU."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import tracegen as tg
import user_stats_ref as us
from fognetsimpp_amd import _abi
from test_user_stats import (HIER_UP, abort_case, batch_case, case, down_case, hier_case, sweep_case, user_links)

pytestmark = pytest.mark.gpu

USER = _abi.USER_STATS_DTYPE
assert USER.itemsize == us.USER_STATS_DTYPE.itemsize == 4 * 72


def device_user(ctx, tr, uu, ud, policy="REF_V3", user_policy=None, **kw):
    """Replay on the device, then the user pass: ([R] records, rep records, (trace, outputs))."""
    d = fa.as_device_trace(tr, torch.device("cuda", ctx.device))
    out = fa.run_batch(ctx, d, policy=policy, **kw)
    g = fa.user_stats(ctx, d, out, uu, ud, policy=user_policy)
    return g, out.rep_stats(), (d, out)


def check(ctx, c, policy="REF_V3", **kw):
    """The device's records equal the oracle's events and the restatement."""
    tr, uu, ud, o, want = c
    g, st, _ = device_user(ctx, tr, uu, ud, policy, **kw)
    np.testing.assert_array_equal(st["status"], o["stats"]["status"])
    np.testing.assert_array_equal(st["n_tasks"], o["stats"]["n_tasks"])
    us.assert_user_parity(g, o["user"])
    us.assert_user_parity(g, want)
    return g, st


# ---------------------------------------------------------------- reduction edges

@pytest.mark.parametrize("links", ["per_task", "per_replication_shared_nodes"])
@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 511, 513])
def test_reduction_edges(ctx, T, links):
    """Fewer tasks than the block's 256 threads, one less / exactly / one more than a
    stride, and the same around two strides; per-task links, and links [R] with node
    parameters shared by the replications (node_stride = 0)."""
    per_task = links == "per_task"
    c = batch_case(3, T, per_task=per_task, shared=not per_task)
    o = c[3]
    if T >= 255:
        assert (o["status"] == 4).any(axis=1).all() and (o["status"] == 5).any(axis=1).all()
    g, _ = check(ctx, c)
    assert (g["delay"]["count"] == T).all()


# ---------------------------------------------------------------- the emission rule

def test_boundary_sweep_on_the_device(ctx):
    """ms_raw(d) = toInt64((double)d * 1000.0) for every d of test_user_stats.SWEEP_D
    (around 2^53 and around 2^63 / 1000), fed in through per-task user links."""
    g, _ = check(ctx, sweep_case())
    h1 = g[0]["latencyH1"]
    assert int(h1["count"]) > 0 and int(h1["overflow"]) > 0 and int(h1["sq_top"]) > 0


# ---------------------------------------------------------------- policies and kernels

@pytest.mark.parametrize("N", [64, 300])  # register kernel / wide kernel
def test_ext_lat(ctx, N):
    check(ctx, batch_case(N, 300, "EXT_LAT"), "EXT_LAT")


def test_rows_from_the_wide_hand_over(ctx):
    """An overloaded replication between two light ones, rings of 4 entries: its rows are
    written by the wide kernel after the register kernel handed it over."""
    def make():
        over, light = tg.make_batch(11, 1, 4, 300, rho=3.0), tg.make_batch(12, 2, 4, 300, rho=0.01)
        tr = {k: np.concatenate([light[k][:1], over[k], light[k][1:]]) for k in over}
        return (tr, *user_links(0x4A, (3, 300)))
    g, st = check(ctx, case("handover", make), ring_capacity=4)
    assert int(st["max_pending"][1]) > 4 and (st["status"] == 0).all()


def test_node_down(ctx):
    c = down_case()
    o = c[3]
    assert (o["status"] == 9).any() and (o["done"] == -1).any()
    check(ctx, c)


def test_ref_aborted_replication_keeps_its_full_record(ctx):
    c = abort_case()
    tr, uu, ud, o, want = c
    check(ctx, c)
    g, st, _ = device_user(ctx, tr, uu, ud, ref_abort=True)
    assert int(st["status"][0]) == _abi.FOGNET_REF_ABORTED
    us.assert_user_parity(g, o["user"])  # the oracle's full run
    assert int(g[0]["taskTime"]["overflow"]) > 0 and not us.is_empty(g[0])


# ---------------------------------------------------------------- failed in mid-trace

@pytest.mark.parametrize("N", [16, 300])  # register kernel / wide kernel
@pytest.mark.parametrize("p", [1, 256, 257])
def test_failed_mid_trace_gets_the_empty_record(ctx, N, p):
    """Replication 1 is refused at publish p (out of order), after its first decisions for
    p = 256, 257.  Its rows are undefined, so the user pass must not read them: the outputs
    are pre-filled with in-range values (node 0, status 5, start = done = 0), so a kernel
    that still walks the rows produces a non-empty record, not an out-of-range index."""
    tr, uu, ud, o, want = batch_case(N, 300, R=3)
    tr = dict(tr, arrive=tr["arrive"].copy())
    tr["arrive"][1, p] = tr["arrive"][1, p - 1] - 1
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    out = fa.allocate_outputs(3, 300, dev)
    out.node.zero_()
    out.status.fill_(5)
    out.start_tick.zero_()
    out.done_tick.zero_()
    fa.run_batch(ctx, d, out=out)
    nres = 3 * USER.itemsize
    res = torch.full((nres,), 0xA5, dtype=torch.uint8, device=dev)
    g = fa.user_stats(ctx, d, out, uu, ud, res=res)
    st = out.rep_stats()
    assert [int(s) for s in st["status"]] == [0, _abi.FOGNET_ERR_ARG, 0]
    assert 0 <= int(st["n_tasks"][1]) <= p
    assert us.is_empty(g[1]), {s: int(g[1][s]["count"]) for s in us.SIGNALS}
    assert res.cpu().numpy()[USER.itemsize:2 * USER.itemsize].tobytes() == us.empty_record().tobytes()  # in full
    us.assert_user_parity(g[[0, 2]], o["user"][[0, 2]])
    us.assert_user_parity(g[[0, 2]], want[[0, 2]])


# ---------------------------------------------------------------- refusal

def test_ext_hier_is_refused(ctx):
    """fognet_user_stats_dev refuses EXT_HIER (test_user_stats.py pins why), whether
    fa.user_stats takes the policy run_batch recorded or is told it, and writes nothing.
    The C ABI goes by the policy its caller states and cannot know better: the same
    outputs passed as REF_V3 are still computed, as the closed form over the rows (every
    ack taken to leave at t + dl_k), which is not what the escalating run emitted."""
    tr, uu, ud, o, want = hier_case(0)
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    out = fa.run_batch(ctx, d, policy="EXT_HIER", hier_threshold_s=0, hier_up_tick=HIER_UP)
    assert out.policy == _abi.FOGNET_POLICY_EXT_HIER and int(out.rep_stats()["status"][0]) == 0
    np.testing.assert_array_equal(out.node.cpu().numpy(), o["node"])
    for kw in ({}, {"policy": "EXT_HIER"}, {"policy": _abi.FOGNET_POLICY_EXT_HIER}):
        res = torch.full((USER.itemsize,), 0xA5, dtype=torch.uint8, device=dev)
        plain = out if not kw else fa.BatchResult(out.node, out.status, out.start_tick, out.done_tick, out.stats)
        with pytest.raises(fa.FognetError) as e:
            fa.user_stats(ctx, d, plain, uu, ud, res=res, **kw)
        assert e.value.code == _abi.FOGNET_ERR_UNSUPPORTED, kw
        assert "escalat" in ctx.last_error() and "escalat" in str(e.value)
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == 0xA5).all(), kw
    g = fa.user_stats(ctx, d, out, uu, ud, policy="REF_V3")
    us.assert_user_parity(g, want)
    assert int(g[0]["latencyH1"]["sum_lo"]) != int(o["user"][0]["latencyH1"]["sum_lo"])


def test_recorded_policy_and_default(ctx):
    """run_batch records the policy it ran on the result it returns or fills; buffers it
    did not fill are taken as REF_V3, as before."""
    tr, uu, ud, o, want = batch_case(3, 257)
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    assert fa.allocate_outputs(3, 257, dev).policy is None
    out = fa.run_batch(ctx, d, policy="EXT_LAT", out=fa.allocate_outputs(3, 257, dev))
    assert out.policy == _abi.FOGNET_POLICY_EXT_LAT
    out = fa.run_batch(ctx, d)
    assert out.policy == _abi.FOGNET_POLICY_REF_V3
    bare = fa.BatchResult(out.node, out.status, out.start_tick, out.done_tick, out.stats)
    us.assert_user_parity(fa.user_stats(ctx, d, bare, uu, ud), want)
