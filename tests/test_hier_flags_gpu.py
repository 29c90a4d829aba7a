"""EXT_HIER on the device: the per-task escalation flags (fognet_batch_out.escalated) of
every replay path, and the user-signal and per-node statistics passes that consume them.

The flags are compared with the ones hier_ref rebuilds from the oracle's run (which
asserts that they reproduce the oracle's decisions), the statistics with the oracle's
event-level records and with the restatements' records built from those flags, all by
exact equality.  test_hier_flags.py checks the same cases and references without a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import hier_ref as hr
import node_stats_ref as ns
import tracegen as tg
import user_stats_ref as us
from fognetsimpp_amd import _abi
from guarded import Arena
from test_parity_gpu import assert_parity, escalations_in_flight

pytestmark = pytest.mark.gpu

NODE, USER, REP = _abi.NODE_STATS_DTYPE, _abi.USER_STATS_DTYPE, _abi.REP_STATS_DTYPE
NEVER = np.iinfo(np.int64).max
HIER_ENV = ("FOGNET_HIER_REGIONS", "FOGNET_HIER_RESUME")
# the replay paths (fognet_hip.h, fognet_hier_path_stats): the region pass handing over at the first
# escalated publish; the region pass and a sequential replay from the start; the sequential replay alone
MODES = {"resume": {}, "restart": {"FOGNET_HIER_REGIONS": "1", "FOGNET_HIER_RESUME": "0"},
         "sequential": {"FOGNET_HIER_REGIONS": "0"}}


def set_mode(monkeypatch, mode):
    for k in HIER_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def replay(ctx, tr, thr, up, **kw):
    """EXT_HIER replay with the flags; the array holds 0xA5 before the call."""
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    R, T = d["arrive"].shape
    out = fa.allocate_outputs(R, T, dev, escalated=True)
    out.escalated.fill_(0xA5)
    fa.run_batch(ctx, d, out=out, policy="EXT_HIER", hier_threshold_s=thr, hier_up_tick=up, **kw)
    return d, out


def host(out) -> dict:
    return dict(node=out.node.cpu().numpy(), status=out.status.cpu().numpy(), start=out.start_tick.cpu().numpy(),
                done=out.done_tick.cpu().numpy(), stats=out.rep_stats(), escalated=out.escalated.cpu().numpy())


def node_records(ctx, d, out, **kw) -> np.ndarray:
    R, N = d["arrive"].shape[0], d["mips"].shape[-1]
    return fa.node_stats(ctx, d, out, policy="EXT_HIER", **kw).cpu().numpy().view(NODE).reshape(R, N)


# ---------------------------------------------------------------- the flags, every path

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(hr.CASES))
def test_flags_equal_the_oracles_decisions(ctx, monkeypatch, name, mode):
    tr, uu, ud, o, flags, thr, up = hr.case(name)
    set_mode(monkeypatch, mode)
    before = ctx.hier_path_stats()
    d, out = replay(ctx, tr, thr, up)
    g = host(out)
    after = ctx.hier_path_stats()
    if tr["mips"].shape[-1] > hr.REGION_NODES:  # the path the mode names ran
        assert (after[0] - before[0], after[1] - before[1]) == ((0, 1) if mode == "sequential" else (1, 0))
    assert_parity(tr, g, o)
    assert g["stats"].tobytes() == o["stats"].tobytes()
    np.testing.assert_array_equal(g["escalated"], flags)
    assert out.policy == _abi.FOGNET_POLICY_EXT_HIER and out.hier_up_tick == up


@pytest.mark.parametrize("up_s", [1000, 60])
def test_flags_of_spilled_escalations(ctx, up_s):
    """test_hier_pending_escalations_spill_to_hbm's shape at T = 1000: every publish is region
    1's (6 nodes), threshold 0, so hundreds of escalated tasks are in flight at once and wait
    in the HBM overflow list; with the 1000-s hop they are all pushed by the end-of-trace flush,
    with the 60-s hop they are drained in mid-trace.  Region 0 always holds a node that
    advertises 0 s, so the parent never chooses region 1: the flag is node // 1024 != region."""
    up = up_s * hr.TPS
    tr, uu, ud = hr.make_trace(22, 3, 1030, 1000, 200 * hr.MS, lambda g, s: np.ones(s, np.int32))
    o = hr.run_oracle(tr, uu, ud, 0, up)
    assert escalations_in_flight(tr, o, tr["region"], up) > 64, "the trace no longer spills past the LDS slots"
    flags = hr.expected_flags(tr, o, tr["region"], 0, up)
    np.testing.assert_array_equal(flags, o["node"] // hr.REGION_NODES != tr["region"])
    d, out = replay(ctx, tr, 0, up)
    g = host(out)
    assert_parity(tr, g, o)
    assert g["stats"].tobytes() == o["stats"].tobytes()
    np.testing.assert_array_equal(g["escalated"], flags)
    us.assert_user_parity(fa.user_stats(ctx, d, out, uu, ud), o["user"])


# ---------------------------------------------------------------- the statistics passes

@pytest.mark.parametrize("name,layout", [("D", "lds"), ("D", "hbm"), ("B", "default"), ("C", "default")])
def test_statistics_on_the_same_replays(ctx, monkeypatch, name, layout):
    """N = 5: the accumulators in LDS, and the caller's records forced (FOGNET_NODE_STATS=hbm);
    N = 1030 / 2052: the caller's records.  With 5 nodes most 64-task steps hold groups of 8
    tasks and more on one node (the grouped commit)."""
    tr, uu, ud, o, flags, thr, up = hr.case(name)
    if layout == "hbm":
        monkeypatch.setenv("FOGNET_NODE_STATS", "hbm")
    else:
        monkeypatch.delenv("FOGNET_NODE_STATS", raising=False)
    d, out = replay(ctx, tr, thr, up)
    np.testing.assert_array_equal(out.escalated.cpu().numpy(), flags)
    g = fa.user_stats(ctx, d, out, uu, ud)  # (policy and hop: what run_batch recorded)
    us.assert_user_parity(g, o["user"])
    us.assert_user_parity(g, hr.user_expected(tr, o, uu, ud, flags, up))
    us.assert_user_parity(fa.user_stats(ctx, d, out, uu, ud, policy="EXT_HIER", hier_up_tick=up), o["user"])
    recs = node_records(ctx, d, out)
    ns.assert_records_equal(recs, hr.node_expected(tr, o, flags, up), name)
    for r in range(flags.shape[0]):
        ns.assert_merge_is_rep_record(recs[r], o["stats"][r])
    # without the array both passes refuse as before, and write nothing
    bare = fa.BatchResult(out.node, out.status, out.start_tick, out.done_tick, out.stats, policy=out.policy)
    for call in (lambda res: fa.user_stats(ctx, d, bare, uu, ud, res=res),
                 lambda res: fa.node_stats(ctx, d, bare, policy="EXT_HIER", res=res)):
        res = torch.full((recs.nbytes,), 0xA5, dtype=torch.uint8, device=d["arrive"].device)
        with pytest.raises(fa.FognetError) as e:
            call(res)
        assert e.value.code == _abi.FOGNET_ERR_UNSUPPORTED and "escalated" in str(e.value)
        torch.cuda.synchronize()
        assert (res.cpu().numpy() == 0xA5).all()


def test_statistics_with_a_crashed_node(ctx):
    """Case D with the node that receives most escalated tasks crashing at publish 150 (EXT_HIER
    with down_tick replays sequentially): escalated tasks are lost at it (status 9, flag 1) and
    accepted ones never complete.  Checked through the records: the oracle's events and record."""
    tr, uu, ud, o, flags, thr, up = hr.case("D")
    k = int(np.argmax(np.bincount(o["node"][0][flags[0] == 1], minlength=5)))
    down = np.full(5, NEVER, np.int64)
    down[k] = int(tr["arrive"][0, 150])
    trd = dict(tr, down=down)
    od = hr.run_oracle(trd, uu, ud, thr, up)
    assert (od["stats"]["status"] == 0).all()
    assert (od["status"] == 9).any(axis=1).all() and ((od["status"] != 9) & (od["done"] == -1)).any()
    d, out = replay(ctx, trd, thr, up)
    g = host(out)
    assert_parity(trd, g, od)
    lost = g["status"] == 9
    assert set(np.unique(g["escalated"])) == {0, 1} and (g["escalated"][lost] == 1).any()
    us.assert_user_parity(fa.user_stats(ctx, d, out, uu, ud), od["user"])
    recs = node_records(ctx, d, out)
    for r in range(2):
        ns.assert_merge_is_rep_record(recs[r], od["stats"][r])
        ns.assert_merge_is_rep_record(recs[r], g["stats"][r])
    np.testing.assert_array_equal(recs["n_lost"].sum(axis=1), lost.sum(axis=1))


@pytest.mark.parametrize("name", ["D", "B"])
def test_failed_replication_between_two_good_ones(ctx, name):
    """Replication 1 is replication 0's trace with publish 150 out of order: refused in
    mid-trace, after escalations.  Its rows are undefined (pre-filled with in-range values and
    flags of 1), so it must get the empty user record and N empty node records."""
    tr, uu, ud, o, flags, thr, up = hr.case(name)
    N = tr["mips"].shape[-1]
    pick = [0, 0, 1]
    t3 = {k: (v[pick].copy() if k in ("arrive", "req", "region") else v) for k, v in tr.items()}
    t3["arrive"][1, 150] = t3["arrive"][1, 149] - 1
    uu3, ud3, f3 = uu[pick], ud[pick], flags[pick]
    o3 = {k: o[k][pick] for k in ("node", "status", "start", "done", "stats", "user")}
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(t3, dev)
    T = t3["arrive"].shape[1]
    out = fa.allocate_outputs(3, T, dev, escalated=True)
    out.node.zero_()
    out.status.fill_(4)
    out.start_tick.zero_()
    out.done_tick.zero_()
    out.escalated.fill_(1)
    fa.run_batch(ctx, d, out=out, policy="EXT_HIER", hier_threshold_s=thr, hier_up_tick=up)
    st = out.rep_stats()
    assert [int(s) for s in st["status"]] == [0, _abi.FOGNET_ERR_ARG, 0]
    ok = [0, 2]
    np.testing.assert_array_equal(out.escalated.cpu().numpy()[ok], f3[ok])
    g = fa.user_stats(ctx, d, out, uu3, ud3)
    assert us.is_empty(g[1])
    us.assert_user_parity(g[ok], o3["user"][ok])
    recs = node_records(ctx, d, out)
    assert recs[1].tobytes() == ns.empty_records(N).tobytes()
    want = hr.node_expected(t3, o3, f3, up, statuses=[0, _abi.FOGNET_ERR_ARG, 0])
    ns.assert_records_equal(recs, want, name)


# ---------------------------------------------------------------- arguments and contract

@pytest.mark.parametrize("N", [5, 300])  # register kernel / wide kernel
@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
def test_other_policies_clear_the_array(ctx, policy, N):
    tr = tg.make_batch(0xE5C + N, 3, N, 257, rho=0.9)
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    plain = fa.run_batch(ctx, d, policy=policy)
    out = fa.allocate_outputs(3, 257, dev, escalated=True)
    out.escalated.fill_(0xA5)
    fa.run_batch(ctx, d, out=out, policy=policy)
    assert (out.escalated.cpu().numpy() == 0).all()
    for k in ("node", "status", "start_tick", "done_tick", "stats"):
        assert torch.equal(getattr(out, k), getattr(plain, k)), k
    fresh = fa.run_batch(ctx, d, policy=policy, escalated=True)  # (run_batch allocates it)
    assert fresh.escalated.shape == (3, 257) and fresh.escalated.dtype == torch.uint8
    assert (fresh.escalated.cpu().numpy() == 0).all() and fresh.hier_up_tick == 0
    assert plain.escalated is None


def test_statistics_only_out_refuses_the_array(ctx):
    tr, uu, ud, o, flags, thr, up = hr.case("D")
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    with pytest.raises(fa.FognetError) as e:
        fa.allocate_outputs(2, 300, dev, per_task=False, escalated=True)
    assert e.value.code == _abi.FOGNET_ERR_ARG
    so = fa.allocate_outputs(2, 300, dev, per_task=False)
    so.escalated = torch.full((2, 300), 0xA5, dtype=torch.uint8, device=dev)
    for policy in ("EXT_HIER", "REF_V3"):
        so.stats.fill_(0xA5)
        with pytest.raises(fa.FognetError) as e:
            fa.run_batch(ctx, d, out=so, policy=policy, hier_threshold_s=thr, hier_up_tick=up)
        assert e.value.code == _abi.FOGNET_ERR_ARG and "escalated" in str(e.value)
        torch.cuda.synchronize()
        assert (so.escalated.cpu().numpy() == 0xA5).all() and (so.stats.cpu().numpy() == 0xA5).all()
    so.escalated = None  # (and without it the statistics-only replay runs as before)
    fa.run_batch(ctx, d, out=so, policy="EXT_HIER", hier_threshold_s=thr, hier_up_tick=up)
    assert so.rep_stats().tobytes() == o["stats"].tobytes()


def test_host_buffer_call_copies_the_flags_out(ctx):
    """fognet_run_batch (host pointers): the array travels like the other per-task outputs."""
    tr, uu, ud, o, flags, thr, up = hr.case("D")
    R, T = tr["arrive"].shape
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    node, status = np.empty((R, T), np.int32), np.empty((R, T), np.uint8)
    start, done = np.empty((R, T), np.int64), np.empty((R, T), np.int64)
    stats, esc = np.zeros(R, REP), np.full((R, T), 0xA5, np.uint8)
    bi = _abi.BatchIn(R, T, 5, _abi.FOGNET_POLICY_EXT_HIER, 0, 0, *(ptr(tr[k]) for k in
                      ("arrive", "req", "mips", "dl", "ul", "init")), None, None, None, ptr(tr["region"]), up, thr, 0)
    bo = _abi.BatchOut(ptr(node), ptr(status), ptr(start), ptr(done), ptr(stats), None, None, ptr(esc))
    assert ctx._lib.fognet_run_batch(ctx.handle, C.byref(bi), C.byref(bo)) == _abi.FOGNET_OK, ctx.last_error()
    np.testing.assert_array_equal(node, o["node"])
    np.testing.assert_array_equal(esc, flags)
    assert stats.tobytes() == o["stats"].tobytes()


def guarded_flags(ctx, tr, thr, up, poison, misalign):
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    R, T = tr["arrive"].shape
    arena = Arena(dev, poison, 1 << 18)
    out = fa.allocate_outputs(R, T, dev)
    out.escalated = arena.alloc((R, T), torch.uint8, misalign, "escalated")
    if misalign:
        assert out.escalated.data_ptr() % 2 == 1
    fa.run_batch(ctx, d, out=out, policy="EXT_HIER", hier_threshold_s=thr, hier_up_tick=up)
    torch.cuda.synchronize()
    arena.check()
    return host(out)


@pytest.mark.parametrize("T", [63, 65, 129])
@pytest.mark.parametrize("name", ["D", "B"])
def test_buffer_contract(ctx, name, T):
    """The array as a poisoned, guard-banded view, R = 2 or 3 rows of T = 63, 65, 129 (a short
    chunk, one publish past a chunk, past two): nothing outside it is written, its contents
    do not depend on what it held, and a 1-B-aligned pointer will do.  D escalates from publish
    34 on (the sequential kernel's stores); B's replications 0 and 1 are finished by the region
    pass up to T = 65, handed over at T = 129 (replication 1 at publish 71), and its
    replication 2 never escalates.  A prefix of a trace is decided like the whole trace."""
    tr, uu, ud, o, flags, thr, up = hr.case(name)
    cut = {k: (np.ascontiguousarray(v[:, :T]) if k in ("arrive", "req", "region") else v) for k, v in tr.items()}
    want = np.ascontiguousarray(flags[:, :T])
    assert want.any() == (name == "D" or T == 129)
    runs = [guarded_flags(ctx, cut, thr, up, poison, misalign) for poison, misalign in
            ((0xA5, False), (0x5A, False), (0xA5, True))]
    for g in runs:
        assert (g["stats"]["status"] == 0).all()
        np.testing.assert_array_equal(g["node"], o["node"][:, :T])
        np.testing.assert_array_equal(g["escalated"], want)
