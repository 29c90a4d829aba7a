"""The assigned replay on the device (fognet_replay_assigned_dev, fognet_run_assigned_dev), byte
for byte: against the oracle where the oracle made the decisions, against the plain-Python
restatement (assigned_ref, pinned on the CPU by test_assigned_ref.py) where it cannot, in the
default layout and with the workspace layout forced (FOGNET_ASSIGNED=hbm)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import assigned_ref as ar
import fognetsimpp_amd as fa
import golden_io
import node_stats_ref as ns
import oracle_lib as ol
import per_user_ref as pu
import signal_vectors_ref as sv
import stream_gate
import tracegen as tg
from fognetsimpp_amd import _abi
from guarded import Arena
from test_parity_gpu import tie_heavy, with_crashes
from test_per_user_stats import draw_links, draw_users

pytestmark = pytest.mark.gpu

REP, NODE, USER = _abi.REP_STATS_DTYPE, _abi.NODE_STATS_DTYPE, _abi.USER_STATS_DTYPE
TPS = 10**12
LAYOUTS = ("lds", "hbm")
RECORD_FIELDS = ("n_tasks", "n_queued", "n_started", "last_tick", "queue_min_raw", "queue_max_raw",
                 "resp_min_ticks", "resp_max_ticks", "queue_sum_lo", "queue_sum_hi", "queue_sq_lo", "queue_sq_hi",
                 "queue_sq_top", "n_qtime", "n_qtime_overflow", "abort_tick", "abort_task",
                 "resp_sum_lo", "resp_sum_hi", "resp_sq_lo", "resp_sq_hi", "events", "max_pending")  # assert_parity's
_oracle: dict = {}


def set_layout(monkeypatch, layout):
    if layout == "hbm":
        monkeypatch.setenv("FOGNET_ASSIGNED", "hbm")
    else:
        monkeypatch.delenv("FOGNET_ASSIGNED", raising=False)


def dev_of(ctx):
    return torch.device("cuda", ctx.device)


def oracle(key, make, policy="REF_V3", power=False):
    """(trace, oracle result), computed once per key and left unchanged."""
    if key not in _oracle:
        tr = make()
        if power:
            pb, pi = fa.power_model(tr["mips"])
            tr = dict(tr, p_busy=pb, p_idle=pi)
        o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=4,
                         policy=ol.POLICIES[policy], down=tr.get("down"), p_busy=tr.get("p_busy"),
                         p_idle=tr.get("p_idle"), hist=True)
        _oracle[key] = (tr, o)
    return _oracle[key]


def run_dev(ctx, tr, assign, stats=True):
    """fa.run_assigned on host arrays; everything back on the host."""
    d = fa.as_device_trace(tr, dev_of(ctx))
    a = torch.from_numpy(np.ascontiguousarray(assign, dtype=np.int32)).to(dev_of(ctx))
    out = fa.run_assigned(ctx, d, a, stats=stats, hist=stats, energy=stats and "p_busy" in tr)
    torch.cuda.synchronize()
    g = dict(node=out.node.cpu().numpy(), status=out.status.cpu().numpy(), start=out.start_tick.cpu().numpy(),
             done=out.done_tick.cpu().numpy(), stats=out.rep_stats().copy(),
             hist=out.hist.cpu().numpy() if out.hist is not None else None,
             energy=out.node_energy.cpu().numpy() if out.node_energy is not None else None)
    return g


def both_layouts(ctx, monkeypatch, tr, assign, **kw):
    """Both layouts, byte-identical in every output; returns the default one's."""
    got = {}
    for layout in LAYOUTS:
        set_layout(monkeypatch, layout)
        got[layout] = run_dev(ctx, tr, assign, **kw)
    a, b = got["lds"], got["hbm"]
    for k in ("node", "status", "start", "done", "stats", "hist", "energy"):
        assert (a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes(), k
    return a


def assert_equals_oracle(g, o, what=""):
    """The four arrays and the whole record (assert_parity's field list, then every byte), the job
    histogram and the energy."""
    np.testing.assert_array_equal(g["stats"]["status"], o["stats"]["status"], err_msg=what)
    for k in ("node", "status", "start", "done"):
        np.testing.assert_array_equal(g[k], o[k], err_msg=f"{what} {k}")
    for f in RECORD_FIELDS:
        np.testing.assert_array_equal(g["stats"][f], o["stats"][f], err_msg=f"{what} {f}")
    assert g["stats"].tobytes() == o["stats"].tobytes(), what
    np.testing.assert_array_equal(g["hist"], o["hist"].sum(axis=0), err_msg=what)
    if o["node_energy"] is not None:
        np.testing.assert_array_equal(g["energy"], o["node_energy"], err_msg=what)


def assert_equals_ref(g, want, what=""):
    """The four arrays and the replay fields against assigned_ref."""
    ok = want["stats"]["status"] == 0
    np.testing.assert_array_equal(g["stats"]["status"], want["stats"]["status"], err_msg=what)
    for f in ("n_tasks", "max_pending", "events"):
        np.testing.assert_array_equal(g["stats"][f], want["stats"][f], err_msg=f"{what} {f}")
    for k in ("node", "status", "start", "done"):
        np.testing.assert_array_equal(g[k][ok], want[k][ok], err_msg=f"{what} {k}")


def assert_empty_record(rec):
    assert int(rec["status"]) == _abi.FOGNET_ERR_ARG
    for f in ("n_tasks", "n_queued", "n_started", "events", "max_pending", "busy_s", "n_qtime", "n_qtime_overflow",
              "queue_sum_lo", "queue_sum_hi", "queue_sq_lo", "queue_sq_hi", "queue_sq_top", "resp_sum_lo",
              "resp_sum_hi", "resp_sq_lo", "resp_sq_hi"):
        assert int(rec[f]) == 0, f
    i64 = np.iinfo(np.int64)
    assert float(rec["energy_j"]) == 0.0 and int(rec["abort_tick"]) == i64.max and int(rec["abort_task"]) == -1
    assert int(rec["queue_min_raw"]) == i64.max == int(rec["resp_min_ticks"])
    assert int(rec["queue_max_raw"]) == i64.min == int(rec["resp_max_ticks"]) == int(rec["last_tick"])


# ---------------------------------------------------------------- 1: the oracle's own decisions

@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
@pytest.mark.parametrize("N", [1, 3, 64, 65, 256, 257, 300])
def test_oracle_round_trip(ctx, monkeypatch, N, policy):
    for T in (1, 63, 64, 65, 129, 300):
        for shared in (False, True):
            def make():
                tr = tg.make_batch(0x5EED0C00 + 31 * N + T, 5, N, T, rho=0.9 if T != 129 else 3.0)
                if shared:
                    tr = dict(tr, mips=tr["mips"][0], dl=tr["dl"][0], ul=tr["ul"][0], init=tr["init"][0])
                return tr
            tr, o = oracle(("rt", N, T, shared, policy), make, policy, power=True)
            assert (o["stats"]["status"] == 0).all()
            g = both_layouts(ctx, monkeypatch, tr, o["node"])
            assert_equals_oracle(g, o, f"N={N} T={T} shared={shared} {policy}")


def test_replay_only_writes_the_four_fields(ctx):
    tr, o = oracle(("only", 64), lambda: tg.make_batch(0x5EED0C01, 5, 64, 300, rho=0.9))
    g = run_dev(ctx, tr, o["node"], stats=False)
    for k in ("node", "status", "start", "done"):
        np.testing.assert_array_equal(g[k], o[k], err_msg=k)
    for f in ("status", "n_tasks", "max_pending", "events"):
        np.testing.assert_array_equal(g["stats"][f], o["stats"][f], err_msg=f)


# ---------------------------------------------------------------- 2: ties, known answers, recordings

@pytest.mark.parametrize("N", [1, 3, 38, 300])
def test_tie_heavy_traces(ctx, monkeypatch, N):
    for policy in ("REF_V3", "EXT_LAT"):
        tr, o = oracle(("tie", N, policy), lambda: tie_heavy(11 + N, 4, N, 300), policy)
        assert_equals_oracle(both_layouts(ctx, monkeypatch, tr, o["node"]), o, f"tie N={N} {policy}")


def test_known_answers_and_recordings(ctx, monkeypatch):
    cases = [(n, tr) for n, tr, _ in golden_io.replay_cases() + golden_io.replay_down_cases() + golden_io.qtime_cases()]
    cases += [(c[0], c[1]) for c in golden_io.ref_v3_replay_cases()]
    assert len(cases) >= 14 + 3
    for name, tr in cases:
        tr = {k: (np.atleast_2d(v) if k in ("arrive", "req") else v) for k, v in tr.items()}
        tr, o = oracle(("kat", name), lambda: tr)
        assert (o["stats"]["status"] == 0).all(), name
        assert_equals_oracle(both_layouts(ctx, monkeypatch, tr, o["node"]), o, name)


# ---------------------------------------------------------------- 3 + 4: assignments the oracle cannot make

def ref_case(key, make_trace, make_assign):
    if key not in _oracle:
        tr = make_trace()
        assign = np.ascontiguousarray(make_assign(tr), np.int32)
        _oracle[key] = (tr, assign, ar.replay(tr, assign))
    return _oracle[key]


def check_ref(ctx, monkeypatch, key, make_trace, make_assign):
    tr, assign, want = ref_case(key, make_trace, make_assign)
    assert (want["stats"]["status"] == 0).all()
    g = both_layouts(ctx, monkeypatch, tr, assign)
    assert_equals_ref(g, want, str(key))
    return tr, assign, want, g


@pytest.mark.parametrize("N", [1, 5, 64, 300])
def test_round_robin_and_random(ctx, monkeypatch, N):
    R, T = 3, 300
    dev = dev_of(ctx)
    rr = fa.assign_round_robin(R, T, N, dev)
    assert rr.dtype == torch.int32 and (rr.cpu().numpy() == (np.arange(T) % N)[None]).all()
    rnd = fa.assign_random(R, T, N, 7, dev)
    assert torch.equal(rnd, fa.assign_random(R, T, N, 7, dev)) and 0 <= int(rnd.min()) <= int(rnd.max()) < N
    assert N == 1 or not torch.equal(rnd, fa.assign_random(R, T, N, 8, dev))
    mk = lambda: tg.make_batch(0x5EED0D00 + N, R, N, T, rho=2.0)  # noqa: E731
    check_ref(ctx, monkeypatch, ("rr", N), mk, lambda tr: rr.cpu().numpy())
    check_ref(ctx, monkeypatch, ("rnd", N), mk, lambda tr: rnd.cpu().numpy())


@pytest.mark.parametrize("T", [300, 20000])
def test_everything_to_one_node(ctx, monkeypatch, T):
    """One segment through every tile: at T = 20,000 it is longer than anything the design holds at once."""
    assert T > _abi.ASSIGNED_TILE
    _, _, want, _ = check_ref(ctx, monkeypatch, ("one", T), lambda: tg.make_batch(0x5EED0E00 + T, 2, 7, T, rho=6.0),
                              lambda tr: np.full((2, T), 3))
    assert T == 300 or int(want["stats"]["max_pending"].max()) > _abi.ASSIGNED_TILE  # pending across many tiles


def test_highest_indices_of_seventy_thousand_nodes(ctx, monkeypatch):
    N, T = 70000, 300
    rng = np.random.default_rng(70000)
    check_ref(ctx, monkeypatch, ("high",), lambda: shared_nodes(tg.make_batch(0x5EED0F00, 2, 64, T, rho=3.0), N),
              lambda tr: N - 1 - rng.integers(0, 5, (2, T)))


def shared_nodes(tr, N):
    """The batch's trace over N shared nodes (the first row's parameters, repeated)."""
    rep = lambda v: np.resize(v[0], N)  # noqa: E731
    return dict(arrive=tr["arrive"], req=tr["req"], mips=rep(tr["mips"]), dl=rep(tr["dl"]), ul=rep(tr["ul"]),
                init=rep(tr["init"]))


def test_two_to_the_twenty_nodes(ctx, monkeypatch):
    N, T = 1 << 20, 64
    rng = np.random.default_rng(20)
    check_ref(ctx, monkeypatch, ("2^20",), lambda: shared_nodes(tg.make_batch(0x5EED1000, 1, 64, T, rho=3.0), N),
              lambda tr: rng.choice([0, 1, N - 1, N - 2, N // 2, 65536, 65535], (1, T)))


def test_zero_service_tasks_at_one_tick(ctx, monkeypatch):
    def make():
        arrive = np.repeat(np.array([[1000, 1000, 2000, 5000]], np.int64) * 10**9, 20, axis=1)
        arrive.sort(axis=1)
        req = np.zeros_like(arrive, dtype=np.int32)
        req[0, ::7] = 2500
        return dict(arrive=arrive, req=req, mips=np.array([1000, 2000], np.int32), dl=np.array([0, 10**9], np.int64),
                    ul=np.array([0, 5 * 10**8], np.int64), init=np.array([10, 10**9], np.int64))
    _, _, want, g = check_ref(ctx, monkeypatch, ("zero",), make, lambda tr: (np.arange(80) % 5 == 0)[None])
    assert (g["start"] == g["done"]).sum() >= 40 and int(want["stats"]["max_pending"][0]) >= 10


# ---------------------------------------------------------------- 5: node-down

@pytest.mark.parametrize("kind", ["random", "tie", "edges"])
def test_node_down(ctx, monkeypatch, kind):
    def make():
        if kind == "random":
            return with_crashes(tg.make_batch(0x5EED1100, 5, 9, 300, rho=1.5), seed=3, frac=0.5)
        if kind == "tie":
            return with_crashes(tie_heavy(301, 5, 24, 300), seed=5, frac=0.5, grid=10**11)
        # one node, 1-s services every 0.25 s: a crash while a task runs with others queued, exactly at
        # an arrival tick, and exactly at a completion tick (one replication each)
        arrive = np.tile((10 + np.arange(40, dtype=np.int64)) * (TPS // 4), (3, 1))
        req = np.full((3, 40), 1000, np.int32)
        one = lambda v: np.full((3, 1), v, np.int64)  # noqa: E731
        a0 = int(arrive[0, 0]) + 1000
        down = np.array([[a0 + 3 * TPS + TPS // 2], [int(arrive[1, 17]) + 1000], [a0 + 5 * TPS]], np.int64)
        return dict(arrive=arrive, req=req, mips=np.full((3, 1), 1000, np.int32), dl=one(1000), ul=one(2000),
                    init=one(5000), down=down)
    tr, o = oracle(("down", kind), make)
    assert (o["stats"]["status"] == 0).all() and (o["status"] == 9).any() and (o["done"] < 0).any()
    if kind == "edges":
        assert ((o["start"] >= 0) & (o["done"] < 0)).any(axis=1).all()  # a running task cut in each
        assert ((o["status"] == 4) & (o["start"] < 0)).any(axis=1).all()  # queued tasks that never start
    assert_equals_oracle(both_layouts(ctx, monkeypatch, tr, o["node"]), o, kind)


# ---------------------------------------------------------------- 6: ranges

def test_arrivals_offset_by_two_to_the_sixty(ctx, monkeypatch):
    def make():
        tr = tg.make_batch(0x5EED1200, 3, 6, 300, rho=0.9)
        return dict(tr, arrive=tr["arrive"] + (1 << 60))
    tr, o = oracle(("2^60",), make)
    assert (o["stats"]["status"] == 0).all()
    assert_equals_oracle(both_layouts(ctx, monkeypatch, tr, o["node"]), o, "2^60")


def test_sums_past_int64_are_refused_not_wrapped(ctx, monkeypatch):
    """mips = 1 and req = 2^31 - 1: one service is 2^31 - 1 s and 300 of them pass 2^63 ticks many
    times over; a wrapped sum must not come back as a valid tick."""
    T = 300
    tr = tg.make_batch(0x5EED1300, 3, 1, T, rho=0.9)
    tr["req"][1, :] = 2**31 - 1
    tr["mips"][1, 0] = 1
    assign = np.zeros((3, T), np.int32)
    want = ar.replay(tr, assign)
    assert want["stats"]["status"].tolist() == [0, 1, 0]
    g = both_layouts(ctx, monkeypatch, tr, assign)
    assert_equals_ref(g, want)
    assert_empty_record(g["stats"][1])
    keep = [0, 2]
    o = ol.run_batch(tr["arrive"][keep], tr["req"][keep], tr["mips"][keep], tr["dl"][keep], tr["ul"][keep],
                     tr["init"][keep], hist=True)
    assert g["stats"][keep].tobytes() == o["stats"].tobytes()
    np.testing.assert_array_equal(g["hist"], o["hist"].sum(axis=0))  # the refused one added nothing


# ---------------------------------------------------------------- 7: refusals

BAD = ["assign_high", "assign_negative", "arrive_decreasing", "req_negative", "mips_zero", "init_below_ul",
       "init_not_before_first_publish", "down_before_init", "tick_past_bound"]


@pytest.mark.parametrize("what", BAD)
def test_bad_replication_between_two_good_ones(ctx, monkeypatch, what):
    tr, o = oracle(("bad",), lambda: tg.make_batch(0x5EED1400, 3, 5, 129, rho=0.9))
    tr = {k: v.copy() for k, v in tr.items()}
    assign = o["node"].copy()
    if what == "assign_high":
        assign[1, 77] = 5
    elif what == "assign_negative":
        assign[1, 0] = -1
    elif what == "arrive_decreasing":
        tr["arrive"][1, 100] = tr["arrive"][1, 99] - 1
    elif what == "req_negative":
        tr["req"][1, 128] = -1
    elif what == "mips_zero":
        tr["mips"][1, 4] = 0
    elif what == "init_below_ul":
        tr["init"][1, 2] = tr["ul"][1, 2] - 1
    elif what == "init_not_before_first_publish":
        tr["init"][1, 0] = tr["arrive"][1, 0]
    elif what == "down_before_init":
        tr["down"] = np.full((3, 5), fa.NEVER, np.int64)
        tr["down"][1, 3] = tr["init"][1, 3] - 1
    elif what == "tick_past_bound":
        tr["arrive"][1, 128] = (1 << 61) + 1
    assert ar.replay(tr, assign)["stats"]["status"].tolist() == [0, 1, 0]
    g = both_layouts(ctx, monkeypatch, tr, assign)
    assert_empty_record(g["stats"][1])
    for r in (0, 2):
        for k in ("node", "status", "start", "done"):
            np.testing.assert_array_equal(g[k][r], o[k][r], err_msg=f"{what} {k}[{r}]")
        assert g["stats"][r].tobytes() == o["stats"][r].tobytes(), (what, r)


def test_call_level_refusals_and_empty_shapes(ctx):
    dev = dev_of(ctx)
    tr = tg.make_batch(3, 2, 4, 65)
    d = fa.as_device_trace(tr, dev)
    assign = fa.assign_round_robin(2, 65, 4, dev)
    lib = ctx._lib

    def call(fn, d, assign, out, N=None, down=None, power=False):
        R, T = d["arrive"].shape
        N = d["mips"].shape[-1] if N is None else N
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        bi = _abi.BatchIn(R, T, N, 77, N if d["mips"].dim() == 2 else 0, 3, p(d["arrive"]), p(d["req"]), p(d["mips"]),
                          p(d["dl"]), p(d["ul"]), p(d["init"]), p(d["dl"]) if power else None,
                          p(d["dl"]) if power else None, p(down), None, -5, -5, 0)  # policy, ring, hier_*: not read
        bo = _abi.BatchOut(p(out.node), p(out.status), p(out.start_tick), p(out.done_tick),
                           p(out.stats) if out.stats is not None else None, None, None, None)
        return fn(ctx.handle, C.byref(bi), p(assign), C.byref(bo), None)

    for fn in (lib.fognet_replay_assigned_dev, lib.fognet_run_assigned_dev):
        full = fa.allocate_outputs(2, 65, dev)
        assert call(fn, d, assign, full) == _abi.FOGNET_OK  # unknown policy, bad ring and hier fields are not read
        assert call(fn, d, assign, fa.allocate_outputs(2, 65, dev, per_task=False)) == _abi.FOGNET_ERR_ARG
        assert call(fn, d, None, full) == _abi.FOGNET_ERR_ARG
        no_stats = fa.allocate_outputs(2, 65, dev)
        no_stats.stats = None
        assert call(fn, d, assign, no_stats) == _abi.FOGNET_ERR_ARG
        assert call(fn, d, assign, full, N=(1 << 20) + 1) == _abi.FOGNET_ERR_UNSUPPORTED
        assert "1048576" in ctx.last_error()
        down = torch.full((2, 4), fa.NEVER, dtype=torch.int64, device=dev)
        assert call(fn, d, assign, full, down=down, power=True) == _abi.FOGNET_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    # R = 0 and T = 0
    e0 = fa.as_device_trace(tg.make_batch(3, 2, 4, 65), dev)
    e0 = dict(e0, arrive=e0["arrive"][:0], req=e0["req"][:0], mips=e0["mips"][:0], dl=e0["dl"][:0], ul=e0["ul"][:0],
              init=e0["init"][:0])
    fa.run_assigned(ctx, e0, torch.zeros((0, 65), dtype=torch.int32, device=dev))
    t0 = dict(d, arrive=d["arrive"][:, :0].contiguous(), req=d["req"][:, :0].contiguous())
    out = fa.run_assigned(ctx, t0, torch.zeros((2, 0), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    st = out.rep_stats()
    assert (st["status"] == 0).all() and (st["n_tasks"] == 0).all() and (st["events"] == 8).all()
    with pytest.raises(fa.FognetError):
        fa.run_assigned(ctx, d, assign.to(torch.int64))


# ---------------------------------------------------------------- 8: the passes over the outputs

def test_downstream_passes_on_a_random_assignment(ctx):
    R, T, N, U = 3, 300, 9, 5
    dev = dev_of(ctx)
    tr = tg.make_batch(0x5EED1500, R, N, T, rho=2.0)
    assign = fa.assign_random(R, T, N, 11, dev)
    want = ar.replay(tr, assign.cpu().numpy())
    d = fa.as_device_trace(tr, dev)
    out = fa.run_assigned(ctx, d, assign)
    nodes = fa.node_stats(ctx, d, out).cpu().numpy().view(NODE).reshape(R, N)
    ns.assert_records_equal(nodes, ns.expected(tr, want), "node_stats")
    st = out.rep_stats()
    for r in range(R):
        ns.assert_merge_is_rep_record(nodes[r], st[r])  # the record of fognet_run_assigned_dev
    who, (uu, ud) = draw_users(5, R, T, U, "random"), draw_links(6, R, U, False)
    buf, un = fa.per_user_stats(ctx, d, out, who, uu, ud)
    w_users, w_un = pu.expected(tr, want, who, uu, ud)
    pu.assert_records_equal(buf.cpu().numpy().view(USER).reshape(R, U), w_users, "per_user_stats")
    np.testing.assert_array_equal(un.cpu().numpy(), w_un)
    sv.assert_equal(fa.signal_vectors(ctx, d, out, who, uu, ud), sv.expected(tr, want, who, uu, ud), "signal_vectors")


# ---------------------------------------------------------------- 9: the buffer contract

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T", [1, 63, 65, 129])
def test_buffer_contract(ctx, monkeypatch, layout, T):
    """Poisoned guard-banded arenas, two poisons, natural alignment only, out->node aliasing assign,
    a refused replication between two good ones."""
    set_layout(monkeypatch, layout)
    R, N = 3, 7
    tr, o = oracle(("guard", T), lambda: tg.make_batch(0x5EED1600 + T, R, N, T, rho=2.0))
    assign = o["node"].copy()
    assign[1, T // 2] = N  # refused
    results = []
    for poison in (0xA5, 0x5A):
        for alias in (False, True):
            a = Arena(dev_of(ctx), poison)
            d = {k: a.put(tr[k], misalign=True, name=k) for k in ("arrive", "req", "mips", "dl", "ul", "init")}
            node = a.put(assign, misalign=True, name="assign/node" if alias else "assign")
            out = fa.BatchResult(node=node if alias else a.alloc((R, T), torch.int32, True, "node"),
                                 status=a.alloc((R, T), torch.uint8, True, "status"),
                                 start_tick=a.alloc((R, T), torch.int64, True, "start"),
                                 done_tick=a.alloc((R, T), torch.int64, True, "done"),
                                 stats=a.alloc(R * REP.itemsize, torch.uint8, False, "stats"),
                                 hist=a.put(np.zeros((2, 64), np.int64), True, "hist"),
                                 escalated=a.alloc((R, T), torch.uint8, True, "escalated"))
            fa.run_assigned(ctx, d, node, out=out)
            torch.cuda.synchronize()
            a.check()
            for k in d:
                assert d[k].cpu().numpy().tobytes() == np.ascontiguousarray(tr[k]).tobytes(), k  # inputs untouched
            st = out.rep_stats()
            assert_empty_record(st[1])
            ok = [0, 2]
            np.testing.assert_array_equal(out.node.cpu().numpy()[ok], o["node"][ok])
            if not alias:
                np.testing.assert_array_equal(node.cpu().numpy(), assign)
            for k, t in (("status", out.status), ("start", out.start_tick), ("done", out.done_tick)):
                np.testing.assert_array_equal(t.cpu().numpy()[ok], o[k][ok], err_msg=k)
            assert st[ok].tobytes() == o["stats"][ok].tobytes()
            assert not out.escalated.cpu().numpy()[ok].any()
            np.testing.assert_array_equal(out.hist.cpu().numpy(), o["hist"][ok].sum(axis=0))
            results.append(st[ok].tobytes())
    assert len(set(results)) == 1


# ---------------------------------------------------------------- 10: stream gate, determinism

def test_gated_side_stream_and_two_runs_byte_identical(ctx):
    R, T, N = 4, 300, 9
    dev = dev_of(ctx)
    tr = tg.make_batch(0x5EED1700, R, N, T, rho=2.0)
    decoy = tg.make_batch(0x5EED1701, R, N, T, rho=0.5)
    rng = np.random.default_rng(17)
    assign, assign_decoy = (rng.integers(0, N, (R, T)).astype(np.int32) for _ in range(2))
    want = ar.replay(tr, assign)
    names = ("arrive", "req", "mips", "dl", "ul", "init")

    class Job:
        def __init__(self):
            d = fa.as_device_trace(tr, dev)
            self.d = d
            self.assign = torch.from_numpy(assign).to(dev)
            self.inputs = dict({k: d[k] for k in names}, assign=self.assign)
            self.out = fa.allocate_outputs(R, T, dev, hist=True)

    def enqueue(job):
        fa.run_assigned(ctx, job.d, job.assign, out=job.out, stream=torch.cuda.current_stream(dev))

    gate = stream_gate.Gate(dev)
    gate.choose(1)
    kinds = dict(arrive=np.int64, req=np.int32, mips=np.int32, dl=np.int64, ul=np.int64, init=np.int64)
    decoys = dict({k: np.ascontiguousarray(decoy[k], dtype=kinds[k]) for k in names}, assign=assign_decoy)
    job = gate.run("assigned", "run_assigned", Job, decoys, enqueue)
    g = dict(node=job.out.node.cpu().numpy(), status=job.out.status.cpu().numpy(),
             start=job.out.start_tick.cpu().numpy(), done=job.out.done_tick.cpu().numpy(), stats=job.out.rep_stats())
    assert_equals_ref(g, want, "gated")
    again = run_dev(ctx, tr, assign)
    for k in ("node", "status", "start", "done", "stats"):
        assert again[k].tobytes() == g[k].tobytes(), k
    assert again["hist"].tobytes() == job.out.hist.cpu().numpy().tobytes()
