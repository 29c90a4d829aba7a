"""The buffer contract of every device entry point (include/fognet_hip.h,
"Buffers"), pinned with guarded, poisoned arenas (tests/guarded.py).

The parity tests compare the R x T (or R, or m) elements the caller asked for,
on 512-B-aligned tensors whose records were zeroed.  Here every input and every
output of a call is a view into a poisoned arena with 4,096 B of poison on
either side, and each case asserts

(a) no byte outside the views changed (a store past a tail mask, a phantom
    replication of a ragged wavefront, a block edge of the reduction);
(b) the defined outputs equal the oracle (or, for the trace generator, its host
    twin): a load outside an input would read poison, which the library's own
    validation refuses or which changes the result;
(c) the defined outputs are byte-identical under the poisons 0xA5 and 0x5A: no
    output depends on what its buffer held before the call (``hist`` is the
    documented exception: it is added to, so it is zeroed inside its view);
(d) the same bytes come back when every pointer has only its element type's
    natural alignment (256 k + itemsize).

"Defined" is everything of a replication with status FOGNET_OK (or
FOGNET_REF_ABORTED); of a failed replication it is the record, written in full
with the empty-set values the header states, while its per-task rows and its
per-node energy row are left out.  A failed replication sits in the middle of
its batch (mips[1, 0] = 0), so both neighbours must be intact.

The shapes are the smallest that still cross each edge (T = 1, 63, 65, 129,
191: below, at and past one and two 64-publish chunks; R = 1, 3, 5 for the
2- and 4-row v2 wavefronts; m = 63, 65, 257 for the decision blocks; R = 4,097
for the reduction's block edge)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import oracle_lib as ol
import tracegen as tg
from fognetsimpp_amd import _abi
from guarded import Arena
from test_parity_gpu import (V2_FIELDS, assert_parity, job_from_reps, v2_random, with_crashes)
from user_stats_ref import assert_user_parity

pytestmark = pytest.mark.gpu

I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
REP, V2, USER, JOB = _abi.REP_STATS_DTYPE, _abi.V2_STATS_DTYPE, _abi.USER_STATS_DTYPE, _abi.JOB_STATS_DTYPE
HIER_KW = dict(hier_threshold_s=0, hier_up_tick=10**12)  # test_hier_region_pass_and_handover's


def records(arena: Arena, n: int, dtype: np.dtype, misalign: bool, name: str) -> torch.Tensor:
    """A device buffer of n records as the uint8 tensor the wrappers take; the
    structs hold 8-B fields, so the view is carved as int64 (natural alignment 8)."""
    assert dtype.itemsize % 8 == 0
    return arena.alloc(n * dtype.itemsize // 8, torch.int64, misalign, name=name).view(torch.uint8)


def host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().copy()


# ---------------------------------------------------------------- cases

def B(id, R, N, T, seed=None, rho=0.9, **p):
    """A fognet_run_batch_dev case: tg.make_batch(seed, R, N, T, rho) plus the options in p."""
    return dict(id=id, kind="batch", R=R, N=N, T=T, seed=seed if seed is not None else 7000 + 13 * N + T, rho=rho, **p)


WIDE = {"FOGNET_REPLAY_KERNEL": "wide"}
INLOOP = {"FOGNET_REPLAY_STATS": "inloop"}
CASES = [
    # register kernel, full outputs
    B("reg-3x5x1", 3, 5, 1), B("reg-3x5x63", 3, 5, 63), B("reg-3x64x65", 3, 64, 65), B("reg-2x256x129", 2, 256, 129),
    B("reg-3x100x191", 3, 100, 191), B("reg-3x100x191-failed", 3, 100, 191, failed=True),
    B("inloop-3x64x65", 3, 64, 65, env=INLOOP), B("inloop-3x100x191", 3, 100, 191, env=INLOOP),
    B("inloop-3x100x191-failed", 3, 100, 191, env=INLOOP, failed=True),
    B("stages-3x64x65", 3, 64, 65, separate=True),
    # a replication refused in mid-trace (arrive[1, 2T/3] out of order): its record covers a prefix
    B("reg-3x100x191-unsorted", 3, 100, 191, failed="unsorted"),
    B("inloop-3x100x191-unsorted", 3, 100, 191, env=INLOOP, failed="unsorted"),
    B("wide-forced-3x5x65-unsorted", 3, 5, 65, env=WIDE, failed="unsorted"),
    B("statsonly-reg-3x64x65-unsorted", 3, 64, 65, per_task=False, failed="unsorted"),
    B("handover-3x4x191", 3, 4, 191, special="handover", ring=4),
    # wide kernel
    B("wide-forced-3x5x65", 3, 5, 65, env=WIDE), B("wide-forced-3x5x65-failed", 3, 5, 65, env=WIDE, failed=True),
    B("wide-2x257x191", 2, 257, 191), B("wide-big-2x300x191", 2, 300, 191, env={"FOGNET_WIDE_BIG": "1"}),
    B("wide-extlat-2x300x129", 2, 300, 129, policy="EXT_LAT"),
    B("wide-down-3x64x191", 3, 64, 191, special="down", power=False),
    # EXT_HIER.  At N = 2,500 the regions hold 1024, 1024 and 452 nodes; a regional broker escalates only once
    # every node of its region has advertised queued work, which 191 publishes cannot bring about (the oracle
    # finds no escalation at any load), so that shape covers the region pass alone.  N = 2,054 keeps three
    # regions, the third of 6 nodes: the middle replication escalates 6 publishes from publish 162 on, is
    # handed to the sequential kernel and resumed there (asserted from the oracle and hier_path_stats)
    B("hier-3x2500x191", 3, 2500, 191, special="hier", policy="EXT_HIER"),
    B("hier-escalating-3x2054x191", 3, 2054, 191, seed=73, rho=0.01, special="hier", policy="EXT_HIER",
      escalates=True),
    # statistics only
    B("statsonly-reg-3x64x65", 3, 64, 65, per_task=False), B("statsonly-wide-2x300x129", 2, 300, 129, per_task=False),
    B("statsonly-reg-3x64x65-failed", 3, 64, 65, per_task=False, failed=True),
    dict(id="generated-3x8x65", kind="generated", R=3, N=8, T=65, power=False),
    dict(id="generated-5x256x191-power", kind="generated", R=5, N=256, T=191, power=True),
    *[dict(id=f"v2-R{R}xN5{tag}", kind="v2", R=R, N=5, T=65, env=env)
      for env, tag in (({}, ""), ({"FOGNET_V2_ROW": "32"}, "-row32"), ({"FOGNET_V2_ACTIVE": "4"}, "-active4"))
      for R in (1, 3, 5)],
    dict(id="v2-R3xN70", kind="v2", R=3, N=70, T=65, env={}),
    dict(id="v2-R3xN5-failed", kind="v2", R=3, N=5, T=65, env={}, failed=True),  # stop_tick[1] past 2^53: refused
    dict(id="user-per-replication", kind="user", per_task=False, failed=False),
    dict(id="user-per-task", kind="user", per_task=True, failed=False),
    dict(id="user-per-task-failed", kind="user", per_task=True, failed=True),
    # refused at publish 65 of 130 (out of order), after its first decisions: its rows are undefined and unread
    dict(id="user-per-task-failed-mid", kind="user", per_task=True, failed="mid", T=130),
    *[dict(id=f"decide-v3-m{m}xn{n}", kind="decide3", m=m, n=n) for m in (1, 63, 65, 257) for n in (1, 65)],
    *[dict(id=f"decide-v2-m{m}xn{n}", kind="decide2", m=m, n=n) for m in (1, 63, 65, 257) for n in (1, 65)],
    dict(id="tracegen-3x5x65", kind="tracegen", R=3, N=5, T=65), dict(id="tracegen-2x65x191", kind="tracegen", R=2, N=65, T=191),
    dict(id="reduce-R1", kind="reduce", R=1), dict(id="reduce-R4097", kind="reduce", R=4097),
]
_cache: dict = {}


def _key(c, decoy):
    return c["id"] + ("/decoy" if decoy else "")


def batch_inputs(c, decoy=False):
    """Host trace, run_batch keywords and the oracle's result of a batch case (computed once).
    ``decoy``: a valid trace of the same shapes and kind from other seeds, without the oracle's
    result (None): what tests/stream_gate.py leaves in the input views until the gate opens."""
    if _key(c, decoy) in _cache:
        return _cache[_key(c, decoy)]
    R, N, T = c["R"], c["N"], c["T"]
    sp = c.get("special")
    ds = 100 if decoy else 0
    if sp == "handover":  # an overloaded replication among light ones, as test_ring_capacity_exceeded (at
        # rho = 0.01 the light ones keep at most 3 tasks pending: they stay on the register kernel)
        over, light = tg.make_batch(11 + ds, 1, N, T, rho=3.0), tg.make_batch(12 + ds, 2, N, T, rho=0.01)
        tr = {k: np.concatenate([light[k][:1], over[k], light[k][1:]]) for k in over}
    else:
        tr = tg.make_batch(c["seed"] + ds, R, N, T, rho=c["rho"])
    tr = {k: v.copy() for k, v in tr.items()}
    if c.get("power", True):
        tr["p_busy"], tr["p_idle"] = fa.power_model(tr["mips"])
    if c.get("failed") == "unsorted":
        i = 2 * T // 3
        tr["arrive"][1, i] = tr["arrive"][1, i - 1] - 1
    elif c.get("failed"):
        tr["mips"][1, 0] = 0
    if sp == "down":
        tr = with_crashes(tr, seed=N + ds)
    kw = dict(policy=c.get("policy", "REF_V3"), ring_capacity=c.get("ring", 0))
    okw = {}
    if sp == "hier":
        tr["region"] = fa.mobility_regions(tr["arrive"], N)
        kw.update(HIER_KW)
        okw = dict(region=tr["region"], **HIER_KW)
    o = None if decoy else ol.run_batch(
        tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=R, hist=True,
        policy=ol.POLICIES[kw["policy"]], p_busy=tr.get("p_busy"), p_idle=tr.get("p_idle"), down=tr.get("down"), **okw)
    _cache[_key(c, decoy)] = (tr, kw, o)
    return _cache[_key(c, decoy)]


def generated_inputs(c, decoy=False):
    """``decoy``: the parameters of the next replications (every row another load and latency
    scale) and another power model; the seed and r0, which are arguments, stay."""
    if _key(c, decoy) not in _cache:
        R, N, T, seed, r0 = c["R"], c["N"], c["T"], 0x5EED0004, 11
        mg, sc = fa.sweep_params(np.arange(r0, r0 + R) + (1 if decoy else 0), N)
        reps = [tg.make_replication(seed, r0 + r, N, T, lat_scale=int(sc[r]), mean_gap_ticks=float(mg[r]))
                for r in range(R)]
        tr = {k: np.stack([rp[k] for rp in reps]) for k in reps[0]}
        pb = pi = None
        if c["power"]:
            pb, pi = fa.power_model(tr["mips"] * 2 if decoy else tr["mips"])
        o = None if decoy else ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"],
                                            threads=R, hist=True, p_busy=pb, p_idle=pi)
        _cache[_key(c, decoy)] = (seed, r0, mg, sc, pb, pi, o)
    return _cache[_key(c, decoy)]


def user_inputs(c, decoy=False):
    if _key(c, decoy) not in _cache:
        R, N, T = 3, 64, c.get("T", 65)
        tr = {k: v.copy() for k, v in tg.make_batch(0x5EED0003 + (100 if decoy else 0), R, N, T, rho=0.9).items()}
        if c["failed"] == "mid":
            tr["arrive"][1, T // 2] = tr["arrive"][1, T // 2 - 1] - 1
        elif c["failed"]:
            tr["mips"][1, 0] = 0
        rng = np.random.default_rng(32 if decoy else 31)
        shape = (R, T) if c["per_task"] else (R,)
        uu = rng.integers(0, 5 * 10**9, shape).astype(np.int64)
        ud = rng.integers(0, 5 * 10**9, shape).astype(np.int64)
        o = None if decoy else ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"],
                                            threads=R, user_ul=uu, user_dl=ud)
        _cache[_key(c, decoy)] = (tr, uu, ud, o)
    return _cache[_key(c, decoy)]


def v2_inputs(c, decoy=False):
    if _key(c, decoy) not in _cache:
        tr, broker, stop, rt = v2_random(900 + 7 * c["R"] + c["N"] + (5000 if decoy else 0), c["R"], c["N"], c["T"])
        o = None
        if not decoy:
            o = ol.run_v2(tr["arrive"], tr["req"], broker, tr["mips"], tr["dl"], tr["ul"], tr["first_adv"], stop, rt,
                          threads=c["R"])
            assert (o["stats"]["status"] == 0).all()
        stop = stop.astype(np.int64)
        if c.get("failed"):
            stop[1] = 2**53 + 1  # (the oracle's rows 0 and 2 are the reference; row 1 is refused)
        _cache[_key(c, decoy)] = (tr, broker.astype(np.int32), stop, rt.astype(np.float64), o)
    return _cache[_key(c, decoy)]


def decide_inputs(c, decoy=False):
    if _key(c, decoy) not in _cache:
        m, n = c["m"], c["n"]
        rng = np.random.default_rng(1000 * m + n + (500000 if decoy else 0))
        if c["kind"] == "decide3":  # as test_decide_batch_matches_oracle
            busy = rng.integers(0, 6, size=(m, n)).astype(np.float64) + rng.choice([0.0, 0.5, 1e-16], size=(m, n))
            busy[rng.random((m, n)) < 0.01] = np.nan
            mips = rng.integers(1, 3000, size=(m, n)).astype(np.int32)
            mips[rng.random(m) < 0.05, 0] = 0
            req = rng.integers(-5000, 70000, size=m).astype(np.int32)
            want = None if decoy else [ol.decide_v3(busy[q], mips[q], int(req[q])) for q in range(m)]
            _cache[_key(c, decoy)] = (busy, mips, req, want)
        else:  # as test_decide_v2_batch_matches_oracle
            mips = rng.choice([0, 500, 999, 1000, 1001, 2000, 4000], size=(m, n)).astype(np.int32)
            local = rng.integers(-100, 3000, size=m).astype(np.int32)
            req = rng.integers(0, 4500, size=m).astype(np.int32)
            want = None if decoy else [ol.decide_v2(mips[q], local[q], req[q]) for q in range(m)]
            _cache[_key(c, decoy)] = (mips, local, req, want)
    return _cache[_key(c, decoy)]


TRACE_KEYS = ("arrive", "req", "mips", "dl", "ul", "init")


def reduce_inputs(ctx, c, decoy=False):
    """R records of generated replays (N = 8, T = 8), made once on plain tensors."""
    if _key(c, decoy) not in _cache:
        R = c["R"]
        mg, sc = fa.sweep_params(np.arange(R), 8)
        out = fa.run_generated(ctx, 8 if decoy else 7, R, 8, 8, mg, sc, hist=False)
        torch.cuda.synchronize()
        _cache[_key(c, decoy)] = host(out.stats).view(np.int64)
    return _cache[_key(c, decoy)]


def tracegen_params(c, decoy=False):
    mg, sc = fa.sweep_params(np.arange(7, 7 + c["R"]) + (1 if decoy else 0), c["N"])
    return mg, sc


def input_arrays(ctx, case: dict, decoy=False) -> dict:
    """Every array a case's calls read, by the name of its view in the input arena (in the
    order the views are carved)."""
    kind = case["kind"]
    if kind == "batch":
        return dict(batch_inputs(case, decoy)[0])
    if kind == "generated":
        _, _, mg, sc, pb, pi, _ = generated_inputs(case, decoy)
        power = dict(p_busy=pb, p_idle=pi) if pb is not None else {}
        return dict(power, mean_gap_ticks=mg.astype(np.float64), lat_scale=sc.astype(np.int64))
    if kind == "v2":
        tr, broker, stop, rt, _ = v2_inputs(case, decoy)
        return dict(tr, broker_mips=broker, stop_tick=stop, required_time_s=rt)
    if kind == "user":
        tr, uu, ud, _ = user_inputs(case, decoy)
        return dict(tr, user_ul=uu, user_dl=ud)
    if kind == "decide3":
        busy, mips, req, _ = decide_inputs(case, decoy)
        return dict(adv_busy=busy, adv_mips=mips, req=req)
    if kind == "decide2":
        mips, local, req, _ = decide_inputs(case, decoy)
        return dict(adv_mips=mips, local_mips=local, req=req)
    if kind == "tracegen":
        mg, sc = tracegen_params(case, decoy)
        return dict(mean_gap_ticks=mg.astype(np.float64), lat_scale=sc.astype(np.int64))
    if kind == "reduce":
        return dict(stats=reduce_inputs(ctx, case, decoy))
    raise AssertionError(kind)


# ---------------------------------------------------------------- the harness

def blank_undefined(g: dict, failed: np.ndarray) -> dict:
    """Zero what the contract leaves undefined: the per-task rows and the
    per-node energy row of a failed replication."""
    for k in ("node", "status", "start", "done", "energy"):
        if g.get(k) is not None:
            g[k][failed] = 0
    return g


def is_failed(stats: np.ndarray) -> np.ndarray:
    return ~np.isin(stats["status"], (_abi.FOGNET_OK, _abi.FOGNET_REF_ABORTED))


class Job:
    """One case's buffers: every input and every output a view into a poisoned arena (inputs
    in one, outputs in another).  ``inputs``: the input views by name (``arrays``: of these
    host arrays instead of input_arrays(ctx, case))."""

    def __init__(self, ctx, case: dict, poison: int, misalign: bool, arrays: dict | None = None):
        dev = torch.device("cuda", ctx.device)
        self.case, self.misalign = case, misalign
        self.ain, self.aout = Arena(dev, poison), Arena(dev, poison)
        arrays = arrays if arrays is not None else input_arrays(ctx, case)
        self.inputs = {k: self.ain.put(a, misalign, name=k) for k, a in arrays.items()}
        self.out = None
        self.hier_before = self.hier_after = None

    @property
    def arenas(self):
        return self.ain, self.aout

    def new(self, shape, dt, name):
        return self.aout.alloc(shape, dt, self.misalign, name=name)

    def records(self, n, dtype, name):
        return records(self.aout, n, dtype, self.misalign, name)


def build_guarded(ctx, case: dict, poison: int, misalign: bool) -> Job:
    """Carve and fill a case's views (on the current stream; nothing of the library runs)."""
    j = Job(ctx, case, poison, misalign)
    kind = case["kind"]
    new = j.new
    if kind == "batch":
        tr = batch_inputs(case)[0]
        R, N, T = case["R"], case["N"], case["T"]
        per_task = case.get("per_task", True)
        j.out = fa.BatchResult(
            node=new((R, T), torch.int32, "node") if per_task else None,
            status=new((R, T), torch.uint8, "status") if per_task else None,
            start_tick=new((R, T), torch.int64, "start_tick") if per_task else None,
            done_tick=new((R, T), torch.int64, "done_tick") if per_task else None,
            stats=j.records(R, REP, "stats"),
            node_energy=new((R, N), torch.float64, "node_energy") if "p_busy" in tr else None,
            hist=new((_abi.HIST_METRICS, _abi.HIST_BINS), torch.int64, "hist"))
        j.out.hist.zero_()  # added to: the one output the caller initialises (its bands stay poisoned)
    elif kind == "generated":
        R, N, T = case["R"], case["N"], case["T"]
        j.power = (j.inputs["p_busy"], j.inputs["p_idle"]) if "p_busy" in j.inputs else None
        j.out = fa.BatchResult(None, None, None, None, stats=j.records(R, REP, "stats"),
                               node_energy=new((R, N), torch.float64, "node_energy") if j.power else None,
                               hist=new((_abi.HIST_METRICS, _abi.HIST_BINS), torch.int64, "hist"))
        j.out.hist.zero_()
    elif kind == "v2":
        R, T = case["R"], case["T"]
        j.out = fa.V2Result(new((R, T), torch.int32, "node"), new((R, T), torch.uint8, "status"),
                            new((R, T), torch.int64, "start_tick"), new((R, T), torch.int64, "done_tick"),
                            j.records(R, V2, "stats"))
    elif kind == "user":
        R, T = j.inputs["arrive"].shape
        j.out = fa.BatchResult(new((R, T), torch.int32, "node"), new((R, T), torch.uint8, "status"),
                               new((R, T), torch.int64, "start_tick"), new((R, T), torch.int64, "done_tick"),
                               stats=j.records(R, REP, "stats"))
        j.res = j.records(R, USER, "user_stats")
    elif kind == "decide3":
        j.out = (new(case["m"], torch.int32, "node"), new(case["m"], torch.int32, "status"))
    elif kind == "decide2":
        j.out = (new(case["m"], torch.int32, "action"), new(case["m"], torch.int32, "node"))
    elif kind == "tracegen":
        R, N, T = case["R"], case["N"], case["T"]
        dts = dict(arrive=torch.int64, req=torch.int32, mips=torch.int32, dl=torch.int64, ul=torch.int64,
                   init=torch.int64)  # fa.allocate_trace's layout
        j.out = {k: new((R, T) if k in ("arrive", "req") else (R, N), dts[k], k) for k in TRACE_KEYS}
    elif kind == "reduce":
        j.job_buf = j.records(1, JOB, "job")
    else:
        raise AssertionError(kind)
    return j


def enqueue_user_stats(ctx, d: dict, out, user_ul, user_dl, res):
    """fognet_user_stats_dev with the caller's buffers and nothing else (fa.user_stats, which
    reads the records back, waits for them)."""
    R, T = d["arrive"].shape
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    bi = _abi.BatchIn(R, T, d["mips"].shape[-1], out.policy, d["mips"].shape[-1] if d["mips"].dim() == 2 else 0, 0,
                      p(d["arrive"]), p(d["req"]), p(d["mips"]), p(d["dl"]), p(d["ul"]), p(d["init"]),
                      None, None, None, None, 0)
    bo = _abi.BatchOut(p(out.node), p(out.status), p(out.start_tick), p(out.done_tick), p(out.stats), None, None, None)
    s = C.c_void_p(torch.cuda.current_stream(res.device).cuda_stream)
    ctx.check(ctx._lib.fognet_user_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), p(user_ul), p(user_dl),
                                             1 if user_ul.dim() == 2 else 0, p(res), s), "user_stats")


def call_guarded(ctx, j: Job, enqueue_only: bool = False):
    """The case's library calls on the current stream.  ``enqueue_only``: where a wrapper ends by
    reading its result back (fa.user_stats, fa.reduce_stats), the entry point itself is called
    with the same buffers, so that nothing here waits for the device."""
    case, d, out = j.case, j.inputs, j.out
    kind = case["kind"]
    if kind == "batch":
        kw = batch_inputs(case)[1]
        j.hier_before = ctx.hier_path_stats()
        if case.get("separate"):
            fa.run_batch(ctx, d, out=out, stage="replay", **kw)
            fa.run_batch(ctx, d, out=out, stage="stats", **kw)
        else:
            fa.run_batch(ctx, d, out=out, **kw)
        j.hier_after = ctx.hier_path_stats()
    elif kind == "generated":
        seed, r0 = generated_inputs(case)[:2]
        fa.run_generated(ctx, seed, case["R"], case["T"], case["N"], d["mean_gap_ticks"], d["lat_scale"], r0=r0,
                         out=out, power=j.power)
    elif kind == "v2":
        fa.run_v2(ctx, d, d["broker_mips"], d["stop_tick"], d["required_time_s"], queue_capacity=4096, out=out)
    elif kind == "user":
        fa.run_batch(ctx, d, out=out)
        if enqueue_only:
            enqueue_user_stats(ctx, d, out, d["user_ul"], d["user_dl"], j.res)
        else:
            j.user = fa.user_stats(ctx, d, out, d["user_ul"], d["user_dl"], res=j.res)
    elif kind == "decide3":
        fa.BrokerBaseApp3(ctx).sendPubAck_batch(d["adv_busy"], d["adv_mips"], d["req"], out=out)
    elif kind == "decide2":
        fa.BrokerBaseApp2(ctx).sendPubAck_batch(d["adv_mips"], d["local_mips"], d["req"], out=out)
    elif kind == "tracegen":
        fa.generate_trace(ctx, 0x5EED0003, case["R"], case["T"], case["N"], d["mean_gap_ticks"], d["lat_scale"],
                          r0=7, out=out)
    elif kind == "reduce":
        stats = d["stats"].view(torch.uint8)
        if enqueue_only:
            s = C.c_void_p(torch.cuda.current_stream(stats.device).cuda_stream)
            ctx.check(ctx._lib.fognet_reduce_stats_dev(ctx.handle, C.c_void_p(stats.data_ptr()), case["R"],
                                                       C.c_void_p(j.job_buf.data_ptr()), s), "reduce_stats")
        else:
            j.job = fa.reduce_stats(ctx, stats, case["R"], out=j.job_buf)
    else:
        raise AssertionError(kind)


def collect_guarded(ctx, j: Job) -> dict:
    """The defined outputs as host arrays, once the calls have finished."""
    case, out = j.case, j.out
    kind = case["kind"]
    if kind == "batch":
        g = dict(stats=host(out.stats).view(REP), hist=host(out.hist),
                 energy=host(out.node_energy) if out.node_energy is not None else None,
                 hier_launches=(j.hier_after[0] - j.hier_before[0], j.hier_after[1] - j.hier_before[1]))
        if case.get("per_task", True):
            g.update(node=host(out.node), status=host(out.status), start=host(out.start_tick), done=host(out.done_tick))
        blank_undefined(g, is_failed(g["stats"]))
    elif kind == "generated":
        g = dict(stats=host(out.stats).view(REP), hist=host(out.hist),
                 energy=host(out.node_energy) if j.power else None)
    elif kind == "v2":
        g = dict(node=host(out.node), status=host(out.status), start=host(out.start_tick), done=host(out.done_tick),
                 stats=host(out.stats).view(V2))
        blank_undefined(g, g["stats"]["status"] != _abi.FOGNET_OK)
    elif kind == "user":
        user = getattr(j, "user", None)
        g = dict(user=user.copy() if user is not None else host(j.res).view(USER), user_bytes=host(j.res),
                 stats=host(out.stats).view(REP))
    elif kind == "decide3":
        g = dict(node=host(out[0]), status=host(out[1]))
    elif kind == "decide2":
        g = dict(action=host(out[0]), node=host(out[1]))
    elif kind == "tracegen":
        g = {k: host(out[k]) for k in TRACE_KEYS}
        g["params"] = tracegen_params(case)
    elif kind == "reduce":
        job = getattr(j, "job", None)
        g = dict(job=job.copy() if job is not None else host(j.job_buf).view(JOB)[0], job_bytes=host(j.job_buf),
                 reps=reduce_inputs(ctx, case).view(REP))
    else:
        raise AssertionError(kind)
    return g


def run_guarded(ctx, case: dict, poison: int, misalign: bool):
    """Run one case with every input and every output carved from poisoned
    arenas (inputs in one, outputs in another) on the session context; returns
    the defined outputs as host arrays and the arenas."""
    j = build_guarded(ctx, case, poison, misalign)
    call_guarded(ctx, j)
    torch.cuda.synchronize()
    return collect_guarded(ctx, j), j.arenas


# ---------------------------------------------------------------- (b): the oracle

ZERO_FIELDS = ("n_queued", "n_started", "queue_sum_lo", "queue_sum_hi", "queue_sq_lo", "queue_sq_hi", "queue_sq_top",
               "resp_sum_lo", "resp_sum_hi", "resp_sq_lo", "resp_sq_hi", "busy_s", "n_qtime", "n_qtime_overflow")


def assert_failed_record(rec, what):
    """The record of a replication refused before its first decision, as the
    header's "Buffers" paragraph states it: written in full, the fields the
    replay does not define at their empty-set values."""
    assert int(rec["status"]) == _abi.FOGNET_ERR_ARG and int(rec["n_tasks"]) == 0, what
    for f in ZERO_FIELDS:
        assert int(rec[f]) == 0, (what, f, int(rec[f]))
    assert float(rec["energy_j"]) == 0.0 and not np.signbit(rec["energy_j"]), what
    for f in ("queue_min_raw", "resp_min_ticks", "abort_tick"):
        assert int(rec[f]) == I64_MAX, (what, f, int(rec[f]))
    for f in ("queue_max_raw", "resp_max_ticks", "last_tick"):
        assert int(rec[f]) == I64_MIN, (what, f, int(rec[f]))
    assert int(rec["abort_task"]) == -1, what


def check_against_oracle(ctx, case, g):
    kind = case["kind"]
    if kind in ("batch", "generated"):
        o = batch_inputs(case)[2] if kind == "batch" else generated_inputs(case)[-1]
        failed = is_failed(g["stats"])
        assert list(failed) == ([False, True, False] if case.get("failed") else [False] * case["R"])
        ok = ~failed
        if "node" in g:
            ref = blank_undefined({k: o[k].copy() for k in ("node", "status", "start", "done")}, failed)
            assert_parity(None, {**g, "stats": g["stats"][ok]}, {**ref, "stats": o["stats"][ok]})
        assert g["stats"][ok].tobytes() == o["stats"][ok].tobytes()
        if case.get("failed") == "unsorted":
            # refused in mid-trace: status and a prefix length; that the rest of the record, and what the prefix
            # added to the histogram, do not depend on the buffers is (c)'s to show
            rec = g["stats"][1]
            assert int(rec["status"]) == _abi.FOGNET_ERR_ARG and 0 <= int(rec["n_tasks"]) <= 2 * case["T"] // 3
            assert (g["hist"] >= o["hist"][ok].sum(axis=0)).all()
            assert int(g["hist"][1].sum()) - int(o["hist"][ok][:, 1].sum()) == int(rec["n_tasks"])
        else:
            for r in np.flatnonzero(failed):
                assert_failed_record(g["stats"][r], f"replication {r}")
            np.testing.assert_array_equal(g["hist"], o["hist"][ok].sum(axis=0))
        if g["energy"] is not None:
            np.testing.assert_array_equal(g["energy"][ok], o["node_energy"][ok])
        if case.get("special") == "handover":
            mp = g["stats"]["max_pending"]
            assert mp[1] > case["ring"] and mp[0] <= case["ring"] and mp[2] <= case["ring"]  # one hand-over
        if case.get("special") == "down":
            assert ((o["status"] == 9) | (o["done"] == -1)).any()  # the crashes bite
        if case.get("special") == "hier":
            tr = batch_inputs(case)[0]
            esc = (o["node"] // _abi.HIER_REGION_NODES != tr["region"]).sum(axis=1)
            assert len(np.unique(tr["region"])) == 3 and g["hier_launches"] == (1, 0)  # the region pass ran
            # (every status is OK: an escalated replication was handed over, resumed and finished)
            assert list(esc > 0) == ([False, True, False] if case.get("escalates") else [False] * 3), esc
            if case.get("escalates"):
                first = int((o["node"][1] // _abi.HIER_REGION_NODES != tr["region"][1]).argmax())
                assert first >= 128  # resumed in the trace's last chunk, not at its start
    elif kind == "v2":
        o = v2_inputs(case)[-1]
        failed = g["stats"]["status"] != _abi.FOGNET_OK
        assert list(failed) == ([False, True, False] if case.get("failed") else [False] * case["R"])
        ref = blank_undefined({k: o[k].copy() for k in ("node", "status", "start", "done")}, failed)
        for k in ("node", "status", "start", "done"):
            np.testing.assert_array_equal(g[k], ref[k], err_msg=k)
        for f in V2_FIELDS:
            np.testing.assert_array_equal(g["stats"][f][~failed], o["stats"][f][~failed], err_msg=f)
        for r in np.flatnonzero(failed):  # refused before its first event: every count 0
            rec = g["stats"][r]
            assert int(rec["status"]) == _abi.FOGNET_ERR_ARG
            for f in V2_FIELDS[:11]:  # (the n_* counts)
                assert int(rec[f]) == 0, (r, f, int(rec[f]))
    elif kind == "user":
        o = user_inputs(case)[-1]
        failed = is_failed(g["stats"])
        assert list(failed) == [False, bool(case["failed"]), False]
        assert_user_parity(g["user"][~failed], o["user"][~failed])
        if case["failed"] == "mid":  # it had decided publishes when it was refused
            assert 0 < int(g["stats"]["n_tasks"][1]) <= case["T"] // 2
        for r in np.flatnonzero(failed):  # an empty record: fognet_moments' count == 0 values
            for n in ol.USER_SIGNALS:
                m = g["user"][r][n]
                assert (int(m["count"]), int(m["min_raw"]), int(m["max_raw"])) == (0, I64_MAX, I64_MIN), (r, n)
                assert all(int(m[f]) == 0 for f in ("sum_lo", "sum_hi", "sq_lo", "sq_hi", "sq_top", "overflow")), (r, n)
    elif kind == "decide3":
        want = decide_inputs(case)[-1]
        for q, (rc, k) in enumerate(want):
            assert g["status"][q] == rc, q
            if rc == 0:
                assert g["node"][q] == k, q
    elif kind == "decide2":
        want = decide_inputs(case)[-1]
        assert list(zip(g["action"].tolist(), g["node"].tolist())) == want
    elif kind == "tracegen":
        mg, sc = g["params"]
        for r in range(case["R"]):
            h = tg.make_replication(0x5EED0003, 7 + r, case["N"], case["T"], lat_scale=int(sc[r]),
                                    mean_gap_ticks=float(mg[r]))
            for k in TRACE_KEYS:
                np.testing.assert_array_equal(g[k][r], h[k], err_msg=f"{k} r={r}")
    elif kind == "reduce":
        job, st = g["job"], g["reps"]
        ref = job_from_reps(st)
        u192 = lambda a: int(a[0]) | (int(a[1]) << 64) | (int(a[2]) << 128)
        assert int(job["n_reps"]) == case["R"] and int(job["n_failed"]) == 0 == ref["n_failed"]
        assert int(job["n_tasks"]) == ref["n_tasks"] == case["R"] * 8 and int(job["n_queued"]) == ref["n_queued"]
        assert u192(job["queue_sum"]) == ref["queue_sum"] and u192(job["queue_sq"]) == ref["queue_sq"]
        assert u192(job["resp_sq"]) == ref["resp_sq"]
        assert int(job["resp_max_ticks"]) == ref["resp_max"] and int(job["max_pending"]) == ref["max_pending"]
        assert int(job["n_qtime"]) == int(st["n_qtime"].sum())
        host_job = fa.job_from_reps(st)  # the library's host twin: every integer field
        for f in JOB.names:
            if f != "energy_j":
                np.testing.assert_array_equal(job[f], host_job[f], err_msg=f)


def same_bytes(a: dict, b: dict, what: str):
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == b[k].tobytes(), f"{what}: {k} differs"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_buffer_contract(ctx, monkeypatch, case):
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    runs = {}
    for poison, misalign in ((0xA5, False), (0x5A, False), (0xA5, True)):
        g, arenas = run_guarded(ctx, case, poison, misalign)
        what = f"poison 0x{poison:02X}, misalign={misalign}"
        for a, name in zip(arenas, ("inputs", "outputs")):
            msg = a.damage()  # (a)
            assert msg is None, f"{what}, {name} arena: {msg}"
        check_against_oracle(ctx, case, g)  # (b)
        runs[(poison, misalign)] = g
    same_bytes(runs[(0xA5, False)], runs[(0x5A, False)], "(c) poison 0xA5 against 0x5A")
    same_bytes(runs[(0xA5, False)], runs[(0xA5, True)], "(d) aligned against naturally aligned")


# ---------------------------------------------------------------- a dirty workspace

def test_dirty_workspace(monkeypatch):
    """One context's workspace is never smaller than its largest past job, so each
    smaller job runs over the rings, chains, views, work lists and progress board
    the larger ones left behind: five jobs from the largest down, then the list
    backwards, each equal to the oracle."""
    over, light = tg.make_batch(11, 3, 256, 2000, rho=3.0), tg.make_batch(12, 5, 256, 2000, rho=0.3)
    big = {k: np.concatenate([light[k][:2], over[k], light[k][2:]]) for k in over}
    o_big = ol.run_batch(big["arrive"], big["req"], big["mips"], big["dl"], big["ul"], big["init"], threads=8, hist=True)
    by_id = {c["id"]: c for c in CASES}
    jobs = [("handover-8x256x2000", big, dict(ring_capacity=4), o_big, {})]
    for cid in ("hier-escalating-3x2054x191", "wide-big-2x300x191", "wide-2x257x191", "reg-3x5x65"):
        c = by_id.get(cid) or B(cid, 3, 5, 65)
        tr, kw, o = batch_inputs(c)
        jobs.append((cid, tr, kw, o, c.get("env", {})))
    c = fa.Context(0)
    try:
        dev = torch.device("cuda", c.device)
        for cid, tr, kw, o, env in jobs + jobs[::-1]:
            with monkeypatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                out = fa.run_batch(c, fa.as_device_trace(tr, dev), hist=True, **kw)
                torch.cuda.synchronize()
            g = dict(node=host(out.node), status=host(out.status), start=host(out.start_tick),
                     done=host(out.done_tick), stats=out.rep_stats())
            assert (g["stats"]["status"] == 0).all(), cid
            assert_parity(tr, g, o)
            assert g["stats"].tobytes() == o["stats"].tobytes(), cid
            np.testing.assert_array_equal(host(out.hist), o["hist"].sum(axis=0), err_msg=cid)
            if out.node_energy is not None:
                np.testing.assert_array_equal(host(out.node_energy), o["node_energy"], err_msg=cid)
            if cid.startswith("handover"):
                assert g["stats"]["max_pending"].max() > 4
    finally:
        c.close()
