"""What engine.py hands the library, per public function: which fields of fognet_batch_in / fognet_batch_out
are non-null, that each pointer is the right tensor's, and the scalar fields.  No device: the public functions run
on CPU tensors (the marshalling reads shapes and data_ptr() only) against a context that records the descriptors
instead of launching, so the table below cannot drift from what the functions really pass."""
import ctypes as C

import pytest
import torch

from fognetsimpp_amd import _abi, engine
from fognetsimpp_amd._abi import FognetError

R, T, N, U = 2, 3, 2, 2
REF, HIER = _abi.FOGNET_POLICY_REF_V3, _abi.FOGNET_POLICY_EXT_HIER
TRACE_IN = {"arrive_tick": "arrive", "req_mips": "req", "mips": "mips", "dl_tick": "dl", "ul_tick": "ul",
            "init_adv_tick": "init"}
POWER = {"p_busy_w": "p_busy", "p_idle_w": "p_idle"}
DOWN, REGION = {"down_tick": "down"}, {"region": "region"}
PER_TASK = {"node": "node", "status": "status", "start_tick": "start_tick", "done_tick": "done_tick", "stats": "stats"}
ENERGY_HIST, ESC = {"node_energy_j": "node_energy", "hist": "hist"}, {"escalated": "escalated"}


class RecordingLib:
    """Every fognet_* entry point records its arguments and returns FOGNET_OK."""

    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        return lambda *args: self._calls.append((name, args)) or _abi.FOGNET_OK


class Recorder:
    """Stands in for a Context."""

    def __init__(self):
        self.handle, self.calls = None, []
        self._lib = RecordingLib(self.calls)

    def check(self, rc, what=""):
        assert rc == 0

    def last(self):
        """(entry point, fognet_batch_in, fognet_batch_out) of the last call."""
        name, args = self.calls[-1]
        structs = [a._obj for a in args if hasattr(a, "_obj")]
        return (name, next(s for s in structs if isinstance(s, _abi.BatchIn)),
                next(s for s in structs if isinstance(s, _abi.BatchOut)))


@pytest.fixture()
def rec(monkeypatch):
    monkeypatch.setattr(engine, "_stream_ptr", lambda device, stream=None: C.c_void_p(0))
    return Recorder()


@pytest.fixture(scope="module")
def trace():
    """Per-replication node parameters, and every optional array at once."""
    i64 = lambda *shape: torch.ones(shape, dtype=torch.int64)  # noqa: E731
    return {"arrive": i64(R, T), "req": torch.ones((R, T), dtype=torch.int32), "mips": torch.ones((R, N), dtype=torch.int32),
            "dl": i64(R, N), "ul": i64(R, N), "init": i64(R, N), "down": i64(R, N),
            "p_busy": torch.ones((R, N), dtype=torch.float64), "p_idle": torch.ones((R, N), dtype=torch.float64),
            "region": torch.zeros((R, T), dtype=torch.int32)}


@pytest.fixture()
def out():
    """A BatchResult that carries every output array."""
    return engine.allocate_outputs(R, T, "cpu", N=N, energy=True, hist=True, escalated=True)


def check(desc, src, want_ptrs, **scalars):
    """Exactly the fields of `want_ptrs` (field -> key of `src`) are set, each to that tensor; scalars as given."""
    get = (lambda k: src[k]) if isinstance(src, dict) else (lambda k: getattr(src, k))
    ptrs = {f: getattr(desc, f) for f, ty in desc._fields_ if ty is C.c_void_p}
    assert {f for f, p in ptrs.items() if p} == set(want_ptrs)
    for f, k in want_ptrs.items():
        assert ptrs[f] == get(k).data_ptr(), f
    for f, v in scalars.items():
        assert getattr(desc, f) == v, f


def links(*shape):
    return torch.ones(shape, dtype=torch.int64)


USER_OF = torch.zeros((R, T), dtype=torch.int32)


@pytest.mark.parametrize("policy,ref_abort", [("EXT_HIER", True), ("REF_V3", False)])
def test_run_batch_forwards_everything(rec, trace, out, policy, ref_abort):
    engine.run_batch(rec, trace, out, ring_capacity=8, policy=policy, hier_threshold_s=9, hier_up_tick=7,
                     ref_abort=ref_abort)
    name, bi, bo = rec.last()
    assert name == "fognet_run_batch_dev"
    check(bi, trace, {**TRACE_IN, **POWER, **DOWN, **REGION}, R=R, T=T, N=N, policy=engine.POLICIES[policy],
          node_stride=N, ring_capacity=8, hier_up_tick=7, hier_threshold_s=9,
          flags=_abi.FLAG_REF_ABORT if ref_abort else 0)
    check(bo, out, {**PER_TASK, **ENERGY_HIST, **ESC})


def test_run_assigned(rec, trace, out):
    engine.run_assigned(rec, trace, torch.zeros((R, T), dtype=torch.int32), out)
    name, bi, bo = rec.last()
    assert name == "fognet_run_assigned_dev"
    check(bi, trace, {**TRACE_IN, **POWER, **DOWN}, R=R, T=T, N=N, policy=REF, node_stride=N, ring_capacity=0,
          hier_up_tick=0, hier_threshold_s=0, flags=0)
    check(bo, out, {**PER_TASK, **ENERGY_HIST, **ESC})


def run_pass(fn, rec, trace, out, policy):
    if fn == "user_stats":
        engine.user_stats(rec, trace, out, links(R), links(R), policy=policy, hier_up_tick=5)
    elif fn == "per_user_stats":
        engine.per_user_stats(rec, trace, out, USER_OF, links(U), links(U), policy=policy, hier_up_tick=5,
                              allow_unassigned=True)
    else:
        engine.node_stats(rec, trace, out, policy=policy, hier_up_tick=5)
    return rec.last()


@pytest.mark.parametrize("fn", ["user_stats", "per_user_stats", "node_stats"])
def test_passes(rec, trace, out, fn):
    """No power model, no energy, no histogram; crash ticks for node_stats alone; region, the escalation flags and
    the hop only under EXT_HIER."""
    down = DOWN if fn == "node_stats" else {}
    name, bi, bo = run_pass(fn, rec, trace, out, "REF_V3")
    assert name == f"fognet_{fn}_dev"
    check(bi, trace, {**TRACE_IN, **down}, R=R, T=T, N=N, policy=REF, node_stride=N, ring_capacity=0,
          hier_up_tick=0, hier_threshold_s=0, flags=0)
    check(bo, out, PER_TASK)
    _, bi, bo = run_pass(fn, rec, trace, out, "EXT_HIER")
    check(bi, trace, {**TRACE_IN, **down, **REGION}, policy=HIER, hier_up_tick=5, hier_threshold_s=0, flags=0)
    check(bo, out, {**PER_TASK, **ESC})


def test_pass_hop_defaults_to_the_replays(rec, trace, out):
    out.policy, out.hier_up_tick = HIER, 11
    engine.user_stats(rec, trace, out, links(R), links(R))
    assert rec.last()[1].policy == HIER and rec.last()[1].hier_up_tick == 11


@pytest.mark.parametrize("policy", ["REF_V3", "EXT_HIER"])
def test_signal_vectors(rec, trace, out, policy):
    engine.signal_vectors(rec, trace, out, USER_OF, links(U), links(U), policy=policy, to_host=False)
    name, bi, bo = rec.last()
    assert name == "fognet_signal_vectors_dev"
    check(bi, trace, {**TRACE_IN, **(REGION if policy == "EXT_HIER" else {})}, R=R, T=T, N=N,
          policy=engine.POLICIES[policy], node_stride=N, ring_capacity=0, hier_up_tick=0, hier_threshold_s=0, flags=0)
    check(bo, out, PER_TASK)


@pytest.mark.parametrize("policy", ["REF_V3", "EXT_HIER"])
def test_run_generated(rec, trace, out, policy):
    hier = policy == "EXT_HIER"
    engine.run_generated(rec, 1, R, T, N, [1.0] * R, [1] * R, out=out, ring_capacity=4, policy=policy,
                         power=(trace["p_busy"], trace["p_idle"]), device="cpu", hier_threshold_s=9, hier_up_tick=7)
    name, bi, bo = rec.last()
    assert name == "fognet_run_generated_dev"
    check(bi, trace, POWER, R=R, T=T, N=N, policy=engine.POLICIES[policy], node_stride=N, ring_capacity=4,
          hier_up_tick=7 if hier else 0, hier_threshold_s=9 if hier else 0, flags=0)
    check(bo, out, {"stats": "stats", **ENERGY_HIST})


def test_node_stride(trace):
    assert engine._dims(trace) == (R, T, N, N)
    shared = {**trace, "mips": trace["mips"][0]}
    assert engine._dims(shared) == (R, T, N, 0)


@pytest.mark.parametrize("fn", [engine.run_batch, lambda c, t: engine.run_assigned(c, t, USER_OF)])
def test_shape_errors(rec, trace, fn):
    with pytest.raises(FognetError) as e:
        fn(rec, {**trace, "dl": links(N)})
    assert e.value.code == _abi.FOGNET_ERR_ARG and str(e.value).endswith(f"dl has shape ({N},), mips ({R}, {N})")
    with pytest.raises(FognetError) as e:
        fn(rec, {**trace, "req": torch.ones((R, T + 1), dtype=torch.int32)})
    assert e.value.code == _abi.FOGNET_ERR_ARG and str(e.value).endswith("trace arrays disagree on R/T")
    assert not rec.calls


def test_policy_of(out):
    assert out.policy is None and engine._policy_of(out, None) == REF
    out.policy = _abi.FOGNET_POLICY_EXT_LAT
    assert engine._policy_of(out, None) == _abi.FOGNET_POLICY_EXT_LAT
    assert engine._policy_of(out, "EXT_HIER") == HIER and engine._policy_of(out, 0) == 0


def test_user_tables():
    uo, uu, ud, u, stride = engine._user_tables(USER_OF, [1] * U, [2] * U, R, T, "cpu")
    assert (uo.dtype, uu.dtype, tuple(uu.shape), u, stride) == (torch.int32, torch.int64, (U,), U, 0)
    assert engine._user_tables(USER_OF, links(R, U), links(R, U), R, T, "cpu")[3:] == (U, U)
    with pytest.raises(FognetError) as e:
        engine._user_tables(USER_OF[:, :2], links(U), links(U), R, T, "cpu")
    assert e.value.code == _abi.FOGNET_ERR_ARG and "user_of must have shape [R, T], got (2, 2)" in str(e.value)
    with pytest.raises(FognetError) as e:
        engine._user_tables(USER_OF, links(U), links(R, U), R, T, "cpu")
    assert e.value.code == _abi.FOGNET_ERR_ARG
    assert "user links must both have shape [U] or [R, U], got (2,) / (2, 2)" in str(e.value)
