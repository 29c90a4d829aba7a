"""Host-side mirror of FogNetSim++'s offload-decision interface over libfognet_hip.

Device memory, streams and (for multi-GPU) RCCL come from PyTorch; every
decision, node update and statistic is computed by the gfx950 kernels in
``csrc/``.  Names follow the reference:

* :class:`BrokerBaseApp3` — the broker's allocation policy plug-in
  (``simple BrokerBaseApp3 like IUDPApp``, src/mqttapp/BrokerBaseApp3.ned:20);
  :meth:`BrokerBaseApp3.sendPubAck` is the decision core of
  ``BrokerBaseApp3::sendPubAck(..., status=false)`` (BrokerBaseApp3.cc:265-281).
* :class:`BrokerBaseApp2` — the v2 broker's local-first / "max-MIPS" forward
  (BrokerBaseApp2.cc:180-192, 235-286).
* :func:`run_v2` — replays of the v2 model (BrokerBaseApp2 + ComputeBrokerApp2).
* :class:`Context` + :func:`run_batch` — R independent trace replays of the
  broker/fog-node loop (BrokerBaseApp3.cc:123-158, ComputeBrokerApp3.cc:205-320).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _abi
from ._abi import FognetError

_TENSOR_DTYPES = {
    "arrive": torch.int64, "req": torch.int32, "mips": torch.int32,
    "dl": torch.int64, "ul": torch.int64, "init": torch.int64, "first_adv": torch.int64,
    "p_busy": torch.float64, "p_idle": torch.float64,  # optional power model (a11)
    "down": torch.int64,  # optional node crash ticks (node-down extension)
    "region": torch.int32,  # EXT_HIER: regional broker of each publish [R, T]
}
NEVER = np.iinfo(np.int64).max  # down tick of a node that never crashes
POLICIES = {"REF_V3": _abi.FOGNET_POLICY_REF_V3, "EXT_LAT": _abi.FOGNET_POLICY_EXT_LAT,
            "EXT_HIER": _abi.FOGNET_POLICY_EXT_HIER}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream_ptr(device, stream=None) -> C.c_void_p:
    """The caller's torch stream, else the device's current one."""
    return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(device)).cuda_stream)


def _check_out(out, m: int, device):
    """Caller-supplied pair of int32 [m] result tensors of a batched decision."""
    a, b = out
    for t in (a, b):
        if t.dtype != torch.int32 or tuple(t.shape) != (m,) or t.device != device or not t.is_contiguous():
            raise FognetError(_abi.FOGNET_ERR_ARG, f"out: a pair of contiguous int32 [{m}] tensors on {device}")
    return a, b


def _check_bytes(t, nbytes: int, device, what: str):
    """Caller-supplied record buffer: contiguous uint8 of at least nbytes on device."""
    if t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < nbytes or t.device != device or not t.is_contiguous():
        raise FognetError(_abi.FOGNET_ERR_ARG, f"{what}: a contiguous uint8 tensor of at least {nbytes} B on {device}")
    return t


# ---- one marshalling of a trace and of a replay's outputs (they read shapes and data_ptr() only) ----

def _dims(trace: dict):
    """R, T, N and the node stride of a trace: N for per-replication node parameters [R, N], 0 for shared [N]."""
    R, T = trace["arrive"].shape
    mips = trace["mips"]
    N = mips.shape[-1]
    return R, T, N, (N if mips.dim() == 2 else 0)


def _check_node_params(trace: dict, keys):
    """Every node-parameter array has the shape of mips: the kernels index them all with its stride."""
    mips = trace["mips"]
    for k in keys:
        if tuple(trace[k].shape) != tuple(mips.shape):
            raise FognetError(_abi.FOGNET_ERR_ARG, f"{k} has shape {tuple(trace[k].shape)}, mips {tuple(mips.shape)}")


def _check_trace_shapes(trace: dict, R: int, T: int):
    """The host-side shape checks of a replay (run_batch, run_assigned); the passes over its outputs make none."""
    power = ("p_busy", "p_idle") if trace.get("p_busy") is not None else ()
    _check_node_params(trace, ("dl", "ul", "init") + power + (("down",) if trace.get("down") is not None else ()))
    mips = trace["mips"]
    if tuple(trace["req"].shape) != (R, T) or (mips.dim() == 2 and mips.shape[0] != R):
        raise FognetError(_abi.FOGNET_ERR_ARG, "trace arrays disagree on R/T")


def _batch_in(trace: dict, R, T, N, stride, policy, *, ring_capacity=0, power=False, down=False, region=False,
              hier_up_tick=0, hier_threshold_s=0, flags=0) -> _abi.BatchIn:
    """fognet_batch_in of a trace; ``power`` / ``down`` / ``region``: forward these optional arrays if it has them."""
    opt = lambda on, k: _ptr(trace.get(k)) if on else None  # noqa: E731
    return _abi.BatchIn(
        R=R, T=T, N=N, policy=policy, node_stride=stride, ring_capacity=ring_capacity,
        arrive_tick=_ptr(trace["arrive"]), req_mips=_ptr(trace["req"]), mips=_ptr(trace["mips"]),
        dl_tick=_ptr(trace["dl"]), ul_tick=_ptr(trace["ul"]), init_adv_tick=_ptr(trace["init"]),
        p_busy_w=opt(power, "p_busy"), p_idle_w=opt(power, "p_idle"), down_tick=opt(down, "down"),
        region=opt(region, "region"), hier_up_tick=hier_up_tick, hier_threshold_s=hier_threshold_s, flags=flags)


def _batch_in_dims(R: int, T: int) -> _abi.BatchIn:
    """fognet_batch_in of a pass that reads R and T alone (fognet_compare_dev): no trace, no policy."""
    return _abi.BatchIn(R=R, T=T)


def _batch_out(out, *, energy=False, hist=False, escalated=False) -> _abi.BatchOut:
    """fognet_batch_out of a BatchResult: the per-task arrays and the records, and what the flags add."""
    return _abi.BatchOut(
        node=_ptr(out.node), status=_ptr(out.status), start_tick=_ptr(out.start_tick), done_tick=_ptr(out.done_tick),
        stats=_ptr(out.stats), node_energy_j=_ptr(out.node_energy) if energy else None,
        hist=_ptr(out.hist) if hist else None, escalated=_ptr(out.escalated) if escalated else None)


def _policy_of(out, policy) -> int:
    """The ABI value of a policy name or number; None: what the replay recorded on ``out`` (REF_V3 if nothing)."""
    if policy is None:
        policy = out.policy if out.policy is not None else _abi.FOGNET_POLICY_REF_V3
    return POLICIES[policy] if isinstance(policy, str) else int(policy)


def _record_buffer(res, nbytes: int, dev, what: str, zero: bool = False, alloc: int | None = None):
    """The caller's record buffer, checked, else a new one of ``alloc`` (default ``nbytes``) bytes."""
    if res is not None:
        return _check_bytes(res, nbytes, dev, what)
    return (torch.zeros if zero else torch.empty)(nbytes if alloc is None else alloc, dtype=torch.uint8, device=dev)


def _reduce_records(ctx, name: str, dtype, recs, what: str, R: int, K=None, stats=None, out=None, stream=None):
    """Job reduction on the device (``fognet_reduce_<name>_dev``) of ``recs``, the caller's argument ``what``:
    [R][K] records of ``dtype`` keyed against ``stats`` into [K], or (``stats`` None) [R] records that
    carry their own statuses into one."""
    nout = (1 if stats is None else K) * dtype.itemsize
    dev = (recs if stats is None else stats).device
    out = _record_buffer(out, nout, dev, "out", alloc=max(nout, 1))
    if stats is None:
        args, short = (R,), recs.numel() < R * nout
    else:
        args, what = (_ptr(stats), R, K), what + " / stats"
        short = recs.numel() < R * nout or stats.numel() < R * _abi.REP_STATS_DTYPE.itemsize
    if short:
        raise FognetError(_abi.FOGNET_ERR_ARG, f"{what} smaller than R replications")
    fn = getattr(ctx._lib, f"fognet_reduce_{name}_dev")
    ctx.check(fn(ctx.handle, _ptr(recs), *args, _ptr(out), _stream_ptr(dev, stream)), f"reduce_{name}")
    return out[:nout].cpu().numpy().view(dtype)


def _merge_records(struct, dtype, init: str, merge: str, records, keyed: bool) -> np.ndarray:
    """Exact host merge through the C ABI's ``init`` / ``merge`` pair.  ``keyed``: ``records`` are arrays
    [K] and index k merges over them, into [K]; else every record of ``records`` merges into one."""
    lib = _abi.load()
    init, merge = getattr(lib, init), getattr(lib, merge)
    if keyed:
        rows = [np.ascontiguousarray(r, dtype=dtype).reshape(-1) for r in records]
        K = rows[0].size if rows else 0
    else:
        rows = np.ascontiguousarray(records, dtype=dtype).reshape(-1, 1)
        K = 1
    acc = (struct * K)()
    for k in range(K):
        init(C.byref(acc[k]))
        for row in rows:
            merge(C.byref(acc[k]), C.byref(struct.from_buffer_copy(row[k].tobytes())))
    out = np.frombuffer(bytes(acc), dtype=dtype).copy()
    return out if keyed else out[0]


def _to_dev(x, dtype, dev) -> torch.Tensor:
    """A host array or tensor as a contiguous tensor of ``dtype`` on ``dev``."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()


def _user_tables(user_of, user_ul, user_dl, R: int, T: int, dev):
    """(user_of int32 [R, T], ul, dl int64 [U] or [R, U], U, link stride) of a pass keyed by user."""
    uo = _to_dev(user_of, torch.int32, dev)
    uu, ud = _to_dev(user_ul, torch.int64, dev), _to_dev(user_dl, torch.int64, dev)
    if tuple(uo.shape) != (R, T):
        raise FognetError(_abi.FOGNET_ERR_ARG, f"user_of must have shape [R, T], got {tuple(uo.shape)}")
    U = uu.shape[-1] if uu.dim() else -1
    if uu.shape != ud.shape or tuple(uu.shape) not in ((U,), (R, U)):
        raise FognetError(_abi.FOGNET_ERR_ARG, f"user links must both have shape [U] or [R, U], got "
                                               f"{tuple(uu.shape)} / {tuple(ud.shape)}")
    return uo, uu, ud, U, (U if uu.dim() == 2 else 0)


def _raise_unassigned(what: str, bad: int, U: int):
    if bad:
        raise FognetError(_abi.FOGNET_ERR_ARG, f"{what}: {bad} decided publishes name a user outside "
                                               f"[0, {U}) (allow_unassigned=True leaves them out)")


class Context:
    """A fognet_ctx bound to one HIP device (gfx950 required)."""

    def __init__(self, device: int | torch.device = 0):
        if isinstance(device, torch.device):
            device = device.index or 0
        self.device = int(device)
        self._lib = _abi.load()
        h = C.c_void_p()
        rc = self._lib.fognet_create(C.byref(h), self.device)
        if rc != _abi.FOGNET_OK:
            raise FognetError(rc, f"fognet_create(device={self.device}) failed: {_abi.status_string(rc)}")
        self._h = h

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fognet_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int, what: str = ""):
        if rc != _abi.FOGNET_OK:
            msg = self._lib.fognet_last_error(self._h).decode()
            raise FognetError(rc, f"{what}: {msg}" if what else msg)

    def last_error(self) -> str:
        """The message of this context's last failed call (fognet_last_error)."""
        return self._lib.fognet_last_error(self._h).decode()

    def sync(self):
        self.check(self._lib.fognet_sync(self._h), "sync")

    def hier_path_stats(self) -> tuple[int, int]:
        """EXT_HIER launches (N > 1024) that took the region pass / went straight to the
        sequential replay (fognet_hier_path_stats; FOGNET_HIER_REGIONS in fognet_hip.h)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self.check(self._lib.fognet_hier_path_stats(self._h, C.byref(a), C.byref(b)), "hier_path_stats")
        return int(a.value), int(b.value)


class BrokerBaseApp3:
    """Allocation policy of BrokerBaseApp3 (src/mqttapp/BrokerBaseApp3.cc).

    ``brokers`` is the broker's view of the registered fog nodes in CONNECT
    order: advertised busy time (double) and MIPS (int) per node
    (Broker.cc:21-22, updated only by adverts, BrokerBaseApp3.cc:123-130).
    """

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def sendPubAck(self, adv_busy, adv_mips, MIPSRequired: int) -> int:  # noqa: N802,N803 (reference names)
        """Index of the node the task is offloaded to (BrokerBaseApp3.cc:267-281).

        Raises FognetError(FOGNET_ERR_NO_NODES) for an empty view (the reference
        dereferences brokers[0], UB) and FognetError(FOGNET_ERR_DIV0) when node 0
        has not advertised yet (MIPS 0: SIGFPE in the reference).
        """
        busy = np.ascontiguousarray(adv_busy, dtype=np.float64)
        mips = np.ascontiguousarray(adv_mips, dtype=np.int32)
        if busy.shape != mips.shape or busy.ndim != 1:
            raise FognetError(_abi.FOGNET_ERR_ARG, "adv_busy/adv_mips must be 1-D and equal length")
        out = C.c_int32(-1)
        lib = self.ctx._lib
        rc = lib.fognet_decide(self.ctx.handle, _abi.FOGNET_POLICY_REF_V3, len(busy),
                               busy.ctypes.data_as(C.c_void_p), mips.ctypes.data_as(C.c_void_p),
                               int(MIPSRequired), C.byref(out))
        self.ctx.check(rc, "sendPubAck")
        return out.value

    def sendPubAck_window(self, adv_busy, adv_mips, MIPSRequired) -> np.ndarray:  # noqa: N802,N803
        """The publishes of one window (no advert in between: one view) decided
        together (fognet_decide_window); equals one sendPubAck per request."""
        busy = np.ascontiguousarray(adv_busy, dtype=np.float64)
        mips = np.ascontiguousarray(adv_mips, dtype=np.int32)
        req = np.ascontiguousarray(MIPSRequired, dtype=np.int32).reshape(-1)
        if busy.shape != mips.shape or busy.ndim != 1:
            raise FognetError(_abi.FOGNET_ERR_ARG, "adv_busy/adv_mips must be 1-D and equal length")
        out = np.empty(len(req), np.int32)
        rc = self.ctx._lib.fognet_decide_window(self.ctx.handle, _abi.FOGNET_POLICY_REF_V3, len(busy),
                                                busy.ctypes.data_as(C.c_void_p), mips.ctypes.data_as(C.c_void_p),
                                                len(req), req.ctypes.data_as(C.c_void_p),
                                                out.ctypes.data_as(C.c_void_p))
        self.ctx.check(rc, "sendPubAck_window")
        return out

    def sendPubAck_batch(self, adv_busy: torch.Tensor, adv_mips: torch.Tensor, req: torch.Tensor,  # noqa: N802
                         out: tuple[torch.Tensor, torch.Tensor] | None = None):
        """M independent decisions on device tensors [M, n]; returns (node, status) int32 [M].
        ``out``: write into these (node, status) tensors instead of new ones."""
        m, n = adv_busy.shape
        if out is not None:
            node, status = _check_out(out, m, adv_busy.device)
        else:
            node = torch.empty(m, dtype=torch.int32, device=adv_busy.device)
            status = torch.empty(m, dtype=torch.int32, device=adv_busy.device)
        rc = self.ctx._lib.fognet_decide_batch_dev(
            self.ctx.handle, _abi.FOGNET_POLICY_REF_V3, m, n,
            _ptr(adv_busy.contiguous()), _ptr(adv_mips.contiguous()), _ptr(req.contiguous()),
            _ptr(node), _ptr(status), _stream_ptr(adv_busy.device))
        self.ctx.check(rc, "decide_batch")
        return node, status


class BrokerBaseApp2:
    """Allocation policy of BrokerBaseApp2 (src/mqttapp/BrokerBaseApp2.cc, the
    module simulations/example/wirelessNet.ini:56 selects).

    Serves a task itself when MIPSRequired < its own remaining MIPS
    (``local_mips``: par MIPS minus its reservations, :181, :211); otherwise
    forwards to the LAST node whose advertised MIPS exceeds node 0's (the
    reference's "best broker" loop never updates its threshold, :241-248),
    and only if MIPSRequired < that node's MIPS (:262).
    """

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def sendPubAck(self, adv_mips, local_mips: int, MIPSRequired: int) -> tuple[int, int]:  # noqa: N802,N803
        """(action, node): action is _abi.V2_LOCAL / V2_FORWARD / V2_DROPPED /
        V2_NO_NODES; node is -1 for LOCAL and NO_NODES."""
        mips = np.ascontiguousarray(adv_mips, dtype=np.int32).reshape(-1)
        node, act = C.c_int32(-1), C.c_int32(0)
        rc = self.ctx._lib.fognet_decide_v2(self.ctx.handle, len(mips), mips.ctypes.data_as(C.c_void_p),
                                            int(local_mips), int(MIPSRequired), C.byref(node), C.byref(act))
        self.ctx.check(rc, "sendPubAck(v2)")
        return act.value, node.value

    def sendPubAck_batch(self, adv_mips: torch.Tensor, local_mips: torch.Tensor, req: torch.Tensor,  # noqa: N802
                         out: tuple[torch.Tensor, torch.Tensor] | None = None):
        """M independent decisions on device tensors adv_mips [M, n], local_mips [M],
        req [M]; returns (action, node) int32 [M].  ``out``: write into these
        (action, node) tensors instead of new ones."""
        m, n = adv_mips.shape
        if out is not None:
            act, node = _check_out(out, m, adv_mips.device)
        else:
            node = torch.empty(m, dtype=torch.int32, device=adv_mips.device)
            act = torch.empty(m, dtype=torch.int32, device=adv_mips.device)
        rc = self.ctx._lib.fognet_decide_v2_batch_dev(
            self.ctx.handle, m, n, _ptr(adv_mips.contiguous()), _ptr(local_mips.contiguous()), _ptr(req.contiguous()),
            _ptr(node), _ptr(act), _stream_ptr(adv_mips.device))
        self.ctx.check(rc, "decide_v2_batch")
        return act, node


@dataclass
class BatchResult:
    node: torch.Tensor | None        # [R, T] int32 (None: statistics only)
    status: torch.Tensor | None      # [R, T] uint8 (5 started / 4 queued)
    start_tick: torch.Tensor | None  # [R, T] int64
    done_tick: torch.Tensor | None   # [R, T] int64
    stats: torch.Tensor       # [R * sizeof(fognet_rep_stats)] uint8 (device)
    node_energy: torch.Tensor | None = None  # [R, N] float64 (power model only)
    hist: torch.Tensor | None = None         # [2, 64] int64 job histogram (queueTime, response), added to
    policy: int | None = None                # fognet_policy of the run_batch that filled these buffers (None: not run)
    escalated: torch.Tensor | None = None    # [R, T] uint8, EXT_HIER: 1 where the parent broker took the decision
    hier_up_tick: int = 0                    # the hop of that run_batch (EXT_HIER; what user_stats / node_stats add)

    def rep_stats(self) -> np.ndarray:
        return self.stats.cpu().numpy().view(_abi.REP_STATS_DTYPE)


def allocate_outputs(R: int, T: int, device, N: int | None = None, energy: bool = False,
                     hist: bool = False, per_task: bool = True, escalated: bool = False) -> BatchResult:
    """Output buffers; ``per_task=False``: statistics only (no per-task arrays:
    the replay writes nothing per task, fognet_batch_out).  ``escalated``: also
    the per-task escalation flags (fognet_batch_out.escalated), which
    :func:`user_stats` and :func:`node_stats` need under EXT_HIER."""
    if escalated and not per_task:
        raise FognetError(_abi.FOGNET_ERR_ARG, "escalated is a per-task output: not with per_task=False")
    mk = (lambda shape, dt: torch.empty(shape, dtype=dt, device=device)) if per_task else (lambda shape, dt: None)
    return BatchResult(
        node=mk((R, T), torch.int32),
        status=mk((R, T), torch.uint8),
        start_tick=mk((R, T), torch.int64),
        done_tick=mk((R, T), torch.int64),
        stats=torch.zeros(R * _abi.REP_STATS_DTYPE.itemsize, dtype=torch.uint8, device=device),
        node_energy=torch.zeros((R, N), dtype=torch.float64, device=device) if energy else None,
        hist=torch.zeros((_abi.HIST_METRICS, _abi.HIST_BINS), dtype=torch.int64, device=device) if hist else None,
        escalated=torch.empty((R, T), dtype=torch.uint8, device=device) if escalated else None,
    )


def as_device_trace(trace: dict, device) -> dict:
    """numpy/torch trace dict -> contiguous device tensors of the ABI dtypes."""
    out = {}
    for k, dt in _TENSOR_DTYPES.items():
        if k not in trace or trace[k] is None:
            continue
        v = trace[k]
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
        out[k] = t.to(device=device, dtype=dt).contiguous()
    if out["arrive"].dim() == 1:
        out["arrive"] = out["arrive"].unsqueeze(0)
        out["req"] = out["req"].unsqueeze(0)
        if "region" in out:
            out["region"] = out["region"].unsqueeze(0)
    return out


def run_batch(ctx: Context, trace: dict, out: BatchResult | None = None, ring_capacity: int = 0,
              stream=None, stage: str = "all", policy: str | int = "REF_V3", hist: bool = False,
              hier_threshold_s: int = 60, hier_up_tick: int = 20 * 10**9, ref_abort: bool = False,
              escalated: bool = False) -> BatchResult:
    """Enqueue R trace replays (fognet_run_batch_dev) on the current stream.

    ``trace``: device tensors arrive/req [R, T], node params mips/dl/ul/init
    [R, N] (per replication) or [N] (shared), optional power model
    p_busy/p_idle (W, same shape as mips), optional node crash ticks ``down``
    (same shape as mips, NEVER = no crash; ComputeBrokerApp3::handleNodeCrash,
    ComputeBrokerApp3.cc:423-427: lost tasks get status 9).  ``stage``: "all", "replay"
    (fognet_replay_dev) or "stats" (fognet_rep_stats_dev).  ``policy``:
    "REF_V3" (BrokerBaseApp3), "EXT_LAT" (north-star cost) or "EXT_HIER"
    (hierarchical brokers with mobility handoff: needs ``trace["region"]``
    [R, T], see :func:`mobility_regions`; escalation above
    ``hier_threshold_s`` busy seconds, extra hop ``hier_up_tick``); the two
    extensions are not in the reference.  ``hist``: allocate the job
    histogram when ``out`` is None.  ``ref_abort`` (FOGNET_FLAG_REF_ABORT): a
    replication the reference run would end at a queueTime overflow gets status
    FOGNET_REF_ABORTED (its abort point, ``abort_tick``/``abort_task``, is in
    every record either way).  ``escalated``: allocate the per-task escalation
    flags when ``out`` is None (``out.escalated`` [R, T] uint8: 1 where the
    parent broker took the decision under EXT_HIER, all 0 under the other
    policies); an ``out`` that carries the array gets it filled either way.
    """
    dims = R, T, N, _ = _dims(trace)
    dev = trace["arrive"].device
    pol = _policy_of(None, policy)
    _check_trace_shapes(trace, R, T)
    if out is not None and ((out.node is not None and tuple(out.node.shape) != (R, T))
                            or out.stats.numel() < R * _abi.REP_STATS_DTYPE.itemsize):
        raise FognetError(_abi.FOGNET_ERR_ARG, "output buffers too small for the trace")
    if out is None:
        out = allocate_outputs(R, T, dev, N=N, energy=trace.get("p_busy") is not None, hist=hist, escalated=escalated)
    if out.escalated is not None and (out.escalated.dtype != torch.uint8 or tuple(out.escalated.shape) != (R, T)
                                      or out.escalated.stride(-1) != 1 or (R > 1 and out.escalated.stride(0) != T)):
        raise FognetError(_abi.FOGNET_ERR_ARG, f"out.escalated: a row-contiguous uint8 [{R}, {T}] tensor")
    region = trace.get("region")
    if pol == _abi.FOGNET_POLICY_EXT_HIER and (region is None or tuple(region.shape) != (R, T)):
        raise FognetError(_abi.FOGNET_ERR_ARG, "EXT_HIER needs trace['region'] of shape [R, T]")
    # every array the trace and the outputs have; region, hop and threshold as given
    bi = _batch_in(trace, *dims, pol, ring_capacity=ring_capacity, power=True, down=True, region=True,
                   hier_up_tick=int(hier_up_tick), hier_threshold_s=int(hier_threshold_s),
                   flags=_abi.FLAG_REF_ABORT if ref_abort else 0)
    bo = _batch_out(out, energy=True, hist=True, escalated=True)
    fn = {"all": ctx._lib.fognet_run_batch_dev, "replay": ctx._lib.fognet_replay_dev,
          "stats": ctx._lib.fognet_rep_stats_dev}[stage]
    ctx.check(fn(ctx.handle, C.byref(bi), C.byref(bo), _stream_ptr(dev, stream)), f"run_batch[{stage}]")
    out.policy = pol  # what user_stats goes by when it is given no policy
    out.hier_up_tick = int(hier_up_tick) if pol == _abi.FOGNET_POLICY_EXT_HIER else 0
    return out


def run_assigned(ctx: Context, trace: dict, assign: torch.Tensor, out: BatchResult | None = None,
                 stats: bool = True, hist: bool = False, energy: bool = False, stream=None) -> BatchResult:
    """The node model under the caller's decisions (fognet_run_assigned_dev): task i of
    replication r goes to node ``assign[r, i]`` (int32 [R, T] on the trace's device: a policy
    evaluated in PyTorch, recorded decisions, :func:`assign_round_robin`, :func:`assign_random`).
    No broker decides; each node is a FIFO single server over the tasks sent to it.

    ``trace``: as :func:`run_batch` (``down`` and the power model included; ``region`` is not
    read).  ``stats=False``: fognet_replay_assigned_dev, which fills the per-task arrays and the
    record's status / n_tasks / max_pending / events only.  ``hist`` / ``energy``: allocate the
    job histogram / the per-node energy rows when ``out`` is None (``energy`` needs the power
    model in the trace).  ``out.node`` receives the assignment and may be ``assign`` itself.
    The result serves :func:`node_stats`, :func:`per_user_stats`, :func:`user_stats` and
    :func:`signal_vectors` as a REF_V3 replay's does.  A replication with a bad input (an
    ``assign`` entry outside [0, N) among them) has status FOGNET_ERR_ARG in its record."""
    dims = R, T, N, _ = _dims(trace)
    dev = trace["arrive"].device
    _check_trace_shapes(trace, R, T)
    if (not isinstance(assign, torch.Tensor) or assign.dtype != torch.int32 or tuple(assign.shape) != (R, T)
            or assign.device != dev or not assign.is_contiguous()):
        raise FognetError(_abi.FOGNET_ERR_ARG, f"assign: a contiguous int32 [{R}, {T}] tensor on {dev}")
    if energy and trace.get("p_busy") is None:
        raise FognetError(_abi.FOGNET_ERR_ARG, "energy needs the power model (p_busy / p_idle) in the trace")
    if out is None:
        out = allocate_outputs(R, T, dev, N=N, energy=energy, hist=hist)
    if out.node is None or tuple(out.node.shape) != (R, T) or out.stats.numel() < R * _abi.REP_STATS_DTYPE.itemsize:
        raise FognetError(_abi.FOGNET_ERR_ARG, "run_assigned needs the per-task output arrays [R, T] and R records")
    bi = _batch_in(trace, *dims, _abi.FOGNET_POLICY_REF_V3, power=True, down=True)  # no region, hop or flags
    bo = _batch_out(out, energy=True, hist=True, escalated=True)
    fn = ctx._lib.fognet_run_assigned_dev if stats else ctx._lib.fognet_replay_assigned_dev
    ctx.check(fn(ctx.handle, C.byref(bi), _ptr(assign), C.byref(bo), _stream_ptr(dev, stream)), "run_assigned")
    out.policy = _abi.FOGNET_POLICY_REF_V3  # what the passes over the outputs go by
    out.hier_up_tick = 0
    return out


def assign_round_robin(R: int, T: int, N: int, device) -> torch.Tensor:
    """Task i to node i mod N in every replication: int32 [R, T] on ``device``."""
    row = torch.arange(T, dtype=torch.int64, device=device).remainder(N).to(torch.int32)
    return row.unsqueeze(0).expand(R, T).contiguous()


def assign_random(R: int, T: int, N: int, seed: int, device) -> torch.Tensor:
    """Uniformly random nodes from a torch generator seeded with ``seed`` on ``device``:
    int32 [R, T].  (The driver's ``--assign random`` draws from std::mt19937_64 instead.)"""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return torch.randint(0, N, (R, T), generator=g, device=device, dtype=torch.int32)


def run_generated(ctx: Context, seed: int, R: int, T: int, N: int, mean_gap_ticks, lat_scale, r0: int = 0,
                  req_lo: int = 1000, req_hi: int = 64000, out: BatchResult | None = None, ring_capacity: int = 0,
                  policy: str | int = "REF_V3", power=None, hist: bool = True, energy: bool = False,
                  device=None, stream=None, hier_threshold_s: int = 60, hier_up_tick: int = 20 * 10**9) -> BatchResult:
    """Statistics-only replay of generated replications r0 .. r0+R-1
    (fognet_run_generated_dev): the trace recipe of
    :func:`generate_trace` is computed inside the replay kernel 64 publishes at
    a time, so neither the trace nor per-task outputs exist in memory.  The
    records equal ``generate_trace`` + ``run_batch`` on the same replications.
    ``power``: optional (p_busy, p_idle) device tensors [R, N] or [N].
    ``policy="EXT_HIER"``: each publish's regional broker is the one
    :func:`mobility_regions` (defaults) gives, computed in the kernel."""
    device = device if device is not None else torch.device("cuda", ctx.device)
    if isinstance(mean_gap_ticks, torch.Tensor):
        mg, ls = mean_gap_ticks.reshape(R).contiguous(), lat_scale.reshape(R).contiguous()
    else:
        mg = torch.as_tensor(np.asarray(mean_gap_ticks, dtype=np.float64).reshape(R), device=device)
        ls = torch.as_tensor(np.asarray(lat_scale, dtype=np.int64).reshape(R), device=device)
    pb, pi = power if power is not None else (None, None)
    stride = 0
    if pb is not None:
        if tuple(pb.shape) != tuple(pi.shape) or pb.shape[-1] != N or (pb.dim() == 2 and pb.shape[0] != R):
            raise FognetError(_abi.FOGNET_ERR_ARG, "power model arrays must be [R, N] or [N]")
        stride = N if pb.dim() == 2 else 0
    if out is None:
        out = allocate_outputs(R, T, device, N=N, energy=energy and pb is not None, hist=hist, per_task=False)
    elif out.stats.numel() < R * _abi.REP_STATS_DTYPE.itemsize:
        raise FognetError(_abi.FOGNET_ERR_ARG, "stats buffer too small")
    pol = _policy_of(None, policy)
    gp = _abi.GenParams(seed & 0xFFFFFFFF, req_lo, req_hi, 0, _ptr(mg), _ptr(ls))
    hier = pol == _abi.FOGNET_POLICY_EXT_HIER
    # stated apart from _batch_in / _batch_out: no trace in memory and no per-task output
    bi = _abi.BatchIn(R=R, T=T, N=N, policy=pol, node_stride=stride, ring_capacity=ring_capacity,
                      p_busy_w=_ptr(pb), p_idle_w=_ptr(pi), hier_up_tick=hier_up_tick if hier else 0,
                      hier_threshold_s=hier_threshold_s if hier else 0)
    bo = _abi.BatchOut(stats=_ptr(out.stats), node_energy_j=_ptr(out.node_energy), hist=_ptr(out.hist))
    ctx.check(ctx._lib.fognet_run_generated_dev(ctx.handle, C.byref(gp), r0, C.byref(bi), C.byref(bo),
                                                _stream_ptr(device, stream)), "run_generated")
    out._keep = (mg, ls)
    return out


def _hier_up(out: BatchResult, hier_up_tick) -> int:
    """The EXT_HIER hop a statistics pass adds to escalated tasks: the caller's, else the replay's."""
    return int(out.hier_up_tick if hier_up_tick is None else hier_up_tick)


def _pass_descriptors(trace, out, dims, pol, hier_up_tick, down=False):
    """What user_stats, per_user_stats and node_stats (``down``: node_stats alone) hand their kernels: no power
    model, no energy rows, no histogram; region, the escalation flags and the hop only under EXT_HIER."""
    hier = pol == _abi.FOGNET_POLICY_EXT_HIER
    hop = _hier_up(out, hier_up_tick) if hier else 0
    return _batch_in(trace, *dims, pol, down=down, region=hier, hier_up_tick=hop), _batch_out(out, escalated=hier)


def user_stats(ctx: Context, trace: dict, out: BatchResult, user_ul, user_dl,
               res: torch.Tensor | None = None, policy: str | int | None = None,
               hier_up_tick: int | None = None) -> np.ndarray:
    """User-side signals (fognet_user_stats_dev) of a finished replay: broker
    ``delay`` and mqttApp2's ``latency`` / ``latencyH1`` / ``taskTime`` as exact
    tick moments per replication (USER_STATS_DTYPE [R]).  ``user_ul`` /
    ``user_dl``: the publishing user's links, [R] (one user per replication)
    or [R, T] (per task), host arrays or device tensors.  ``res``: the device
    buffer the records are written to (uint8, R * sizeof(fognet_user_stats)).
    ``policy``: the replay's; None takes the one :func:`run_batch` recorded on
    ``out`` (REF_V3 for buffers it did not fill).  "REF_V3" and "EXT_LAT";
    "EXT_HIER" when ``out.escalated`` holds the replay's escalation flags
    (``run_batch(..., escalated=True)``): the node ack of an escalated task
    leaves ``hier_up_tick`` later (None: the hop run_batch recorded on
    ``out``).  Without the flags EXT_HIER is refused (FOGNET_ERR_UNSUPPORTED,
    nothing is written): the other per-task outputs do not say which tasks
    were escalated.  A failed
    replication (status other than FOGNET_OK / FOGNET_REF_ABORTED) gets the
    empty record."""
    dims = R, T, _, _ = _dims(trace)
    dev = trace["arrive"].device
    uu, ud = _to_dev(user_ul, torch.int64, dev), _to_dev(user_dl, torch.int64, dev)
    per_task = 1 if uu.dim() == 2 else 0
    want = (R, T) if per_task else (R,)
    if tuple(uu.shape) != want or tuple(ud.shape) != want:
        raise FognetError(_abi.FOGNET_ERR_ARG, f"user links must both have shape [R] or [R, T], got "
                                               f"{tuple(uu.shape)} / {tuple(ud.shape)}")
    nres = R * _abi.USER_STATS_DTYPE.itemsize
    res = _record_buffer(res, nres, dev, "res", zero=True)
    bi, bo = _pass_descriptors(trace, out, dims, _policy_of(out, policy), hier_up_tick)
    ctx.check(ctx._lib.fognet_user_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), _ptr(uu), _ptr(ud), per_task,
                                             _ptr(res), _stream_ptr(dev)), "user_stats")
    return res[:nres].cpu().numpy().view(_abi.USER_STATS_DTYPE)


def node_stats(ctx: Context, trace: dict, out: BatchResult, policy: str | int = "REF_V3",
               res: torch.Tensor | None = None, hier_up_tick: int | None = None) -> torch.Tensor:
    """Per-node statistics (fognet_node_stats_dev) of a finished replay on the
    current stream: what the reference records per ComputeBroker module.
    Returns the device buffer of the records, uint8 [R, N * sizeof(fognet_node_stats)]
    (``.cpu().numpy().view(_abi.NODE_STATS_DTYPE)`` gives [R, N] records); ``res``:
    write into this buffer instead of a new one.  ``policy``: the replay's
    ("REF_V3" or "EXT_LAT"; "EXT_HIER" when ``out.escalated`` holds the replay's
    escalation flags, ``run_batch(..., escalated=True)`` -- an escalated task is
    enqueued ``hier_up_tick`` later (None: the hop run_batch recorded on ``out``) --
    and refused without them, FOGNET_ERR_UNSUPPORTED)."""
    dims = R, _, N, _ = _dims(trace)
    dev = trace["arrive"].device
    nres = R * N * _abi.NODE_STATS_DTYPE.itemsize
    res = _record_buffer(res, nres, dev, "res")
    bi, bo = _pass_descriptors(trace, out, dims, _policy_of(out, policy), hier_up_tick, down=True)
    ctx.check(ctx._lib.fognet_node_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), _ptr(res), _stream_ptr(dev)),
              "node_stats")
    return res[:nres].view(R, N * _abi.NODE_STATS_DTYPE.itemsize)


def reduce_node_stats(ctx: Context, node_stats: torch.Tensor, stats: torch.Tensor, R: int, N: int,
                      out: torch.Tensor | None = None) -> np.ndarray:
    """Exact job reduction of per-node records on the device
    (fognet_reduce_node_stats_dev): record j merges node j over the replications
    whose status is OK.  ``node_stats``: :func:`node_stats`'s buffer; ``stats``:
    the replications' records (BatchResult.stats).  Returns NODE_STATS_DTYPE [N];
    ``out``: the device buffer written to (uint8, N * sizeof(fognet_node_stats))."""
    return _reduce_records(ctx, "node_stats", _abi.NODE_STATS_DTYPE, node_stats, "node_stats", R, N, stats, out)


def merge_node_stats(records) -> np.ndarray:
    """Exact host merge of per-node record arrays [N] (e.g. one per GPU after an
    all-gather; fognet_node_stats_merge) into one [N]."""
    return _merge_records(_abi.NodeStats, _abi.NODE_STATS_DTYPE, "fognet_node_stats_init", "fognet_node_stats_merge",
                          records, keyed=True)


QUEUE_LEVELS = (1, 2, 4, 8, 16, 32, 64, 128)


def queue_stats(ctx: Context, trace: dict, out: BatchResult, levels=QUEUE_LEVELS, t0_tick: int = 0,
                t1_tick: int | None = None, policy: str | int | None = None,
                res: torch.Tensor | None = None) -> torch.Tensor:
    """Queue-length statistics (fognet_queue_stats_dev) of a finished replay on the current
    stream: per fog node the longest ``requests`` vector, its time integral and the ticks it held
    each of ``levels`` (1 to 8 strictly ascending lengths >= 1) or more, over the ticks
    [``t0_tick``, ``t1_tick``).  ``t1_tick`` None: one past the latest ``last_tick`` of the
    replications' records, which covers every replication whole (this reads the records back).
    Returns the device buffer of the records, uint8 [R, N * sizeof(fognet_queue_stats)]
    (``.cpu().numpy().view(_abi.QUEUE_STATS_DTYPE)`` gives [R, N] records); ``res``: write into this
    buffer instead of a new one.  ``policy``: the replay's ("REF_V3" or "EXT_LAT", the outputs of
    :func:`run_assigned` among them; None takes the one recorded on ``out``); "EXT_HIER" is refused
    (FOGNET_ERR_UNSUPPORTED).  A failed replication gets all-zero records."""
    dims = R, _, N, _ = _dims(trace)
    dev = trace["arrive"].device
    lv = [int(x) for x in levels]
    if t1_tick is None:
        st = out.rep_stats()
        ok = st["last_tick"][np.isin(st["status"], (_abi.FOGNET_OK, _abi.FOGNET_REF_ABORTED))] if R else np.zeros(0)
        t1_tick = max(int(ok.max()) + 1, int(t0_tick)) if ok.size and int(ok.max()) >= 0 else int(t0_tick)
    nres = R * N * _abi.QUEUE_STATS_DTYPE.itemsize
    res = _record_buffer(res, nres, dev, "res")
    pol = _policy_of(out, policy)
    bi = _batch_in(trace, *dims, pol, down=True, region=pol == _abi.FOGNET_POLICY_EXT_HIER)
    bo = _batch_out(out)
    arr = (C.c_int64 * max(len(lv), 1))(*lv)
    ctx.check(ctx._lib.fognet_queue_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), arr, len(lv), int(t0_tick),
                                              int(t1_tick), _ptr(res), _stream_ptr(dev)), "queue_stats")
    return res[:nres].view(R, N * _abi.QUEUE_STATS_DTYPE.itemsize)


def reduce_queue_stats(ctx: Context, queue_stats: torch.Tensor, stats: torch.Tensor, R: int, N: int,
                       out: torch.Tensor | None = None) -> np.ndarray:
    """Exact job reduction of queue records on the device (fognet_reduce_queue_stats_dev): record k
    merges node k over the replications whose status is OK (sums, and the maximum of max_len).
    ``queue_stats``: :func:`queue_stats`'s buffer; ``stats``: the replications' records
    (BatchResult.stats).  Returns QUEUE_STATS_DTYPE [N]; ``out``: the device buffer written to."""
    return _reduce_records(ctx, "queue_stats", _abi.QUEUE_STATS_DTYPE, queue_stats, "queue_stats", R, N, stats, out)


def merge_queue_stats(records) -> np.ndarray:
    """Exact host merge of queue record arrays [N] (fognet_queue_stats_merge) into one [N]."""
    return _merge_records(_abi.QueueStats, _abi.QUEUE_STATS_DTYPE, "fognet_queue_stats_init",
                          "fognet_queue_stats_merge", records, keyed=True)


def compare(ctx: Context, out_a: BatchResult, out_b: BatchResult, res: torch.Tensor | None = None,
            hist: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Paired comparison (fognet_compare_dev) of two finished replays of the same traces on the
    current stream (or ``stream``): per replication the tasks that moved to another node, the
    status transitions, which run completed what, and the exact moments of B minus A of the start,
    the service and the completion of the tasks both completed (ticks).  ``out_a`` / ``out_b``:
    the results of :func:`run_batch` under any policy or of :func:`run_assigned` on one trace;
    no trace is read, and that both belong to the same traces is the caller's word.
    Returns the device buffer of the records, uint8 [R * sizeof(fognet_compare_stats)]
    (``.cpu().numpy().view(_abi.COMPARE_STATS_DTYPE)`` gives [R] records); ``res``: write into this
    buffer instead of a new one.  ``hist``: int64 [2, 64] on the device, ADDED to: the pairs that
    finished earlier (row 0) and later (row 1) under B by |difference|, whole ms in log2 bins, of
    the replications that are OK in both runs.  A replication that failed in either run gets the
    empty record with the two statuses."""
    shaped = next((o.node for o in (out_a, out_b) if o.node is not None), None)
    if shaped is None:
        raise FognetError(_abi.FOGNET_ERR_ARG, "compare needs the per-task outputs (a statistics-only result has none)")
    R, T = shaped.shape
    dev = shaped.device
    for o in (out_a, out_b):
        if o.stats.numel() < R * _abi.REP_STATS_DTYPE.itemsize or (o.node is not None and tuple(o.node.shape) != (R, T)):
            raise FognetError(_abi.FOGNET_ERR_ARG, "compare: the two results disagree on R/T")
    if hist is not None and (hist.dtype != torch.int64 or hist.numel() != 2 * _abi.HIST_BINS or hist.device != dev
                             or not hist.is_contiguous()):
        raise FognetError(_abi.FOGNET_ERR_ARG, f"hist: a contiguous int64 [2, {_abi.HIST_BINS}] tensor on {dev}")
    nres = R * _abi.COMPARE_STATS_DTYPE.itemsize
    res = _record_buffer(res, nres, dev, "res", alloc=max(nres, 1))
    bi, ba, bb = _batch_in_dims(R, T), _batch_out(out_a), _batch_out(out_b)
    ctx.check(ctx._lib.fognet_compare_dev(ctx.handle, C.byref(bi), C.byref(ba), C.byref(bb), _ptr(res), _ptr(hist),
                                          _stream_ptr(dev, stream)), "compare")
    return res[:nres]


def reduce_compare(ctx: Context, cmp: torch.Tensor, R: int, out: torch.Tensor | None = None, stream=None) -> np.ndarray:
    """Exact job reduction of comparison records on the device (fognet_reduce_compare_dev): the
    merge of the records whose two statuses are OK.  ``cmp``: :func:`compare`'s buffer.  Returns
    COMPARE_STATS_DTYPE [1]; ``out``: the device buffer written to."""
    return _reduce_records(ctx, "compare", _abi.COMPARE_STATS_DTYPE, cmp, "cmp", R, out=out, stream=stream)


def merge_compare(records) -> np.ndarray:
    """Exact host merge of comparison records (fognet_compare_stats_merge) into one, a
    COMPARE_STATS_DTYPE scalar array: counts and moments add, extrema combine, statuses OK."""
    return _merge_records(_abi.CompareStats, _abi.COMPARE_STATS_DTYPE, "fognet_compare_stats_init",
                          "fognet_compare_stats_merge", records, keyed=False)


def reduce_groups(ctx: Context, stats: torch.Tensor, R: int, group_of=None, G: int = 1, metrics: bool = False,
                  out: torch.Tensor | None = None, stream=None):
    """Replication groups (fognet_reduce_groups_dev) on the current stream (or ``stream``): the job
    reduction keyed by ``group_of`` (int32 [R], host or device; None: one group) and, per group,
    the exact moments of the nine per-replication metrics (``_abi.REP_METRICS``) across its OK
    replications.  ``stats``: the device buffer of [R] fognet_rep_stats of any replay
    (``BatchResult.stats``).  Returns GROUP_STATS_DTYPE [G] and the number of replications whose
    group lies outside [0, G); with ``metrics`` also int64 [R, 9] and uint32 [R] (the values and
    which of them the moments took; every other entry is INT64_MIN).  ``out``: the device buffer
    the records are written to (uint8, G * 848)."""
    dev = stats.device
    if R < 0 or stats.numel() < R * _abi.REP_STATS_DTYPE.itemsize:
        raise FognetError(_abi.FOGNET_ERR_ARG, "stats smaller than R replications")
    gof = None
    if group_of is not None:
        gof = _to_dev(group_of, torch.int32, dev).reshape(-1)
        if gof.numel() != R:
            raise FognetError(_abi.FOGNET_ERR_ARG, "group_of: int32 [R]")
    nout = max(G, 0) * _abi.GROUP_STATS_DTYPE.itemsize
    out = _record_buffer(out, nout, dev, "out", alloc=max(nout, 1))
    met = torch.empty((R, len(_abi.REP_METRICS)), dtype=torch.int64, device=dev) if metrics else None
    dfn = torch.empty(max(R, 1), dtype=torch.int32, device=dev) if metrics else None
    ung = torch.empty(1, dtype=torch.int64, device=dev)
    ctx.check(ctx._lib.fognet_reduce_groups_dev(ctx.handle, _ptr(stats), R, _ptr(gof), G, _ptr(out), _ptr(met),
                                                _ptr(dfn), _ptr(ung), _stream_ptr(dev, stream)), "reduce_groups")
    rec = out[:nout].cpu().numpy().view(_abi.GROUP_STATS_DTYPE)
    if not metrics:
        return rec, int(ung.item())
    return rec, int(ung.item()), met.cpu().numpy(), dfn[:R].cpu().numpy().view(np.uint32)


def rep_metrics(rep):
    """The nine metrics of one REP_STATS_DTYPE record (fognet_rep_metrics, host): int64 [9] values
    (INT64_MIN where undefined or overflowed), the bits of the defined ones, the bits of those that
    do not fit int64.  The record's status is not looked at."""
    b = _abi.RepStats.from_buffer_copy(np.ascontiguousarray(rep).tobytes())
    val = (C.c_int64 * len(_abi.REP_METRICS))()
    dfn, ovf = C.c_uint32(), C.c_uint32()
    _abi.load().fognet_rep_metrics(C.byref(b), val, C.byref(dfn), C.byref(ovf))
    return np.array(val[:], dtype=np.int64), dfn.value, ovf.value


def group_from_reps(reps) -> np.ndarray:
    """Exact host reduction of REP_STATS_DTYPE records into one group record
    (fognet_group_stats_add_rep, the host twin of fognet_reduce_groups_dev)."""
    lib = _abi.load()
    acc = _abi.GroupStats()
    lib.fognet_group_stats_init(C.byref(acc))
    for rec in np.atleast_1d(reps):
        b = _abi.RepStats.from_buffer_copy(np.ascontiguousarray(rec).tobytes())
        lib.fognet_group_stats_add_rep(C.byref(acc), C.byref(b))
    return np.frombuffer(bytes(acc), dtype=_abi.GROUP_STATS_DTYPE).copy()[0]


def merge_group_stats(records) -> np.ndarray:
    """Exact host merge of group records (fognet_group_stats_merge) into one: ranks, shards, or
    groups folded together."""
    return _merge_records(_abi.GroupStats, _abi.GROUP_STATS_DTYPE, "fognet_group_stats_init",
                          "fognet_group_stats_merge", records, keyed=False)


def group_job(group) -> np.ndarray:
    """One group record as a job record (fognet_group_stats_job): the integer fields of
    :func:`reduce_stats` over the group's members, energy_j from the exact sum of microjoules."""
    g = _abi.GroupStats.from_buffer_copy(np.ascontiguousarray(group, dtype=_abi.GROUP_STATS_DTYPE).tobytes())
    job = _abi.JobStats()
    _abi.load().fognet_group_stats_job(C.byref(g), C.byref(job))
    return np.frombuffer(bytes(job), dtype=_abi.JOB_STATS_DTYPE).copy()[0]


# reported unit of each metric as a power of ten (fognet_write_sca_groups): ms, ms, ms, ms, a fraction, s, s, tasks, J
GROUP_METRIC_KEYS = ("respMean_ms", "respMax_ms", "queueMean_ms", "queueMax_ms", "queuedShare", "makespan_s", "busy_s",
                     "maxPending", "energy_j")
_GROUP_METRIC_EXP = (9, 9, 12, 12, 6, 12, 0, 0, 6)


def summarize_group(group) -> dict:
    """:func:`summarize` of the group's job record plus, under ``"replications_by_metric"``, per metric the
    count, mean, stddev (unbiased, over replications), min and max in the units of the `.sca`
    writer, and the replications lost to the int64 range."""
    d = summarize(group_job(group))
    across = {}
    for k, (name, e) in enumerate(zip(GROUP_METRIC_KEYS, _GROUP_METRIC_EXP)):
        m = group["across"][k]
        n = int(m["count"])
        s = _signed(int(m["sum_lo"]) | (int(m["sum_hi"]) << 64), 128)
        q = int(m["sq_lo"]) | (int(m["sq_hi"]) << 64) | (int(m["sq_top"]) << 128)
        unit = 10.0 ** -e
        f = dict(count=n, overflow=int(m["overflow"]))
        if n:
            var = (n * q - s * s) / (n * (n - 1)) if n > 1 else 0
            f.update(mean=s / n * unit, stddev=max(var, 0) ** 0.5 * unit if n > 1 else float("nan"),
                     min=int(m["min_raw"]) * unit, max=int(m["max_raw"]) * unit)
        across[name] = f
    d["replications_by_metric"] = across
    return d


def per_user_stats(ctx: Context, trace: dict, out: BatchResult, user_of, user_ul, user_dl,
                   policy: str | int | None = None, res: torch.Tensor | None = None,
                   hier_up_tick: int | None = None, allow_unassigned: bool = False,
                   n_unassigned: torch.Tensor | None = None):
    """Per-user signals (fognet_per_user_stats_dev) of a finished replay on the current
    stream: what the reference records per user module.  ``user_of``: the publishing
    user of every trace entry, int32 [R, T]; ``user_ul`` / ``user_dl``: the users' links,
    [U] (shared by all replications) or [R, U]; host arrays or device tensors.  Returns
    ``(records, n_unassigned)``: the device buffer uint8 [R, U * sizeof(fognet_user_stats)]
    (``.cpu().numpy().view(_abi.USER_STATS_DTYPE)`` gives [R, U] records) and the int64 [R]
    device tensor of decided publishes whose user lies outside [0, U).  A non-zero count
    raises FognetError (FOGNET_ERR_ARG) unless ``allow_unassigned`` (this check
    synchronises).  ``res`` / ``n_unassigned``: write the records / the counts (int64 [R])
    into these buffers instead of new ones.
    ``policy`` and ``hier_up_tick``: as for :func:`user_stats` (None: what run_batch
    recorded on ``out``); EXT_HIER needs ``out.escalated`` and is refused without it."""
    dims = R, T, _, _ = _dims(trace)
    dev = trace["arrive"].device
    uo, uu, ud, U, link_stride = _user_tables(user_of, user_ul, user_dl, R, T, dev)
    nres = R * U * _abi.USER_STATS_DTYPE.itemsize
    res = _record_buffer(res, nres, dev, "res")
    un = n_unassigned if n_unassigned is not None else torch.empty(R, dtype=torch.int64, device=dev)
    if un.dtype != torch.int64 or un.numel() != R or un.device != dev or not un.is_contiguous():
        raise FognetError(_abi.FOGNET_ERR_ARG, "n_unassigned must be a contiguous int64 [R] tensor on the trace's device")
    bi, bo = _pass_descriptors(trace, out, dims, _policy_of(out, policy), hier_up_tick)
    ctx.check(ctx._lib.fognet_per_user_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), _ptr(uo), U, link_stride,
                                                 _ptr(uu), _ptr(ud), _ptr(res), _ptr(un), _stream_ptr(dev)),
              "per_user_stats")
    if not allow_unassigned and R > 0:
        _raise_unassigned("per_user_stats", int(un.sum().item()), U)
    return res[:nres].view(R, U * _abi.USER_STATS_DTYPE.itemsize), un


def signal_vectors(ctx: Context, trace: dict, out: BatchResult, user_of, user_ul, user_dl, r0: int = 0,
                   Rv: int | None = None, policy: str | int | None = None, bufs: dict | None = None,
                   allow_unassigned: bool = False, to_host: bool = True) -> dict:
    """The recorded signals of replications [r0, r0 + Rv) of a finished replay as ordered
    vectors (fognet_signal_vectors_dev), on the current stream: per replication one CSR over
    V = N + 1 + 3U vectors (the N nodes' ``queueTime``, the broker's ``delay``, U x ``latency``,
    U x ``latencyH1``, U x ``taskTime``), every vector in the order the module made the
    emissions (include/fognet_hip.h "Signal vectors").  ``user_of`` / ``user_ul`` /
    ``user_dl``: as :func:`per_user_stats`.  Returns numpy arrays: ``offset`` int64 [Rv, V + 1],
    ``time`` / ``value`` int64 [Rv, 6T] (ticks; raw values in the records' units), ``task``
    int32 [Rv, 6T] and ``n_unassigned`` int64 [Rv]; vector v of replication q is
    ``[offset[q, v], offset[q, v + 1])``, and what lies at and past ``offset[q, V]`` is
    unwritten memory.  ``bufs``: device tensors ``offset`` / ``time`` / ``value`` / ``task`` /
    ``n_unassigned`` of those shapes to write into.  ``to_host=False``: the call only enqueues
    and returns the device tensors instead (no copy back, no check of ``n_unassigned``).  A
    non-zero ``n_unassigned`` raises FognetError (FOGNET_ERR_ARG) unless ``allow_unassigned``.  ``policy``: the replay's (None: what run_batch recorded on ``out``);
    "REF_V3" and "EXT_LAT"; "EXT_HIER" is refused (FOGNET_ERR_UNSUPPORTED, nothing written)."""
    dims = R, T, N, _ = _dims(trace)
    dev = trace["arrive"].device
    Rv = R - r0 if Rv is None else Rv
    uo, uu, ud, U, link_stride = _user_tables(user_of, user_ul, user_dl, R, T, dev)
    V, cap, rows = N + 1 + 3 * U, 6 * T, max(Rv, 0)
    shapes = dict(offset=((rows, V + 1), torch.int64), time=((rows, cap), torch.int64), value=((rows, cap), torch.int64),
                  task=((rows, cap), torch.int32), n_unassigned=((rows,), torch.int64))
    b = dict(bufs or {})
    for k, (shape, dt) in shapes.items():
        if b.get(k) is None:
            b[k] = torch.empty(shape, dtype=dt, device=dev)
        t = b[k]
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise FognetError(_abi.FOGNET_ERR_ARG, f"signal_vectors: {k} must be a contiguous {dt} tensor of shape "
                                                   f"{shape} on the trace's device")
    pol = _policy_of(out, policy)
    bi, bo = _batch_in(trace, *dims, pol, region=pol == _abi.FOGNET_POLICY_EXT_HIER), _batch_out(out)  # no hop
    vec = _abi.SignalVectors(cap, _ptr(b["offset"]), _ptr(b["time"]), _ptr(b["value"]), _ptr(b["task"]))
    ctx.check(ctx._lib.fognet_signal_vectors_dev(ctx.handle, C.byref(bi), C.byref(bo), _ptr(uo), U, link_stride,
                                                 _ptr(uu), _ptr(ud), r0, Rv, C.byref(vec), _ptr(b["n_unassigned"]),
                                                 _stream_ptr(dev)), "signal_vectors")
    if not to_host:
        return {k: b[k] for k in shapes}
    got = {k: b[k].cpu().numpy() for k in shapes}
    if not allow_unassigned and rows > 0:
        _raise_unassigned("signal_vectors", int(got["n_unassigned"].sum()), U)
    return got


def reduce_user_stats(ctx: Context, user_stats: torch.Tensor, stats: torch.Tensor, R: int, U: int,
                      out: torch.Tensor | None = None) -> np.ndarray:
    """Exact job reduction of user records on the device (fognet_reduce_user_stats_dev):
    record u merges user u over the replications whose status is OK.  ``user_stats``:
    :func:`per_user_stats`'s buffer, or with U = 1 the [R] records of :func:`user_stats`
    as a device buffer; ``stats``: the replications' records (BatchResult.stats).
    Returns USER_STATS_DTYPE [U]; ``out``: the device buffer written to (uint8,
    U * sizeof(fognet_user_stats))."""
    return _reduce_records(ctx, "user_stats", _abi.USER_STATS_DTYPE, user_stats, "user_stats", R, U, stats, out)


def merge_user_stats(records) -> np.ndarray:
    """Exact host merge of user record arrays [U] (e.g. one per GPU after an
    all-gather; fognet_user_stats_merge) into one [U]."""
    return _merge_records(_abi.UserStats, _abi.USER_STATS_DTYPE, "fognet_user_stats_init", "fognet_user_stats_merge",
                          records, keyed=True)


def window_stats(ctx: Context, trace: dict, out: BatchResult, user_of, user_ul, user_dl, t0: int, window: int, W: int,
                 policy: str | int | None = None, res: torch.Tensor | None = None, hier_up_tick: int | None = None,
                 n_outside: torch.Tensor | None = None, n_unassigned: torch.Tensor | None = None):
    """Statistics per window of sim time (fognet_window_stats_dev) of a finished replay on the
    current stream: window w covers the ticks [t0 + w * window, t0 + (w + 1) * window), w < W.
    ``user_of`` / ``user_ul`` / ``user_dl``: as :func:`per_user_stats`; all three None: no user
    side (U = 0).  Returns ``(records, n_outside, n_unassigned)``: the device buffer uint8
    [R, W * sizeof(fognet_window_stats)] (``.cpu().numpy().view(_abi.WINDOW_STATS_DTYPE)`` gives
    [R, W] records), the int64 [R, 2] device tensor of point events before and at or past the
    range, and the int64 [R] device tensor of decided publishes whose user lies outside [0, U)
    (they keep their node-side events; nothing is raised for them).  ``res`` / ``n_outside`` /
    ``n_unassigned``: write into these buffers instead of new ones.  ``policy`` and
    ``hier_up_tick``: as for :func:`user_stats`; EXT_HIER needs ``out.escalated`` and is refused
    without it."""
    dims = R, T, _, _ = _dims(trace)
    dev = trace["arrive"].device
    if user_of is None and user_ul is None and user_dl is None:
        uo = uu = ud = None
        U = link_stride = 0
    else:
        uo, uu, ud, U, link_stride = _user_tables(user_of, user_ul, user_dl, R, T, dev)
    nres = R * max(W, 0) * _abi.WINDOW_STATS_DTYPE.itemsize
    res = _record_buffer(res, nres, dev, "res", alloc=max(nres, 1))
    cnt = []
    for t, shape, what in ((n_outside, (R, 2), "n_outside"), (n_unassigned, (R,), "n_unassigned")):
        t = t if t is not None else torch.empty(shape, dtype=torch.int64, device=dev)
        if t.dtype != torch.int64 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise FognetError(_abi.FOGNET_ERR_ARG, f"{what} must be a contiguous int64 {list(shape)} tensor on the "
                                                   f"trace's device")
        cnt.append(t)
    bi, bo = _pass_descriptors(trace, out, dims, _policy_of(out, policy), hier_up_tick)
    ctx.check(ctx._lib.fognet_window_stats_dev(ctx.handle, C.byref(bi), C.byref(bo), _ptr(uo), U, link_stride,
                                               _ptr(uu), _ptr(ud), t0, window, W, _ptr(res), _ptr(cnt[0]),
                                               _ptr(cnt[1]), _stream_ptr(dev)), "window_stats")
    return res[:nres].view(R, max(W, 0) * _abi.WINDOW_STATS_DTYPE.itemsize), cnt[0], cnt[1]


def reduce_window_stats(ctx: Context, win: torch.Tensor, stats: torch.Tensor, R: int, W: int,
                        out: torch.Tensor | None = None) -> np.ndarray:
    """Exact job reduction of window records on the device (fognet_reduce_window_stats_dev):
    record w merges window w over the replications whose status is OK.  ``win``:
    :func:`window_stats`'s buffer; ``stats``: the replications' records (BatchResult.stats).
    Returns WINDOW_STATS_DTYPE [W]; ``out``: the device buffer written to (uint8,
    W * sizeof(fognet_window_stats))."""
    return _reduce_records(ctx, "window_stats", _abi.WINDOW_STATS_DTYPE, win, "win", R, W, stats, out)


def merge_window_stats(records) -> np.ndarray:
    """Exact host merge of window record arrays [W] (e.g. one per GPU after an all-gather;
    fognet_window_stats_merge) into one [W]."""
    return _merge_records(_abi.WindowStats, _abi.WINDOW_STATS_DTYPE, "fognet_window_stats_init",
                          "fognet_window_stats_merge", records, keyed=True)


def _quantile_args(trace, user_of, user_ul, user_dl, ppm):
    """(dims, device, user tables, the ranks as a C array, Q) of the two quantile calls."""
    dims = R, T, _, _ = _dims(trace)
    dev = trace["arrive"].device
    if user_of is None and user_ul is None and user_dl is None:
        tables = (None, None, None, 0, 0)
    else:
        tables = _user_tables(user_of, user_ul, user_dl, R, T, dev)
    ranks = [int(p) for p in np.asarray(ppm).reshape(-1)]
    return dims, dev, tables, (C.c_int32 * max(len(ranks), 1))(*ranks), len(ranks)


def _int64_out(t, shape, dev, what):
    """The caller's int64 result tensor, checked, else a new one."""
    if t is None:
        return torch.empty(shape, dtype=torch.int64, device=dev)
    if t.dtype != torch.int64 or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise FognetError(_abi.FOGNET_ERR_ARG, f"{what} must be a contiguous int64 {list(shape)} tensor on the trace's "
                                               f"device")
    return t


def quantiles(ctx: Context, trace: dict, out: BatchResult, user_of, user_ul, user_dl, ppm,
              policy: str | int | None = None, hier_up_tick: int | None = None, value: torch.Tensor | None = None,
              count: torch.Tensor | None = None, n_unassigned: torch.Tensor | None = None):
    """Exact quantiles of the five recorded signals per replication (fognet_quantiles_dev) of a
    finished replay on the current stream.  ``ppm``: up to ``_abi.QUANTILE_MAX`` ranks in parts per
    million, in any order; the result for a population of n raw values is the k-th smallest,
    k = max(1, ceil(n * ppm / 10^6)).  ``user_of`` / ``user_ul`` / ``user_dl``: as
    :func:`window_stats`.  Returns the device tensors ``(value, count, n_unassigned)``: int64
    [R, 5, Q] raw values in ``_abi.WINDOW_SIGNALS`` order (INT64_MAX for an empty population;
    :func:`summarize_quantiles` gives recorded units), int64 [R, 5] population sizes and int64
    [R] decided publishes whose user lies outside [0, U).  ``value`` / ``count`` /
    ``n_unassigned``: write into these tensors instead of new ones.  ``policy`` and
    ``hier_up_tick``: as for :func:`user_stats`; EXT_HIER needs ``out.escalated``."""
    dims, dev, (uo, uu, ud, U, link_stride), ranks, Q = _quantile_args(trace, user_of, user_ul, user_dl, ppm)
    R = dims[0]
    value = _int64_out(value, (R, _abi.QUANTILE_SIGNALS, Q), dev, "value")
    count = _int64_out(count, (R, _abi.QUANTILE_SIGNALS), dev, "count")
    n_unassigned = _int64_out(n_unassigned, (R,), dev, "n_unassigned")
    bi, bo = _pass_descriptors(trace, out, dims, _policy_of(out, policy), hier_up_tick)
    ctx.check(ctx._lib.fognet_quantiles_dev(ctx.handle, C.byref(bi), C.byref(bo), _ptr(uo), U, link_stride, _ptr(uu),
                                            _ptr(ud), ranks, Q, _ptr(value), _ptr(count), _ptr(n_unassigned),
                                            _stream_ptr(dev)), "quantiles")
    return value, count, n_unassigned


def job_quantiles(ctx: Context, trace: dict, out: BatchResult, user_of, user_ul, user_dl, ppm,
                  policy: str | int | None = None, hier_up_tick: int | None = None, value: torch.Tensor | None = None,
                  count: torch.Tensor | None = None):
    """Exact quantiles of the job (fognet_job_quantiles_dev): of each signal's population pooled
    over the replications whose status is OK.  Arguments as :func:`quantiles`.  Returns
    ``(value, count)`` as numpy arrays, int64 [5, Q] and int64 [5]; ``value`` / ``count``: the
    device tensors written to."""
    dims, dev, (uo, uu, ud, U, link_stride), ranks, Q = _quantile_args(trace, user_of, user_ul, user_dl, ppm)
    value = _int64_out(value, (_abi.QUANTILE_SIGNALS, Q), dev, "value")
    count = _int64_out(count, (_abi.QUANTILE_SIGNALS,), dev, "count")
    bi, bo = _pass_descriptors(trace, out, dims, _policy_of(out, policy), hier_up_tick)
    ctx.check(ctx._lib.fognet_job_quantiles_dev(ctx.handle, C.byref(bi), C.byref(bo), _ptr(uo), U, link_stride,
                                                _ptr(uu), _ptr(ud), ranks, Q, _ptr(value), _ptr(count),
                                                _stream_ptr(dev)), "job_quantiles")
    return value.cpu().numpy(), count.cpu().numpy()


def summarize_quantiles(ppm, value, count) -> dict:
    """Recorded units of one population set's quantiles (``value`` [5, Q] raw, ``count`` [5]), as
    :func:`summarize_moments` gives a record's min and max: per signal a dict ``{"count": n,
    ppm: value}`` with queueTime, latency, latencyH1 and taskTime in ms (raw * 1e-12) and delay in
    ms from ticks (raw * 1e-9); a signal without a member has the count alone."""
    names = ("queueTime_ms", "delay_ms", "latency_ms", "latencyH1_ms", "taskTime_ms")
    value, count = np.asarray(value), np.asarray(count)
    res = {}
    for s, name in enumerate(names):
        d = {"count": int(count[s])}
        if d["count"]:
            unit = 1e-9 if name == "delay_ms" else 1e-12
            d.update({int(p): int(v) * unit for p, v in zip(np.asarray(ppm).reshape(-1), value[s])})
        res[name] = d
    return res


@dataclass
class V2Result:
    node: torch.Tensor        # [R, T] int32 (-1: served by the broker / no node)
    status: torch.Tensor      # [R, T] uint8 (_abi.V2_ST_*; 0: not published before the stop)
    start_tick: torch.Tensor  # [R, T] int64 reservation tick (-1: never reserved)
    done_tick: torch.Tensor   # [R, T] int64 release tick (-1: not released)
    stats: torch.Tensor       # [R * sizeof(fognet_v2_stats)] uint8

    def rep_stats(self) -> np.ndarray:
        return self.stats.cpu().numpy().view(_abi.V2_STATS_DTYPE)


def run_v2(ctx: Context, trace: dict, broker_mips, stop_tick, required_time_s=0.01, queue_capacity: int = 0,
           stream=None, out: V2Result | None = None) -> V2Result:
    """R replays of the v2 model (BrokerBaseApp2 + ComputeBrokerApp2, the modules
    simulations/example/wirelessNet.ini:56,62 select) on the device
    (fognet_run_v2_dev).  ``trace``: device tensors arrive/req [R, T], node
    parameters mips/dl/ul and first_adv (first ADVERTISEMIPS firing) [R, N] or
    [N]; ``broker_mips``, ``stop_tick``, ``required_time_s``: scalars or [R]
    (host values, or device tensors [R] of the ABI dtype, used as they are).
    ``out``: write into these buffers (V2Result layout) instead of new ones."""
    arrive, req, mips = trace["arrive"], trace["req"], trace["mips"]
    R, T, N, stride = _dims(trace)
    dev = arrive.device
    _check_node_params(trace, ("dl", "ul", "first_adv"))

    def per(v, dt):
        if isinstance(v, torch.Tensor):
            if v.dtype != dt or tuple(v.shape) != (R,) or v.device != dev or not v.is_contiguous():
                raise FognetError(_abi.FOGNET_ERR_ARG, f"per-replication tensor: contiguous {dt} [{R}] on {dev}")
            return v
        return torch.as_tensor(np.array(np.broadcast_to(np.asarray(v), (R,))), dtype=dt).to(dev)
    bm, st_, rt = per(broker_mips, torch.int32), per(stop_tick, torch.int64), per(required_time_s, torch.float64)
    if out is None:
        out = V2Result(torch.empty((R, T), dtype=torch.int32, device=dev),
                       torch.empty((R, T), dtype=torch.uint8, device=dev),
                       torch.empty((R, T), dtype=torch.int64, device=dev),
                       torch.empty((R, T), dtype=torch.int64, device=dev),
                       torch.zeros(R * _abi.V2_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev))
    else:
        for k, dt in (("node", torch.int32), ("status", torch.uint8), ("start_tick", torch.int64),
                      ("done_tick", torch.int64)):
            t = getattr(out, k)
            if t.dtype != dt or tuple(t.shape) != (R, T) or t.device != dev or not t.is_contiguous():
                raise FognetError(_abi.FOGNET_ERR_ARG, f"out.{k}: contiguous {dt} [{R}, {T}] on {dev}")
        _check_bytes(out.stats, R * _abi.V2_STATS_DTYPE.itemsize, dev, "out.stats")
    vi = _abi.V2In(R, T, N, stride, queue_capacity, 0, _ptr(arrive), _ptr(req), _ptr(bm), _ptr(rt),
                   _ptr(st_), _ptr(mips), _ptr(trace["dl"]), _ptr(trace["ul"]), _ptr(trace["first_adv"]))
    vo = _abi.V2Out(_ptr(out.node), _ptr(out.status), _ptr(out.start_tick), _ptr(out.done_tick), _ptr(out.stats))
    ctx.check(ctx._lib.fognet_run_v2_dev(ctx.handle, C.byref(vi), C.byref(vo), _stream_ptr(dev, stream)), "run_v2")
    out._keep = (bm, st_, rt)
    return out


def _signed(v: int, bits: int) -> int:
    return v - (1 << bits) if v >> (bits - 1) else v


def _fields(n, s, q, lo, hi, unit) -> dict:
    """cStdDev's `.sca` fields (count/mean/stddev/sum/sqrsum/min/max) of n values
    with exact sum s and sum of squares q, in units of ``unit`` ms."""
    if n == 0:
        return dict(count=0)
    var = (q - s * s / n) / (n - 1) if n > 1 else 0.0
    return dict(count=n, mean=s / n * unit, stddev=max(var, 0.0) ** 0.5 * unit, sum=s * unit, sqrsum=q * unit * unit,
                min=int(lo) * unit, max=int(hi) * unit)


def summarize_moments(m, raw_ms: bool = True) -> dict:
    """count/mean/stddev/sum/sqrsum/min/max of one signal-moments record
    (fognet_moments) like cStdDev's `.sca` fields.  ``raw_ms``: the values are
    raw emitted simtime_t of a ms signal (recorded value raw * 1e-12 ms); False
    for ``delay`` (raw ticks, reported in ms)."""
    n = int(m["count"])
    s = _signed(int(m["sum_lo"]) | (int(m["sum_hi"]) << 64), 128)
    q = int(m["sq_lo"]) | (int(m["sq_hi"]) << 64) | (int(m["sq_top"]) << 128)
    d = _fields(n, s, q, m["min_raw"], m["max_raw"], 1e-12 if raw_ms else 1e-9)
    d["overflow"] = int(m["overflow"])
    return d


def summarize_node(rec) -> dict:
    """`.sca`-style view of one per-node record (NODE_STATS_DTYPE): the counts and
    the node's queueTime (raw values * 1e-12 ms) and response (ticks / 1e9 ms) fields."""
    resp = summarize_moments(rec["resp"], raw_ms=False)
    resp.pop("overflow")
    return {"tasks": int(rec["n_tasks"]), "queued": int(rec["n_queued"]), "started": int(rec["n_started"]),
            "lost": int(rec["n_lost"]), "busy_s": int(rec["busy_s"]),
            "last_tick": int(rec["last_tick"]) if int(rec["resp"]["count"]) else None,
            "queueTime_ms": summarize_moments(rec["queue"]), "response_ms": resp}


def summarize_window(rec, N: int, window: int, reps: int = 1) -> dict:
    """`.sca`-style view of one window record (WINDOW_STATS_DTYPE) of ``reps`` merged replications
    with ``N`` nodes and windows of ``window`` ticks: the counts, the two time averages
    (utilisation = busy / (N * window * reps), tasks in system = insys / (window * reps)) and the
    five signals' fields (delay in ms from ticks, the others raw values * 1e-12 ms)."""
    busy = int(rec["busy_lo"]) | (int(rec["busy_hi"]) << 64)
    insys = int(rec["insys_lo"]) | (int(rec["insys_hi"]) << 64)
    span = window * max(reps, 1)
    return {"publishes": int(rec["n_publish"]), "completions": int(rec["n_complete"]),
            "utilisation": busy / (N * span), "tasks_in_system": insys / span,
            "queueTime_ms": summarize_moments(rec["queue"]), "delay_ms": summarize_moments(rec["delay"], raw_ms=False),
            "latency_ms": summarize_moments(rec["latency"]), "latencyH1_ms": summarize_moments(rec["latencyH1"]),
            "taskTime_ms": summarize_moments(rec["taskTime"])}


def reduce_stats(ctx: Context, stats: torch.Tensor, R: int, out: torch.Tensor | None = None) -> np.ndarray:
    """Exact job-level reduction on the device; returns a JOB_STATS_DTYPE record.
    ``out``: the device buffer the record is written to (uint8, sizeof(fognet_job_stats))."""
    nout = _abi.JOB_STATS_DTYPE.itemsize
    if out is None:
        out = torch.zeros(nout, dtype=torch.uint8, device=stats.device)
    else:
        _check_bytes(out, nout, stats.device, "out")
    ctx.check(ctx._lib.fognet_reduce_stats_dev(ctx.handle, _ptr(stats), R, _ptr(out), _stream_ptr(stats.device)),
              "reduce_stats")
    return out[:nout].cpu().numpy().view(_abi.JOB_STATS_DTYPE)[0]


def merge_job_stats(records) -> np.ndarray:
    """Exact host merge of job records (e.g. one per GPU after an all-gather)."""
    return _merge_records(_abi.JobStats, _abi.JOB_STATS_DTYPE, "fognet_job_stats_init", "fognet_job_stats_merge",
                          records, keyed=False)


def job_from_reps(reps) -> np.ndarray:
    """Exact host reduction of per-replication records (REP_STATS_DTYPE) into a
    job record (fognet_job_stats_add_rep, the host twin of fognet_reduce_stats_dev)."""
    lib = _abi.load()
    acc = _abi.JobStats()
    lib.fognet_job_stats_init(C.byref(acc))
    for rec in np.atleast_1d(reps):
        b = _abi.RepStats.from_buffer_copy(np.ascontiguousarray(rec).tobytes())
        lib.fognet_job_stats_add_rep(C.byref(acc), C.byref(b))
    return np.frombuffer(bytes(acc), dtype=_abi.JOB_STATS_DTYPE)[0]


def _u192(limbs) -> int:
    return int(limbs[0]) | (int(limbs[1]) << 64) | (int(limbs[2]) << 128)


def summarize(job) -> dict:
    """`.sca`-style fields (count/mean/stddev/sum/sqrsum/min/max, ms) of a job record:
    queueTime as the reference records it (ComputeBrokerApp3.cc:238,
    ComputeBrokerApp3.ned:45-46; raw values * 1e-12), response in ticks / 1e9."""
    qs = _signed(_u192(job["queue_sum"]), 192)
    queue = _fields(int(job["n_qtime"]), qs, _u192(job["queue_sq"]), job["queue_min_raw"], job["queue_max_raw"], 1e-12)
    queue["overflow"] = int(job["n_qtime_overflow"])
    return {
        "replications": int(job["n_reps"]), "failed": int(job["n_failed"]),
        "decisions": int(job["n_tasks"]), "queued": int(job["n_queued"]), "started": int(job["n_started"]),
        "queueTime_ms": queue,
        "response_ms": _fields(int(job["n_tasks"]), _u192(job["resp_sum"]), _u192(job["resp_sq"]),
                               job["resp_min_ticks"], job["resp_max_ticks"], 1e-9),
        "max_pending": int(job["max_pending"]),
        "busy_s": int(job["busy_s"]),
        "energy_j": float(job["energy_j"]),
        # replications the reference run would have ended at a queueTime overflow (fognet_hip.h)
        "ref_aborted": int(job["n_ref_aborted"]),
    }


def allocate_trace(R: int, T: int, N: int, device) -> dict:
    """Device buffers of one trace batch (arrive/req [R, T], node params [R, N])."""
    return {
        "arrive": torch.empty((R, T), dtype=torch.int64, device=device),
        "req": torch.empty((R, T), dtype=torch.int32, device=device),
        "mips": torch.empty((R, N), dtype=torch.int32, device=device),
        "dl": torch.empty((R, N), dtype=torch.int64, device=device),
        "ul": torch.empty((R, N), dtype=torch.int64, device=device),
        "init": torch.empty((R, N), dtype=torch.int64, device=device),
    }


def generate_trace(ctx: Context, seed: int, R: int, T: int, N: int, mean_gap_ticks, lat_scale,
                   r0: int = 0, req_lo: int = 1000, req_hi: int = 64000, device=None, out: dict | None = None) -> dict:
    """Device trace generator (recipe: csrc/tracegen.hip); per-replication
    ``mean_gap_ticks`` (float64 [R]) and ``lat_scale`` (int64 [R]), host arrays
    or device tensors.  ``out``: reuse these buffers (allocate_trace layout)."""
    device = device if device is not None else torch.device("cuda", ctx.device)
    if isinstance(mean_gap_ticks, torch.Tensor):
        mg, ls = mean_gap_ticks.reshape(R).contiguous(), lat_scale.reshape(R).contiguous()
    else:
        mg = torch.as_tensor(np.asarray(mean_gap_ticks, dtype=np.float64).reshape(R), device=device)
        ls = torch.as_tensor(np.asarray(lat_scale, dtype=np.int64).reshape(R), device=device)
    tr = out if out is not None else allocate_trace(R, T, N, device)
    gp = _abi.GenParams(seed & 0xFFFFFFFF, req_lo, req_hi, 0, _ptr(mg), _ptr(ls))
    rc = ctx._lib.fognet_gen_trace_dev(ctx.handle, C.byref(gp), r0, R, T, N, _ptr(tr["arrive"]), _ptr(tr["req"]),
                                       _ptr(tr["mips"]), _ptr(tr["dl"]), _ptr(tr["ul"]), _ptr(tr["init"]),
                                       _stream_ptr(device))
    ctx.check(rc, "gen_trace")
    tr["_keep"] = (mg, ls)
    return tr


def sweep_params(r_global: np.ndarray, N: int, rho=None, lat_scale=None, req_lo=1000, req_hi=64000):
    """Per-replication (mean_gap_ticks, lat_scale) for the C3 policy sweep:
    rho = (0.5, 0.8, 0.95)[r % 3], latency x(1, 10, 100)[(r // 3) % 3]
    unless fixed values are given.  mips pattern 1000*(1 + j % 4)."""
    r_global = np.asarray(r_global, dtype=np.int64)
    mips = 1000.0 * (1 + (np.arange(N) % 4))
    es = 0.5 * (req_lo + req_hi) * float(np.mean(1.0 / mips))
    rho_r = np.full(r_global.shape, rho, np.float64) if rho is not None else np.array((0.5, 0.8, 0.95))[r_global % 3]
    sc = (np.full(r_global.shape, lat_scale, np.int64) if lat_scale is not None
          else np.array((1, 10, 100), np.int64)[(r_global // 3) % 3])
    mean_gap = es / (N * rho_r) * _abi.TICKS_PER_SECOND
    return mean_gap, sc


def c5_params(r_global: np.ndarray, N: int, req_lo=1000, req_hi=64000):
    """Per-replication (mean_gap_ticks, lat_scale) of the C5 large-topology
    recipe (builder-defined: the reference has no C5 parameters):
    rho = (0.002, 0.01, 0.05)[r % 3], latency x(1, 10, 100)[(r // 3) % 3].
    Light loads: under REF_V3 the C3 loads herd all of T onto node 0 when N is
    in the thousands (the stale view keeps every node at busy 0 until its first
    completion advert), so C5 uses loads at which decisions spread over nodes."""
    r_global = np.asarray(r_global, dtype=np.int64)
    mg, sc = sweep_params(r_global, N, req_lo=req_lo, req_hi=req_hi)
    rho = np.array((0.002, 0.01, 0.05))[r_global % 3]
    mips = 1000.0 * (1 + (np.arange(N) % 4))
    es = 0.5 * (req_lo + req_hi) * float(np.mean(1.0 / mips))
    return es / (N * rho) * _abi.TICKS_PER_SECOND, sc


def mobility_regions(arrive, N: int, users: int = 256, period_s=(30, 45, 60, 75)):
    """Regional broker of every publish under a builder-defined mobility model
    (FOGNET_POLICY_EXT_HIER; not in the reference, whose only mobility is the
    users' radio mobility, simulations/example/wirelessNet.ini:13-29): publish i
    of a replication comes from user u = i mod ``users``; user u starts in
    region u mod B (B = ceil(N / 1024) regions of 1024 consecutive nodes) and
    hands off to the next region (+1 for even u, -1 for odd u, mod B) every
    period_s[u mod 4] seconds from the replication's first publish.  Integer
    arithmetic only, so numpy (host) and torch (device) give the same regions.
    ``arrive``: [R, T] int64 ticks (numpy array or tensor); returns int32 [R, T]."""
    B = -(-N // _abi.HIER_REGION_NODES)
    torch_in = isinstance(arrive, torch.Tensor)
    xp = torch if torch_in else np
    R, T = arrive.shape
    i = xp.arange(T, device=arrive.device) if torch_in else np.arange(T)
    u = (i % users).to(torch.int64) if torch_in else (i % users).astype(np.int64)
    per = [p * _abi.TICKS_PER_SECOND for p in period_s]
    period = (torch.tensor(per, device=arrive.device, dtype=torch.int64) if torch_in else np.array(per, np.int64))[u % 4]
    sign = 1 - 2 * (u % 2)
    t0 = arrive[:, :1]
    hops = (arrive - t0) // period
    reg = (u % B) + sign * hops
    reg = reg % B  # floor modulo in both numpy and torch
    return reg.to(torch.int32) if torch_in else reg.astype(np.int32)


def _saturation_template(arrive0: np.ndarray, region: np.ndarray, sizes: list[int], lat_max: int):
    """Roles of the publishes of one region sequence (saturating_trace): per
    region, walk its publishes; a free publish p starts a pair on the region's
    next fresh node (small task of S1 seconds, the region's next publish q a
    giant task), S1 the smallest whole second above q's gap, so q reaches the
    node before p completes; every publish up to p's completion advert (S1 + the
    link latencies, bounded by ``lat_max``) is a zero-service filler.  Once every
    node of the region has its pair, the publishes are zero-service tasks, which
    the saturated regional broker escalates.
    Returns role [T] (0 filler / escalation, 1 small, 2 giant), the pair's node
    offset within its region [T] (-1 for fillers) and S1 [T]."""
    T = arrive0.shape[0]
    role = np.zeros(T, np.int8)
    node = np.full(T, -1, np.int64)
    s1 = np.zeros(T, np.int64)
    tps = TICKS_PER_SECOND_I
    for b, size in enumerate(sizes):
        idx = np.flatnonzero(region == b)
        m = 0
        i = 0
        while i + 1 < len(idx) and m < size:
            p, q = idx[i], idx[i + 1]
            S1 = (int(arrive0[q]) - int(arrive0[p])) // tps + 1
            role[p], role[q] = 1, 2
            node[p] = node[q] = m
            s1[p] = S1
            adv = int(arrive0[p]) + S1 * tps + lat_max  # the advert has reached the broker by then
            i += 2
            while i < len(idx) and int(arrive0[idx[i]]) <= adv:
                i += 1
            m += 1
    return role, node, s1


TICKS_PER_SECOND_I = 10**12


def saturating_trace(seed: int, R: int, T: int, N: int, gap_s: float = 0.1, giant_s=(4000, 6000),
                     users: int = 256, lat_ticks=(10**9, 10**10), escalate=None, r0: int = 0) -> dict:
    """Builder-defined overload recipe for EXT_HIER at the C5 topology, host
    numpy (the reference has no hierarchy; DESIGN.md §3.8 "Escalations at
    N = 10,000").  Under the reference's stale view a regional broker herds its
    publishes onto its lowest-index node until that node's first completion
    advert arrives (BrokerBaseApp3.cc:123-130, 265-281), and it escalates only
    when every node of its region advertises more than the threshold, so an
    i.i.d. trace needs ~1024^2 publishes per region to saturate one.  This trace
    saturates every region within ~3 publishes per node: each node gets one
    pair -- a short task, then a giant one (giant_s seconds, more than the whole
    filling phase) that reaches it before the short one completes, so its first
    advert carries the giant's backlog -- and zero-service fillers until that
    advert lands; afterwards every publish is a zero-service task escalated to
    the parent's global argmin (the smallest advertised giant).  Publishes every
    ``gap_s`` seconds (plus jitter), regions from :func:`mobility_regions`
    (``users`` users), per-node link latencies in ``lat_ticks``, MIPS
    1000 * (1 + j % 4).  The publish ticks and regions are shared by all
    replications; global replication r0 + i gets its own giants and latencies
    (Philox-free numpy streams keyed by (seed, r0 + i), so a shard equals the
    same rows of the whole job), and its smallest giant sits in region
    3 + (r0 + i) % 7 (B = 10), so escalations land in the wide kernel's upper
    rows.  ``escalate`` ([R] bools, default all): a replication given False
    gets 30-s tasks instead of giants, so its nodes advertise at most 30 s
    (below the bench's 60-s threshold) and no region escalates (the region pass
    finishes it).  Returns host arrays (make_batch layout) + ``region`` [R, T]."""
    tps = TICKS_PER_SECOND_I
    B = -(-N // _abi.HIER_REGION_NODES)
    sizes = [min(_abi.HIER_REGION_NODES, N - b * _abi.HIER_REGION_NODES) for b in range(B)]
    lo, hi = lat_ticks
    shared = np.random.default_rng([seed & 0xFFFFFFFF, T, N])
    g = int(gap_s * tps)
    base = 2 * hi  # after every first advert (init = ul < hi)
    arrive0 = base + np.arange(T, dtype=np.int64) * g + shared.integers(0, g // 2, size=T, dtype=np.int64)
    region0 = mobility_regions(arrive0[None, :], N, users=users)[0]
    role, off, s1 = _saturation_template(arrive0, region0, sizes, 2 * hi)
    k = np.where(off >= 0, region0.astype(np.int64) * _abi.HIER_REGION_NODES + off, 0)
    mips1 = (1000 * (1 + np.arange(N) % 4)).astype(np.int32)
    mk = mips1[k].astype(np.int64)  # [T]: the MIPS of the pair's node
    esc = np.ones(R, bool) if escalate is None else np.asarray(escalate, bool)
    dl = np.empty((R, N), np.int64)
    ul = np.empty((R, N), np.int64)
    req = np.empty((R, T), np.int32)
    for i in range(R):
        rng = np.random.default_rng([seed & 0xFFFFFFFF, r0 + i])
        dl[i] = rng.integers(lo, hi, size=N, dtype=np.int64)
        ul[i] = rng.integers(lo, hi, size=N, dtype=np.int64)
        giant = rng.integers(giant_s[0] + 1, giant_s[1], size=N, dtype=np.int64)
        b = (3 + (r0 + i) % 7) % B  # the smallest giant of this replication
        giant[b * _abi.HIER_REGION_NODES + int(rng.integers(0, sizes[b]))] = giant_s[0]
        if not esc[i]:
            giant[:] = 30
        zero = rng.integers(0, 1000, size=T, dtype=np.int64)  # below every MIPS: zero service
        req[i] = np.where(role == 1, s1 * mk, np.where(role == 2, giant[k] * mk, zero))
    return dict(arrive=np.broadcast_to(arrive0, (R, T)).copy(), req=req, mips=np.broadcast_to(mips1, (R, N)).copy(),
                dl=dl, ul=ul, init=ul.copy(), region=np.broadcast_to(region0, (R, T)).copy())


def power_model(mips) -> tuple[np.ndarray, np.ndarray]:
    """Synthetic node power model for the a11 energy statistic (builder-defined;
    the reference has no fog-node energy model): busy power
    grows with MIPS, idle power is 35% of it.  Same shape as ``mips``."""
    m = np.asarray(mips, dtype=np.float64)
    p_busy = 20.125 + 0.02 * m
    return p_busy, 0.35 * p_busy
