"""Host-side formats on either side of the decision path (include/fognet_io.h).

* :func:`save_trace` / :func:`load_trace` — binary SoA trace files
  ("FOGNTRC1"): node parameters in CONNECT order + the broker-side publish
  trace, the exact inputs of :func:`fognetsimpp_amd.run_batch`.
* :func:`write_sca` / :func:`write_vec` — OMNeT++ 4.6 result files in the
  layout of simulations/example/results/General-0.sca / General-0.vec.
* :func:`gen_trace_mqtt` — the reference task source (mqttApp2.cc:198-409):
  one glibc rand() stream shared by all users in FES order,
  MIPSRequired = 200 + rand() % 701.

All of it is host C++ in libfognet_hip (no GPU, no context).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import FognetError

_NODE_KEYS = (("mips", np.int32), ("dl", np.int64), ("ul", np.int64), ("init", np.int64))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _check(rc: int, what: str):
    if rc != _abi.FOGNET_OK:
        raise FognetError(rc, f"{what}: {_abi.load().fognet_io_last_error().decode()}")


def trace_info(path: str) -> dict:
    info = _abi.TraceInfo()
    _check(_abi.load().fognet_trace_info_read(path.encode(), C.byref(info)), "trace_info")
    return dict(R=info.R, T=info.T, N=info.N, node_stride=info.node_stride, flags=info.flags,
                version=info.version, payload_bytes=info.payload_bytes, checksum=info.checksum,
                note=info.note.decode())


def save_trace(path: str, trace: dict, node_id=None, note: str = "") -> None:
    """Write a trace dict (arrive/req [R, T] or [T]; mips/dl/ul/init [R, N] or
    [N] shared; optional p_busy/p_idle like mips) to ``path``."""
    arrive = np.ascontiguousarray(np.atleast_2d(np.asarray(trace["arrive"])), dtype=np.int64)
    req = np.ascontiguousarray(np.atleast_2d(np.asarray(trace["req"])), dtype=np.int32)
    R, T = arrive.shape
    if req.shape != (R, T):
        raise FognetError(_abi.FOGNET_ERR_ARG, "arrive/req shapes differ")
    nodes = {k: np.ascontiguousarray(trace[k], dtype=dt) for k, dt in _NODE_KEYS}
    shared = nodes["mips"].ndim == 1
    N = nodes["mips"].shape[-1]
    for k, a in nodes.items():
        if a.shape != nodes["mips"].shape or (not shared and a.shape[0] != R):
            raise FognetError(_abi.FOGNET_ERR_ARG, f"{k} has shape {a.shape}")
    pb = pi = None
    if trace.get("p_busy") is not None:
        pb = np.ascontiguousarray(trace["p_busy"], dtype=np.float64)
        pi = np.ascontiguousarray(trace["p_idle"], dtype=np.float64)
    nid = np.ascontiguousarray(node_id, dtype=np.int32) if node_id is not None else None
    bi = _abi.BatchIn(R, T, N, _abi.FOGNET_POLICY_REF_V3, 0 if shared else N, 0,
                      _p(arrive), _p(req), _p(nodes["mips"]), _p(nodes["dl"]), _p(nodes["ul"]), _p(nodes["init"]),
                      _p(pb), _p(pi))
    _check(_abi.load().fognet_trace_write(path.encode(), C.byref(bi), _p(nid), note.encode()), "save_trace")


def load_trace(path: str) -> dict:
    """Read a trace file into numpy arrays (the save_trace layout; node arrays
    are [N] when the file stores them shared).  Verifies the checksum."""
    info = trace_info(path)
    R, T, N, stride = info["R"], info["T"], info["N"], info["node_stride"]
    nshape = (R, N) if stride else (N,)
    out = {"arrive": np.empty((R, T), np.int64), "req": np.empty((R, T), np.int32)}
    for k, dt in _NODE_KEYS:
        out[k] = np.empty(nshape, dt)
    pw = bool(info["flags"] & _abi.TRACE_FLAG_POWER)
    if pw:
        out["p_busy"] = np.empty(nshape, np.float64)
        out["p_idle"] = np.empty(nshape, np.float64)
    nid = np.empty(nshape, np.int32) if info["flags"] & _abi.TRACE_FLAG_NODE_ID else None
    bi = _abi.BatchIn(0, 0, 0, 0, 0, 0, _p(out["arrive"]), _p(out["req"]), _p(out["mips"]), _p(out["dl"]),
                      _p(out["ul"]), _p(out["init"]), _p(out.get("p_busy")), _p(out.get("p_idle")))
    _check(_abi.load().fognet_trace_read(path.encode(), C.byref(bi), _p(nid)), "load_trace")
    if nid is not None:
        out["node_id"] = nid
    out["note"] = info["note"]
    return out


def write_sca(path: str, job, hist=None, run_id: str = "General-0-fognet", network: str = "FogNet") -> None:
    """OMNeT++ .sca of a job record (JOB_STATS_DTYPE) and optional histogram [2, 64]."""
    js = _abi.JobStats.from_buffer_copy(np.ascontiguousarray(job).tobytes())
    h = np.ascontiguousarray(hist, dtype=np.int64) if hist is not None else None
    if h is not None and h.shape != (_abi.HIST_METRICS, _abi.HIST_BINS):
        raise FognetError(_abi.FOGNET_ERR_ARG, f"hist shape {h.shape}")
    _check(_abi.load().fognet_write_sca(path.encode(), run_id.encode(), network.encode(), C.byref(js), _p(h)),
           "write_sca")


def write_sca_nodes(path: str, nodes, node_id=None, append: bool = False, run_id: str = "General-0-fognet",
                    network: str = "FogNet") -> None:
    """Per-node `.sca` blocks of NODE_STATS_DTYPE records [N] (fognet_write_sca_nodes):
    one module <network>.fogNode[<node_id or index>].udpApp[0] each.  ``append``: add
    them to the file :func:`write_sca` wrote instead of starting a new one."""
    rec = np.ascontiguousarray(nodes, dtype=_abi.NODE_STATS_DTYPE).reshape(-1)
    nid = np.ascontiguousarray(node_id, dtype=np.int32).reshape(-1) if node_id is not None else None
    if nid is not None and nid.size != rec.size:
        raise FognetError(_abi.FOGNET_ERR_ARG, "write_sca_nodes: node_id length differs from the records'")
    _check(_abi.load().fognet_write_sca_nodes(path.encode(), run_id.encode(), network.encode(), rec.size, _p(rec),
                                              _p(nid), 1 if append else 0), "write_sca_nodes")


def write_sca_queue(path: str, queue, levels, node_id=None, append: bool = False, run_id: str = "General-0-fognet",
                    network: str = "FogNet") -> None:
    """Per-node queue scalars of QUEUE_STATS_DTYPE records [N] (fognet_write_sca_queue) under
    <network>.fogNode[<node_id or index>].udpApp[0]: queueLength:max, :enqueued, :timeavg and one
    :ge<level> per entry of ``levels`` (the levels of the call that made the records).  ``append``:
    add them to the file :func:`write_sca` wrote instead of starting a new one."""
    rec = np.ascontiguousarray(queue, dtype=_abi.QUEUE_STATS_DTYPE).reshape(-1)
    lv = np.ascontiguousarray(levels, dtype=np.int64).reshape(-1)
    nid = np.ascontiguousarray(node_id, dtype=np.int32).reshape(-1) if node_id is not None else None
    if nid is not None and nid.size != rec.size:
        raise FognetError(_abi.FOGNET_ERR_ARG, "write_sca_queue: node_id length differs from the records'")
    _check(_abi.load().fognet_write_sca_queue(path.encode(), run_id.encode(), network.encode(), rec.size, _p(rec),
                                              _p(lv), lv.size, _p(nid), 1 if append else 0), "write_sca_queue")


def write_sca_compare(path: str, job, hist=None, module: str | None = None, append: bool = False,
                      run_id: str = "General-0-fognet", network: str = "FogNet") -> None:
    """`.sca` block of one COMPARE_STATS_DTYPE job record (fognet_write_sca_compare) under ``module``
    (default <network>.compare): the compare:* scalars, startDiff / serviceDiff / responseDiff
    statistics in ms and, with ``hist`` (int64 [2, 64]), the earlier / later histograms.
    ``append``: add it to the file :func:`write_sca` wrote instead of starting a new one."""
    rec = np.ascontiguousarray(job, dtype=_abi.COMPARE_STATS_DTYPE).reshape(-1)
    if rec.size != 1:
        raise FognetError(_abi.FOGNET_ERR_ARG, "write_sca_compare: one job record")
    h = np.ascontiguousarray(hist, dtype=np.int64).reshape(-1) if hist is not None else None
    if h is not None and h.size != 2 * _abi.HIST_BINS:
        raise FognetError(_abi.FOGNET_ERR_ARG, f"write_sca_compare: hist is int64 [2, {_abi.HIST_BINS}]")
    c = _abi.CompareStats.from_buffer_copy(rec.tobytes())
    _check(_abi.load().fognet_write_sca_compare(path.encode(), run_id.encode(), network.encode(),
                                                module.encode() if module is not None else None, C.byref(c), _p(h),
                                                1 if append else 0), "write_sca_compare")


def write_sca_groups(path: str, groups, module=None, append: bool = False, run_id: str = "General-0-fognet",
                     network: str = "FogNet") -> None:
    """`.sca` blocks of GROUP_STATS_DTYPE records [G] (fognet_write_sca_groups): per group the
    replication counts and one `<metric>:replications` statistic per metric across its
    replications, under ``module[g]`` (default <network>.replications for one record, else
    <network>.group[g]).  ``append``: add them to the file :func:`write_sca` wrote."""
    rec = np.ascontiguousarray(groups, dtype=_abi.GROUP_STATS_DTYPE).reshape(-1)
    names = None
    if module is not None:
        mods = [str(m).encode() for m in module]
        if len(mods) != rec.size:
            raise FognetError(_abi.FOGNET_ERR_ARG, "write_sca_groups: module length differs from the records'")
        names = (C.c_char_p * len(mods))(*mods)
    _check(_abi.load().fognet_write_sca_groups(path.encode(), run_id.encode(), network.encode(), rec.size, _p(rec),
                                               C.cast(names, C.c_void_p) if names is not None else None,
                                               1 if append else 0), "write_sca_groups")


def write_sca_users(path: str, users, user_module=None, append: bool = False, run_id: str = "General-0-fognet",
                    network: str = "FogNet") -> None:
    """Per-user `.sca` blocks of USER_STATS_DTYPE records [U] (fognet_write_sca_users):
    `latency`, `latencyH1` and `taskTime` under <network>.<user_module[u] or "user[u]">.udpApp[0]
    each, then the broker's `delay` from the merge of the records.  ``append``: add them to
    the file :func:`write_sca` wrote instead of starting a new one."""
    rec = np.ascontiguousarray(users, dtype=_abi.USER_STATS_DTYPE).reshape(-1)
    names = None
    if user_module is not None:
        mods = [str(m).encode() for m in user_module]
        if len(mods) != rec.size:
            raise FognetError(_abi.FOGNET_ERR_ARG, "write_sca_users: user_module length differs from the records'")
        names = (C.c_char_p * len(mods))(*mods)
    _check(_abi.load().fognet_write_sca_users(path.encode(), run_id.encode(), network.encode(), rec.size, _p(rec),
                                              C.cast(names, C.c_void_p) if names is not None else None,
                                              1 if append else 0), "write_sca_users")


def write_vec(path: str, arrive, dl, node, status, start, node_id=None, run_id: str = "General-0-fognet",
              network: str = "FogNet") -> None:
    """OMNeT++ .vec of ONE replication: arrive/node/status/start [T], dl [N]."""
    a = np.ascontiguousarray(arrive, dtype=np.int64).reshape(-1)
    d = np.ascontiguousarray(dl, dtype=np.int64).reshape(-1)
    n = np.ascontiguousarray(node, dtype=np.int32).reshape(-1)
    s = np.ascontiguousarray(status, dtype=np.uint8).reshape(-1)
    st = np.ascontiguousarray(start, dtype=np.int64).reshape(-1)
    nid = np.ascontiguousarray(node_id, dtype=np.int32).reshape(-1) if node_id is not None else None
    T, N = a.size, d.size
    if not (n.size == s.size == st.size == T) or (nid is not None and nid.size != N):
        raise FognetError(_abi.FOGNET_ERR_ARG, "write_vec: array lengths differ")
    _check(_abi.load().fognet_write_vec(path.encode(), run_id.encode(), network.encode(), T, N, _p(a), _p(d), _p(n),
                                        _p(s), _p(st), _p(nid)), "write_vec")


def write_vec_users(path: str, offset, time, value, U: int, id_base: int = 0, user_module=None, append: bool = False,
                    run_id: str = "General-0-fognet", network: str = "FogNet") -> None:
    """The user-side vectors of ONE replication as an OMNeT++ `.vec` (fognet_write_vec_users):
    ``offset`` is the replication's offset row from the `delay` vector on (``row[N:]``, 3U + 2
    entries), ``time`` / ``value`` its rows (engine.signal_vectors, copied to the host).
    ``append``: add the vectors to the file :func:`write_vec` wrote (``id_base`` = N + 1)."""
    off = np.ascontiguousarray(offset, dtype=np.int64).reshape(-1)
    t = np.ascontiguousarray(time, dtype=np.int64).reshape(-1)
    v = np.ascontiguousarray(value, dtype=np.int64).reshape(-1)
    if U < 0 or off.size != 3 * U + 2 or t.size != v.size or (off.size and int(off.max()) > t.size):
        raise FognetError(_abi.FOGNET_ERR_ARG, "write_vec_users: offset must hold 3U + 2 entries within time / value")
    names = None
    if user_module is not None:
        mods = [str(m).encode() for m in user_module]
        if len(mods) != U:
            raise FognetError(_abi.FOGNET_ERR_ARG, "write_vec_users: user_module length differs from U")
        names = (C.c_char_p * len(mods))(*mods)
    _check(_abi.load().fognet_write_vec_users(path.encode(), run_id.encode(), network.encode(), U, id_base, _p(off),
                                              _p(t), _p(v), C.cast(names, C.c_void_p) if names is not None else None,
                                              1 if append else 0), "write_vec_users")


def write_vec_windows(path: str, job, N: int, t0: int, window: int, replications: int, id_base: int = 0,
                      append: bool = False, run_id: str = "General-0-fognet", network: str = "FogNet") -> None:
    """A job's window records (WINDOW_STATS_DTYPE [W], the merge of ``replications`` replications of
    ``N`` nodes) as fourteen OMNeT++ `.vec` vectors with a row per window at its end time
    (fognet_write_vec_windows): utilisation, tasks in system, completions, publishes, and the mean
    and count of the five signals.  ``append``: add the vectors to a file :func:`write_vec` /
    :func:`write_vec_users` wrote (``id_base``: the first free vector id)."""
    rec = np.ascontiguousarray(job, dtype=_abi.WINDOW_STATS_DTYPE).reshape(-1)
    _check(_abi.load().fognet_write_vec_windows(path.encode(), run_id.encode(), network.encode(), N, rec.size, t0, window,
                                                replications, _p(rec), id_base, 1 if append else 0), "write_vec_windows")


def write_sca_quantiles(path: str, ppm, value, count, modules=None, append: bool = False,
                        run_id: str = "General-0-fognet", network: str = "FogNet") -> None:
    """A job's quantiles (``ppm`` [Q] ranks, ``value`` [5, Q] raw, ``count`` [5]; engine.job_quantiles)
    as OMNeT++ `.sca` scalars ``"<signal>:p<percent>"`` in recorded units (fognet_write_sca_quantiles).
    ``modules``: the five module paths (default: the window vectors' modules); ``append``: add the
    lines to an existing `.sca`."""
    ranks = np.ascontiguousarray(ppm, dtype=np.int32).reshape(-1)
    val = np.ascontiguousarray(value, dtype=np.int64).reshape(-1)
    cnt = np.ascontiguousarray(count, dtype=np.int64).reshape(-1)
    if val.size != _abi.QUANTILE_SIGNALS * ranks.size or cnt.size != _abi.QUANTILE_SIGNALS:
        raise FognetError(_abi.FOGNET_ERR_ARG, "write_sca_quantiles: value must be [5, Q] and count [5]")
    mods = None
    if modules is not None:
        if len(modules) != _abi.QUANTILE_SIGNALS:
            raise FognetError(_abi.FOGNET_ERR_ARG, "write_sca_quantiles: five module paths")
        mods = (C.c_char_p * _abi.QUANTILE_SIGNALS)(*(m.encode() for m in modules))
    _check(_abi.load().fognet_write_sca_quantiles(path.encode(), run_id.encode(), network.encode(), mods, ranks.size,
                                                  _p(ranks), _p(val), _p(cnt), 1 if append else 0), "write_sca_quantiles")


def gen_trace_mqtt(seed: int, start, interval, uplink, downlink, stop: int, req_base: int = 200, req_span: int = 701,
                   cap: int | None = None) -> dict:
    """Reference task source (fognet_gen_trace_mqtt): per-user tick arrays
    start/interval/uplink/downlink (downlink < 0: no CONNACK); returns
    arrive [T] (broker arrival ticks), req [T], user [T]."""
    st, iv, up, dn = (np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in (start, interval, uplink, downlink))
    U = st.size
    if not (iv.size == up.size == dn.size == U):
        raise FognetError(_abi.FOGNET_ERR_ARG, "per-user arrays differ in length")
    if U and (iv.min() <= 0 or st.min() < 0 or up.min() < 0):
        raise FognetError(_abi.FOGNET_ERR_ARG, "need start >= 0, interval > 0, uplink >= 0")
    if cap is None:  # upper bound: CONNACK + every timer before stop
        span = np.maximum(stop - st, 0)
        cap = int((span // iv + 2).sum()) if U else 0
    arrive = np.empty(cap, np.int64)
    req = np.empty(cap, np.int32)
    user = np.empty(cap, np.int32)
    t = C.c_int32(0)
    _check(_abi.load().fognet_gen_trace_mqtt(seed & 0xFFFFFFFF, U, _p(st), _p(iv), _p(up), _p(dn), int(stop), req_base,
                                             req_span, cap, _p(arrive), _p(req), _p(user), C.byref(t)),
           "gen_trace_mqtt")
    n = t.value
    return dict(arrive=arrive[:n], req=req[:n], user=user[:n])
