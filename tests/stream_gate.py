"""A stream gate: makes work that went to the wrong stream show up as wrong bytes
(test infrastructure for tests/test_streams_gpu.py; needs a GPU).

Every test of the library but that file runs on the null stream, where a kernel, a
clear or a copy enqueued on another stream than the caller's is still ordered, and a
host-side wait inside an enqueue-only call cannot be seen.  Here the calls under test
are enqueued on a side stream S behind a gate:

1. On the default stream the case's real inputs are kept in plain device tensors and
   the views the library will read are filled with a *decoy*: a valid input set of the
   same shapes from another seed (not poison: a kernel that ran too early must compute
   a wrong answer, not index memory by garbage).  ``torch.cuda.synchronize()``.
2. On S: ``torch.cuda._sleep(cycles)`` (the gate), device-to-device copies of the real
   inputs over the decoy, an optional dirtying job, then the calls under test.
3. Among those, one copy of an input view into a probe tensor goes, on purpose, to the
   default stream: the control.
4. Right after the last call returns ``S.query()`` must be false: the calls only
   enqueued, and every launch was submitted while the gate still held S.  After
   ``S.synchronize()`` the probe must hold the decoy: work on another stream did run
   ahead of the gate where the tests run, so a launch on the wrong stream would have read
   the decoy as well (the gate has power).

The gate's length is measured, not chosen: ``_sleep`` cycles per millisecond from two
events, the host-side submission time of the same sequence without the gate, and a gate
of FACTOR times that (the only requirement is that it outlasts the submission, which
step 4 asserts; the factor covers first-use jitter), at most MAX_GATE_MS and at least
MIN_GATE_MS (a pause of the host between two launches, such as a garbage collection, is
not 100 times shorter than a submission of 50 us; a longer gate hides nothing, since a
call that waits for the device waits for the gate whatever its length).  Which
hardware queue a stream gets is the runtime's choice, so the side stream is chosen once
from up to CANDIDATES fresh streams: the first whose control shows power.  The
measurements (submission time and gate per case and per case kind, the candidates) are
written to the file FOGNET_STREAM_GATE_REPORT names, by default build/stream_gate.json.
"""
from __future__ import annotations

import json
import os
import time
from dataclasses import dataclass, field
from typing import Callable

import numpy as np
import torch

FACTOR = 100
MAX_GATE_MS = 500.0
MIN_GATE_MS = 20.0
CANDIDATES = 4
REPORT_ENV = "FOGNET_STREAM_GATE_REPORT"
DEFAULT_REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "stream_gate.json")


def _same(a: torch.Tensor, b) -> bool:
    """Byte equality of a tensor and a tensor or host array (NaNs compare by their bits)."""
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.ascontiguousarray(b)
    return a.cpu().numpy().tobytes() == b.tobytes()


class NoPower(Exception):
    """No candidate stream let default-stream work run ahead of the gate."""


def calibrate(device) -> float:
    """``torch.cuda._sleep`` cycles per millisecond, from two events (a sleep of at least 5 ms)."""
    with torch.cuda.device(device):
        torch.cuda._sleep(1000)  # first use
        torch.cuda.synchronize()
        n = 1_000_000
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(n)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0 or n >= 10**11:
                return n / max(ms, 1e-3)
            n *= 10


@dataclass
class Lane:
    """One gated sequence: ``make()`` builds a fresh job on the default stream (an object
    whose ``inputs`` maps names to the device views the calls read, holding the real
    inputs), ``decoys`` maps the same names to host arrays of the same shape and dtype,
    ``enqueue(job)`` issues the calls under test on the current stream, ``dirty()`` (optional)
    a job whose outputs are discarded, issued just before them."""
    stream: torch.cuda.Stream
    make: Callable
    decoys: dict
    enqueue: Callable
    dirty: Callable | None = None
    job: object = None
    real: dict = field(default_factory=dict)
    probe_name: str = ""
    probe: torch.Tensor | None = None

    def stage(self):
        """Step 1 (default stream; the caller synchronises)."""
        self.job = self.make()
        views = self.job.inputs
        assert set(views) == set(self.decoys), (sorted(views), sorted(self.decoys))
        self.real = {k: v.clone() for k, v in views.items()}
        self.probe_name = ""
        for k, v in views.items():
            src = torch.from_numpy(np.ascontiguousarray(self.decoys[k]))
            assert src.dtype == v.dtype and tuple(src.shape) == tuple(v.shape), (k, src.dtype, v.dtype, src.shape, v.shape)
            if not self.probe_name and not _same(src, self.real[k]):
                self.probe_name = k  # the control copies a view whose decoy differs from the real input
            v.copy_(src)
        assert self.probe_name, "the decoy equals the real inputs"
        self.probe = torch.zeros_like(self.real[self.probe_name])

    def submit(self, cycles: int):
        """Steps 2 and 3; returns nothing and waits for nothing."""
        views = self.job.inputs
        dev = self.probe.device
        with torch.cuda.stream(self.stream):
            if cycles:
                torch.cuda._sleep(cycles)
            for k, v in views.items():
                v.copy_(self.real[k], non_blocking=True)
            with torch.cuda.stream(torch.cuda.default_stream(dev)):  # the control
                self.probe.copy_(views[self.probe_name], non_blocking=True)
            if self.dirty is not None:
                self.dirty()
            self.enqueue(self.job)

    def has_power(self) -> bool:
        """After the streams have finished: the control read the decoy."""
        if _same(self.probe, self.decoys[self.probe_name]):
            return True
        assert _same(self.probe, self.real[self.probe_name]), "the control holds neither the decoy nor the real input"
        return False


class Gate:
    def __init__(self, device):
        self.device = torch.device(device)
        self.cycles_per_ms = calibrate(self.device)
        self.stream: torch.cuda.Stream | None = None
        self.streams: list = []
        self.report: dict = {"cycles_per_ms": self.cycles_per_ms, "factor": FACTOR, "max_gate_ms": MAX_GATE_MS,
                             "min_gate_ms": MIN_GATE_MS, "candidates": [], "kinds": {}, "cases": {}}

    # ------------------------------------------------------------ the side stream
    def choose(self, want: int = 2) -> torch.cuda.Stream:
        """Up to ``want`` of CANDIDATES fresh streams whose control shows power, chosen once per
        module: ``stream`` is the first of them, ``streams`` all (a test that gates two streams
        at once needs two).  Every candidate stays alive, so the runtime's mapping of streams
        to hardware queues does not change under the tests."""
        src = np.arange(256, dtype=np.int64)

        class _Job:
            def __init__(self, dev):
                self.inputs = {"x": torch.from_numpy(src).to(dev)}
        self.streams, self._tried = [], []
        for i in range(CANDIDATES):
            s = torch.cuda.Stream(self.device)
            self._tried.append(s)
            lane = Lane(s, lambda: _Job(self.device), {"x": src + 1}, lambda job: None)
            power = self._run([lane], "candidate", f"candidate-{i}", require_power=False)
            self.report["candidates"].append({"index": i, "power": bool(power)})
            if power:
                self.streams.append(s)
                self.report.setdefault("used", []).append(i)
            self.write()
            if len(self.streams) == want:
                break
        if not self.streams:
            raise NoPower(f"none of {CANDIDATES} side streams let default-stream work run ahead of a gated stream")
        self.stream = self.streams[0]
        return self.stream

    # ------------------------------------------------------------ one gated run
    def run(self, kind: str, label: str, make, decoys, enqueue, dirty=None, stream=None, **kw):
        """Gate one sequence on the chosen stream (or ``stream``); returns the job of the gated run."""
        lane = Lane(stream or self.stream, make, decoys, enqueue, dirty)
        self._run([lane], kind, label, **kw)
        return lane.job

    def run_lanes(self, kind: str, label: str, lanes: list, **kw):
        self._run(lanes, kind, label, **kw)
        return [l.job for l in lanes]

    def _run(self, lanes, kind, label, require_power=True, also=(), during=None, final_check=True):
        """``also``: further streams that must still be busy after the last enqueue (streams the
        lanes' own calls order behind the gate).  ``during(check)``: host-side work done while the
        gate holds, after the last enqueue; ``check()`` asserts that the gate still holds.
        ``final_check=False``: no assertion after ``during`` returned (it may legitimately wait)."""
        streams = [l.stream for l in lanes]

        def finish():
            for s in streams:
                s.synchronize()
            torch.cuda.synchronize(self.device)

        # the submission time of the same sequence without the gate
        for l in lanes:
            l.stage()
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        for l in lanes:
            l.submit(0)
        if during is not None:
            during(lambda: None)
        submit_ms = (time.perf_counter() - t0) * 1e3
        finish()
        gate_ms = min(MAX_GATE_MS, max(MIN_GATE_MS, FACTOR * submit_ms))
        cycles = max(1, int(gate_ms * self.cycles_per_ms))

        # the gated run, on fresh buffers
        for l in lanes:
            l.stage()
        torch.cuda.synchronize(self.device)

        def check():
            idle = [i for i, s in enumerate(list(streams) + list(also)) if s.query()]
            assert not idle, (f"{label}: stream(s) {idle} had nothing left to do when the last call returned: a call "
                              f"waited for the device, or the gate of {gate_ms:.1f} ms (submission {submit_ms:.3f} ms "
                              f"ungated) did not outlast the submission")
        t0 = time.perf_counter()
        for l in lanes:
            l.submit(cycles)
        gated_submit_ms = (time.perf_counter() - t0) * 1e3
        try:
            if during is not None:
                during(check)
            if final_check:
                check()
        finally:
            finish()
        power = all([l.has_power() for l in lanes])
        rec = {"kind": kind, "submit_ms": round(submit_ms, 4), "gate_ms": round(gate_ms, 3),
               "gated_submit_ms": round(gated_submit_ms, 4), "power": bool(power)}
        self.report["cases"][label] = rec
        k = self.report["kinds"].setdefault(kind, {"cases": 0, "submit_ms_max": 0.0, "gate_ms_max": 0.0})
        k["cases"] += 1
        k["submit_ms_max"] = max(k["submit_ms_max"], rec["submit_ms"])
        k["gate_ms_max"] = max(k["gate_ms_max"], rec["gate_ms"])
        self.write()
        if require_power:
            assert power, (f"{label}: the control on the default stream read the real input: nothing ran ahead of "
                           f"the gate, so this run could not have seen a launch on the wrong stream")
        return power

    def write(self):
        try:
            path = os.path.abspath(os.environ.get(REPORT_ENV) or DEFAULT_REPORT)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                json.dump(self.report, f, indent=1, sort_keys=True)
        except OSError:
            pass  # (a read-only checkout: the report is a by-product)
