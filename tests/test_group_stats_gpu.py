"""Replication groups on the device (fognet_reduce_groups_dev), byte for byte against the
Python-integer restatement (group_ref) on uploaded crafted records, and against the whole-job
reduction on real replays.  The pass reads the [R] records alone, so most cases need no replay."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import group_ref as gr
import stream_gate
import tracegen as tg
from fognetsimpp_amd import _abi, formats
from guarded import Arena
from test_compare_stats_gpu import finish_the_rotation
from test_group_stats import JOB_INT_FIELDS, assert_job_equal

pytestmark = pytest.mark.gpu

GRP, REP = _abi.GROUP_STATS_DTYPE, _abi.REP_STATS_DTYPE
NMET = len(_abi.REP_METRICS)
ENV = "FOGNET_GROUP_STATS"


def dev_of(ctx):
    return torch.device("cuda", ctx.device)


def upload(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def raw_call(ctx, stats, R, group_of, G, out, metrics=None, defined=None, n_ungrouped=None, stream=None):
    """The entry point itself, enqueued on the current stream (no host synchronisation)."""
    p = fa.engine._ptr
    dev = out.device if out is not None else dev_of(ctx)
    return ctx._lib.fognet_reduce_groups_dev(ctx.handle, p(stats), R, p(group_of), G, p(out), p(metrics), p(defined),
                                             p(n_ungrouped), stream if stream is not None else fa.engine._stream_ptr(dev))


def memberships(R: int, G: int, rng) -> dict:
    """The issue's memberships of R replications in G groups (None: a NULL group_of)."""
    block = -(-max(R, 1) // G)   # contiguous blocks of equal length
    mixed = rng.integers(0, G, R)
    mixed[rng.random(R) < 0.2] = -1
    mixed[rng.random(R) < 0.2] = G
    return {"one": np.full(R, G - 1), "mod": np.arange(R) % G, "blocks": np.arange(R) // block,
            "random": rng.integers(0, G, R), "null": None, "out_of_range": mixed,
            "all_out": rng.choice(np.array([-1, G, G + 5, -2**31, 2**31 - 1]), R)}


_cache: dict = {}


def crafted(R: int):
    """(records, their rows for group_ref.reduce_rows, the metrics table and defined words), once per R."""
    if R not in _cache:
        reps = gr.crafted(R, seed=R + 1)
        met = [gr.metrics_row(x) for x in reps]
        _cache[R] = (reps, gr.rows(reps), np.array([m[0] for m in met], np.int64).reshape(R, NMET),
                     np.array([m[1] for m in met], np.uint32))
    return _cache[R]


# ---------------------------------------------------------------- crafted records: every shape

@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 9000])
def test_device_bytes_equal_the_restatement(ctx, monkeypatch, R):
    """Every G and membership, with the accumulators in LDS and forced into the caller's records, with and
    without the metrics table: out [G], metrics [R][9], defined [R] and n_ungrouped equal the restatement."""
    dev = dev_of(ctx)
    reps, rws, want_met, want_def = crafted(R)
    stats = upload(reps.view(np.uint8).reshape(-1), dev) if R else torch.empty(0, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(1000 + R)
    for G in (1, 2, 9, 64, 65, 1000):
        out = torch.empty(G * GRP.itemsize, dtype=torch.uint8, device=dev)
        for name, of in memberships(R, G, rng).items():
            want, want_lost = gr.reduce_rows(rws, of, G)
            gof = upload(of.astype(np.int32), dev) if of is not None else None
            for hbm in (False, True):
                monkeypatch.setenv(ENV, "hbm") if hbm else monkeypatch.delenv(ENV, raising=False)
                for with_metrics in (False, True):
                    out.fill_(0xEE)
                    met = torch.full((R, NMET), 0x7E7E7E7E, dtype=torch.int64, device=dev) if with_metrics else None
                    dfn = torch.full((max(R, 1),), 0x7E7E7E7E, dtype=torch.int32, device=dev) if with_metrics else None
                    ung = torch.full((1,), -77, dtype=torch.int64, device=dev)
                    ctx.check(raw_call(ctx, stats, R, gof, G, out, met, dfn, ung), "reduce_groups")
                    what = (R, G, name, "hbm" if hbm else "lds", with_metrics)
                    assert out.cpu().numpy().tobytes() == want, what
                    assert int(ung.item()) == want_lost, what
                    if with_metrics:
                        assert np.array_equal(met.cpu().numpy(), want_met), what
                        assert np.array_equal(dfn[:R].cpu().numpy().view(np.uint32), want_def), what
    monkeypatch.delenv(ENV, raising=False)
    if R >= 257:   # the crafted set holds what it says: failures at the wavefront and workgroup edges
        st = reps["status"]
        assert st[0] != 0 and st[63] == st[64] == st[255] == gr.REF_ABORTED and st[256] != 0 and st[R - 1] != 0
        assert (want_def == 0).sum() == (st != 0).sum() and len(set(want_def.tolist())) > 4


def test_python_binding_and_two_calls_give_identical_bytes(ctx):
    dev = dev_of(ctx)
    R = 4097
    reps, rws, want_met, want_def = crafted(R)
    stats = upload(reps.view(np.uint8).reshape(-1), dev)
    of = np.arange(R) % 9
    of[5::50] = 9
    want, lost = gr.reduce_rows(rws, of, 9)
    first = fa.reduce_groups(ctx, stats, R, of, G=9, metrics=True)
    second = fa.reduce_groups(ctx, stats, R, torch.from_numpy(of.astype(np.int32)).to(dev), G=9, metrics=True)
    for rec, ung, met, dfn in (first, second):
        assert rec.tobytes() == want and ung == lost and rec.dtype == GRP and rec.shape == (9,)
        assert np.array_equal(met, want_met) and np.array_equal(dfn, want_def)
    rec, ung = fa.reduce_groups(ctx, stats, R)   # NULL group_of, G = 1
    assert rec.tobytes() == gr.reduce_rows(rws, None, 1)[0] and ung == 0
    assert fa.merge_group_stats(first[0]).tobytes() == gr.reduce_rows(rws, np.where(of < 9, 0, 1), 1)[0]
    with pytest.raises(fa.FognetError):
        fa.reduce_groups(ctx, stats, R, of[:-1], G=9)


# ---------------------------------------------------------------- real replays

def by_group(ctx, out, R, of, G):
    """The device's group records, and per group fa.reduce_stats over the members' records gathered
    into a buffer of their own."""
    rec, lost = fa.reduce_groups(ctx, out.stats, R, of, G=G)
    assert lost == 0
    st = out.rep_stats()
    assert rec.tobytes() == gr.reduce_rows(gr.rows(st), of, G)[0]
    dev = out.stats.device
    for g in range(G):
        idx = np.flatnonzero(np.asarray(of) == g) if of is not None else np.arange(R)
        gathered = upload(st[idx].view(np.uint8).reshape(-1), dev) if len(idx) else torch.empty(0, dtype=torch.uint8, device=dev)
        want = fa.reduce_stats(ctx, gathered, len(idx))
        # |dE| <= members * 0.5 uJ (the rounding to microjoules) + 1e-9 |E| (the header's bound for another order)
        assert_job_equal(fa.group_job(rec[g]), want, len(idx), g)
        assert int(want["n_reps"]) == len(idx)
    return rec, st


def test_c3_shape_by_its_nine_points(ctx):
    """C3 in small: R = 27 over sweep_params' nine points, T = 300, N = 8, a power model, one replication
    made to fail; every point's job record equals the plain reduction of its three replications."""
    R, T, N = 27, 300, 8
    tr = tg.make_batch(0x63, R, N, T, sweep=True)
    tr["mips"][13, 2] = 0   # replication 13 is refused: a node that cannot serve
    pb, pi = fa.power_model(tr["mips"])
    dev = dev_of(ctx)
    out = fa.run_batch(ctx, fa.as_device_trace(dict(tr, p_busy=pb, p_idle=pi), dev))
    torch.cuda.synchronize()
    of = np.arange(R) % 9
    rec, st = by_group(ctx, out, R, of, 9)
    assert st["status"][13] != 0 and (np.delete(st["status"], 13) == 0).all()
    assert rec["n_reps"].tolist() == [3] * 9 and rec["n_failed"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert rec["across"]["count"][:, 0].tolist() == [3, 3, 3, 3, 2, 3, 3, 3, 3]
    assert (rec["across"]["sum_lo"][:, 8] > 0).all()   # E != 0: the energy bound is not vacuous
    whole, _ = by_group(ctx, out, R, None, 1)            # G = 1 equals the whole-job reduction the same way
    assert fa.merge_group_stats(rec).tobytes() == whole[0].tobytes()
    s = fa.summarize_group(rec[0])
    assert s["replications"] == 3 and s["replications_by_metric"]["respMean_ms"]["count"] == 3


def test_generated_replay(ctx):
    """A generated replay (no per-task output exists): R = 64 over the nine sweep points, with energy."""
    R, T, N = 64, 500, 16
    dev = dev_of(ctx)
    mg, sc = fa.sweep_params(np.arange(R), N)
    pb, pi = fa.power_model(1000 * (1 + np.arange(N) % 4))
    power = tuple(upload(x, dev) for x in (pb, pi))
    out = fa.run_generated(ctx, 0x5EED0004, R, T, N, mg, sc, power=power, hist=False)
    torch.cuda.synchronize()
    rec, st = by_group(ctx, out, R, np.arange(R) % 9, 9)
    assert (st["status"] == 0).all() and float(st["energy_j"].min()) > 0
    assert rec["n_reps"].tolist() == [8] + [7] * 8
    by_group(ctx, out, R, None, 1)


# ---------------------------------------------------------------- the buffer contract

@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "natural"])
def test_guard_bands_poisoned_buffers_and_natural_alignment(ctx, monkeypatch, misalign):
    """Every array between guard bands in arenas of two poisons: nothing outside the views changes, the
    outputs equal the restatement under both poisons (so none depends on what it held), also where the
    views have only their element's natural alignment."""
    R, G = 321, 9
    reps, rws, want_met, want_def = crafted(R)
    of = np.arange(R) % (G + 1) - (np.arange(R) % 17 == 0)   # -1 and G among them
    want, want_lost = gr.reduce_rows(rws, of, G)
    seen = set()
    for poison in (0xA5, 0x5A):
        for hbm in (False, True):
            monkeypatch.setenv(ENV, "hbm") if hbm else monkeypatch.delenv(ENV, raising=False)
            arena = Arena(dev_of(ctx), poison, 1 << 20)
            stats = arena.put(reps.view(np.int64).reshape(-1), misalign, "stats")
            gof = arena.put(of.astype(np.int32), misalign, "group_of")
            out = arena.alloc(G * GRP.itemsize // 8, torch.int64, misalign, "out")
            met = arena.alloc((R, NMET), torch.int64, misalign, "metrics")
            dfn = arena.alloc(R, torch.int32, misalign, "defined")
            ung = arena.alloc(1, torch.int64, misalign, "n_ungrouped")
            ctx.check(raw_call(ctx, stats, R, gof, G, out, met, dfn, ung), "reduce_groups")
            torch.cuda.synchronize()
            arena.check()
            got = out.cpu().numpy().tobytes()
            assert got == want and int(ung.item()) == want_lost
            assert np.array_equal(met.cpu().numpy(), want_met) and np.array_equal(dfn.cpu().numpy().view(np.uint32), want_def)
            assert stats.cpu().numpy().tobytes() == reps.tobytes() and np.array_equal(gof.cpu().numpy(), of)  # inputs unchanged
            seen.add(got)
    assert len(seen) == 1


def test_refused_calls_write_nothing(ctx):
    dev = dev_of(ctx)
    R, G = 10, 3
    reps = crafted(63)[0][:R]
    stats = upload(reps.view(np.uint8).reshape(-1), dev)
    out = torch.full((G * GRP.itemsize,), 0xCD, dtype=torch.uint8, device=dev)
    met = torch.full((R, NMET), 0x0123456789ABCDEF, dtype=torch.int64, device=dev)
    dfn = torch.full((R,), 0x1234567, dtype=torch.int32, device=dev)
    ung = torch.full((1,), 0x0123456789ABCDEF, dtype=torch.int64, device=dev)
    gof = upload(np.zeros(R, np.int32), dev)
    E = _abi.FOGNET_ERR_ARG
    assert raw_call(ctx, stats, R, gof, 0, out, met, dfn, ung) == E
    assert raw_call(ctx, stats, R, gof, -1, out, met, dfn, ung) == E
    assert raw_call(ctx, stats, R, gof, G, None, met, dfn, ung) == E
    assert raw_call(ctx, None, R, gof, G, out, met, dfn, ung) == E
    assert raw_call(ctx, stats, -1, gof, G, out, met, dfn, ung) == E
    assert ctx._lib.fognet_reduce_groups_dev(None, None, 0, None, 1, None, None, None, None, None) == E
    torch.cuda.synchronize()
    assert bytes(out.cpu().numpy()) == b"\xCD" * out.numel()
    assert bool((met == 0x0123456789ABCDEF).all()) and bool((dfn == 0x1234567).all()) and int(ung.item()) == 0x0123456789ABCDEF
    with pytest.raises(fa.FognetError) as e:
        fa.reduce_groups(ctx, stats, R, G=0)
    assert e.value.code == E
    # R = 0 with NULL stats succeeds: G empty records, nobody ungrouped, the tables untouched
    assert raw_call(ctx, None, 0, None, G, out, met, dfn, ung) == _abi.FOGNET_OK
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == gr.Group().pack() * G and int(ung.item()) == 0
    assert bool((met == 0x0123456789ABCDEF).all())


# ---------------------------------------------------------------- a side stream

class StreamJob:
    """Device tensors of one call (stream_gate's job: ``inputs`` are the views the call reads)."""

    def __init__(self, ctx, reps, of, G):
        dev = dev_of(ctx)
        self.R, self.G = len(reps), G
        self.stats = upload(reps.view(np.uint8).reshape(-1), dev)
        self.gof = upload(of.astype(np.int32), dev)
        self.inputs = {"stats": self.stats, "group_of": self.gof}
        self.out = torch.empty(G * GRP.itemsize, dtype=torch.uint8, device=dev)
        self.met = torch.empty((self.R, NMET), dtype=torch.int64, device=dev)
        self.dfn = torch.empty(self.R, dtype=torch.int32, device=dev)
        self.ung = torch.empty(1, dtype=torch.int64, device=dev)


def test_on_a_side_stream_behind_a_gate(ctx, monkeypatch, tmp_path):
    """Both kernels run on the caller's stream and on no other: behind a gate the inputs still hold a
    decoy, so a launch on another stream computes other records."""
    monkeypatch.setenv(stream_gate.REPORT_ENV, str(tmp_path / "gate.json"))
    gate = stream_gate.Gate(dev_of(ctx))
    try:
        gate.choose(1)
    except stream_gate.NoPower as e:
        pytest.skip(str(e))
    finally:
        finish_the_rotation(gate, dev_of(ctx))
    R, G = 700, 9
    reps, rws, want_met, want_def = crafted(R)
    of = np.arange(R) % (G + 1)
    other, other_of = gr.crafted(R, seed=4242), (np.arange(R) * 7) % G
    decoy = {"stats": other.view(np.uint8).reshape(-1), "group_of": other_of.astype(np.int32)}

    def enqueue(j):
        ctx.check(raw_call(ctx, j.stats, j.R, j.gof, j.G, j.out, j.met, j.dfn, j.ung), "reduce_groups")

    job = gate.run("groups", "groups-R700", lambda: StreamJob(ctx, reps, of, G), decoy, enqueue)
    want, lost = gr.reduce_rows(rws, of, G)
    assert job.out.cpu().numpy().tobytes() == want and int(job.ung.item()) == lost
    assert np.array_equal(job.met.cpu().numpy(), want_met) and np.array_equal(job.dfn.cpu().numpy().view(np.uint32), want_def)
    assert gr.reduce_rows(gr.rows(other), other_of, G)[0] != want   # (the decoy would have shown)


# ---------------------------------------------------------------- the driver

def test_driver_appends_the_block_of_its_replications(ctx, tmp_path):
    """fognet_replay --rep-spread: the appended block equals formats.write_sca_groups of the Python
    path's record on the driver's own trace, and the summary line states its mean."""
    from test_driver import INI, drive
    sca, plain, trc, mine = (str(tmp_path / n) for n in ("a.sca", "b.sca", "a.fogntrc", "c.sca"))
    R = 5
    args = ("-f", INI, "--users", "user[6]", "--reps", str(R))
    stdout = drive(*args, "--sca", sca, "--trace-out", trc, "--rep-spread").stdout
    drive(*args, "--sca", plain)
    text, before = open(sca).read(), open(plain).read()
    assert text.startswith(before) and ":replications" not in before and text.count("version 2") == 1
    d = fa.as_device_trace(formats.load_trace(trc), dev_of(ctx))
    out = fa.run_batch(ctx, d)
    rec, lost = fa.reduce_groups(ctx, out.stats, R)
    assert lost == 0 and int(rec[0]["n_reps"]) == R
    network = re.search(r"^attr network (\S+)$", text, re.M).group(1)
    open(mine, "w").write(before)
    formats.write_sca_groups(mine, rec, append=True, network=network)
    assert open(mine).read() == text
    assert f"scalar {network}.replications \treplications \t{R}" in text
    m = rec[0]["across"][0]
    mean = gr.signed(int(m["sum_lo"]) | (int(m["sum_hi"]) << 64), 128) / int(m["count"]) / 1e9
    line = next(ln for ln in stdout.splitlines() if ln.startswith("rep-spread "))
    assert f"rep-spread reps={R} failed=0 ok={R} resp_mean_ms=" in line
    assert abs(float(re.search(r"resp_mean_ms=(\S+)", line).group(1)) - mean) <= 1e-8 * abs(mean)
    assert "rep-spread " not in drive(*args, "--sca", sca, "--rep-spread", "--quiet").stdout
