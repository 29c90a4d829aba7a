"""Parity with the oracle above one resident round of replications.

The other GPU parity tests keep R small, so every workgroup and every
workspace slot replays one replication.  Here R passes the residency
thresholds, at small T:

  * generated replays: min(R, CUs * kGenWavesPerCu) workgroups (3,072 on 256
    CUs) take the replications from a work counter and reuse ring slot, LDS
    and reserved registers from one replication to the next;
  * hand-overs to the wide kernel: at most kWideFallbackSlots = 1,024
    workspace slots, walked with a grid stride;
  * EXT_HIER resume: min(R, 1,024) slots continue the escalated replications;
  * the job reduction: blocks of kReduceChunk = 4,096 records plus a merge;
  * the v2 rows kernels: 2 or 4 replications per wavefront, ragged R.

Every expected value is the oracle's (bit-exact), and every "the path was
taken" condition comes from the oracle's census or from device properties.
"""
import numpy as np
import pytest
import torch

import fognetsimpp_amd as fa
import oracle_lib as ol
import tracegen as tg
from fognetsimpp_amd import _abi
from test_parity_gpu import assert_parity, assert_v2_parity, job_from_reps, run_v2_gpu, v2_random

pytestmark = pytest.mark.gpu

GEN_WAVES_PER_CU = 12      # kGenWavesPerCu, csrc/internal.h:288
WIDE_FALLBACK_SLOTS = 1024  # kWideFallbackSlots, csrc/capi.hip:56 (fallback_slots() only lowers it)
DEFAULT_RING = 2048        # kDefaultRing, csrc/capi.hip:53
REDUCE_CHUNK = 4096        # kReduceChunk, csrc/internal.h:402
NODE_KEYS = ("arrive", "req", "mips", "dl", "ul", "init")


def assert_records_equal(st_g, st_o, what=""):
    """Bit-exact per-replication records; a mismatch names the field and the
    first replications that differ."""
    if st_g.tobytes() == st_o.tobytes():
        return
    for f in st_o.dtype.names:
        bad = np.flatnonzero(st_g[f] != st_o[f])
        if bad.size:
            raise AssertionError(f"{what}: record field {f} differs in {bad.size} of {len(st_o)} replications, "
                                 f"first at r = {bad[:8].tolist()} (device {st_g[f][bad[:4]].tolist()}, "
                                 f"oracle {st_o[f][bad[:4]].tolist()})")
    raise AssertionError(f"{what}: records differ outside the named fields")


def assert_rows_equal(g, o, what):
    """Bit-exact [R, ...] arrays; a mismatch names the first replications that differ."""
    if np.array_equal(g, o):
        return
    bad = np.flatnonzero((g != o).reshape(len(o), -1).any(axis=1))
    raise AssertionError(f"{what} differs in {bad.size} of {len(o)} replications, first at r = {bad[:8].tolist()}")


def per_task(out):
    return dict(node=out.node.cpu().numpy(), status=out.status.cpu().numpy(), start=out.start_tick.cpu().numpy(),
                done=out.done_tick.cpu().numpy(), stats=out.rep_stats())


# ------------------------------------------------------------------ 1, 2: generated replays (replay_gen_kernel)

GEN_SEED, GEN_R, GEN_T = 0x5EED0004, 10_000, 200  # T: three 64-publish chunks plus a partial one


def generated_job_against_oracle(ctx, N, policy, r0, ring):
    """Replications r0 .. r0 + GEN_R - 1 of the C4 recipe (sweep parameters, the
    bench's power model): run_generated's records, histogram and per-node energy
    against the oracle's replay of the same replications materialised by
    generate_trace.  Returns the oracle's result (the census)."""
    dev = torch.device("cuda", ctx.device)
    R, T = GEN_R, GEN_T
    mg, sc = fa.sweep_params(np.arange(r0, r0 + R), N)
    d = fa.generate_trace(ctx, GEN_SEED, R, T, N, mg, sc, r0=r0)
    torch.cuda.synchronize()
    h = {k: d[k].cpu().numpy() for k in NODE_KEYS}
    del d
    pb, pi = fa.power_model(1000 * (1 + np.arange(N) % 4))
    o = ol.run_batch(h["arrive"], h["req"], h["mips"], h["dl"], h["ul"], h["init"], threads=16, hist=True,
                     policy=ol.POLICIES[policy], p_busy=np.tile(pb, (R, 1)), p_idle=np.tile(pi, (R, 1)))
    power = (torch.from_numpy(pb).to(dev), torch.from_numpy(pi).to(dev))
    gen = fa.run_generated(ctx, GEN_SEED, R, T, N, mg, sc, r0=r0, ring_capacity=ring, policy=policy, power=power,
                           hist=True, energy=True)
    torch.cuda.synchronize()
    what = f"generated N={N} {policy} r0={r0} ring={ring}"
    assert (o["stats"]["n_tasks"][o["stats"]["status"] == 0] == T).all()
    assert_records_equal(gen.rep_stats(), o["stats"], what)
    assert_rows_equal(gen.node_energy.cpu().numpy(), o["node_energy"], what + ": node_energy")
    np.testing.assert_array_equal(gen.hist.cpu().numpy(), o["hist"].sum(axis=0), err_msg=what + ": hist")
    return o


def assert_past_one_resident_round(ctx):
    # generated mode launches min(R, CUs * kGenWavesPerCu) workgroups (capi.hip, fognet_run_generated_dev;
    # replay.hip:1377); three rounds' worth: most workgroups replay a third replication
    cus = torch.cuda.get_device_properties(torch.device("cuda", ctx.device)).multi_processor_count
    assert GEN_R >= 3 * GEN_WAVES_PER_CU * cus, (GEN_R, cus)


@pytest.mark.parametrize("N,policy,r0", [(8, "REF_V3", 0), (100, "REF_V3", 0), (256, "REF_V3", 0),
                                         (100, "EXT_LAT", 0), (256, "REF_V3", 1_000_000 - GEN_R)])
def test_generated_past_one_resident_round(ctx, N, policy, r0):
    """replay_gen_kernel<1|2|4, POL> with R = 10,000: on 256 CUs 3,072 workgroups
    take 6,928 replications as their second or later one (work counter,
    replay.hip:1321-1332).  N = 8 / 100 / 256 reach NPL = 1 / 2 / 4; the last
    case is the last block of C4's 1,000,000-replication job.  No ring overflows
    (oracle: max_pending <= T < the default ring), so the generated kernel itself
    wrote every record."""
    assert_past_one_resident_round(ctx)
    o = generated_job_against_oracle(ctx, N, policy, r0, 0)
    assert o["stats"]["max_pending"].max() <= DEFAULT_RING


@pytest.mark.parametrize("N,ring,mixed", [(256, 4, False), (8, 16, True)])
def test_generated_hand_over_past_slot_count(ctx, N, ring, mixed):
    """The same job with small rings: the replications that exceed the ring are
    handed to the wide kernel, which generates their traces too and walks the
    hand-over list with a grid stride over at most 1,024 workspace slots
    (replay_wide.hip:343-345).  N = 256, ring 4: all 10,000 are handed over.
    N = 8, ring 16: 5,876 are and 4,124 are not, so handed-over and staying
    replications interleave in the work-counter loop (oracle census)."""
    assert_past_one_resident_round(ctx)
    o = generated_job_against_oracle(ctx, N, "REF_V3", 0, ring)
    over = o["stats"]["max_pending"] > ring
    assert int(over.sum()) > WIDE_FALLBACK_SLOTS
    if mixed:
        assert int((~over).sum()) > WIDE_FALLBACK_SLOTS


# ------------------------------------------------------------------ 3: materialised register kernel, hand-over

@pytest.fixture(scope="module")
def overloaded_mix():
    """1,500 overloaded replications (rho = 3) with a light one (rho = 0.3) after
    every third, and the oracle's replay."""
    over = tg.make_batch(11, 1500, 4, 300, rho=3.0)
    light = tg.make_batch(12, 500, 4, 300, rho=0.3)
    is_light = np.arange(2000) % 4 == 3
    tr = {}
    for k in over:
        a = np.empty((2000,) + over[k].shape[1:], over[k].dtype)
        a[~is_light], a[is_light] = over[k], light[k]
        tr[k] = a
    o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=16, hist=True)
    return tr, o, is_light


@pytest.mark.parametrize("variant", ["full", "inloop", "stats_only"])
def test_materialised_hand_over_past_slot_count(ctx, monkeypatch, overloaded_mix, variant):
    """replay_kernel / replay_inl_kernel with a 4-entry ring hand more than 1,024
    replications to the wide kernel (oracle: max_pending 48 .. 89 on the 1,500
    overloaded ones), whose workspace has at most 1,024 slots: every slot replays
    several.  Full outputs, in-loop statistics and statistics only."""
    tr, o, is_light = overloaded_mix
    ring = 4
    st_o = o["stats"]
    assert (st_o["status"] == 0).all()
    assert int((st_o["max_pending"][~is_light] > ring).sum()) == 1500 > WIDE_FALLBACK_SLOTS
    assert int((st_o["max_pending"] > ring).sum()) > WIDE_FALLBACK_SLOTS
    if variant == "inloop":
        monkeypatch.setenv("FOGNET_REPLAY_STATS", "inloop")
    dev = torch.device("cuda", ctx.device)
    d = fa.as_device_trace(tr, dev)
    R, T = tr["arrive"].shape
    if variant == "stats_only":
        out = fa.allocate_outputs(R, T, dev, hist=True, per_task=False)
        fa.run_batch(ctx, d, out=out, ring_capacity=ring)
    else:
        out = fa.run_batch(ctx, d, ring_capacity=ring, hist=True)
    torch.cuda.synchronize()
    assert_records_equal(out.rep_stats(), st_o, variant)
    np.testing.assert_array_equal(out.hist.cpu().numpy(), o["hist"].sum(axis=0))
    if variant != "stats_only":
        g = per_task(out)
        for k in ("node", "status", "start", "done"):
            assert_rows_equal(g[k], o[k], f"{variant}: {k}")
        assert_parity(tr, g, o)


# ------------------------------------------------------------------ 4: EXT_HIER, more escalating replications than slots

HIER_KW = dict(hier_threshold_s=0, hier_up_tick=10**11)


@pytest.fixture(scope="module")
def hier_many():
    """1,280 replications on 1,030 nodes (regions of 1,024 and 6 nodes); from a
    replication-specific publish on, 60 % of the publishes belong to the small
    region, which saturates and escalates (threshold 0)."""
    R, N, T = 1280, 1030, 400
    tr = tg.make_batch(33, R, N, T, rho=0.01)
    rng = np.random.default_rng(5)
    s0 = rng.integers(0, 300, R)
    reg = np.zeros_like(tr["req"])
    for r in range(R):
        reg[r, s0[r]:][rng.random(T - s0[r]) < 0.6] = 1
    pb, pi = fa.power_model(tr["mips"])
    tr = dict(tr, region=reg, p_busy=pb, p_idle=pi)
    o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=16, hist=True,
                     policy=ol.POLICY_EXT_HIER, region=reg, p_busy=pb, p_idle=pi, **HIER_KW)
    return tr, o


@pytest.mark.parametrize("regions,resume", [("1", "1"), ("1", "0"), ("0", "1")])
def test_hier_more_escalating_replications_than_slots(ctx, monkeypatch, hier_many, regions, resume):
    """EXT_HIER with 1,088 of 1,280 replications escalating (oracle census; first
    escalations at publishes 73 .. 399, every residue mod 64): the sequential
    continuation has min(R, 1,024) slots (capi.hip, run_regions), so 64 slots continue a
    second escalated replication, importing its region state from the resume
    records (resume), or replay it from the start (FOGNET_HIER_RESUME=0); 192
    replications are finished by the region pass.  FOGNET_HIER_REGIONS=0: the
    sequential kernel alone.  Outputs, records, energy and histogram equal the
    oracle's."""
    tr, o = hier_many
    assert (o["stats"]["status"] == 0).all()
    esc = o["node"] // _abi.HIER_REGION_NODES != tr["region"]
    escalating = esc.any(axis=1)
    assert int(escalating.sum()) > WIDE_FALLBACK_SLOTS and int((~escalating).sum()) >= 64
    first = esc.argmax(axis=1)[escalating]
    assert first.min() > 0 and len(set((first % 64).tolist())) == 64
    monkeypatch.setenv("FOGNET_HIER_REGIONS", regions)
    monkeypatch.setenv("FOGNET_HIER_RESUME", resume)
    before = ctx.hier_path_stats()
    out = fa.run_batch(ctx, fa.as_device_trace(tr, torch.device("cuda", ctx.device)), policy="EXT_HIER", hist=True,
                       **HIER_KW)
    torch.cuda.synchronize()
    after = ctx.hier_path_stats()
    launched = (after[0] - before[0], after[1] - before[1])
    assert launched == ((1, 0) if regions == "1" else (0, 1))
    what = f"regions={regions} resume={resume}"
    g = per_task(out)
    assert_records_equal(g["stats"], o["stats"], what)
    for k in ("node", "status", "start", "done"):
        assert_rows_equal(g[k], o[k], f"{what}: {k}")
    assert_parity(tr, g, o)
    assert_rows_equal(out.node_energy.cpu().numpy(), o["node_energy"], what + ": node_energy")
    np.testing.assert_array_equal(out.hist.cpu().numpy(), o["hist"].sum(axis=0))


# ------------------------------------------------------------------ 5: v2 rows and lane kernels, large ragged R

@pytest.mark.parametrize("N,R,env", [(5, 4099, None), (5, 4099, ("FOGNET_V2_ACTIVE", "4")), (20, 2049, None),
                                     (40, 1500, None)])
def test_v2_many_ragged_replications(ctx, monkeypatch, N, R, env):
    """replay_v2_rows_kernel<16, 2> (N = 5: two replications per wavefront, R odd),
    <16> with FOGNET_V2_ACTIVE=4 (four per wavefront, R % 4 = 3), <32> (N = 20: two
    per wavefront, R odd) and replay_v2_kernel<1> (N = 40), each over more
    wavefronts than are resident at once (replay_v2.hip:1711-1726)."""
    assert R % 2 == 1 or N > 32
    assert env is None or R % 4 == 3
    if env is not None:
        monkeypatch.setenv(*env)
    tr, broker, stop, rt = v2_random(70 + N, R, N, 150)
    g = run_v2_gpu(ctx, tr, broker, stop, rt, qcap=256)
    o = ol.run_v2(tr["arrive"], tr["req"], broker, tr["mips"], tr["dl"], tr["ul"], tr["first_adv"], stop, rt,
                  threads=16)
    assert (o["stats"]["status"] == 0).all()
    for k in ("node", "status", "start", "done"):
        assert_rows_equal(g[k], o[k], f"v2 N={N} R={R}: {k}")
    assert_v2_parity(g, o)


# ------------------------------------------------------------------ 6: multi-block job reduction with failed records

def test_reduce_stats_multi_block_with_failed_records(ctx):
    """9,000 records: three reduce blocks of kReduceChunk = 4,096 (the last one
    partial) plus the merge, with failed records at the block edges (r = 4095,
    4096, 4097), inside a block and at the very end.  The records are checked
    against the oracle's, and the job record against the exact host reduction of
    the oracle's records and against the host merge of the three slices'
    single-block reductions."""
    R, T, N = 9000, 64, 4
    failed = [5, REDUCE_CHUNK - 1, REDUCE_CHUNK, REDUCE_CHUNK + 1, R - 1]
    assert R > 2 * REDUCE_CHUNK
    mg, sc = fa.sweep_params(np.arange(R), N)
    d = {k: v for k, v in fa.generate_trace(ctx, 7, R, T, N, mg, sc).items() if not k.startswith("_")}
    d["mips"][failed, 0] = 0
    out = fa.run_batch(ctx, d, ring_capacity=64, hist=False)  # (T = 64: a 64-entry ring cannot overflow)
    torch.cuda.synchronize()
    h = {k: d[k].cpu().numpy() for k in NODE_KEYS}
    o = ol.run_batch(h["arrive"], h["req"], h["mips"], h["dl"], h["ul"], h["init"], threads=16, outputs=False)
    st_o, st_g = o["stats"], out.rep_stats()
    ok = st_o["status"] == 0
    assert sorted(np.flatnonzero(~ok).tolist()) == failed
    # (MIPS 0: the oracle reports the reference's division fault, the engine refuses the precondition)
    np.testing.assert_array_equal(st_g["status"], np.where(ok, 0, _abi.FOGNET_ERR_ARG))
    assert_records_equal(st_g[ok], st_o[ok], "records of the completed replications")
    ref = job_from_reps(st_o)
    job = fa.reduce_stats(ctx, out.stats, R)
    u192 = lambda a: int(a[0]) | (int(a[1]) << 64) | (int(a[2]) << 128)
    assert int(job["n_reps"]) == R and int(job["n_failed"]) == 5 == ref["n_failed"]
    assert int(job["n_tasks"]) == ref["n_tasks"] == (R - 5) * T and int(job["n_queued"]) == ref["n_queued"]
    assert u192(job["queue_sum"]) == ref["queue_sum"] and u192(job["queue_sq"]) == ref["queue_sq"]
    assert u192(job["resp_sq"]) == ref["resp_sq"]
    assert int(job["resp_max_ticks"]) == ref["resp_max"] and int(job["max_pending"]) == ref["max_pending"]
    assert int(job["n_qtime"]) == int(st_o["n_qtime"][ok].sum())
    assert int(job["n_started"]) == int(st_o["n_started"][ok].sum())
    assert int(job["events"]) == int(st_o["events"][ok].sum())
    assert fa.job_from_reps(st_o).tobytes() == job.tobytes()  # (the library's host twin, every field)
    sz = _abi.REP_STATS_DTYPE.itemsize
    parts = [fa.reduce_stats(ctx, out.stats[a * sz:b * sz], b - a)
             for a, b in ((0, REDUCE_CHUNK), (REDUCE_CHUNK, 2 * REDUCE_CHUNK), (2 * REDUCE_CHUNK, R))]
    assert [int(p["n_failed"]) for p in parts] == [2, 2, 1]
    assert fa.merge_job_stats(parts).tobytes() == job.tobytes()
