"""The oracle against the reference's own handlers (CPU).

Every GPU parity test compares a kernel with oracle/fognet_oracle.c, our own
restatement of BrokerBaseApp3.cc / ComputeBrokerApp3.cc.  Here the restatement
is held to the reference itself: oracle/_ref/ref_v3 compiles the two reference
translation units in place against a stand-in kernel and runs their handlers
(oracle/ref_shim/README.md).  What it recorded is committed as
tests/golden/ref_v3_*.json, so the first half of this file runs anywhere; the
second half runs the binary on fresh traces wherever it exists.
"""
import os

import numpy as np
import pytest

import golden_io
import oracle_lib as ol
import ref_harness as rh
import tracegen as tg

REPLAY = golden_io.ref_v3_replay_cases()
DECIDE = golden_io.ref_v3_decide_cases()


# ------------------------------------------------------------------ fixtures against the oracle

@pytest.mark.parametrize("case", REPLAY, ids=lambda c: c[0])
def test_recorded_replays_equal_oracle(case):
    """node, status, start and done of all T tasks, every queueTime emission and the
    record's moments, the abort point and the four user signals (ref_harness.compare_with_oracle)."""
    name, tr, uu, ud, rec = case
    T, N = len(tr["arrive"]), len(tr["mips"])
    n = rh.compare_with_oracle(tr, uu, ud, rec, ol)
    assert n == rh.values_compared(T, N, len(rec["qtime"])) and n >= 4 * T + 2 * N + 35


def test_recorded_cases_are_the_ones_meant():
    """The shapes the fixtures exist for are in them (a regenerated file that lost one fails here)."""
    by = {c[0]: c for c in REPLAY}
    TPS = 10**12
    for N in (1, 3, 5):
        _, tr, _, _, rec = by[f"tie_heavy_n{N}"]
        S = (tr["req"] // tr["mips"][np.array(rec["node"])]).astype(np.int64)
        assert (S == 0).any() and len(rec["qtime"]) > 20
        if N > 1:  # both branches of dl_k >= S * 1e12, with S the service of a completing task
            node = np.array(rec["node"])
            assert (tr["dl"][node][S > 0] >= S[S > 0] * TPS).any() and (tr["dl"][node][S > 0] < S[S > 0] * TPS).any()
        # ties: a task reaching its node at the very tick another one completes there
        arr = tr["arrive"] + tr["dl"][np.array(rec["node"])]
        assert len(set(arr.tolist()) & set(rec["done"])) > 0
    for N in (5, 64):
        _, tr, _, _, rec = by[f"herding_n{N}"]
        assert len(set(tr["mips"].tolist())) > 1 and len(set(rec["node"])) > 1
        assert (tr["req"] < tr["mips"][0]).any() and (tr["req"] > tr["mips"][0]).any()
    _, tr, _, _, rec = by["many_nodes_n100"]
    assert len(tr["mips"]) == 100 and len(tr["arrive"]) == 300 and len(set(rec["node"])) == 100
    assert len(set(rec["node"][200:])) >= 2  # past the first sweep: minima over positive views that still change
    assert (by["req_zero"][1]["req"] == 0).sum() >= 4 and len(by["one_node"][1]["mips"]) == 1
    ab = by["overflow_one_node"][4]["abort"]
    assert ab["task"] == 2 and by["overflow_one_node"][4]["status"][4] == 4  # published after, decided before the abort
    # The same-tick double overflow.  The reference throws at the emission whose RELEASERESOURCE
    # timer was set first: the lowest task index in one recording, NOT the lowest in the other.
    lo, hi = by["overflow_same_tick_low_first"], by["overflow_same_tick_high_first"]
    assert (lo[4]["abort"]["node"], lo[4]["abort"]["task"]) == (0, 2)
    assert (hi[4]["abort"]["node"], hi[4]["abort"]["task"]) == (1, 5)
    for c, other in ((lo, 4), (hi, 3)):  # the other node's emission overflows at that very tick
        tr, rec = c[1], c[4]
        o = ol.run_batch(tr["arrive"][None], tr["req"][None], tr["mips"], tr["dl"], tr["ul"], tr["init"])
        assert int(o["stats"]["n_qtime_overflow"][0]) == 2 and int(o["start"][0][other]) == rec["abort"]["tick"]
        # run to the end, the field is the lowest index of that tick (fognet_hip.h), whichever threw
        assert int(o["stats"]["abort_tick"][0]) == rec["abort"]["tick"]
        assert int(o["stats"]["abort_task"][0]) == min(other, rec["abort"]["task"])
    for name in ("past_2p53_round_trip", "past_2p53_same_tick", "past_2p60_round_trip"):
        assert by[name][1]["arrive"][0] > 2**53 and by[name][4]["qtime"][0][0] % 1000 == 0
    assert by["past_2p53_same_tick"][4]["qtime"][0][0] == -1000


def test_recorded_decisions_equal_oracle():
    n_big = 0
    for name, busy, mips, req, node in DECIDE:
        rc, k = ol.decide_v3(busy, mips, req)
        assert rc == 0 and k == node, name
        n_big += len(busy) in (64, 65, 257)
    flat = np.concatenate([c[1] for c in DECIDE])
    assert len(DECIDE) >= 200 and n_big >= 6
    assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any()
    assert (np.signbit(flat) & (flat == 0)).any() and (flat == 5e-324).any() and (flat == 1e300).any()
    assert (flat == 1e16 + 2).any() and any(c[3] < 0 for c in DECIDE)
    assert {1, 2**31 - 1} <= {int(c[2][0]) for c in DECIDE}


# ------------------------------------------------------------------ live differential

def live_traces():
    """42 seeded traces: (label, trace, user_ul, user_dl)."""
    from test_parity_gpu import tie_heavy
    rng = np.random.default_rng(0x5EED0009)
    out = []
    for i, N in enumerate((1, 2, 5, 17, 64, 100)):
        for j, rho in enumerate((0.3, 0.9, 3.0)):
            T = (2000, 1200, 700)[j]
            tr = rh.rebase(tg.make_batch(0x5EED0100 + 3 * i + j, 1, N, T, rho=rho, lat_scale=(1, 10, 100)[j]))
            out.append((f"batch_n{N}_rho{rho}", tr, rng.integers(0, 5 * 10**9, T), rng.integers(0, 5 * 10**9, T)))
        for seed in range(3):
            T = (2000, 900, 333)[seed]
            tr = rh.rebase(tie_heavy(100 + 3 * i + seed, 1, N, T))
            out.append((f"tie_n{N}_s{seed}", tr, int(rng.integers(0, 3)) * 10**11, int(rng.integers(0, 3)) * 10**11))
    # long services on two slow nodes: runs the reference ends at a queueTime overflow
    for seed in range(6):
        tr = tg.make_replication(0x5EED0200 + seed, 0, 2, 600, rho=(0.9, 3.0)[seed % 2], req_lo=100_000,
                                 req_hi=2_000_000)
        tr = rh.rebase({k: v[None] if k in ("arrive", "req") else v for k, v in tr.items()})
        out.append((f"long_s{seed}", tr, 10**9, 2 * 10**9))
    return out


LIVE_ABORT_FREE = 35  # of 42; counted on the CPU with the seeds above


def needs_binary():
    if not rh.have_binary():
        if rh.have_reference():
            pytest.fail("the reference tree is here but oracle/_ref/ref_v3 is not built (make -C oracle ref)")
        pytest.skip("no reference tree and no harness binary on this machine")


def test_live_differential():
    needs_binary()
    traces = live_traces()
    recs = rh.run_replays([(tr, uu, ud) for _, tr, uu, ud in traces])
    free = 0
    for (label, tr, uu, ud), rec in zip(traces, recs):
        T, N = len(tr["arrive"]), len(tr["mips"])
        n = rh.compare_with_oracle(tr, uu, ud, rec, ol)
        assert n == rh.values_compared(T, N, len(rec["qtime"])), label
        if rec["abort"] is None:
            free += 1
            assert len(rec["qtime"]) == rec["status"].count(4), label
    assert len(traces) == 42 and free == LIVE_ABORT_FREE and 3 * free >= 2 * len(traces)


def test_live_decisions():
    """Fresh views, larger than the committed ones, through the reference's decide path."""
    needs_binary()
    rng = np.random.default_rng(0x5EED000A)
    special = [np.nan, np.inf, -np.inf, -0.0, 5e-324, 1e300, 1e16, 1e16 + 2, -2.5]
    views = []
    for _ in range(400):
        n = int(rng.choice([1, 2, 3, 5, 8, 33, 64, 65, 200]))
        busy = rng.integers(0, 4, n).astype(np.float64)
        m = rng.random(n) < 0.2
        busy[m] = rng.choice(special, int(m.sum()))
        mips = rng.choice([1, 999, 1000, 2**31 - 1], n)
        views.append((busy, mips, int(rng.choice([-7000, 0, 1, 1000, 2999, 2**31 - 1]))))
    for (busy, mips, req), node in zip(views, rh.run_decides(views)):
        assert ol.decide_v3(busy, mips, req) == (0, node)


def test_fixtures_reproduce():
    """Regenerating the fixtures gives the committed bytes."""
    needs_binary()
    import sys
    sys.path.insert(0, golden_io.GOLDEN)
    try:
        import make_ref_v3_fixtures as gen
    finally:
        sys.path.remove(golden_io.GOLDEN)
    made = gen.generate()
    import glob
    have = sorted(os.path.basename(p) for p in glob.glob(os.path.join(golden_io.GOLDEN, "ref_v3_*.json")))
    assert sorted(made) == have
    for name, text in made.items():
        assert open(os.path.join(golden_io.GOLDEN, name)).read() == text, name
