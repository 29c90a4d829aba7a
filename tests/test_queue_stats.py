"""Queue-length statistics, host side (no GPU): the event-level restatement (queue_ref) on
hand-traced cases, the fognet_queue_stats layout and symbols, the exact host merge, the `.sca`
writer and the driver's refusals."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fognetsimpp_amd as fa
import fognetsimpp_amd._abi as abi
import oracle_lib as ol
import queue_ref as qr
from fognetsimpp_amd import formats
from test_driver import INI, drive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 10**12  # one second of ticks: MIPS 1000 serves 1000 MIPS-seconds per second
NEVER = qr.NEVER


def run(t, req, dl, levels, t0=0, t1=100 * U, down=NEVER, tie="fes"):
    status, start, done, trail = qr.node_events(t, req, 1000, dl, down, tie)
    return status, start, done, qr.measure(trail, levels, t0, t1)


# ---------------------------------------------------------------- hand-traced cases

@pytest.mark.parametrize("dl,want_max", [(3 * U, 2), (2 * U, 2), (1 * U, 1)])
def test_enqueue_and_dequeue_at_one_tick(dl, want_max):
    """Task 0 (2 s) reaches the idle node at 10 + dl and starts: its timer is inserted at 10 + dl
    and fires at 12 + dl.  Task 1 (1 s) arrives one tick later and waits: L = 1.  Task 2 is
    published at 12, so it arrives at 12 + dl, the very tick at which task 0 completes and task 1
    is dequeued.  Its arrival event was inserted at 12, the timer at 10 + dl:
      dl = 3 s (above task 0's service): 12 < 13, the enqueue comes first: L = 2, then 1;
      dl = 2 s (equal): both inserted at 12, where the pre-inserted publish ran first: the
                enqueue comes first again, L = 2, then 1;
      dl = 1 s (below): 12 > 11, the dequeue comes first: L = 0, then 1.
    Task 2 is queued either way (task 1 is in service by then) and leaves at 13 + dl.  L >= 1 from
    10 + dl + 1 to 13 + dl; L >= 2 only within the tick 12 + dl, which has no length."""
    status, start, done, rec = run([10 * U, 10 * U + 1, 12 * U], [2000, 1000, 0], dl, [1, 2])
    assert status == [5, 4, 4]
    assert start == [10 * U + dl, 12 * U + dl, 13 * U + dl] and done == [12 * U + dl, 13 * U + dl, 13 * U + dl]
    assert rec == dict(n_enq=2, max_len=want_max, observed=100 * U, area=3 * U - 1, time_ge=[3 * U - 1, 0])


def test_chain_of_zero_service_tasks_popping_at_one_tick():
    """dl = 1 s.  Task 0 (2 s) starts at 11 and completes at 13 (timer inserted at 11).  Tasks 1, 2
    and 3 (0 s each) arrive at 11 + 1, 11 + 2, 11 + 3 ticks: L = 1, 2, 3.  Task 4 is published at 12
    and arrives at 13.  At tick 13 the events run in insertion order: task 0's timer (inserted at
    11) pops task 1 (L = 2) and inserts task 1's timer; task 4's arrival (inserted at 12) finds
    the node busy: L = 3; then the timers of tasks 1, 2, 3 and 4, each inserted at 13 by the one
    before, pop one task each: L = 2, 1, 0.  So task 4 saw one dequeue before it, not three."""
    t = [10 * U, 10 * U + 1, 10 * U + 2, 10 * U + 3, 12 * U]
    status, start, done, rec = run(t, [2000, 0, 0, 0, 0], U, [1, 2, 3, 4])
    assert status == [5, 4, 4, 4, 4] and start == [11 * U] + [13 * U] * 4 and done == [13 * U] * 5
    assert rec == dict(n_enq=4, max_len=3, observed=100 * U, area=6 * U - 6,
                       time_ge=[2 * U - 1, 2 * U - 2, 2 * U - 3, 0])
    # "dequeue always first" empties the queue before task 4 arrives; task 4 then meets an idle node
    assert run(t, [2000, 0, 0, 0, 0], U, [1], tie="dequeue")[0] == [5, 4, 4, 4, 5]


def test_zero_downlink():
    """dl = 0: an arrival is inserted at its own tick, by the pre-inserted publish, which runs
    before every event inserted during the run.  Task 0 (1 s) starts at 10; task 1 (0 s), published
    at the same tick, waits: L = 1.  Tasks 2 and 3 (0 s) are published at 11.  At tick 11: the two
    publishes insert their arrivals; task 0's timer (inserted at 10) pops task 1 (L = 0) and
    inserts task 1's timer behind the arrivals; the arrivals find the node busy: L = 1, 2; the
    timers pop: L = 1, 0.  Both dequeues of the zero-service chain come after the enqueues."""
    status, start, done, rec = run([10 * U, 10 * U, 11 * U, 11 * U], [1000, 0, 0, 0], 0, [1, 2])
    assert status == [5, 4, 4, 4] and start == [10 * U, 11 * U, 11 * U, 11 * U] and done == [11 * U] * 4
    assert rec == dict(n_enq=3, max_len=2, observed=100 * U, area=U, time_ge=[U, 0])


DOWN_CASE = ([10 * U, 10 * U + 1, 12 * U, 13 * U], [5000, 1000, 1000, 1000], U)


def test_node_crash_with_tasks_waiting():
    """dl = 1 s, the node crashes at 14.  Task 0 (5 s) starts at 11 and never completes.  Task 1
    waits from 11 + 1 tick, task 2 from 13: L = 1, 2.  Neither starts: both leave at the crash,
    which precedes every event of tick 14, so task 3, which arrives at 14, is lost and never
    enters."""
    t, req, dl = DOWN_CASE
    status, start, done, rec = run(t, req, dl, [1, 2, 3], down=14 * U)
    assert status == [5, 4, 4, 9] and start == [11 * U, -1, -1, -1] and done == [-1] * 4
    assert rec == dict(n_enq=2, max_len=2, observed=100 * U, area=4 * U - 1, time_ge=[3 * U - 1, U, 0])


def test_ranges_clip_the_times_and_select_the_enqueues():
    t, req, dl = DOWN_CASE
    # [12, 13.5): the enqueue at 13 alone; L = 1 for a second, then 2 for half a second
    rec = run(t, req, dl, [1, 2], 12 * U, 13 * U + U // 2, down=14 * U)[3]
    assert rec == dict(n_enq=1, max_len=2, observed=3 * U // 2, area=2 * U, time_ge=[3 * U // 2, U // 2])
    # [13 + 1 tick, 14): L = 2 throughout, carried in from before: no enqueue of the range, max_len 0
    rec = run(t, req, dl, [1, 2], 13 * U + 1, 14 * U, down=14 * U)[3]
    assert rec == dict(n_enq=0, max_len=0, observed=U - 1, area=2 * (U - 1), time_ge=[U - 1, U - 1])
    # t1 = t0, and a range that ends at the enqueue tick (excluded) or starts at it (included)
    assert run(t, req, dl, [1], 13 * U, 13 * U, down=14 * U)[3] == dict(n_enq=0, max_len=0, observed=0, area=0, time_ge=[0])
    assert run(t, req, dl, [1], 0, 13 * U, down=14 * U)[3]["n_enq"] == 1
    assert run(t, req, dl, [1], 13 * U, 20 * U, down=14 * U)[3]["n_enq"] == 1


# ---------------------------------------------------------------- the same-tick order matters

def test_wrong_same_tick_orders_fail_on_tie_heavy_traces():
    """"Arrival always first" and "dequeue always first" each give other records than the FES order
    on the tie-heavy traces (so those traces pin the rule), on the oracle's replay of them."""
    levels = [1, 2, 3, 5]
    differ = {"arrival": 0, "dequeue": 0}
    reps = 0
    for seed in range(6):
        tr = qr.tie_heavy_trace(seed, 4, 1 + seed % 3, 150)
        o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"])
        assert (o["stats"]["status"] == 0).all()
        t1 = int(o["stats"]["last_tick"].max()) + 1
        want = qr.expected(tr, o, levels, 0, t1)  # (and the events' statuses and ticks equal the oracle's)
        reps += 4
        for tie in differ:
            other = qr.expected(tr, o, levels, 0, t1, tie=tie)
            differ[tie] += sum(other[r].tobytes() != want[r].tobytes() for r in range(4))
    print(f"records that differ from the FES order in {reps} replications: {differ}")
    assert differ["arrival"] > 0 and differ["dequeue"] > 0


# ---------------------------------------------------------------- the device pass's closed form, on the CPU

def closed_form(tr, o, levels, t0, t1) -> np.ndarray:
    """queue_stats.hip's build and measure steps in plain Python (fognet_hip.h "Queue-length
    statistics"): per node the elements (at, leave, prev) of its queued tasks in
    trace order, one bisection per element for the dequeues before it, one interval per level."""
    import bisect
    arrive = np.atleast_2d(tr["arrive"])
    R, N = arrive.shape[0], int(np.asarray(tr["mips"]).shape[-1])
    out = np.zeros((R, N), qr.QUEUE)
    clip = lambda a, b: max(0, min(b, t1) - max(a, t0))  # noqa: E731
    for r in range(R):
        n = int(o["stats"]["n_tasks"][r])
        for k in range(N):
            _, dl, down = qr.node_row(tr, r, k)
            el, last = [], -1
            for i in np.nonzero(np.asarray(o["node"][r][:n]) == k)[0]:
                status, start = int(o["status"][r][i]), int(o["start"][r][i])
                if status == 4:
                    at = int(arrive[r][i]) + dl
                    el.append((at, start if start >= 0 else down, last))
                last = start
            rec = dict(n_enq=0, max_len=0, observed=t1 - t0, area=0, time_ge=[0] * len(levels))
            keys = [(leave, prev) for _, leave, prev in el]
            for j, (at, leave, _) in enumerate(el):
                if t0 <= at < t1:
                    rec["n_enq"] += 1
                    rec["max_len"] = max(rec["max_len"], j + 1 - bisect.bisect_left(keys, (at, at - dl), 0, j))
                rec["area"] += clip(at, leave)
                nxt = el[j + 1][0] if j + 1 < len(el) else NEVER
                for q, lv in enumerate(levels):
                    if lv <= j + 1:
                        rec["time_ge"][q] += clip(at, min(nxt, el[j + 1 - lv][1]))
            out[r, k] = qr.to_record(rec)
    return out


def test_closed_form_equals_the_events_on_tie_heavy_traces_with_crashes_and_clipped_ranges():
    levels = [1, 2, 3, 5]
    for seed in range(8):
        tr = qr.tie_heavy_trace(100 + seed, 3, 1 + seed % 4, 150)
        if seed % 2:  # crashes on the traces' coarse grid, so that they collide with events
            rng = np.random.default_rng(seed)
            last = int(tr["arrive"].max())
            down = (rng.integers(int(tr["init"].max()), last, size=tr["mips"].shape) // 10**11) * 10**11
            tr["down"] = np.where(rng.random(tr["mips"].shape) < 0.5, np.maximum(down, tr["init"]), NEVER).astype(np.int64)
        o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], down=tr.get("down"))
        assert (o["stats"]["status"] == 0).all()
        end = int(o["stats"]["last_tick"].max()) + 1
        mid = int(tr["arrive"][0, 75])
        for t0, t1 in ((0, end), (end // 3, 2 * end // 3), (mid, mid + 10**12), (mid, mid)):
            qr.assert_records_equal(closed_form(tr, o, levels, t0, t1), qr.expected(tr, o, levels, t0, t1), 4,
                                    f"seed {seed} range [{t0}, {t1})")


# ---------------------------------------------------------------- layout, symbols, ABI version

FIELDS = ("n_enq", "max_len", "observed_lo", "observed_hi", "area_lo", "area_hi", "time_ge")


def test_queue_stats_layout_matches_header(tmp_path):
    lines = ['printf("size %zu\\n", sizeof(fognet_queue_stats));', 'printf("levels %d\\n", FOGNET_QUEUE_LEVELS_MAX);',
             'printf("abi %d\\n", FOGNET_ABI_VERSION);',
             'printf("ge %zu\\n", sizeof(((fognet_queue_stats*)0)->time_ge));']
    lines += [f'printf("{f} %zu\\n", offsetof(fognet_queue_stats, {f}));' for f in FIELDS]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fognet_hip.h\"\nint main(void){" + "\n".join(lines) +
                   "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.QueueStats) == abi.QUEUE_STATS_DTYPE.itemsize == 176
    assert int(got["levels"]) == abi.QUEUE_LEVELS_MAX == 8 and int(got["ge"]) == 8 * 2 * 8
    for f in FIELDS:
        assert int(got[f]) == getattr(abi.QueueStats, f).offset == abi.QUEUE_STATS_DTYPE.fields[f][1], f
    assert int(got["abi"]) == 10


def test_symbols_and_abi_version():
    lib = abi.load()
    assert lib.fognet_abi_version() == 10  # the ABI grew by additions only
    for name in ("fognet_queue_stats_dev", "fognet_reduce_queue_stats_dev", "fognet_queue_stats_init",
                 "fognet_queue_stats_merge", "fognet_write_sca_queue"):
        assert name in abi.SIGNATURES and getattr(lib, name)
    for name in ("queue_stats", "reduce_queue_stats", "merge_queue_stats"):
        assert callable(getattr(fa, name)) and name in fa.__all__
    header = open(os.path.join(ROOT, "include", "fognet_hip.h")).read()
    assert "Queue-length statistics" in header and "#define FOGNET_ABI_VERSION 10" in header


# ---------------------------------------------------------------- host identity and merge

def rec_of(**kw) -> np.ndarray:
    d = dict(n_enq=0, max_len=0, observed=0, area=0, time_ge=[0] * 8)
    d.update(kw)
    return qr.to_record(d)


def test_init_is_all_zero_and_merge_is_exact():
    s = abi.QueueStats()
    ctypes.memset(ctypes.byref(s), 0x5A, ctypes.sizeof(s))
    abi.load().fognet_queue_stats_init(ctypes.byref(s))
    assert bytes(s) == bytes(176)
    big = 2**64 - 5
    a = rec_of(n_enq=3, max_len=7, observed=big, area=big + 2**70, time_ge=[big, 1, 2, 3, 4, 5, 6, 2**100])
    b = rec_of(n_enq=4, max_len=5, observed=10, area=11, time_ge=[12, 0, 0, 0, 0, 0, 0, 2**64 - 1])
    m = fa.merge_queue_stats([a.reshape(1), b.reshape(1)])[0]
    assert m.tobytes() == qr.merged([a, b], 8).tobytes() == fa.merge_queue_stats([b.reshape(1), a.reshape(1)])[0].tobytes()
    d = qr.from_record(m, 8)
    assert d["n_enq"] == 7 and d["max_len"] == 7 and d["observed"] == big + 10 and d["observed"] >> 64 == 1
    assert d["time_ge"][0] == big + 12 and d["time_ge"][7] == 2**100 + 2**64 - 1
    assert fa.merge_queue_stats([a.reshape(1)])[0].tobytes() == a.tobytes()  # the empty record is the identity


# ---------------------------------------------------------------- the .sca writer

def scalars(text: str) -> dict:
    out: dict = {}
    for m in re.finditer(r'^scalar (\S+) \t(\S+) \t(\S+)$', text, re.M):
        out.setdefault(m.group(1), {})[m.group(2)] = m.group(3)
    return out


def test_write_sca_queue_parsed_back(tmp_path):
    """timeavg and ge<level> equal the exact fraction to 1e-13 relative: the %.14g print loses up
    to 5e-14, and three roundings (two conversions, one division) 2^-53 each."""
    levels = [1, 2, 7]
    obs = 3 * (300 * U + 1)
    recs = [dict(n_enq=12345, max_len=41, observed=obs, area=2**66 + 12345678901, time_ge=[obs, obs // 3 + 1, 7]),
            dict(n_enq=0, max_len=0, observed=obs, area=0, time_ge=[0, 0, 0]),
            dict(n_enq=1, max_len=1, observed=2**64 + 99, area=2**63 + 1, time_ge=[2**63 + 1, 0, 0])]
    arr = np.array([qr.to_record(r) for r in recs], abi.QUEUE_STATS_DTYPE)
    path = str(tmp_path / "q.sca")
    formats.write_sca_queue(path, arr, levels, network="Net")
    text = open(path).read()
    assert text.startswith("version 2\nrun General-0-fognet\n")
    got = scalars(text)
    assert sorted(got) == [f"Net.fogNode[{j}].udpApp[0]" for j in range(3)]
    for j, r in enumerate(recs):
        s = got[f"Net.fogNode[{j}].udpApp[0]"]
        assert list(s) == ["queueLength:max", "queueLength:enqueued", "queueLength:timeavg"] + [f"queueLength:ge{l}" for l in levels]
        assert s["queueLength:max"] == str(r["max_len"]) and s["queueLength:enqueued"] == str(r["n_enq"])
        for name, num in [("queueLength:timeavg", r["area"])] + [(f"queueLength:ge{l}", r["time_ge"][q]) for q, l in enumerate(levels)]:
            exact = Fraction(num, r["observed"])
            val = Fraction(s[name])
            assert abs(val - exact) <= Fraction(1, 10**13) * exact, (j, name, s[name], float(exact))
    assert got["Net.fogNode[0].udpApp[0]"]["queueLength:ge1"] == "1"
    # appended behind a job file: no second header; the empty range prints -nan; node ids name the modules
    job = fa.job_from_reps(np.zeros(0, abi.REP_STATS_DTYPE))
    formats.write_sca(path, job)
    before = open(path, "rb").read()
    formats.write_sca_queue(path, np.zeros(2, abi.QUEUE_STATS_DTYPE), [1], node_id=[7, 3], append=True)
    after = open(path, "rb").read()
    assert after.startswith(before) and after.count(b"version 2") == 1
    tail = scalars(after[len(before):].decode())
    assert sorted(tail) == ["FogNet.fogNode[3].udpApp[0]", "FogNet.fogNode[7].udpApp[0]"]
    assert tail["FogNet.fogNode[7].udpApp[0]"]["queueLength:timeavg"] == "-nan"
    with pytest.raises(fa.FognetError) as e:
        formats.write_sca_queue(str(tmp_path / "no" / "dir.sca"), arr, levels)
    assert e.value.code == abi.FOGNET_ERR_ARG and b"cannot open" in abi.load().fognet_io_last_error()
    with pytest.raises(fa.FognetError):
        formats.write_sca_queue(path, arr, list(range(1, 10)))  # nine levels
    with pytest.raises(fa.FognetError):
        formats.write_sca_queue(path, arr, levels, node_id=[1])


# ---------------------------------------------------------------- the driver's refusals

def test_driver_refusals(tmp_path):
    sca = str(tmp_path / "a.sca")
    base = ("-f", INI, "--users", "user[2]", "--dry-run")
    for bad, msg in ((("--queue-stats",), "give --sca FILE"),
                     (("--sca", sca, "--queue-stats", "0,1"), "a queue length >= 1"),
                     (("--sca", sca, "--queue-stats", "2,2"), "strictly ascending"),
                     (("--sca", sca, "--queue-stats", "4,2"), "strictly ascending"),
                     (("--sca", sca, "--queue-stats", "1,2,3,4,5,6,7,8,9"), "1 to 8 levels"),
                     (("--sca", sca, "--queue-stats", "--reps", "2", "--world", "2", "--comm-id", str(tmp_path / "id")),
                      "--world 1")):
        p = drive(*base, *bad, check=False)
        assert p.returncode != 0 and msg in p.stderr, (bad, p.stderr)
    p = drive("-f", INI, "-c", "Example", "--nodes", "5", "--sca", sca, "--queue-stats", "--dry-run", check=False)
    assert p.returncode != 0 and "BrokerBaseApp3 runs" in p.stderr  # the v2 broker
    # accepted: the default levels, a list, and together with --assign
    drive(*base, "--sca", sca, "--queue-stats")
    drive(*base, "--sca", sca, "--queue-stats", "1,3,9", "--assign", "random:7")
    assert "--queue-stats [L,...]" in drive("--help").stdout
