"""Time-window statistics, host side (no GPU): the restatement (window_ref) in its two ways and
its defining invariants on the oracle's outputs and the reference's recordings, the host
identity and merge of fognet_window_stats, the ABI mirror and the `.vec` writer.  The cases here
are the ones test_window_stats_gpu.py runs on the device."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import fognetsimpp_amd as fa
import fognetsimpp_amd._abi as abi
import hier_ref as hr
import node_stats_ref as ns
import per_user_ref as pu
import signal_vectors_ref as sv
import user_stats_ref as us
import window_ref as wr
from fognetsimpp_amd import formats
from test_driver import INI, drive
from test_per_user_stats import carry_case, down_trace, draw_links, draw_users, mqtt_case, replay_oracle, trace_case
from test_signal_vectors import herded_case, recording_cases, tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = abi.WINDOW_STATS_DTYPE
TPS = 10**12
_cache: dict = {}


# ---------------------------------------------------------------- the cases (shared with the GPU tests)

def oracle_case(name):
    """(trace, oracle result, user_of, user_ul, user_dl, flags or None, hop) by name, computed once."""
    if name in _cache:
        return _cache[name]
    flags, up = None, 0
    if name in ("tracegen", "ext_lat"):
        tr, o = trace_case(5, 191, "EXT_LAT" if name == "ext_lat" else "REF_V3")
        who, (uu, ud) = draw_users(7, 3, 191, 7, "random"), draw_links(8, 3, 7, True)
    elif name == "ties":
        tr, o, who, uu, ud = tie_case(3)
    elif name == "down":
        tr = down_trace()
        o = replay_oracle(tr)
        who, (uu, ud) = draw_users(0xD0, 3, 257, 10, "rr"), draw_links(0xD1, 3, 10, True)
    elif name == "herded":
        tr, o, who, uu, ud = herded_case()
    elif name == "carry":
        tr, who, uu, ud = carry_case()
        o = replay_oracle(tr)
    elif name == "mqtt":
        tr, who, uu, ud = mqtt_case(3)
        o = replay_oracle(tr)
    elif name == "hier":
        tr, tu, td, o, flags, _, up = hr.case("D")
        R, T = np.atleast_2d(tr["arrive"]).shape
        who, (uu, ud) = draw_users(0x41, R, T, 3, "rr"), draw_links(0x42, R, 3, False)
    else:
        raise KeyError(name)
    _cache[name] = (tr, o, who, uu, ud, flags, up)
    return _cache[name]


ORACLE_CASES = ("tracegen", "ties", "ext_lat", "down", "herded", "carry", "mqtt", "hier")


def covering(last: int, W: int):
    """(window, W) of a range [0, W * window) that holds every tick up to ``last``."""
    return last // W + 1, W


def check_invariants(tr, o, who, uu, ud, flags, up, W, node_recs, user_recs):
    """The defining invariants of a covering range, replication by replication."""
    last = wr.latest_tick(tr, o, who, uu, ud, flags, up)
    window, W = covering(last, W)
    recs, outside, un = wr.expected(tr, o, who, uu, ud, 0, window, W, flags, up)
    assert (outside == 0).all() and (un == 0).all()
    arrive = np.atleast_2d(tr["arrive"])
    for r in range(arrive.shape[0]):
        n = int(o["stats"]["n_tasks"][r])
        m = wr.merged(recs[r])
        nodes, users = ns.merged(node_recs[r]), pu.merged(user_recs[r])
        q = m.sig["queue"]
        assert (q.n, q.ovf, q.mn, q.mx, q.s, q.q) == (nodes.queue.n, nodes.queue.ovf, nodes.queue.mn, nodes.queue.mx,
                                                      nodes.queue.s, nodes.queue.q), r
        for s in us.SIGNALS:
            g, w = m.sig[s], pu.load_mom(users[s])
            assert (g.n, g.ovf, g.mn, g.mx, g.s, g.q) == (w.n, w.ovf, w.mn, w.mx, w.s, w.q), (r, s)
        assert m.n_publish == n
        assert m.n_complete == int((o["done"][r][:n] >= 0).sum()) == nodes.resp.n
        assert m.busy == TPS * nodes.busy
        dl = np.asarray(tr["dl"][r] if np.ndim(tr["dl"]) == 2 else tr["dl"], np.int64)
        insys = 0
        for i in range(n):
            if int(o["done"][r][i]) >= 0:
                hop = int(up) if flags is not None and int(flags[r][i]) else 0
                insys += int(o["done"][r][i]) - (int(arrive[r][i]) + int(dl[int(o["node"][r][i])]) + hop)
        assert m.insys == insys and m.insys >= m.busy
    return recs, window


# ---------------------------------------------------------------- the restatement's invariants

@pytest.mark.parametrize("name", ORACLE_CASES)
def test_covering_range_merges_to_the_node_and_user_records(name):
    tr, o, who, uu, ud, flags, up = oracle_case(name)
    assert all(int(s) in wr.OK_STATUSES for s in o["stats"]["status"])
    if flags is None:
        node_recs, (user_recs, _) = ns.expected(tr, o), pu.expected(tr, o, who, uu, ud)
    else:
        assert flags.any()
        node_recs, (user_recs, _) = hr.node_expected(tr, o, flags, up), pu.expected(tr, o, who, uu, ud, flags=flags, up=up)
    for W in (1, 7, 300):
        check_invariants(tr, o, who, uu, ud, flags, up, W, node_recs, user_recs)
    if name == "carry":
        recs, _, _ = wr.expected(tr, o, who, uu, ud, 0, *covering(wr.latest_tick(tr, o, who, uu, ud), 1))
        assert sum(int(recs[0, 0][s]["overflow"]) for s in us.SIGNALS) > 0  # lost emissions are counted
    if name == "herded":
        recs, _, _ = wr.expected(tr, o, who, uu, ud, 0, *covering(wr.latest_tick(tr, o, who, uu, ud), 1))
        assert int(recs[0, 0]["queue"]["overflow"]) > 0
    if name == "down":
        assert (o["status"] == 9).any() and ((o["status"] != 9) & (o["done"] == -1)).any()


@pytest.mark.parametrize("name", [n for n in ORACLE_CASES if n != "hier"])
def test_direct_and_binned_rows_agree(name):
    """The five signals binned from signal_vectors_ref's rows equal the direct restatement's, on
    a covering range and on a narrow one that leaves events outside on both sides."""
    tr, o, who, uu, ud, _, _ = oracle_case(name)
    last = wr.latest_tick(tr, o, who, uu, ud)
    ticks = wr.event_ticks(tr, o, who, uu, ud)
    t_mid = ticks[len(ticks) // 3]
    rows = sv.expected(tr, o, who, uu, ud, with_rows=True)["rows"]
    N, U = np.shape(tr["dl"])[-1], np.shape(uu)[-1]
    for t0, window, W in ((0, last // 13 + 1, 13), (t_mid, max((last - t_mid) // 40, 1), 9)):
        recs, outside, _ = wr.expected(tr, o, who, uu, ud, t0, window, W)
        for r in range(recs.shape[0]):
            wr.assert_signals_match_rows(recs[r], wr.binned(rows[r], N, U, t0, window, W))
        if t0:
            assert outside[0, 0] > 0 and outside[0, 1] > 0


def test_recordings_of_the_reference():
    """On the reference's 14 recorded runs the windows hold the recording's own emissions:
    every queueTime and every relayed ack, binned by its recorded time."""
    cases = recording_cases()
    assert len(cases) == 14
    for name, tr, o, who, uu, ud, rec in cases:
        N, U = len(tr["dl"]), len(uu)
        last = wr.latest_tick(tr, o, who, uu, ud)
        window, W = covering(last, 11)
        recs, outside, un = wr.expected(tr, o, who, uu, ud, 0, window, W)
        assert (outside == 0).all() and (un == 0).all()
        rows = sv.expected(tr, o, who, uu, ud, with_rows=True)["rows"][0]
        wr.assert_signals_match_rows(recs[0], wr.binned(rows, N, U, 0, window, W))
        if rec["abort"]:
            continue  # (an aborted run defines the rows before its abort tick only)
        got = [int(x) for x in recs[0]["queue"]["count"]]
        want = [0] * W
        for e in rec["qtime"]:
            want[e[1] // window] += 1
        assert got == want, name
        acks = {4: [0] * W, 5: [0] * W, 6: [0] * W}
        for _, status, at in (tuple(a) for a in rec["user_acks"]):
            acks[status][at // window] += 1
        for status, sig in ((5, "latency"), (4, "latencyH1"), (6, "taskTime")):
            assert [int(x) + int(y) for x, y in zip(recs[0][sig]["count"], recs[0][sig]["overflow"])] == acks[status], (name, sig)


def test_window_edges_and_intervals():
    """A hand-made replication: events exactly on the edges, an interval ending on an edge and on
    the range's end, a zero-service task, a task over many windows, t0 > 0 cutting on the left."""
    tr = dict(arrive=np.array([[100, 200, 200, 1000]], np.int64), dl=np.array([10], np.int64), ul=np.array([5], np.int64))
    stats = np.zeros(1, abi.REP_STATS_DTYPE)
    stats["n_tasks"] = 4
    o = dict(node=np.zeros((1, 4), np.int32), status=np.array([[5, 4, 4, 5]], np.uint8),
             start=np.array([[110, 300, 400, 1010]], np.int64), done=np.array([[300, 400, 400, 1010]], np.int64), stats=stats)
    recs, outside, un = wr.expected(tr, o, None, None, None, 100, 100, 4)  # [100, 500)
    assert [int(x) for x in recs[0]["n_publish"]] == [1, 2, 0, 0] and list(un) == [4]
    assert [int(x) for x in recs[0]["n_complete"]] == [0, 0, 1, 2]  # done = 400 lies in [400, 500)
    assert [int(x) for x in recs[0]["busy_lo"]] == [90, 100, 100, 0]  # [110, 300) + [300, 400) + nothing
    assert [int(x) for x in recs[0]["insys_lo"]] == [90, 100 + 90 + 90, 200, 0]
    assert [int(x) for x in recs[0]["queue"]["count"]] == [0, 0, 1, 1]
    assert list(outside[0]) == [0, 2]  # the last task's publish and completion
    recs, outside, _ = wr.expected(tr, o, None, None, None, 101, 1, 299)  # [101, 400): every tick a window
    assert int(recs[0]["busy_lo"].sum()) == (300 - 110) + (400 - 300) and set(recs[0]["busy_lo"][9:].tolist()) == {1}
    # before: the publish at 100; at or past 400: the publish at 1000, the queueTime at 400, three completions
    assert list(outside[0]) == [1, 1 + 1 + 3]
    assert int(recs[0, 298]["n_complete"]) == 0 and int(recs[0, 199]["n_complete"]) == 1


def test_failed_replications_and_unassigned_users():
    tr, o = trace_case(5, 65)
    who = draw_users(1, 3, 65, 4, "rr")
    who[0, [3, 17, 64]] = (-1, 4, 2**31 - 1)
    uu, ud = draw_links(2, 3, 4, False)
    window, W = covering(wr.latest_tick(tr, o, who, uu, ud), 5)
    recs, outside, un = wr.expected(tr, o, who, uu, ud, 0, window, W, statuses=[0, 1, 9])
    assert list(un) == [3, 0, 0] and recs[1].tobytes() == wr.empty_records(W).tobytes() and (outside == 0).all()
    m = wr.merged(recs[0])
    assert m.n_publish == 65 and m.sig["delay"].n == 62
    assert wr.merged(recs[2]).n_publish == 65  # a REF_ABORTED one keeps its records


# ---------------------------------------------------------------- host identity and merge

def c_rec(rec) -> abi.WindowStats:
    return abi.WindowStats.from_buffer_copy(np.ascontiguousarray(rec).tobytes())


def host_merge(a, b) -> np.ndarray:
    x, y = c_rec(a), c_rec(b)
    abi.load().fognet_window_stats_merge(C.byref(x), C.byref(y))
    return np.frombuffer(bytes(x), dtype=WINDOW)[0]


def random_records(rng, *shape) -> np.ndarray:
    recs = np.zeros(shape, WINDOW)
    flat = recs.view(np.uint64).reshape(*shape, WINDOW.itemsize // 8)
    flat[:] = np.frombuffer(rng.randbytes(flat.nbytes), np.uint64).reshape(flat.shape)
    for k in ("n_publish", "n_complete"):
        recs[k] >>= 24
    for s in wr.SIGNALS:
        recs[s]["count"] >>= 24  # counts that cannot overflow int64 when summed
        recs[s]["overflow"] >>= 24
    return recs


def test_init_is_the_empty_record_and_the_identity():
    s = abi.WindowStats()
    C.memset(C.byref(s), 0x5A, C.sizeof(s))
    abi.load().fognet_window_stats_init(C.byref(s))
    empty = np.frombuffer(bytes(s), dtype=WINDOW)[0]
    assert empty.tobytes() == wr.empty_records(1).tobytes()
    x = random_records(random.Random(3), 1)[0]
    assert host_merge(empty, x).tobytes() == x.tobytes() == host_merge(x, empty).tobytes()
    abi.load().fognet_window_stats_init(None)
    abi.load().fognet_window_stats_merge(None, None)


def test_merge_is_commutative_and_exact_on_random_limbs():
    recs = random_records(random.Random(12), 60, 2)
    for a, b in recs:
        ab = host_merge(a, b)
        assert ab.tobytes() == host_merge(b, a).tobytes() == wr.to_records([wr.merged([a, b], wrap=True)])[0].tobytes()
    carry = wr.Win()
    carry.busy, carry.insys = 2**64 - 1, 2**127
    one = wr.Win()
    one.busy = 1
    got = wr.Win.load(host_merge(wr.to_records([carry])[0], wr.to_records([one])[0]))
    assert got.busy == 2**64 and got.insys == 2**127
    got = fa.merge_window_stats([recs[:, 0], recs[:, 1]])
    assert got.tobytes() == wr.to_records([wr.merged(p, wrap=True) for p in recs]).tobytes()


# ---------------------------------------------------------------- the ABI

NAMES = ("fognet_window_stats_dev", "fognet_reduce_window_stats_dev", "fognet_window_stats_init",
         "fognet_window_stats_merge", "fognet_write_vec_windows")


def test_abi_layout_and_mirror():
    lib = abi.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in abi.SIGNATURES, n
    header = open(os.path.join(ROOT, "include", "fognet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct fognet_window_stats \{(.*?)\} fognet_window_stats;", src, re.S).group(1)
    fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).split(",") if f.strip()]
    assert fields == list(WINDOW.names) == [n for n, _ in abi.WindowStats._fields_]
    assert WINDOW.itemsize == C.sizeof(abi.WindowStats) == 408 == 6 * 8 + 5 * abi.MOMENTS_DTYPE.itemsize
    assert [WINDOW.fields[n][1] for n in WINDOW.names] == [getattr(abi.WindowStats, n).offset for n in WINDOW.names]
    m = re.search(r"\bint\s+fognet_window_stats_dev\s*\(([^)]*)\)\s*;", src)
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["fognet_ctx *ctx", "const fognet_batch_in *in", "const fognet_batch_out *out", "const int32_t *user_of",
                      "int32_t U", "int32_t link_stride", "const int64_t *user_ul_tick", "const int64_t *user_dl_tick",
                      "int64_t t0_tick", "int64_t window_tick", "int32_t W", "fognet_window_stats *win", "int64_t *n_outside",
                      "int64_t *n_unassigned", "void *hip_stream"]
    P = C.c_void_p
    assert abi.SIGNATURES["fognet_window_stats_dev"] == (C.c_int, [P, C.POINTER(abi.BatchIn), C.POINTER(abi.BatchOut), P,
                                                                   C.c_int32, C.c_int32, P, P, C.c_int64, C.c_int64,
                                                                   C.c_int32, P, P, P, P])
    defs = dict(re.findall(r"^#define\s+(FOGNET_WINDOW_\w+)\s+(.+?)\s*$", header, re.M))
    assert eval(defs["FOGNET_WINDOW_MAX"]) == abi.WINDOW_MAX == 2**20
    assert int(defs["FOGNET_WINDOW_LDS_WINDOWS"]) == abi.WINDOW_LDS_WINDOWS
    assert re.search(r"#define FOGNET_ABI_VERSION 10\b", header) and abi.ABI_VERSION == 10  # additive
    for n in ("window_stats", "reduce_window_stats", "merge_window_stats", "summarize_window"):
        assert callable(getattr(fa, n)) and n in fa.__all__


def test_null_arguments_are_refused_without_a_device():
    lib = abi.load()
    assert lib.fognet_window_stats_dev(None, None, None, None, 0, 0, None, None, 0, 1, 1, None, None, None, None) == abi.FOGNET_ERR_ARG
    assert lib.fognet_reduce_window_stats_dev(None, None, None, 0, 1, None, None) == abi.FOGNET_ERR_ARG


# ---------------------------------------------------------------- the summary and the .vec writer

def job_of_case(W=7):
    """(job [W], window, R, N) of the tracegen case, whose tasks are served for whole seconds and wait
    in queues: the first W - 2 windows cover the run, the last two hold nothing."""
    tr, o, who, uu, ud, _, _ = oracle_case("tracegen")
    window, _ = covering(wr.latest_tick(tr, o, who, uu, ud), W - 2)
    recs, outside, _ = wr.expected(tr, o, who, uu, ud, 0, window, W)
    assert not outside.any()
    R = recs.shape[0]
    return wr.to_records([wr.merged(recs[:, w]) for w in range(W)]), window, R, np.shape(tr["dl"])[-1]


def test_summarize_window():
    job, window, R, N = job_of_case()
    total_busy = sum(wr.Win.load(r).busy for r in job)
    s = [fa.summarize_window(r, N, window, R) for r in job]
    assert sum(x["utilisation"] for x in s) == pytest.approx(total_busy / (N * window * R), rel=1e-12)
    assert total_busy > 0 and all(0.0 < x["utilisation"] <= 1.0 for x in s[:5]) and s[6]["utilisation"] == 0.0
    assert all(x["tasks_in_system"] >= x["utilisation"] * N for x in s) and s[2]["tasks_in_system"] > s[2]["utilisation"] * N
    for w in range(7):  # each figure against its own record, in exact integers
        rec = wr.Win.load(job[w])
        assert s[w]["utilisation"] == pytest.approx(rec.busy / (N * window * R), rel=1e-15)
        assert s[w]["tasks_in_system"] == pytest.approx(rec.insys / (window * R), rel=1e-15)
    big = job[0].copy()
    big["busy_hi"], big["busy_lo"], big["insys_hi"] = 3, 5, 1  # the high limbs count
    x = fa.summarize_window(big, 1, 2**40, 1)
    assert x["utilisation"] == pytest.approx((3 * 2**64 + 5) / 2**40, rel=1e-15)
    assert x["tasks_in_system"] == pytest.approx((2**64 + int(big["insys_lo"])) / 2**40, rel=1e-15)
    assert sum(x["publishes"] for x in s) == int(job["n_publish"].sum()) > 0
    w = wr.Win.load(job[1])
    assert s[1]["latencyH1_ms"]["count"] == w.sig["latencyH1"].n
    assert s[1]["latencyH1_ms"]["mean"] == pytest.approx(w.sig["latencyH1"].s / w.sig["latencyH1"].n * 1e-12, rel=1e-12)
    assert s[1]["delay_ms"]["mean"] == pytest.approx(w.sig["delay"].s / w.sig["delay"].n * 1e-9, rel=1e-12)


def parse_vec(text):
    """({id: (module, name)}, {id: [(time string, value string)]}) of a .vec file."""
    decl, rows = {}, {}
    for line in text.splitlines():
        m = re.match(r"vector (\d+)  (\S+)  (\S+)  TV$", line)
        if m:
            decl[int(m.group(1))] = (m.group(2), m.group(3))
            rows[int(m.group(1))] = []
        elif re.match(r"\d+\t", line):
            v, t, x = line.split("\t")
            rows[int(v)].append((t, x))
    return decl, rows


def test_write_vec_windows_golden_and_fields(tmp_path):
    job, window, R, N = job_of_case()
    path = str(tmp_path / "w.vec")
    formats.write_vec_windows(path, job, N, 0, window, R, network="Net")
    text = open(path).read()
    golden = os.path.join(ROOT, "tests", "golden", "window_stats_tracegen.vec")
    assert text == open(golden).read()
    assert text.startswith("version 2\nrun General-0-fognet\n")
    decl, rows = parse_vec(text)
    by_name = {v: k for k, v in decl.items()}
    assert sorted(decl) == list(range(14))
    nodes, broker, users = "Net.fogNodes.udpApp[0]", "Net.broker.udpApp[0]", "Net.users.udpApp[0]"
    assert decl[0] == (nodes, "utilisation:window") and decl[1] == (nodes, "tasksInSystem:window")
    assert decl[2] == (nodes, "completions:window") and decl[5] == (broker, "publishes:window")
    assert decl[3] == (nodes, "queueTime:window(mean)") and decl[4] == (nodes, "queueTime:window(count)")
    assert decl[6] == (broker, "delay:window(mean)") and decl[7] == (broker, "delay:window(count)")
    assert [decl[i] for i in range(8, 14)] == [(users, f"{s}:window({k})") for s in ("latency", "latencyH1", "taskTime")
                                                for k in ("mean", "count")]
    W = len(job)
    fmt = lambda v: "%.14g" % v
    for w in range(W):
        rec = wr.Win.load(job[w])
        t, x = rows[0][w]
        end = (w + 1) * window
        assert t == (f"{end // TPS}.{end % TPS:012d}".rstrip("0").rstrip("."))
        assert x == fmt(rec.busy / (N * window * R)) and (x != "0") == (w < 5)  # real service in every window of the run
        assert rows[1][w][1] == fmt(rec.insys / (window * R)) and (rows[1][w][1] != "0") == (w < 5)
        assert rows[2][w][1] == str(rec.n_complete) and rows[5][w][1] == str(rec.n_publish)
    for sig, mean_id in (("queue", 3), ("delay", 6), ("latency", 8), ("latencyH1", 10), ("taskTime", 12)):
        moms = [wr.Win.load(r).sig[sig] for r in job]
        assert [x for _, x in rows[mean_id + 1]] == [str(m.n) for m in moms]
        assert len(rows[mean_id]) == sum(1 for m in moms if m.n)  # no row where nothing was emitted
        for (_, x), m in zip(rows[mean_id], [m for m in moms if m.n]):
            assert float(x) == pytest.approx(m.s / m.n * 1e-12, rel=1e-13)
    assert sum(int(x) for _, x in rows[by_name[(broker, "publishes:window")]]) == int(job["n_publish"].sum())
    assert len(rows[3]) == len(rows[8]) == 5 and float(rows[3][2][1]) > 0  # queueing; the two empty windows have no mean


def test_write_vec_windows_append_and_errors(tmp_path):
    job, window, R, N = job_of_case()
    path, alone = str(tmp_path / "a.vec"), str(tmp_path / "alone.vec")
    z = np.zeros(1, np.int64)
    formats.write_vec(path, z, z, np.zeros(1, np.int32), np.zeros(1, np.uint8), z)
    before = open(path, "rb").read()
    formats.write_vec_windows(path, job, N, 0, window, R, id_base=2, append=True)
    formats.write_vec_windows(alone, job, N, 0, window, R, id_base=2)
    after, created = open(path, "rb").read(), open(alone, "rb").read()
    assert after.startswith(before) and after.count(b"version 2") == 1 and created.endswith(after[len(before):])
    assert sorted(parse_vec(after[len(before):].decode())[0]) == list(range(2, 16))
    empty = str(tmp_path / "e.vec")
    formats.write_vec_windows(empty, np.zeros(0, WINDOW), N, 0, window, R)
    decl, rows = parse_vec(open(empty).read())
    assert len(decl) == 14 and not any(rows.values())
    for bad in (dict(N=0), dict(window=0), dict(replications=0), dict(t0=-1), dict(id_base=-1), dict(t0=2**62)):
        kw = dict(N=N, t0=0, window=window, replications=R, id_base=0)
        kw.update(bad)
        with pytest.raises(fa.FognetError) as e:
            formats.write_vec_windows(str(tmp_path / "x.vec"), job, kw["N"], kw["t0"], kw["window"], kw["replications"],
                                      id_base=kw["id_base"])
        assert e.value.code == abi.FOGNET_ERR_ARG
    with pytest.raises(fa.FognetError):
        formats.write_vec_windows(str(tmp_path / "no" / "such" / "dir.vec"), job, N, 0, window, R)
    assert b"cannot open" in abi.load().fognet_io_last_error()


# ---------------------------------------------------------------- the driver's refusals

@pytest.mark.parametrize("args,msg", [
    (("--users", "user[3]", "--windows", "1s"), "--windows appends to the .vec"),
    (("-c", "Example", "--nodes", "5", "--vec", "x.vec", "--windows", "1s"), "--windows applies to BrokerBaseApp3 runs"),
    (("--users", "user[3]", "--reps", "4", "--vec", "x.vec", "--windows", "1s", "--world", "2", "--comm-id", "c.id"),
     "--windows: the window records of several ranks are not combined"),
    (("--users", "user[3]", "--vec", "x.vec", "--windows", "0"), "--windows: DT must be positive"),
    (("--users", "user[3]", "--vec", "x.vec", "--windows", "1s,0"), "--windows: W must lie in"),
])
def test_driver_refusals(tmp_path, args, msg):
    args = [str(tmp_path / a) if a in ("x.vec", "c.id") else a for a in args]
    p = drive("-f", INI, *args, "--dry-run", check=False)
    assert p.returncode == 2 and msg in p.stderr, (p.returncode, p.stderr)
    assert not (tmp_path / "x.vec").exists()
