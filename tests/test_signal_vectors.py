"""Signal vectors, host side (no GPU): the emission order (signal_vectors_ref, the restatement of
include/fognet_hip.h "Signal vectors") held to the reference's own recorded runs, the vectors'
rows against the per-node and per-user records on oracle runs, the `.vec` writer of the
user-side vectors, and the driver's refusals.  The cases here are the ones
test_signal_vectors_gpu.py runs on the device."""
import numpy as np
import pytest

import fognetsimpp_amd as fa
import fognetsimpp_amd._abi as abi
import golden_io as gio
import node_stats_ref as ns
import per_user_ref as pu
import signal_vectors_ref as sv
import tracegen as tg
from fognetsimpp_amd import formats
from test_driver import INI, drive
from test_per_user_stats import down_trace, draw_links, draw_users, mqtt_case, replay_oracle, trace_case

MS = 10**9
GRID = 10**11  # 100 ms
_cache: dict = {}


# ---------------------------------------------------------------- the cases (shared with the GPU tests)

def recording_cases():
    """(name, trace [1, T], recorded outputs as a replay result, user_of [1, T], user_ul [U],
    user_dl [U], the recording) of every tests/golden/ref_v3_*.json run with user_acks.  The users
    are the distinct (user_ul, user_dl) pairs of the recording's per-task links, in sorted order."""
    if "rec" not in _cache:
        out = []
        for name, tr, uu, ud, rec in gio.ref_v3_replay_cases():
            if "user_acks" not in rec:
                continue
            T = len(tr["arrive"])
            uu, ud = (np.broadcast_to(x, (T,)) if x.size == 1 else x for x in (uu, ud))
            pairs = sorted(set(zip(uu.tolist(), ud.tolist())))
            who = np.array([pairs.index(p) for p in zip(uu.tolist(), ud.tolist())], np.int32)[None]
            stats = np.zeros(1, abi.REP_STATS_DTYPE)
            stats["n_tasks"] = sum(1 for k in rec["node"] if k >= 0)  # an aborted run decided a prefix
            o = dict(node=np.array(rec["node"], np.int32)[None], status=np.array(rec["status"], np.uint8)[None],
                     start=np.array(rec["start"], np.int64)[None], done=np.array(rec["done"], np.int64)[None], stats=stats)
            tr2 = {k: (v[None] if k in ("arrive", "req") else v) for k, v in tr.items()}
            out.append((name, tr2, o, who, np.array([p[0] for p in pairs], np.int64),
                        np.array([p[1] for p in pairs], np.int64), rec))
        _cache["rec"] = out
    return _cache["rec"]


def tie_trace(seed, R, N, T, U):
    """The generator idea of the tie_heavy recordings: everything on a 100-ms grid -- gaps, node
    links (some downlinks 0, some whole seconds) and user links -- and service times that are
    often 0, so acks of many nodes meet at one tick at one user.  (trace, user_of, ul, dl [U])."""
    rng = np.random.default_rng(seed)
    mips = rng.choice([1000, 2000, 500], size=(R, N)).astype(np.int32)
    dl = rng.choice([0, 0, GRID, 2 * GRID, 10 * GRID], size=(R, N)).astype(np.int64)
    ul = rng.choice([0, GRID, 3 * GRID], size=(R, N)).astype(np.int64)
    init = ul + rng.integers(0, 3, size=(R, N)) * GRID
    start = init.max(axis=1, keepdims=True) + GRID
    arrive = start + np.cumsum(rng.choice([0, 0, GRID, 5 * GRID, 10 * GRID], size=(R, T)).astype(np.int64), axis=1)
    req = rng.choice([0, 0, 400, 999, 1000, 1500, 2000, 3000], size=(R, T)).astype(np.int32)
    who = rng.integers(0, U, (R, T)).astype(np.int32)
    uu, ud = (rng.integers(0, 3, U) * GRID).astype(np.int64), (rng.integers(0, 3, U) * GRID).astype(np.int64)
    return dict(arrive=arrive, req=req, mips=mips, dl=dl, ul=ul, init=init), who, uu, ud


def tie_case(N, T=300, U=4, R=2):
    key = ("tie", N, T, U, R)
    if key not in _cache:
        tr, who, uu, ud = tie_trace(0x71E + N, R, N, T, U)
        _cache[key] = (tr, replay_oracle(tr), who, uu, ud)
    return _cache[key]


def level_counts(want, N, U):
    """Adjacent pairs of every user's merged sequence that each level of the key decided."""
    n = [0] * len(sv.LEVELS)
    for vec in want["rows"]:
        for u in range(U):
            for j, c in enumerate(sv.deciding_levels(sv.user_sequence(vec, N, U, u))):
                n[j] += c
    return n


def herded_case():
    """node_stats_ref.herded_trace: most rows on node 0, some queueTime emissions lost to the
    simtime_t range (no row)."""
    if "herd" not in _cache:
        tr = ns.herded_trace(N=64, T=320, burst=260)
        _cache["herd"] = (tr, replay_oracle(tr), draw_users(0xE, 1, 320, 3, "rr"), *draw_links(0xF, 1, 3, False))
    return _cache["herd"]


# ---------------------------------------------------------------- the order, against the reference's runs

def test_order_rule_holds_on_every_recorded_run():
    """Every ack that reached a user in the reference's own runs, in the reference's own sequence,
    equals the restatement's rows vector by vector and as one sequence per user; every queueTime
    emission per node and every delay emission likewise.  A run the reference aborted defines the
    rows before its abort tick (fognet_hip.h "Reference signal values")."""
    cases = recording_cases()
    acks = tied = 0
    levels = [0] * len(sv.LEVELS)
    for name, tr, o, who, uu, ud, rec in cases:
        N, U = len(tr["dl"]), len(uu)
        want = sv.expected(tr, o, who, uu, ud, with_rows=True)
        vec = want["rows"][0]
        end = rec["abort"]["tick"] if rec["abort"] else None
        before = lambda rows: [row for row in rows if end is None or row[1] < end]
        status_of = lambda row: rec["status"][row[3]] if row[4] == sv.FIRST else sv.ACK_STATUS[row[4]]
        for u in range(U):
            mine = [tuple(a) for a in rec["user_acks"] if who[0, a[0]] == u]
            for v, status in ((N + 1 + u, 5), (N + 1 + U + u, 4), (N + 1 + 2 * U + u, 6)):
                got = [(row[3], status_of(row), row[1]) for row in before(vec[v])]
                assert got == [a for a in mine if a[1] == status], (name, u, status)
            seq = before(sv.user_sequence(vec, N, U, u))
            assert [(row[3], status_of(row), row[1]) for row in seq] == mine, (name, u)
            acks += len(seq)
            tied += sv.same_tick_rows(seq)
            levels = [a + b for a, b in zip(levels, sv.deciding_levels(seq))]
        for k in range(N):
            got = [(row[2], row[1], k, row[3]) for row in before(vec[k])]
            assert got == [tuple(e) for e in rec["qtime"] if e[2] == k], (name, k)
            assert [row[1] for row in vec[k]] == sorted(row[1] for row in vec[k]), (name, k)  # FIFO
        assert [row[2] for row in vec[N]] == rec["delay"] and [row[3] for row in vec[N]] == list(range(len(rec["delay"])))
    assert len(cases) == 14 and acks == sum(len(c[6]["user_acks"]) for c in cases) and acks >= 3900
    assert tied >= 800, tied  # not an empty comparison: acks inside same-tick groups
    assert all(n > 0 for n in levels), dict(zip(sv.LEVELS, levels))


def test_tie_cases_exercise_every_level_of_the_key():
    for N in (1, 3, 5):
        tr, o, who, uu, ud = tie_case(N)
        assert (o["stats"]["status"] == 0).all()
        want = sv.expected(tr, o, who, uu, ud, with_rows=True)
        n = level_counts(want, N, len(uu))
        # (with one node, acks of one user at one time left the node at one tick: the send tick cannot decide)
        assert all(c > 0 for lv, c in zip(sv.LEVELS, n) if N > 1 or lv != "send tick"), (N, dict(zip(sv.LEVELS, n)))


# ---------------------------------------------------------------- the rows, against the records

def check_rows_against_records(tr, o, who, uu, ud):
    """count, sum, min and max of every vector's rows equal the matching per-node / per-user
    record; times within a vector are nondecreasing; offsets are the running row counts."""
    want = sv.expected(tr, o, who, uu, ud)
    nodes = ns.expected(tr, o)
    users, _ = pu.expected(tr, o, who, uu, ud)
    R, N, U = nodes.shape[0], nodes.shape[1], users.shape[1]
    for r in range(R):
        off = want["offset"][r]
        assert off[0] == 0 and (np.diff(off) >= 0).all()

        def check(v, mom):
            vals = [int(x) for x in want["value"][r][off[v]:off[v + 1]]]
            assert len(vals) == mom.n and sum(vals) == mom.s, (r, v)
            assert (min(vals), max(vals)) == (mom.mn, mom.mx) if vals else (mom.mn, mom.mx) == (ns.I64_MAX, ns.I64_MIN)
            t = want["time"][r][off[v]:off[v + 1]]
            assert (np.diff(t) >= 0).all(), (r, v)
        for k in range(N):
            check(k, ns.Mom.load(nodes[r, k]["queue"]))
        delay = pu.load_mom(pu.merged(users[r])["delay"]) if U else None
        if U:
            check(N, delay)
        for s, sig in enumerate(("latency", "latencyH1", "taskTime")):
            for u in range(U):
                check(N + 1 + s * U + u, pu.load_mom(users[r, u][sig]))
    return want


@pytest.mark.parametrize("N,T,U", [(1, 65, 1), (5, 129, 3), (64, 300, 10)])
def test_rows_equal_the_records_on_oracle_runs(N, T, U):
    tr, o = trace_case(N, T)
    for per_rep in (False, True):
        check_rows_against_records(tr, o, draw_users(T + U, 3, T, U, "random"), *draw_links(T + U + 1, 3, U, per_rep))


def test_rows_equal_the_records_mqtt_down_herded_and_ties():
    tr, who, uu, ud = mqtt_case(3)
    check_rows_against_records(tr, replay_oracle(tr), who, uu, ud)
    tr = down_trace()
    o = replay_oracle(tr)
    assert (o["status"] == 9).any()
    check_rows_against_records(tr, o, draw_users(0xD0, 3, 257, 10, "rr"), *draw_links(0xD1, 3, 10, True))
    tr, o, who, uu, ud = herded_case()
    want = check_rows_against_records(tr, o, who, uu, ud)
    assert int(o["stats"]["n_qtime_overflow"][0]) > 0  # lost emissions are no rows
    assert int(want["offset"][0][1]) > 100 and 2 * int(want["offset"][0][1]) > int(want["offset"][0][64])  # most on node 0
    check_rows_against_records(*tie_case(3))


def test_unassigned_users_give_no_user_side_row():
    tr, o = trace_case(5, 65)
    who = draw_users(1, 3, 65, 4, "rr")
    who[0, [3, 17, 64]] = (-1, 4, 2**31 - 1)
    uu, ud = draw_links(2, 3, 4, False)
    want = sv.expected(tr, o, who, uu, ud)
    full = sv.expected(tr, o, draw_users(1, 3, 65, 4, "rr"), uu, ud)
    assert int(want["offset"][0][6] - want["offset"][0][5]) == 62 and int(full["offset"][0][6] - full["offset"][0][5]) == 65
    np.testing.assert_array_equal(want["offset"][0][:6], full["offset"][0][:6])  # the queueTime vectors stay


# ---------------------------------------------------------------- the .vec writer

def small_csr():
    """U = 2 after N = 3 nodes: delay 3 rows, latency (1, 0), latencyH1 (2, 1), taskTime (0, 2)."""
    off = np.array([4, 7, 8, 8, 10, 11, 11, 13], np.int64)  # from the delay vector on; 4 queueTime rows before
    time = np.arange(13, dtype=np.int64) * 250 * MS + 1
    time[7] = 2 * 10**12  # a whole second
    value = np.array([0, 0, 0, 0, MS, 2 * MS, MS, 5 * 10**12, 6 * 10**12, 6 * 10**12 + 1, 7 * 10**12, 3 * 10**15, -1000], np.int64)
    return off, time, value


def test_write_vec_users_golden_text(tmp_path):
    off, time, value = small_csr()
    path = str(tmp_path / "u.vec")
    formats.write_vec_users(path, off, time, value, U=2, id_base=4, network="Net", user_module=["user[0]", "usr"])
    text = open(path).read()
    head = "version 2\nrun General-0-fognet\n"
    assert text.startswith(head) and text.count("version 2") == 1
    decl = lambda i, mod, name: (f"vector {i}  Net.{mod}.udpApp[0]  {name}:vector  TV\nattr interpolationmode  none\n"
                                 f"attr source  {name}\nattr title  \"{name}, vector\"\n")
    want = decl(4, "broker", "delay") + "".join(decl(5 + 3 * u + s, mod, name) for u, mod in enumerate(("user[0]", "usr"))
                                                 for s, name in enumerate(("latency", "latencyH1", "taskTime")))
    want += ("4\t1.000000000001\t0.001\n4\t1.250000000001\t0.002\n4\t1.500000000001\t0.001\n"  # delay (s)
             "5\t2\t5\n"                                                                         # user[0] latency (ms)
             "6\t2.000000000001\t6\n6\t2.250000000001\t6.000000000001\n"                         # user[0] latencyH1
             "9\t2.500000000001\t7\n"                                                            # usr latencyH1
             "10\t2.750000000001\t3000\n10\t3.000000000001\t-1e-09\n")                           # usr taskTime
    assert text[text.index("vector 4"):] == want
    # (the last line of the header block is the blank-free run header of the other writers)
    other = str(tmp_path / "v.vec")
    formats.write_vec(other, [MS], [MS], [0], [5], [MS], network="Net")
    assert open(other).read().split("vector")[0] == text.split("vector")[0]


def test_write_vec_users_appends_after_write_vec_with_id_base_and_zero_row_vectors(tmp_path):
    path, alone = str(tmp_path / "a.vec"), str(tmp_path / "alone.vec")
    formats.write_vec(path, [MS, 2 * MS], [MS, MS, MS], [0, 1], [5, 4], [2 * MS, 3 * MS])
    before = open(path, "rb").read()
    off, time, value = small_csr()
    formats.write_vec_users(path, off, time, value, U=2, id_base=4, append=True)
    formats.write_vec_users(alone, off, time, value, U=2, id_base=4)
    after, created = open(path, "rb").read(), open(alone, "rb").read()
    assert after.startswith(before) and after.count(b"version 2") == 1 and created.count(b"version 2") == 1
    assert created.endswith(after[len(before):])
    lines = after.decode().splitlines()
    ids = [int(ln.split()[1]) for ln in lines if ln.startswith("vector ")]
    assert ids == list(range(0, 11)) and len(set(ids)) == 11  # 0: decision, 1-3: queueTime, 4: delay, 5-10: the users
    names = [ln.split()[2] for ln in lines if ln.startswith("vector ")][4:]
    assert names == ["FogNet.broker.udpApp[0]"] + ["FogNet.user[0].udpApp[0]"] * 3 + ["FogNet.user[1].udpApp[0]"] * 3
    data = [ln for ln in after[len(before):].decode().splitlines() if ln[0].isdigit()]
    by_id = {i: [ln for ln in data if ln.split("\t")[0] == str(i)] for i in range(4, 11)}
    assert [len(by_id[i]) for i in range(4, 11)] == [3, 1, 2, 0, 0, 1, 2]  # zero-row vectors are declared, no data
    # another id_base moves every id; all-empty vectors write declarations only
    formats.write_vec_users(alone, np.zeros(8, np.int64), [], [], U=2, id_base=100)
    text = open(alone).read()
    assert [int(ln.split()[1]) for ln in text.splitlines() if ln.startswith("vector ")] == list(range(100, 107))
    assert not [ln for ln in text.splitlines() if ln[:1].isdigit()]
    formats.write_vec_users(alone, np.zeros(2, np.int64), [], [], U=0)  # the broker's delay alone
    assert sum(ln.startswith("vector ") for ln in open(alone).read().splitlines()) == 1
    with pytest.raises(fa.FognetError) as e:
        formats.write_vec_users(str(tmp_path / "no" / "such" / "dir.vec"), off, time, value, U=2)
    assert e.value.code == abi.FOGNET_ERR_ARG and b"cannot open" in abi.load().fognet_io_last_error()
    with pytest.raises(fa.FognetError):
        formats.write_vec_users(alone, off[:-1], time, value, U=2)
    with pytest.raises(fa.FognetError):
        formats.write_vec_users(alone, off, time, value, U=2, user_module=["a"])
    bad = off.copy()
    bad[3] = 2
    with pytest.raises(fa.FognetError) as e:
        formats.write_vec_users(alone, bad, time, value, U=2)
    assert e.value.code == abi.FOGNET_ERR_ARG and b"nondecreasing" in abi.load().fognet_io_last_error()


# ---------------------------------------------------------------- the driver's refusals

@pytest.mark.parametrize("args,msg", [
    (("--users", "user[3]", "--vec-users"), "--vec-users appends to replication 0's .vec"),
    (("-c", "Example", "--nodes", "5", "--vec", "x.vec", "--vec-users"), "--vec-users applies to BrokerBaseApp3 runs"),
    (("--users", "user[3]", "--vec", "x.vec", "--vec-users", "--user-dl", "none"), "--vec-users needs a broker->user latency"),
])
def test_driver_refusals(tmp_path, args, msg):
    args = [str(tmp_path / a) if a == "x.vec" else a for a in args]
    p = drive("-f", INI, *args, "--dry-run", check=False)
    assert p.returncode == 2 and msg in p.stderr, (p.returncode, p.stderr)
    assert not (tmp_path / "x.vec").exists()


def test_driver_refuses_a_trace_file(tmp_path):
    trc = str(tmp_path / "t.fogntrc")
    tr = tg.make_batch(7, 1, 5, 20, rho=0.5)
    formats.save_trace(trc, tr)
    p = drive("--trace", trc, "--vec", str(tmp_path / "x.vec"), "--vec-users", "--dry-run", check=False)
    assert p.returncode == 2 and "a trace file names no users" in p.stderr, (p.returncode, p.stderr)
