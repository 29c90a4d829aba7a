"""Per-user signals, host side (no GPU): the host identity and exact merge of
fognet_user_stats, the test-side record builder (per_user_ref) against the oracle's
event-level records, the `.sca` writer of per-user blocks, and the driver's refusals.
The cases here are the ones test_per_user_stats_gpu.py runs on the device."""
import ctypes
import random
from fractions import Fraction

import numpy as np
import pytest

import fognetsimpp_amd as fa
import fognetsimpp_amd._abi as abi
import oracle_lib as ol
import per_user_ref as pu
import tracegen as tg
import user_stats_ref as us
from fognetsimpp_amd import formats
from test_driver import INI, drive
from test_node_stats import blocks, fmt, want_fields

MS = 10**9
USER = abi.USER_STATS_DTYPE
assert USER == us.USER_STATS_DTYPE and USER.itemsize == 288
_cache: dict = {}


# ---------------------------------------------------------------- the cases (shared with the GPU tests)

def replay_oracle(tr, policy="REF_V3", uu=None, ud=None, **kw):
    return ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], threads=4, user_ul=uu,
                        user_dl=ud, policy=ol.POLICIES[policy], down=tr.get("down"), region=tr.get("region"), **kw)


def trace_case(N, T, policy="REF_V3", R=3):
    """(trace, oracle result) of a tracegen batch, computed once per key and left unchanged
    (the replay does not depend on the users)."""
    key = ("trace", N, T, policy, R)
    if key not in _cache:
        tr = tg.make_batch(0x9E5 + 7 * N + T, R, N, T, rho=0.9)
        _cache[key] = (tr, replay_oracle(tr, policy))
    return _cache[key]


def draw_users(seed, R, T, U, kind):
    """user_of [R, T] int32: "rr" round-robin from a per-replication offset (mqttApp2's users
    publish in turn), "random" uniform over the users but the last (so U > 1 has a user
    without a publish)."""
    rng = np.random.default_rng(seed)
    if kind == "rr":
        return ((np.arange(T)[None, :] + 3 * np.arange(R)[:, None]) % U).astype(np.int32)
    return rng.integers(0, max(U - 1, 1), (R, T)).astype(np.int32)


def draw_links(seed, R, U, per_rep):
    """Links in [0, 5 ms): [U], or [R, U] per replication."""
    rng = np.random.default_rng(seed)
    shape = (R, U) if per_rep else (U,)
    return rng.integers(0, 5 * MS, shape).astype(np.int64), rng.integers(0, 5 * MS, shape).astype(np.int64)


def mqtt_case(U, R=3, N=5):
    """R replications from the reference task source (fognet_gen_trace_mqtt, glibc seeds
    1 .. R) with its user_of: U users 50-59 ms apart, started 100 ms in, with links
    [U] of 1-4 ms; N nodes of 1000-4000 MIPS 1 ms away.  (trace, user_of, ul, dl)."""
    key = ("mqtt", U, R, N)
    if key not in _cache:
        uu = ((1 + np.arange(U) % 4) * MS + 1000 * np.arange(U)).astype(np.int64)
        ud = ((1 + (np.arange(U) + 1) % 4) * MS + 7 * np.arange(U)).astype(np.int64)
        start = np.full(U, 100 * MS, np.int64)
        interval = ((50 + np.arange(U) % 10) * MS).astype(np.int64)
        reps = [formats.gen_trace_mqtt(1 + r, start, interval, uu, ud, stop=1600 * MS)
                for r in range(R)]
        assert len({len(g["arrive"]) for g in reps}) == 1
        n = np.full(N, MS, np.int64)
        tr = dict(arrive=np.stack([g["arrive"] for g in reps]), req=np.stack([g["req"] for g in reps]),
                  mips=(1000 * (1 + np.arange(N) % 4)).astype(np.int32), dl=n, ul=n.copy(), init=np.full(N, 50 * MS, np.int64))
        _cache[key] = (tr, np.stack([g["user"] for g in reps]).astype(np.int32), uu, ud)
    return _cache[key]


def grouping_trace(T):
    """One replication of T publishes 20 ms apart over five 1000-MIPS nodes."""
    n = np.full(5, MS, np.int64)
    return dict(arrive=(100 * MS + 20 * MS * np.arange(T, dtype=np.int64))[None],
                req=(1000 + 37 * np.arange(T) % 3000).astype(np.int32)[None], mips=np.full(5, 1000, np.int32), dl=n,
                ul=n.copy(), init=n.copy())


def staircase_users():
    """One 64-task step whose users own 1, 2, ..., 10 and 9 tasks (64 in all), interleaved:
    every group size a grouping threshold up to 10 can split at."""
    who = [u for u, m in enumerate(list(range(1, 11)) + [9]) for _ in range(m)]
    assert len(who) == 64
    return np.random.default_rng(64).permutation(np.array(who, np.int32))[None]


B = 2**63 // 1000  # the largest d whose exact d * 1000 is still below 2^63


def carry_case():
    """Links around 2^53 (the conversion starts to round) and around 2^63 / 1000 (the
    product leaves the range), and user 0 with links whose sum puts every pubAck value in
    [2^62, 2^63): its eight and more emissions carry into sum_hi, sq_hi and sq_top."""
    T = 96
    tr = grouping_trace(T)
    uu = np.array([B // 2 - 10**12, 2**52, 2**53 - 1, B // 2, B - 5, 1 * MS, B // 2 + 40], np.int64)
    ud = np.array([B // 4, 2**52 + 1, 3, B // 2 - 2, 4, 2 * MS, B // 2 + 40], np.int64)
    who = (np.arange(T) % 9 % 7).astype(np.int32)[None]  # users 0 and 1 own the most
    return tr, who, uu, ud


def down_trace():
    from test_user_stats import down_case
    return down_case()[0]


def merged_rows(recs) -> np.ndarray:
    """[R, U] records -> [R] merges."""
    return np.array([pu.merged(recs[r]) for r in range(recs.shape[0])], USER)


def check_against_oracle_events(tr, who, uu, ud, policy="REF_V3", **kw):
    """The helper's U records merge to the oracle's event-level record with the per-task
    links expanded from user_of."""
    tu, td = pu.expand_links(who, uu, ud)
    o = replay_oracle(tr, policy, tu, td, **kw)
    want, un = pu.expected(tr, o, who, uu, ud)
    assert (un == 0).all()
    us.assert_user_parity(merged_rows(want), o["user"])
    return o, want


# ---------------------------------------------------------------- host identity and merge

def c_rec(rec) -> abi.UserStats:
    return abi.UserStats.from_buffer_copy(np.ascontiguousarray(rec).tobytes())


def np_rec(c) -> np.ndarray:
    return np.frombuffer(bytes(c), dtype=USER)[0]


def host_merge(a, b) -> np.ndarray:
    x, y = c_rec(a), c_rec(b)
    abi.load().fognet_user_stats_merge(ctypes.byref(x), ctypes.byref(y))
    return np_rec(x)


def make(**signals) -> np.ndarray:
    m = {s: us.Mom() for s in us.SIGNALS}
    for s, vals in signals.items():
        for v in vals:
            m[s].add(v)
    return us.to_record(m)


def test_init_is_the_empty_record_and_the_identity():
    s = abi.UserStats()
    ctypes.memset(ctypes.byref(s), 0x5A, ctypes.sizeof(s))
    abi.load().fognet_user_stats_init(ctypes.byref(s))
    empty = np_rec(s)
    assert empty.tobytes() == us.empty_record().tobytes()
    x = make(delay=(5, 7), latency=(-3, 2**62), latencyH1=(10**15,), taskTime=(1, 2, 3))
    x["taskTime"]["overflow"] = 4
    assert host_merge(empty, x).tobytes() == x.tobytes() == host_merge(x, empty).tobytes()


def test_merge_is_exact_with_carries():
    big = 2**63 - 1
    a, b = make(latency=(big, big)), make(latency=(big, big, big))  # a sum_lo carry; squares ~2^126 each
    m = pu.load_mom(host_merge(a, b)["latency"])
    assert m.s == 5 * big and m.s >> 64 and m.q == 5 * big * big and m.q >> 128 and m.n == 5
    top = make()
    top["taskTime"]["sq_lo"], top["taskTime"]["sq_hi"] = 2**64 - 1, 2**64 - 1  # the carry runs through sq_hi into sq_top
    one = make()
    one["taskTime"]["sq_lo"] = 1
    got = host_merge(top, one)["taskTime"]
    assert (int(got["sq_lo"]), int(got["sq_hi"]), int(got["sq_top"])) == (0, 0, 1)
    hi = make()
    hi["latencyH1"]["sq_hi"] = 2**64 - 1  # sq_hi -> sq_top without a carry from below
    got = host_merge(hi, hi)["latencyH1"]
    assert (int(got["sq_lo"]), int(got["sq_hi"]), int(got["sq_top"])) == (0, 2**64 - 2, 1)
    neg = host_merge(make(delay=(-5, 3)), make(delay=(-2**62,)))["delay"]
    assert pu.load_mom(neg).s == -2 - 2**62 and (int(neg["min_raw"]), int(neg["max_raw"])) == (-2**62, 3)
    assert int(host_merge(make(delay=(-5,)), make())["delay"]["sum_hi"]) == 2**64 - 1  # two's complement
    # every signal is merged, each into its own
    x = host_merge(make(delay=(1,), latency=(2,)), make(latencyH1=(3,), taskTime=(4,), delay=(5,)))
    assert [int(x[s]["count"]) for s in us.SIGNALS] == [2, 1, 1, 1]
    assert [pu.load_mom(x[s]).s for s in us.SIGNALS] == [6, 2, 3, 4]


def random_records(rng, *shape) -> np.ndarray:
    recs = np.zeros(shape, USER)
    flat = recs.view(np.uint64).reshape(*shape, USER.itemsize // 8)
    flat[:] = np.frombuffer(rng.randbytes(flat.nbytes), np.uint64).reshape(flat.shape)
    for s in us.SIGNALS:
        recs[s]["count"] >>= 24  # counts that cannot overflow int64 when summed
        recs[s]["overflow"] >>= 24
        recs[s]["sq_top"] >>= np.uint64(16)
    return recs


def test_merge_is_commutative_and_exact_on_random_limbs():
    rng = random.Random(11)
    recs = random_records(rng, 100, 2)
    for a, b in recs:
        ab = host_merge(a, b)
        assert ab.tobytes() == host_merge(b, a).tobytes() == pu.merged([a, b], wrap=True).tobytes()
    got = fa.merge_user_stats([recs[:, 0], recs[:, 1]])
    assert got.tobytes() == np.array([pu.merged(p, wrap=True) for p in recs], USER).tobytes()


# ---------------------------------------------------------------- the helper against the oracle's events

@pytest.mark.parametrize("U", [3, 10])
def test_helper_merges_to_oracle_events_mqtt_users(U):
    tr, who, uu, ud = mqtt_case(U)
    assert who.min() == 0 and who.max() == U - 1 and tr["arrive"].shape[1] >= 60
    o, want = check_against_oracle_events(tr, who, uu, ud)
    assert (o["stats"]["status"] == 0).all()
    np.testing.assert_array_equal(want["delay"]["count"], np.stack([np.bincount(w, minlength=U) for w in who]))
    for u in range(U):  # a user's delay is its uplink, every time
        assert (want["delay"]["min_raw"][:, u] == uu[u]).all() and (want["delay"]["max_raw"][:, u] == uu[u]).all()


@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
@pytest.mark.parametrize("U,per_rep,kind", [(1, False, "rr"), (7, True, "random"), (65, False, "random"), (200, True, "rr")])
def test_helper_merges_to_oracle_events_random(U, per_rep, kind, policy):
    tr, _ = trace_case(5, 191, policy)
    who = draw_users(U, 3, 191, U, kind)
    uu, ud = draw_links(U + 1, 3, U, per_rep)
    o, want = check_against_oracle_events(tr, who, uu, ud, policy)
    assert (o["status"] == 4).any() and (o["status"] == 5).any()
    if U > 1:
        assert (want["delay"]["count"] == 0).any()  # a user without a publish: the empty record
        r, u = np.argwhere(want["delay"]["count"] == 0)[0]
        assert us.is_empty(want[r, u])


def test_helper_special_cases_merge_to_oracle_events():
    tr, who, uu, ud = carry_case()
    o, want = check_against_oracle_events(tr, who, uu, ud)
    h1 = want[0, 0]["latencyH1"]
    assert int(h1["count"]) >= 8 and int(h1["min_raw"]) >= 2**62 and int(h1["sum_hi"]) and int(h1["sq_hi"]) and int(h1["sq_top"])
    assert sum(int(want[0, u][s]["overflow"]) for u in range(7) for s in us.SIGNALS) > 0
    tr = down_trace()
    who = draw_users(0xD0, 3, 257, 10, "rr")
    uu, ud = draw_links(0xD1, 3, 10, True)
    o, want = check_against_oracle_events(tr, who, uu, ud)
    assert (o["status"] == 9).any() and ((o["status"] != 9) & (o["done"] == -1)).any()
    tr = grouping_trace(64)
    check_against_oracle_events(tr, staircase_users(), *draw_links(5, 1, 11, False))


def test_helper_counts_out_of_range_users_and_empties_failed_replications():
    tr, o = trace_case(5, 65)
    who = draw_users(1, 3, 65, 4, "rr")
    bad = who.copy()
    bad[0, [3, 17, 64]] = (-1, 4, 2**31 - 1)
    uu, ud = draw_links(2, 3, 4, False)
    want, un = pu.expected(tr, o, who, uu, ud)
    got, un_bad = pu.expected(tr, o, bad, uu, ud)
    assert list(un) == [0, 0, 0] and list(un_bad) == [3, 0, 0]
    assert int(got["delay"]["count"][0].sum()) == 62 and got[1:].tobytes() == want[1:].tobytes()
    failed, un = pu.expected(tr, o, bad, uu, ud, statuses=[1, 0, 9])
    assert failed[0].tobytes() == pu.empty_records(4).tobytes() and list(un) == [0, 0, 0]
    assert failed[2].tobytes() == want[2].tobytes()  # a REF_ABORTED one keeps its full records


# ---------------------------------------------------------------- the .sca writer

def test_write_sca_users_names_fields_and_empty_user(tmp_path):
    big = 2**63 - 1000
    m = {s: us.Mom() for s in us.SIGNALS}
    for v in (big, big - 10**15, big - 7 * 10**17, 1000, big - 3, big - 1, big - 10**18):  # sum_hi and sq_top in use
        m["latencyH1"].add(v)
    m["latencyH1"].ovf = 2
    for v in (5 * 10**12, 7 * 10**12 + 1):
        m["latency"].add(v)
    m["taskTime"].add(3 * 10**15)
    for v in (2 * MS, 2 * MS, 2 * MS):
        m["delay"].add(v)
    assert m["latencyH1"].s >> 64 and m["latencyH1"].q >> 128
    m2 = {s: us.Mom() for s in us.SIGNALS}
    m2["delay"].add(5 * MS)
    recs = np.array([us.to_record(m), us.empty_record(), us.to_record(m2)], USER)
    path = str(tmp_path / "u.sca")
    formats.write_sca_users(path, recs, network="Net")
    text = open(path).read()
    assert text.startswith("version 2\nrun General-0-fognet\n") and text.count("version 2") == 1
    b = blocks(text)
    assert sorted(b) == ["Net.broker.udpApp[0]"] + [f"Net.user[{u}].udpApp[0]" for u in range(3)]
    u0 = b["Net.user[0].udpApp[0]"]
    assert sorted(k for k in u0 if k != "scalars") == ["latency:stats", "latencyH1:stats", "taskTime:stats"]
    unit = Fraction(1, 10**12)
    for sig in ("latency", "latencyH1", "taskTime"):
        w = want_fields(m[sig], unit)
        for k in ("count", "mean", "stddev", "sum", "sqrsum"):
            assert u0[sig + ":stats"][k] == w[k], (sig, k)
    assert u0["latencyH1:stats"]["min"] == fmt(1000 * 1e-12) and u0["latencyH1:stats"]["max"] == fmt(float(big - 1) * 1e-12)
    assert u0["taskTime:stats"]["stddev"] == "-nan" and u0["taskTime:stats"]["mean"] == fmt(3 * 10**15 * 1e-12)
    assert u0["scalars"] == {"latencyH1 emissions lost": "2"}  # only where overflow > 0
    u1 = b["Net.user[1].udpApp[0]"]  # a user without an emission: count 0 statistics
    assert u1["scalars"] == {} and all(u1[s + ":stats"]["count"] == "0" and u1[s + ":stats"]["mean"] == "-nan"
                                       for s in ("latency", "latencyH1", "taskTime"))
    # delay is the broker's, from the merge of the users' shares, in s
    d = b["Net.broker.udpApp[0]"]["delay:stats"]
    md = pu.load_mom(pu.merged(recs)["delay"])
    assert md.n == 4 and d == dict(want_fields(md, unit), min=fmt(2 * MS * 1e-12), max=fmt(5 * MS * 1e-12))
    assert "delay:stats" not in u0
    # custom module names
    formats.write_sca_users(path, recs, user_module=["user[3]", "usr[0]", "gw"], network="Net")
    assert sorted(blocks(open(path).read())) == ["Net.broker.udpApp[0]", "Net.gw.udpApp[0]", "Net.user[3].udpApp[0]",
                                                  "Net.usr[0].udpApp[0]"]


def test_write_sca_users_append_and_errors(tmp_path):
    job = fa.job_from_reps(np.zeros(0, abi.REP_STATS_DTYPE))
    path, alone = str(tmp_path / "job.sca"), str(tmp_path / "alone.sca")
    formats.write_sca(path, job, hist=np.zeros((2, 64), np.int64))
    before = open(path, "rb").read()
    recs = pu.empty_records(3)
    formats.write_sca_users(path, recs, append=True)
    formats.write_sca_users(alone, recs)
    after, created = open(path, "rb").read(), open(alone, "rb").read()
    assert after.startswith(before) and after.count(b"version 2") == 1 and after.count(b"\nrun ") + after.startswith(b"run ") == 1
    assert created.count(b"version 2") == 1 and created.endswith(after[len(before):])  # the same blocks after one header
    assert sorted(blocks(after[len(before):].decode())) == ["FogNet.broker.udpApp[0]"] + [f"FogNet.user[{u}].udpApp[0]" for u in range(3)]
    with pytest.raises(fa.FognetError) as e:
        formats.write_sca_users(str(tmp_path / "no" / "such" / "dir.sca"), recs)
    assert e.value.code == abi.FOGNET_ERR_ARG and b"cannot open" in abi.load().fognet_io_last_error()
    with pytest.raises(fa.FognetError):
        formats.write_sca_users(path, recs, user_module=["a"])


# ---------------------------------------------------------------- the driver's refusals

@pytest.mark.parametrize("args,msg", [
    (("--users", "user[3]", "--user-stats"), "--user-stats appends to the job's .sca"),
    (("-c", "Example", "--nodes", "5", "--sca", "x.sca", "--user-stats"), "--user-stats applies to BrokerBaseApp3 runs"),
    (("--users", "user[3]", "--reps", "4", "--sca", "x.sca", "--user-stats", "--world", "2", "--comm-id", "c.id"),
     "--user-stats: the per-user records of several ranks are not combined"),
])
def test_driver_refusals(tmp_path, args, msg):
    args = [str(tmp_path / a) if a in ("x.sca", "c.id") else a for a in args]
    p = drive("-f", INI, *args, "--dry-run", check=False)
    assert p.returncode == 2 and msg in p.stderr, (p.returncode, p.stderr)
    assert not (tmp_path / "x.sca").exists()
