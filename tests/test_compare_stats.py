"""Paired comparison of two replays, host side (no GPU): symbols and layout of
fognet_compare_stats, the exact host merge against the plain-integer reference (compare_ref),
the `.sca` writer parsed back, the driver's refusals, and the reference's identities on the
oracle's outputs of one trace under two policies."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import compare_ref as cr
import fognetsimpp_amd as fa
import fognetsimpp_amd._abi as abi
import oracle_lib as ol
import tracegen as tg
from fognetsimpp_amd import formats
from test_driver import INI, drive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMP = abi.COMPARE_STATS_DTYPE


# ---------------------------------------------------------------- layout, symbols, ABI version

def test_compare_stats_layout_matches_header(tmp_path):
    fields = [f for f, _ in abi.CompareStats._fields_]
    lines = ['printf("size %zu\\n", sizeof(fognet_compare_stats));', 'printf("abi %d\\n", FOGNET_ABI_VERSION);',
             'printf("trans_size %zu\\n", sizeof(((fognet_compare_stats*)0)->trans));']
    lines += [f'printf("{f} %zu\\n", offsetof(fognet_compare_stats, {f}));' for f in fields]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fognet_hip.h\"\nint main(void){" + "\n".join(lines) +
                   "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.CompareStats) == CMP.itemsize == 400
    assert int(got["trans_size"]) == 9 * 8 and int(got["abi"]) == 10
    for f in fields:
        assert int(got[f]) == getattr(abi.CompareStats, f).offset == CMP.fields[f][1], f


def test_symbols_and_abi_version():
    lib = abi.load()
    assert lib.fognet_abi_version() == 10  # the ABI grew by additions only
    for name in ("fognet_compare_dev", "fognet_reduce_compare_dev", "fognet_compare_stats_init",
                 "fognet_compare_stats_merge", "fognet_write_sca_compare"):
        assert name in abi.SIGNATURES and getattr(lib, name)
    for name in ("compare", "reduce_compare", "merge_compare"):
        assert callable(getattr(fa, name)) and name in fa.__all__
    header = open(os.path.join(ROOT, "include", "fognet_hip.h")).read()
    assert "Paired comparison" in header and "#define FOGNET_ABI_VERSION 10" in header


# ---------------------------------------------------------------- host identity and merge

def mom(count=0, mn=cr.I64_MAX, mx=cr.I64_MIN, s=0, sq=0) -> dict:
    return dict(count=count, min=mn, max=mx, sum=s, sq=sq)


def hand(status=(0, 0), trans=None, **kw) -> dict:
    d = cr.empty(*status)
    if trans is not None:
        d["trans"] = trans
    d.update(kw)
    return d


def host_merge(dicts) -> np.ndarray:
    return fa.merge_compare(cr.to_records(dicts))


def test_init_is_the_empty_record():
    s = abi.CompareStats()
    ctypes.memset(ctypes.byref(s), 0x5A, ctypes.sizeof(s))
    abi.load().fognet_compare_stats_init(ctypes.byref(s))
    assert bytes(s) == cr.to_record(cr.empty()).tobytes()
    assert s.status_a == s.status_b == 0 and s.n_reps == 0 and s.d_resp.min_raw == cr.I64_MAX and s.d_resp.max_raw == cr.I64_MIN


def test_merge_is_exact_with_limb_carries_and_negative_sums():
    big = 2**62 - 1
    a = hand(n_reps=1, n_pairs=70, n_moved=3, trans=[[1, 2, 3], [4, 5, 6], [7, 8, 9]], n_done_both=65, n_done_only_a=2,
             n_done_only_b=1, n_done_neither=2, n_better=60, n_equal=1, n_worse=4, rep_better=1,
             d_start=mom(65, -big, 5, -(2**64) - 7, 2**128 - 1),          # the sum's low limb borrows, sq fills two limbs
             d_service=mom(65, -3, big, 2**64 - 1, 2**64 - 1),
             d_resp=mom(65, -big, big, -65 * big, 65 * big * big))
    b = hand(n_reps=1, n_pairs=5, n_moved=5, trans=[[9, 8, 7], [6, 5, 4], [3, 2, 1]], n_done_both=3, n_worse=3, rep_worse=1,
             d_start=mom(3, -9, 9, -(2**64), 1),                           # sum: both limbs move; sq: carries into the top limb
             d_service=mom(3, -4, 1, 1, 1),                                # sum and sq: carry out of the low limb
             d_resp=mom(3, 1, big, 3 * big, 2**191))
    c = hand(status=(9, 9), n_reps=1, n_pairs=1, n_done_both=1, n_equal=1, rep_equal=1, d_start=mom(1, 0, 0), d_service=mom(1, 0, 0),
             d_resp=mom(1, 0, 0))
    want = cr.merge(cr.merge(cr.merge(cr.empty(), a), b), c)
    got = host_merge([a, b, c])
    cr.assert_equal(got, cr.to_record(want), "host merge")
    d = cr.from_record(got)
    assert d["d_start"]["sum"] == -(2**65) - 7 and d["d_start"]["sq"] == 2**128 and d["d_service"]["sum"] == 2**64
    assert d["d_resp"]["sum"] == -62 * big and d["d_resp"]["sum"] < 0 and d["d_resp"]["sq"] == (65 * big * big + 2**191) % 2**192
    assert d["n_reps"] == 3 and d["trans"] == [[10] * 3] * 3 and d["status_a"] == d["status_b"] == 0  # acc's statuses stay
    # any order, any grouping
    assert host_merge([c, b, a]).tobytes() == got.tobytes()
    ab, bc = host_merge([a, b]), host_merge([b, c])
    assert fa.merge_compare(np.array([ab, cr.to_record(c)], CMP)).tobytes() == got.tobytes()
    assert fa.merge_compare(np.array([cr.to_record(a), bc], CMP)).tobytes() == got.tobytes()
    assert host_merge([a]).tobytes() == cr.to_record(dict(a)).tobytes()  # the empty record is the identity
    # merge leaves acc's statuses alone
    lib = abi.load()
    acc = abi.CompareStats.from_buffer_copy(cr.to_record(hand(status=(7, 9))).tobytes())
    lib.fognet_compare_stats_merge(ctypes.byref(acc), ctypes.byref(abi.CompareStats.from_buffer_copy(cr.to_record(a).tobytes())))
    assert (acc.status_a, acc.status_b, acc.n_pairs) == (7, 9, 70)


# ---------------------------------------------------------------- the .sca writer

def parse(text: str):
    """(scalars {module: {name: value}}, statistics {(module, name): {field: value, "bins": [...]}})"""
    scal: dict = {}
    stats: dict = {}
    cur = None
    for line in text.splitlines():
        m = re.match(r'^scalar (\S+) \t(\S+) \t(\S+)$', line)
        if m:
            scal.setdefault(m.group(1), {})[m.group(2)] = m.group(3)
            continue
        m = re.match(r'^statistic (\S+) \t(\S+)$', line)
        if m:
            cur = stats.setdefault((m.group(1), m.group(2)), {"bins": []})
            continue
        m = re.match(r'^field (\S+) (\S+)$', line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
        m = re.match(r'^bin\t(\S+)\t(\S+)$', line)
        if m and cur is not None:
            cur["bins"].append((m.group(1), int(m.group(2))))
    return scal, stats


SCALARS = ["compare:replications", "compare:pairs", "compare:moved", "compare:better", "compare:equal", "compare:worse",
           "compare:doneOnlyA", "compare:doneOnlyB", "compare:repsBetter", "compare:repsEqual", "compare:repsWorse"] + \
          [f"compare:status{a}to{b}" for a in (5, 4, 9) for b in (5, 4, 9)]


def check_block(scal: dict, stats: dict, mod: str, d: dict, hist=None):
    """One parsed block against the record it was written from: counts as integers; mean and
    stddev from the exact sums to 1e-13 relative (the %.14g print loses up to 5e-14, the
    long-double arithmetic less than 1e-18)."""
    s = scal[mod]
    assert list(s) == SCALARS
    keys = ["n_reps", "n_pairs", "n_moved", "n_better", "n_equal", "n_worse", "n_done_only_a", "n_done_only_b", "rep_better",
            "rep_equal", "rep_worse"]
    assert [int(s[n]) for n in SCALARS[:11]] == [d[k] for k in keys]
    assert [int(s[n]) for n in SCALARS[11:]] == [d["trans"][i][j] for i in range(3) for j in range(3)]
    for name, sig in (("startDiff", "d_start"), ("serviceDiff", "d_service"), ("responseDiff", "d_resp")):
        st, m = stats[(mod, f"{name}:stats")], d[sig]
        n = m["count"]
        assert int(st["count"]) == n
        if n == 0:
            assert st["mean"] == st["stddev"] == st["min"] == st["max"] == "-nan" and st["sum"] == "0"
            continue
        near = lambda got, exact: abs(Fraction(got) - exact) <= Fraction(1, 10**13) * abs(exact)  # noqa: E731
        assert near(st["mean"], Fraction(m["sum"], n * 10**9)) and near(st["sum"], Fraction(m["sum"], 10**9)), (name, st)
        assert near(st["min"], Fraction(m["min"], 10**9)) and near(st["max"], Fraction(m["max"], 10**9))
        if n >= 2:
            var = Fraction(n * m["sq"] - m["sum"] ** 2, n * (n - 1) * 10**18)
            got = Fraction(st["stddev"])
            assert abs(got * got - var) <= Fraction(3, 10**13) * var, (name, st["stddev"], float(var) ** 0.5)
        else:
            assert st["stddev"] == "-nan"
    if hist is not None:
        for side, name in enumerate(("responseDiff:earlier:histogram", "responseDiff:later:histogram")):
            h = stats[(mod, name)]
            assert int(h["count"]) == sum(hist[side]) and h["mean"] == "-nan"
            assert h["bins"][0] == ("-INF", 0) and [c for _, c in h["bins"][1:]] == list(hist[side])
            assert [lo for lo, _ in h["bins"][1:4]] == ["0", "1", "2"]
    else:
        assert not any("histogram" in k[1] for k in stats if k[0] == mod)


def test_write_sca_compare_parsed_back(tmp_path):
    ms = 10**9
    d = hand(n_reps=3, n_pairs=300, n_moved=17, trans=[[100, 20, 1], [30, 140, 2], [3, 4, 0]], n_done_both=290, n_done_only_a=4,
             n_done_only_b=5, n_done_neither=1, n_better=200, n_equal=10, n_worse=80, rep_better=2, rep_worse=1,
             d_start=mom(290, -7 * ms, 3 * ms, -290 * ms - 12345, 1234567 * ms * ms),
             d_service=mom(290, -2 * ms, 9 * ms, 2**70, 2**140 // 145),
             d_resp=mom(290, -5 * ms, 8 * ms + 1, 2**70 - 290 * ms - 12345, 2**141))
    hist = cr.new_hist()
    hist[0][0], hist[0][3], hist[1][1], hist[1][63] = 150, 50, 79, 1
    rec = cr.to_record(d)
    path = str(tmp_path / "c.sca")
    formats.write_sca_compare(path, rec, hist, network="Net")
    text = open(path).read()
    assert text.startswith("version 2\nrun General-0-fognet\n")
    scal, stats = parse(text)
    assert list(scal) == ["Net.compare"]
    check_block(scal, stats, "Net.compare", d, hist)
    # appended behind a job file: no second header; a count-0 statistic; a single value; a named module; no hist
    formats.write_sca(path, fa.job_from_reps(np.zeros(0, abi.REP_STATS_DTYPE)))
    before = open(path, "rb").read()
    one = hand(n_reps=1, n_pairs=1, n_done_both=1, n_worse=1, rep_worse=1, d_start=mom(1, 5, 5, 5, 25), d_service=mom(),
               d_resp=mom(1, 7, 7, 7, 49))
    formats.write_sca_compare(path, cr.to_record(one), module="FogNet.rrVsRef", append=True)
    after = open(path, "rb").read()
    assert after.startswith(before) and after.count(b"version 2") == 1
    scal, stats = parse(after[len(before):].decode())
    assert list(scal) == ["FogNet.rrVsRef"]
    check_block(scal, stats, "FogNet.rrVsRef", one)
    with pytest.raises(fa.FognetError) as e:
        formats.write_sca_compare(str(tmp_path / "no" / "dir.sca"), rec)
    assert e.value.code == abi.FOGNET_ERR_ARG and b"cannot open" in abi.load().fognet_io_last_error()
    assert abi.load().fognet_write_sca_compare(path.encode(), b"r", b"n", None, None, None, 0) == abi.FOGNET_ERR_ARG


# ---------------------------------------------------------------- the driver's refusals

def test_driver_refusals(tmp_path):
    sca = str(tmp_path / "a.sca")
    base = ("-f", INI, "--users", "user[2]", "--dry-run")
    for bad, msg in ((("--compare", "rr"), "give --sca FILE"),
                     (("--sca", sca, "--compare", "fastest"), "rr, random[:SEED], REF_V3 or EXT_LAT"),
                     (("--sca", sca, "--compare", "random:-1"), "SEED must be >= 0"),
                     (("--sca", sca, "--compare", "EXT_LAT", "--reps", "2", "--world", "2", "--comm-id", str(tmp_path / "id")),
                      "--world 1")):
        p = drive(*base, *bad, check=False)
        assert p.returncode != 0 and msg in p.stderr and "--compare" in p.stderr, (bad, p.stderr)
    p = drive("-f", INI, "-c", "Example", "--nodes", "5", "--sca", sca, "--compare", "rr", "--dry-run", check=False)
    assert p.returncode != 0 and "--compare applies to BrokerBaseApp3 runs" in p.stderr  # the v2 broker
    # accepted: every rule, and together with --assign and --policy
    for rule in ("rr", "random", "random:7", "REF_V3", "EXT_LAT"):
        drive(*base, "--sca", sca, "--compare", rule)
    drive(*base, "--sca", sca, "--compare", "REF_V3", "--assign", "random:7")
    drive(*base, "--sca", sca, "--compare", "rr", "--policy", "EXT_LAT")
    assert "--compare rr|random[:SEED]|REF_V3|EXT_LAT" in drive("--help").stdout


# ---------------------------------------------------------------- the reference on the oracle's outputs

def test_reference_identities_on_the_oracle():
    """REF_V3 against EXT_LAT on one small trace, every task completing in both: the paired sums
    are the differences of the two runs' own records."""
    tr = tg.make_batch(0xC0DE, 3, 5, 200, rho=1.5)
    args = [tr[k] for k in ("arrive", "req", "mips", "dl", "ul", "init")]
    a, b = ol.run_batch(*args, policy=ol.POLICY_REF_V3), ol.run_batch(*args, policy=ol.POLICY_EXT_LAT)
    assert (a["stats"]["status"] == 0).all() and (b["stats"]["status"] == 0).all()
    recs, job, hist = cr.compare(a, b)
    moved = 0
    for r, d in enumerate(recs):
        sa, sb = a["stats"][r], b["stats"][r]
        assert d["n_pairs"] == d["n_done_both"] == 200 and d["n_reps"] == 1
        rsum = lambda s: int(s["resp_sum_lo"]) | (int(s["resp_sum_hi"]) << 64)  # noqa: E731
        assert d["d_resp"]["sum"] == rsum(sb) - rsum(sa)
        assert d["d_service"]["sum"] == (int(sb["busy_s"]) - int(sa["busy_s"])) * 10**12
        assert d["d_start"]["sum"] + d["d_service"]["sum"] == d["d_resp"]["sum"]
        assert [sum(row) for row in d["trans"]][:2] == [int(sa["n_started"]), int(sa["n_queued"])]
        assert [sum(d["trans"][i][j] for i in range(3)) for j in range(2)] == [int(sb["n_started"]), int(sb["n_queued"])]
        assert d["n_better"] + d["n_equal"] + d["n_worse"] == 200 and d["rep_better"] + d["rep_equal"] + d["rep_worse"] == 1
        moved += d["n_moved"]
    assert moved > 0  # the two policies do decide differently on this trace
    assert job["n_reps"] == 3 and job["n_pairs"] == 600
    assert [sum(h) for h in hist] == [job["n_better"], job["n_worse"]]
    same, _, h0 = cr.compare(a, a)
    assert all(d["n_moved"] == 0 and d["n_equal"] == 200 and d["d_resp"]["min"] == d["d_resp"]["max"] == 0 for d in same)
    assert h0 == cr.new_hist()
