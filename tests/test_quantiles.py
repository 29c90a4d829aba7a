"""Quantiles without a GPU: the rank rule of the restatement (quantile_ref) against a literal
restatement and numpy's sort, the restatement against the window records and the signal vectors'
rows on the oracle cases, the ABI and the header, the `.sca` writer and the driver's refusals.
test_quantiles_gpu.py holds the device to quantile_ref."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import fognetsimpp_amd as fa
import quantile_ref as qr
import signal_vectors_ref as sv
import window_ref as wr
from fognetsimpp_amd import _abi as abi
from fognetsimpp_amd import formats
from test_driver import INI, drive
from test_window_stats import ORACLE_CASES, oracle_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX, I64_MIN = 2**63 - 1, -2**63
PPMS = (0, 1, 499999, 500000, 500001, 999999, 1000000)


# ---------------------------------------------------------------- the rank rule

def literal_rank(n: int, ppm: int) -> int:
    """The smallest k >= 1 with k * 10^6 >= n * ppm, found by counting."""
    k = 1
    while k * 10**6 < n * ppm:
        k += 1
    return k


@pytest.mark.parametrize("n", [1, 2, 4, 5, 1000])
def test_rank_rule_table(n):
    for ppm in PPMS:
        assert qr.rank_of(n, ppm) == literal_rank(n, ppm), (n, ppm)
    assert qr.rank_of(n, 0) == 1 and qr.rank_of(n, 10**6) == n


def test_rank_rule_literals():
    """Spelled out: the median of four is the second smallest; 1,000,001 values."""
    assert [qr.rank_of(4, p) for p in PPMS] == [1, 1, 2, 2, 3, 4, 4]
    assert [qr.rank_of(5, p) for p in PPMS] == [1, 1, 3, 3, 3, 5, 5]
    assert [qr.rank_of(1, p) for p in PPMS] == [1] * 7 and [qr.rank_of(2, p) for p in PPMS] == [1, 1, 1, 1, 2, 2, 2]
    assert [qr.rank_of(1000, p) for p in PPMS] == [1, 1, 500, 500, 501, 1000, 1000]
    n = 1000001
    assert [qr.rank_of(n, p) for p in PPMS] == [1, 2, 500000, 500001, 500002, 1000000, 1000001]
    for p in (1, 499999, 500001, 999999):  # ceil, exactly: k - 1 falls short and k reaches
        k = qr.rank_of(n, p)
        assert (k - 1) * 10**6 < n * p <= k * 10**6
    assert qr.nearest_rank([7, 1, 5, 3], 500000) == 3 and qr.nearest_rank([], 500000) == I64_MAX


@pytest.mark.parametrize("n", [1, 2, 4, 5, 1000])
def test_nearest_rank_against_numpy_sort(n):
    rng = np.random.default_rng(n)
    for draw in range(3):
        a = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        if draw == 1:
            a[rng.integers(0, n)] = I64_MIN
            a[rng.integers(0, n)] = I64_MAX
        if draw == 2:
            a = rng.integers(-3, 4, n, dtype=np.int64)  # ties
        s = np.sort(a)
        for ppm in PPMS:
            assert qr.nearest_rank(a.tolist(), ppm) == int(s[qr.rank_of(n, ppm) - 1])
    if n == 1000:  # and once at 1,000,001 values, where ppm = 1 is the second smallest
        a = rng.integers(I64_MIN, I64_MAX, 1000001, dtype=np.int64, endpoint=True)
        s, ordered = np.sort(a), sorted(a.tolist())
        for ppm in PPMS:
            assert ordered[qr.rank_of(1000001, ppm) - 1] == int(s[literal_rank(1000001, ppm) - 1])
    key = lambda v: (v & (2**64 - 1)) ^ 2**63  # the device's key keeps the order of int64
    vals = [I64_MIN, -1, 0, 1, I64_MAX]
    assert [key(v) for v in vals] == sorted(key(v) for v in vals)


# ---------------------------------------------------------------- the restatement on the oracle cases

@pytest.mark.parametrize("name", ORACLE_CASES)
def test_restatement_against_window_records_and_rows(name):
    tr, o, who, uu, ud, flags, up = oracle_case(name)
    ppm = [0, 10**6, 500000]
    value, count, un = qr.expected(tr, o, who, uu, ud, ppm, flags, up)
    last = wr.latest_tick(tr, o, who, uu, ud, flags, up)
    recs, outside, un_w = wr.expected(tr, o, who, uu, ud, 0, last + 1, 1, flags, up)
    assert not outside.any() and list(un) == list(un_w)
    rows = None if name == "hier" else sv.expected(tr, o, who, uu, ud, with_rows=True)["rows"]
    N, U = np.shape(tr["dl"])[-1], np.shape(uu)[-1]
    names = ["queue"] * N + ["delay"] + ["latency"] * U + ["latencyH1"] * U + ["taskTime"] * U
    pops = qr.replication_populations(tr, o, who, uu, ud, flags, up)
    for r in range(value.shape[0]):
        for s, sig in enumerate(qr.SIGNALS):
            m = recs[r, 0][sig]
            assert int(count[r, s]) == int(m["count"]), (r, sig)
            if count[r, s]:
                assert int(value[r, s, 0]) == int(m["min_raw"]) and int(value[r, s, 1]) == int(m["max_raw"]), (r, sig)
                assert int(m["min_raw"]) <= int(value[r, s, 2]) <= int(m["max_raw"])
            else:
                assert (value[r, s] == I64_MAX).all()
            if rows is not None:
                pooled = sorted(int(row[2]) for v, vec in zip(names, rows[r]) if v == sig for row in vec)
                assert pooled == sorted(pops[r][0][sig]), (r, sig)
    jv, jc = qr.expected_job(tr, o, who, uu, ud, ppm, flags, up)
    assert list(jc) == list(count.sum(axis=0))
    assert (jv[:, 0] == value[:, :, 0].min(axis=0)).all()
    assert all(jv[s, 1] == value[:, s, 1][count[:, s] > 0].max() for s in range(5) if jc[s])


# ---------------------------------------------------------------- the ABI and the header

NAMES = ("fognet_quantiles_dev", "fognet_job_quantiles_dev", "fognet_write_sca_quantiles")


def test_abi_header_and_mirror():
    lib = abi.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in abi.SIGNATURES, n
    header = open(os.path.join(ROOT, "include", "fognet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    defs = dict(re.findall(r"^#define\s+(FOGNET_QUANTILE_\w+)\s+(\d+)", header, re.M))
    assert int(defs["FOGNET_QUANTILE_SIGNALS"]) == abi.QUANTILE_SIGNALS == 5 == len(abi.WINDOW_SIGNALS)
    assert int(defs["FOGNET_QUANTILE_MAX"]) == abi.QUANTILE_MAX == 8
    assert re.search(r"#define FOGNET_ABI_VERSION 10\b", header) and abi.ABI_VERSION == 10 == lib.fognet_abi_version()
    common = ["fognet_ctx *ctx", "const fognet_batch_in *in", "const fognet_batch_out *out", "const int32_t *user_of",
              "int32_t U", "int32_t link_stride", "const int64_t *user_ul_tick", "const int64_t *user_dl_tick",
              "const int32_t *ppm", "int32_t Q", "int64_t *value", "int64_t *count"]
    for name, tail in (("fognet_quantiles_dev", ["int64_t *n_unassigned", "void *hip_stream"]),
                       ("fognet_job_quantiles_dev", ["void *hip_stream"])):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == common + tail, name
    P = C.c_void_p
    head = [P, C.POINTER(abi.BatchIn), C.POINTER(abi.BatchOut), P, C.c_int32, C.c_int32, P, P, C.POINTER(C.c_int32), C.c_int32]
    assert abi.SIGNATURES["fognet_quantiles_dev"] == (C.c_int, head + [P, P, P, P])
    assert abi.SIGNATURES["fognet_job_quantiles_dev"] == (C.c_int, head + [P, P, P])
    assert "Quantiles." in header
    for n in ("quantiles", "job_quantiles", "summarize_quantiles"):
        assert callable(getattr(fa, n)) and n in fa.__all__


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    lib = abi.load()
    one = (C.c_int32 * 1)(500000)
    assert lib.fognet_quantiles_dev(None, None, None, None, 0, 0, None, None, one, 1, None, None, None, None) == abi.FOGNET_ERR_ARG
    assert lib.fognet_job_quantiles_dev(None, None, None, None, 0, 0, None, None, one, 1, None, None, None) == abi.FOGNET_ERR_ARG
    assert lib.fognet_quantiles_dev(None, None, None, None, 0, 0, None, None, None, 9, None, None, None, None) == abi.FOGNET_ERR_ARG
    assert lib.fognet_job_quantiles_dev(None, None, None, None, -1, 0, None, None, None, 0, None, None, None) == abi.FOGNET_ERR_ARG


def test_summarize_quantiles():
    value = np.array([[5 * 10**12, 7 * 10**12], [2 * 10**9, 3 * 10**9], [I64_MAX] * 2, [10**12, 10**12], [-10**12, 0]], np.int64)
    s = fa.summarize_quantiles([500000, 990000], value, [3, 2, 0, 1, 4])
    assert s["queueTime_ms"] == {"count": 3, 500000: 5.0, 990000: 7.0}
    assert s["delay_ms"] == {"count": 2, 500000: 2.0, 990000: 3.0}  # ticks of a second, in ms
    assert s["latency_ms"] == {"count": 0} and s["taskTime_ms"][500000] == -1.0


# ---------------------------------------------------------------- the writer

PPM3 = [500000, 999000, 999999]  # 50, 99.9, 99.9999


def test_writer_lines(tmp_path):
    path = str(tmp_path / "q.sca")
    value = np.full((5, 3), I64_MAX, np.int64)
    value[0] = [1500 * 10**9, 2 * 10**12, 123456789012345]  # queueTime: 1.5, 2 and 123.456789012345 ms
    value[3] = [-25 * 10**10, 0, 7]                         # latencyH1: -0.25, 0 and 7e-12 ms
    formats.write_sca_quantiles(path, PPM3, value, [10, 0, 0, 2, 0], network="Net")
    text = open(path).read()
    assert text.startswith("version 2\nrun General-0-fognet\n")
    lines = [ln for ln in text.splitlines() if ln.startswith("scalar")]
    assert lines == ['scalar Net.fogNodes.udpApp[0] \t"queueTime:p50" \t1.5',
                     'scalar Net.fogNodes.udpApp[0] \t"queueTime:p99.9" \t2',
                     'scalar Net.fogNodes.udpApp[0] \t"queueTime:p99.9999" \t123.45678901234',
                     'scalar Net.users.udpApp[0] \t"latencyH1:p50" \t-0.25',
                     'scalar Net.users.udpApp[0] \t"latencyH1:p99.9" \t0',
                     'scalar Net.users.udpApp[0] \t"latencyH1:p99.9999" \t7e-12']
    assert ":p" not in "".join(ln for ln in text.splitlines() if not ln.startswith("scalar"))
    mods = ["a.q", "a.d", "a.l", "a.h", "a.t"]
    formats.write_sca_quantiles(path, [0, 10**6, 10000, 12300], np.arange(20).reshape(5, 4) * 10**12, [1] * 5, modules=mods)
    lines = [ln for ln in open(path).read().splitlines() if ln.startswith("scalar")]
    assert len(lines) == 20 and lines[0] == 'scalar a.q \t"queueTime:p0" \t0' and lines[5] == 'scalar a.d \t"delay:p100" \t5'
    assert lines[10] == 'scalar a.l \t"latency:p1" \t10' and lines[19] == 'scalar a.t \t"taskTime:p1.23" \t19'


def test_writer_append_and_errors(tmp_path):
    path, alone = str(tmp_path / "a.sca"), str(tmp_path / "alone.sca")
    with open(path, "w") as f:
        f.write("version 2\nrun r\n\nscalar m \tx \t1\n")
    before = open(path, "rb").read()
    value = np.arange(15, dtype=np.int64).reshape(5, 3) * 10**12
    formats.write_sca_quantiles(path, PPM3, value, [1, 1, 0, 1, 1], append=True)
    formats.write_sca_quantiles(alone, PPM3, value, [1, 1, 0, 1, 1])
    after, created = open(path, "rb").read(), open(alone, "rb").read()
    assert after.startswith(before) and after.count(b"version 2") == 1 and created.endswith(after[len(before):])
    assert after[len(before):].count(b"scalar") == 12 and b"latency:p" not in after
    for bad in ([-1, 0, 5], [0, 10**6 + 1, 5]):
        with pytest.raises(fa.FognetError) as e:
            formats.write_sca_quantiles(str(tmp_path / "x.sca"), bad, value, [1] * 5)
        assert e.value.code == abi.FOGNET_ERR_ARG and not (tmp_path / "x.sca").exists()
    with pytest.raises(fa.FognetError):
        formats.write_sca_quantiles(str(tmp_path / "no" / "such" / "dir.sca"), PPM3, value, [1] * 5)
    assert b"cannot open" in abi.load().fognet_io_last_error()


# ---------------------------------------------------------------- the driver's refusals

@pytest.mark.parametrize("args,msg", [
    (("--users", "user[3]", "--quantiles", "50"), "--quantiles appends to the job's .sca"),
    (("--users", "user[3]", "--reps", "4", "--sca", "x.sca", "--quantiles", "50", "--world", "2", "--comm-id", "c.id"),
     "--quantiles: the quantiles of several ranks cannot be merged"),
    (("-c", "Example", "--nodes", "5", "--sca", "x.sca", "--quantiles", "50"), "--quantiles applies to BrokerBaseApp3 runs"),
    (("--users", "user[3]", "--sca", "x.sca", "--quantiles", "101"), "lies outside [0, 100]"),
    (("--users", "user[3]", "--sca", "x.sca", "--quantiles", "50,,90"), "an empty rank"),
    (("--users", "user[3]", "--sca", "x.sca", "--quantiles", "1,2,3,4,5,6,7,8,9"), "at most 8 ranks"),
    (("--users", "user[3]", "--sca", "x.sca", "--quantiles", "99.99999"), "more than four decimals"),
    (("--users", "user[3]", "--sca", "x.sca", "--quantiles", "5e1"), "is not a percent"),
])
def test_driver_refusals(tmp_path, args, msg):
    args = [str(tmp_path / a) if a in ("x.sca", "c.id") else a for a in args]
    p = drive("-f", INI, *args, "--dry-run", check=False)
    assert p.returncode == 2 and msg in p.stderr, (p.returncode, p.stderr)
    assert not (tmp_path / "x.sca").exists()


def test_driver_usage_names_the_option():
    p = drive("--help", check=False)
    assert "--quantiles P[,P...]" in p.stdout + p.stderr
