"""Per-node statistics, host side (no GPU): the fognet_node_stats layout, the exact
host merge, the `.sca` writer of per-node blocks, and the test-side record builder
(node_stats_ref) against the oracle's replication records."""
import ctypes
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fognetsimpp_amd as fa
import fognetsimpp_amd._abi as abi
import node_stats_ref as ns
import oracle_lib as ol
import tracegen as tg
from fognetsimpp_amd import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX, I64_MIN = ns.I64_MAX, ns.I64_MIN


def test_node_stats_layout_matches_header(tmp_path):
    """sizeof/offsetof as the C compiler lays out include/fognet_hip.h (the method of
    test_abi.test_struct_layouts_match_header), against the ctypes and numpy mirrors."""
    fields = [f for f, _ in abi.NodeStats._fields_] + [f"{m}.{f}" for m in ("queue", "resp") for f, _ in abi.Moments._fields_]
    lines = ['printf("size %zu\\n", sizeof(fognet_node_stats));']
    lines += [f'printf("{f} %zu\\n", offsetof(fognet_node_stats, {f}));' for f in fields]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fognet_hip.h\"\nint main(void){" + "\n".join(lines) +
                   "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.NodeStats) == abi.NODE_STATS_DTYPE.itemsize == 192
    for f in fields:
        if "." in f:
            m, sub = f.split(".")
            want = getattr(abi.NodeStats, m).offset + getattr(abi.Moments, sub).offset
            assert abi.NODE_STATS_DTYPE.fields[m][1] + abi.MOMENTS_DTYPE.fields[sub][1] == want
        else:
            want = getattr(abi.NodeStats, f).offset
            assert abi.NODE_STATS_DTYPE.fields[f][1] == want
        assert int(got[f]) == want, f


def c_rec(rec) -> abi.NodeStats:
    return abi.NodeStats.from_buffer_copy(np.ascontiguousarray(rec).tobytes())


def np_rec(c) -> np.ndarray:
    return np.frombuffer(bytes(c), dtype=abi.NODE_STATS_DTYPE)[0]


def host_merge(a, b) -> np.ndarray:
    x, y = c_rec(a), c_rec(b)
    abi.load().fognet_node_stats_merge(ctypes.byref(x), ctypes.byref(y))
    return np_rec(x)


def make(tasks=0, queue=(), resp=(), ovf=0, last=I64_MIN) -> np.ndarray:
    n = ns.Node()
    n.tasks, n.last, n.queue.ovf = tasks, last, ovf
    for v in queue:
        n.queue.add(v)
    for v in resp:
        n.resp.add(v)
    return ns.to_records([n])[0]


def test_init_is_the_empty_record_and_the_identity():
    s = abi.NodeStats()
    ctypes.memset(ctypes.byref(s), 0x5A, ctypes.sizeof(s))
    abi.load().fognet_node_stats_init(ctypes.byref(s))
    empty = np_rec(s)
    assert empty.tobytes() == ns.empty_records(1)[0].tobytes()
    assert (int(empty["last_tick"]), int(empty["queue"]["min_raw"]), int(empty["resp"]["max_raw"])) == (I64_MIN, I64_MAX, I64_MIN)
    x = make(tasks=3, queue=(5, -7, 2**62), resp=(10**15,), ovf=2, last=77)
    assert host_merge(empty, x).tobytes() == x.tobytes() == host_merge(x, empty).tobytes()


def test_merge_carries_negative_sums_and_extrema():
    big = 2**63 - 1
    a, b = make(queue=(big, big)), make(queue=(big, big, big))  # sum 5 (2^63 - 1) > 2^65; squares ~2^126 each
    m = ns.Node.load(host_merge(a, b))
    assert m.queue.s == 5 * big and m.queue.s >> 64 and m.queue.q == 5 * big * big and m.queue.q >> 128
    lo = make(queue=(2**64 - 1 - 2**63,))  # carry out of sq_lo alone
    assert ns.Node.load(host_merge(lo, lo)).queue.q == 2 * (2**63 - 1) ** 2
    top = make()
    top["queue"]["sq_lo"], top["queue"]["sq_hi"] = 2**64 - 1, 2**64 - 1  # the carry runs through sq_hi into sq_top
    one = make()
    one["queue"]["sq_lo"] = 1
    got = host_merge(top, one)["queue"]
    assert (int(got["sq_lo"]), int(got["sq_hi"]), int(got["sq_top"])) == (0, 0, 1)
    neg = ns.Node.load(host_merge(make(queue=(-5, 3)), make(queue=(-2**62,))))
    assert neg.queue.s == -2 - 2**62 and (neg.queue.mn, neg.queue.mx) == (-2**62, 3)
    assert int(host_merge(make(queue=(-5,)), make())["queue"]["sum_hi"]) == 2**64 - 1  # two's complement
    e = host_merge(make(resp=(9,), last=40), make(resp=(4, 11), last=30))
    assert (int(e["last_tick"]), int(e["resp"]["min_raw"]), int(e["resp"]["max_raw"]), int(e["resp"]["count"])) == (40, 4, 11, 3)


def test_merge_is_commutative_and_exact_on_random_limbs():
    rng = random.Random(7)
    for _ in range(200):
        recs = []
        for _ in range(2):
            r = ns.empty_records(1)[0]
            for k in ("n_tasks", "n_queued", "n_started", "n_lost", "busy_s"):
                r[k] = rng.randrange(2**40)
            r["last_tick"] = rng.randrange(-2**62, 2**62)
            for m in ("queue", "resp"):
                r[m]["count"], r[m]["overflow"] = rng.randrange(2**40), rng.randrange(2**40)
                r[m]["min_raw"], r[m]["max_raw"] = rng.randrange(-2**63, 2**63), rng.randrange(-2**63, 2**63)
                for f in ("sum_lo", "sum_hi", "sq_lo", "sq_hi"):
                    r[m][f] = rng.choice((rng.randrange(2**64), 2**64 - 1, 0))
                r[m]["sq_top"] = rng.randrange(2**62)
            recs.append(r)
        ab, ba = host_merge(*recs), host_merge(*recs[::-1])
        assert ab.tobytes() == ba.tobytes()
        want = ns.merged(recs)
        want.queue.q %= 1 << 192
        want.resp.q %= 1 << 192
        assert ab.tobytes() == ns.to_records([want])[0].tobytes()


def test_record_builder_merges_to_the_oracles_replication_record():
    """The invariant of fognet_hip.h on the reference side: the records node_stats_ref
    builds from the oracle's per-task outputs merge to the oracle's own record."""
    for pol in ("REF_V3", "EXT_LAT"):
        tr = tg.make_batch(0x4E0D + len(pol), 2, 65, 191, rho=0.9)
        o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"], policy=ol.POLICIES[pol])
        e = ns.expected(tr, o)
        for r in range(2):
            ns.assert_merge_is_rep_record(e[r], o["stats"][r])
    tr = ns.herded_trace()
    o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"])
    ns.assert_merge_is_rep_record(ns.expected(tr, o)[0], o["stats"][0])


# ---------------------------------------------------------------- the .sca writer

def fmt(x) -> str:
    return "%.14g" % x


def want_fields(m: ns.Mom, unit: Fraction) -> dict:
    """cStdDev's fields from the exact sums, in rational arithmetic."""
    d = {"count": str(m.n), "sum": fmt(float(m.s * unit)), "sqrsum": fmt(float(m.q * unit * unit))}
    if m.n == 0:
        d.update(mean="-nan", stddev="-nan", min="-nan", max="-nan")
        return d
    d["mean"] = fmt(float(Fraction(m.s, m.n) * unit))
    var = Fraction(m.n * m.q - m.s * m.s, m.n * (m.n - 1)) if m.n > 1 else None
    d["stddev"] = "-nan" if var is None else fmt(float(var) ** 0.5 * float(unit))
    return d


def blocks(text: str) -> dict:
    """module -> {"scalars": {name: value}, "<stat>": {field: value}} of a .sca text."""
    out: dict = {}
    cur = None
    for ln in text.splitlines():
        p = ln.split("\t")
        if ln.startswith("scalar "):
            out.setdefault(p[0].split()[1], {"scalars": {}})["scalars"][p[1].strip().strip('"')] = p[2].strip()
        elif ln.startswith("statistic "):
            cur = out.setdefault(p[0].split()[1], {"scalars": {}}).setdefault(p[1].strip(), {})
        elif ln.startswith("field ") and cur is not None:
            _, k, v = ln.split()
            cur[k] = v
    return out


def test_write_sca_nodes_names_fields_and_empty_node(tmp_path):
    big = 2**63 - 1000
    n0 = ns.Node()
    n0.tasks, n0.queued, n0.started, n0.lost, n0.busy = 9, 6, 2, 1, 123
    for v in (big, big - 10**15, big - 7 * 10**17, -1000, big - 3, big - 1, big - 10**18):  # the sum needs sum_hi, the squares sq_top
        n0.queue.add(v)
    n0.queue.ovf = 2
    for v in (5 * 10**12, 7 * 10**12 + 1, 10**16):
        n0.resp.add(v)
    assert n0.queue.s >> 64 and n0.queue.q >> 128
    recs = ns.to_records([n0, ns.Node()])
    path = str(tmp_path / "n.sca")
    formats.write_sca_nodes(path, recs, network="Net")
    text = open(path).read()
    assert text.startswith("version 2\nrun General-0-fognet\n") and text.count("version 2") == 1
    b = blocks(text)
    assert sorted(b) == ["Net.fogNode[0].udpApp[0]", "Net.fogNode[1].udpApp[0]"]
    m0 = b["Net.fogNode[0].udpApp[0]"]
    assert m0["scalars"] == {"tasks": "9", "tasks queued": "6", "tasks started": "2", "tasks lost": "1", "busy seconds": "123"}
    q = want_fields(n0.queue, Fraction(1, 10**12))
    for k in ("count", "mean", "stddev", "sum"):
        assert m0["queueTime:stats"][k] == q[k], k
    assert m0["queueTime:stats"]["min"] == fmt(-1000 * 1e-12) and m0["queueTime:stats"]["max"] == fmt(float(big) * 1e-12)
    r = want_fields(n0.resp, Fraction(1, 10**9))
    for k in ("count", "mean", "stddev", "sum"):
        assert m0["response:stats"][k] == r[k], k
    m1 = b["Net.fogNode[1].udpApp[0]"]  # a node without a task: count 0 blocks
    assert set(m1["scalars"].values()) == {"0"} and m1["queueTime:stats"]["count"] == "0" == m1["response:stats"]["count"]
    assert m1["queueTime:stats"]["mean"] == "-nan"
    formats.write_sca_nodes(path, recs, node_id=[7, 3], network="Net")
    assert sorted(blocks(open(path).read())) == ["Net.fogNode[3].udpApp[0]", "Net.fogNode[7].udpApp[0]"]


def test_write_sca_nodes_append_and_errors(tmp_path):
    job = fa.job_from_reps(np.zeros(0, abi.REP_STATS_DTYPE))
    path = str(tmp_path / "job.sca")
    formats.write_sca(path, job, hist=np.zeros((2, 64), np.int64))
    before = open(path, "rb").read()
    formats.write_sca_nodes(path, ns.empty_records(3), append=True)
    after = open(path, "rb").read()
    assert after.startswith(before) and after.count(b"version 2") == 1 and after.count(b"\nrun ") + after.startswith(b"run ") == 1
    assert sorted(k for k in blocks(after[len(before):].decode())) == [f"FogNet.fogNode[{j}].udpApp[0]" for j in range(3)]
    with pytest.raises(fa.FognetError) as e:
        formats.write_sca_nodes(str(tmp_path / "no" / "such" / "dir.sca"), ns.empty_records(1))
    assert e.value.code == abi.FOGNET_ERR_ARG and b"cannot open" in abi.load().fognet_io_last_error()
    with pytest.raises(fa.FognetError):
        formats.write_sca_nodes(path, ns.empty_records(2), node_id=[1])


def test_summarize_node():
    tr = ns.herded_trace()
    o = ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"])
    s = fa.summarize_node(ns.expected(tr, o)[0, 0])
    assert s["tasks"] == 262 and s["queueTime_ms"]["overflow"] > 0 and s["queueTime_ms"]["min"] < 0
    assert fa.summarize_node(ns.empty_records(1)[0])["last_tick"] is None
