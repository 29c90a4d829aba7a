"""Replication groups on the host (fognet_hip.h "Replication groups"): fognet_rep_metrics and the
group twins (init / add_rep / merge / job) against the Python-integer restatement of tests/group_ref
on crafted records, the struct layout through the C compiler, fognet_write_sca_groups read back, and
the stand-alone sanitizer program.  CPU only."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fognetsimpp_amd as fa
import fognetsimpp_amd._abi as abi
from fognetsimpp_amd import formats

import group_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = gr.edge_cases()
PLAIN = gr.plain(np.random.default_rng(77), 40)


def test_constants_and_layout_match_header(tmp_path):
    """sizeof / offsetof of fognet_group_stats and the new macros, as the C compiler has them."""
    lines = ['printf("size %zu\\n", sizeof(fognet_group_stats));',
             'printf("metrics %d\\n", FOGNET_REP_METRICS);', 'printf("lds %d\\n", FOGNET_GROUP_LDS_MAX);',
             'printf("energy %d\\n", (int)FOGNET_METRIC_ENERGY_UJ);']
    for f, _ in abi.GroupStats._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(fognet_group_stats, {f}));')
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fognet_hip.h\"\nint main(void){" +
                   "\n".join(lines) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                    text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.GroupStats) == abi.GROUP_STATS_DTYPE.itemsize == 848
    assert int(got["metrics"]) == len(abi.REP_METRICS) == 9 and int(got["lds"]) == abi.GROUP_LDS_MAX == 64
    assert int(got["energy"]) == abi.REP_METRICS.index("ENERGY_UJ") == 8
    for f, _ in abi.GroupStats._fields_:
        assert int(got[f]) == getattr(abi.GroupStats, f).offset == abi.GROUP_STATS_DTYPE.fields[f][1], f
    assert abi.GROUP_STATS_DTYPE.fields["queue"][1] == 56 and abi.GROUP_STATS_DTYPE.fields["across"][1] == 56 + 2 * 72


@pytest.mark.parametrize("recs", [EDGES, PLAIN], ids=["edges", "plain"])
def test_rep_metrics_equal_the_restatement(recs):
    for i, rec in enumerate(recs):
        val, dfn, ovf = fa.rep_metrics(rec)
        for k, (d, v) in enumerate(gr.metrics(rec)):
            fits = d and v is not None
            assert bool(dfn >> k & 1) == fits, (i, k)
            assert bool(ovf >> k & 1) == (d and v is None), (i, k)
            assert int(val[k]) == (v if fits else gr.I64_MIN), (i, k)


def test_the_named_edge_values():
    """The cases the record's definition names, as literal expectations (not via the restatement)."""
    def one(**kw):
        r = gr.blank(1)
        for k, v in kw.items():
            r[k] = v
        return fa.rep_metrics(r[0])
    m64 = 2**64 - 1
    v, d, o = one(n_qtime=2, queue_sum_lo=(-7) & m64, queue_sum_hi=m64)
    assert v[2] == -4 and d >> 2 & 1                      # -7 / 2 -> -4
    v, d, o = one(n_qtime=2, queue_sum_lo=(-8) & m64, queue_sum_hi=m64)
    assert v[2] == -4
    v, d, o = one(n_qtime=1, queue_sum_lo=0, queue_sum_hi=2**63)          # -2^127
    assert not d >> 2 & 1 and o >> 2 & 1 and v[2] == gr.I64_MIN
    v, d, o = one(n_qtime=1, queue_sum_lo=2**63, queue_sum_hi=m64)        # INT64_MIN fits
    assert d >> 2 & 1 and not o >> 2 & 1 and v[2] == gr.I64_MIN
    v, d, o = one(n_tasks=7, resp_sum_lo=5, resp_sum_hi=1)
    assert v[0] == (2**64 + 5) // 7
    v, d, o = one(n_tasks=1, resp_sum_lo=2**63)
    assert o & 1 and not d & 1
    v, d, o = one(n_tasks=3, n_queued=2)
    assert v[4] == 666666
    v, d, o = one(energy_j=2.5e-6)
    assert v[8] == 3                                      # x.5 rounds up: floor(x + 0.5)
    v, d, o = one(energy_j=9.3e12)
    assert o >> 8 & 1 and v[8] == gr.I64_MIN
    v, d, o = one(energy_j=float("nan"))
    assert o >> 8 & 1
    v, d, o = one()
    assert d == 0b111000000 and o == 0                    # nothing decided: busy, pending, energy only


def test_add_rep_equals_the_restatement():
    lib = abi.load()
    empty = abi.GroupStats()
    lib.fognet_group_stats_init(ctypes.byref(empty))
    assert bytes(empty) == gr.Group().pack()
    for i, rec in enumerate(EDGES):
        g = gr.Group()
        g.add_rep(rec)
        assert fa.group_from_reps(rec).tobytes() == g.pack(), i
    allrec = np.concatenate([EDGES, PLAIN])
    groups, lost = gr.reduce_groups(allrec)
    assert lost == 0 and fa.group_from_reps(allrec).tobytes() == groups[0].pack()
    g = groups[0]
    assert g.head[1] == len(gr.FAILED) + 3 and g.head[2] == 2 and g.head[0] == len(allrec)


def test_merging_any_split_equals_the_whole():
    rng = np.random.default_rng(5)
    allrec = np.concatenate([EDGES, PLAIN])
    whole = fa.group_from_reps(allrec).tobytes()
    for parts in (1, 2, 3, 9, len(allrec)):
        of = rng.integers(0, parts, len(allrec))
        recs = [fa.group_from_reps(allrec[of == p]) if (of == p).any() else gr.Group().record() for p in range(parts)]
        assert fa.merge_group_stats(np.array(recs, dtype=abi.GROUP_STATS_DTYPE)).tobytes() == whole, parts
        ref, _ = gr.reduce_groups(allrec, of, parts)
        acc = gr.Group()
        for p in range(parts):
            assert recs[p].tobytes() == ref[p].pack(), (parts, p)
            acc.merge(ref[p])
        assert acc.pack() == whole


def test_the_column_form_of_the_restatement_equals_the_record_form():
    """group_ref.reduce_rows (what the GPU tests use for their many memberships) against Group.add_rep."""
    reps = gr.crafted(300)
    rws = gr.rows(reps)
    rng = np.random.default_rng(9)
    for G, of in ((1, None), (9, np.arange(300) % 9), (65, rng.integers(-1, 66, 300)), (1000, rng.integers(0, 1000, 300))):
        groups, lost = gr.reduce_groups(reps, of, G)
        got, got_lost = gr.reduce_rows(rws, of, G)
        assert got == gr.records(groups).tobytes() and got_lost == lost, G
    assert (reps["status"] != 0).sum() >= 7 and (reps["status"] == gr.REF_ABORTED).sum() >= 3


JOB_INT_FIELDS = [n for n in abi.JOB_STATS_DTYPE.names if n != "energy_j"]


def assert_job_equal(got, want, members, what=""):
    """Every integer field, and the energy within the derived bound: members * 0.5 uJ for the
    rounding to microjoules plus the header's 1e-9 * |E| for another summation order."""
    for n in JOB_INT_FIELDS:
        assert np.array_equal(got[n], want[n]), (what, n, got[n], want[n])
    e = float(want["energy_j"])
    if np.isfinite(e):
        assert abs(float(got["energy_j"]) - e) <= members * 0.5e-6 + 1e-9 * abs(e), (what, got["energy_j"], e)


def test_group_job_equals_job_from_reps():
    """Each edge record among plain ones (a group whose pooled sums stay inside 128 bits, the
    header's condition), the plain set, the empty set and failed records alone."""
    for i, rec in enumerate(EDGES):
        members = np.concatenate([EDGES[i:i + 1], PLAIN[:5]])
        finite = members[np.isfinite(members["energy_j"]) & (np.abs(members["energy_j"]) < 9.2e12)]
        got = fa.group_job(fa.group_from_reps(members))
        want = fa.job_from_reps(members)
        for n in JOB_INT_FIELDS:
            assert np.array_equal(got[n], want[n]), (i, n)
        if len(finite) == len(members):
            assert_job_equal(got, want, len(members), i)
    assert_job_equal(fa.group_job(fa.group_from_reps(PLAIN)), fa.job_from_reps(PLAIN), len(PLAIN))
    assert_job_equal(fa.group_job(gr.Group().record()), fa.job_from_reps(PLAIN[:0]), 0)
    failed = EDGES[EDGES["status"] != 0]
    assert_job_equal(fa.group_job(fa.group_from_reps(failed)), fa.job_from_reps(failed), 0)


def test_summarize_group():
    recs = PLAIN[:6]
    s = fa.summarize_group(fa.group_from_reps(recs))
    assert s["replications"] == 6 and s["decisions"] == int(recs["n_tasks"].sum())
    vals = [gr.metrics(r)[0][1] for r in recs]
    f = s["replications_by_metric"]["respMean_ms"]
    assert f["count"] == 6 and f["overflow"] == 0
    assert f["mean"] == pytest.approx(np.mean(vals) * 1e-9, rel=1e-12)
    assert f["stddev"] == pytest.approx(np.std(np.array(vals, dtype=np.float64), ddof=1) * 1e-9, rel=1e-9)
    assert f["min"] == min(vals) * 1e-9 and f["max"] == max(vals) * 1e-9
    e = s["replications_by_metric"]["energy_j"]
    assert e["mean"] == pytest.approx(float(recs["energy_j"].mean()), abs=1e-6)
    assert fa.summarize_group(gr.Group().record())["replications_by_metric"]["makespan_s"] == dict(count=0, overflow=0)


def parse_sca(path):
    """{module: {"scalars": {name: text}, "stats": {name: {field: text}}}} in file order."""
    mods, cur = {}, None
    for ln in open(path).read().splitlines():
        m = re.match(r'scalar (\S+) \t("?)(.+?)\2 \t(\S+)$', ln)
        if m:
            mods.setdefault(m.group(1), {"scalars": {}, "stats": {}})["scalars"][m.group(3)] = m.group(4)
            continue
        m = re.match(r"statistic (\S+) \t(\S+)$", ln)
        if m:
            cur = mods.setdefault(m.group(1), {"scalars": {}, "stats": {}})["stats"].setdefault(m.group(2), {})
            continue
        m = re.match(r"field (\S+) (\S+)$", ln)
        if m:
            cur[m.group(1)] = m.group(2)
    return mods


def expected_fields(mom: gr.Mom, e: int):
    """cStdDev's fields from the exact sums, as exact rationals in units of 10^-e (None: -nan)."""
    n, s, q, u = mom.count, gr.signed(mom.sum, 128), mom.sq, Fraction(1, 10**e)
    f = {"sum": s * u, "sqrsum": q * u * u, "mean": None, "stddev": None, "min": None, "max": None}
    if n:
        f.update(mean=Fraction(s, n) * u, min=mom.mn * u, max=mom.mx * u)
    if n > 1:
        f["stddev"] = Fraction(max(n * q - s * s, 0), n * (n - 1)) * u * u   # the variance; compared squared
    return f


def test_writer_blocks_read_back(tmp_path):
    """Names, counts and the %.14g values of every field: 14 significant digits of the exact
    rational (a relative 5e-14 for the print, plus the writer's long double arithmetic)."""
    allrec = np.concatenate([EDGES, PLAIN])
    of = np.arange(len(allrec)) % 3
    of[::11] = 3   # group 3 takes a few, group 4 none
    ref, _ = gr.reduce_groups(allrec, of, 5)
    recs = gr.records(ref)
    path = str(tmp_path / "g.sca")
    formats.write_sca(path, fa.job_from_reps(PLAIN))
    formats.write_sca_groups(path, recs, append=True)
    formats.write_sca_groups(path, recs[:1], append=True)                            # G == 1: .replications
    formats.write_sca_groups(path, recs[:2], module=["FogNet.low", "FogNet.high"], append=True)
    mods = parse_sca(path)
    want_mods = {f"FogNet.group[{g}]": ref[g] for g in range(5)}
    want_mods.update({"FogNet.replications": ref[0], "FogNet.low": ref[0], "FogNet.high": ref[1]})
    for mod, g in want_mods.items():
        blk = mods[mod]
        assert blk["scalars"]["replications"] == str(g.head[0])
        assert blk["scalars"]["failed replications"] == str(g.head[1])
        assert blk["scalars"]["replications the reference aborts"] == str(g.head[2])
        assert list(blk["stats"]) == [n + ":replications" for n in gr.SCA_NAMES]
        for k, name in enumerate(gr.SCA_NAMES):
            got, mom = blk["stats"][name + ":replications"], g.across[k]
            assert got["count"] == str(mom.count)
            lost = blk["scalars"].get(f"{name} replications lost")
            assert lost == (str(mom.overflow) if mom.overflow else None), (mod, name)
            for fld, want in expected_fields(mom, gr.UNIT_EXP[k]).items():
                if want is None:
                    assert got[fld] == "-nan", (mod, name, fld)
                    continue
                val = float(got[fld])
                exact = Fraction(val) ** 2 if fld == "stddev" else Fraction(val)
                tol = Fraction(4 if fld == "stddev" else 2, 10**13)
                assert abs(exact - want) <= tol * abs(want), (mod, name, fld, got[fld], float(want))
                assert got[fld] == "%.14g" % val                                   # the %.14g form itself
    assert mods["FogNet.group[4]"]["stats"]["energy:replications"]["count"] == "0"
    with pytest.raises(fa.FognetError):
        formats.write_sca_groups(path, recs[:2], module=["one"])


def test_group_check_under_sanitizers(tmp_path):
    """tests/c/group_check.cpp with AddressSanitizer and UBSan: the floor rule over the edge cases
    and 2 * 10^6 random quotients, the twins on random splits, the writer's paths."""
    exe = str(tmp_path / "group_check")
    csrc = os.path.join(ROOT, "fognetsimpp_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "group_check.cpp"), os.path.join(csrc, "stats_host.cpp"),
                    os.path.join(csrc, "io.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "group_check: all checks passed" in p.stdout


def test_driver_refusals(tmp_path):
    from test_driver import INI, drive
    sca = str(tmp_path / "a.sca")
    base = ("-f", INI, "--users", "user[2]", "--dry-run")
    for bad, msg in ((("--rep-spread",), "give --sca FILE"),
                     (("--sca", sca, "--rep-spread", "--reps", "2", "--world", "2", "--comm-id", str(tmp_path / "id")),
                      "--world 1")):
        p = drive(*base, *bad, check=False)
        assert p.returncode != 0 and msg in p.stderr and "--rep-spread" in p.stderr, (bad, p.stderr)
    p = drive("-f", INI, "-c", "Example", "--nodes", "5", "--sca", sca, "--rep-spread", "--dry-run", check=False)
    assert p.returncode != 0 and "--rep-spread applies to BrokerBaseApp3 runs" in p.stderr  # the v2 broker
    drive(*base, "--sca", sca, "--rep-spread")
    drive(*base, "--sca", sca, "--rep-spread", "--compare", "rr", "--node-stats")
    assert "--rep-spread" in drive("--help").stdout
