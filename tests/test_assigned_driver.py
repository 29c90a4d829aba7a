"""fognet_replay --assign: option parsing (CPU, --dry-run) and, on the GPU, the totals of the
result file against a Python replay of the same assignment (tests/assigned_ref.py)."""
import re

import numpy as np
import pytest

import assigned_ref as ar
from test_driver import INI, drive


class Mt19937_64:
    """std::mt19937_64 (Matsumoto & Nishimura 2004, the C++11 parameters), raw 64-bit draws."""
    NN, MM, M = 312, 156, (1 << 64) - 1

    def __init__(self, seed: int):
        self.mt = [seed & self.M]
        for i in range(1, self.NN):
            x = self.mt[-1]
            self.mt.append((6364136223846793005 * (x ^ (x >> 62)) + i) & self.M)
        self.i = self.NN

    def __call__(self) -> int:
        if self.i >= self.NN:
            mt, nn, mm = self.mt, self.NN, self.MM
            for k in range(nn):
                x = (mt[k] & 0xFFFFFFFF80000000) | (mt[(k + 1) % nn] & 0x7FFFFFFF)
                mt[k] = mt[(k + mm) % nn] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
            self.i = 0
        x = self.mt[self.i]
        self.i += 1
        x ^= (x >> 29) & 0x5555555555555555
        x ^= (x << 17) & 0x71D67FFFEDA60000
        x ^= (x << 37) & 0xFFF7EEE000000000
        x ^= x >> 43
        return x & self.M


def test_mt19937_64_known_answer():
    g = Mt19937_64(5489)  # the C++ standard's check value: the 10000th draw of the default seed
    for _ in range(9999):
        g()
    assert g() == 9981545732273789042


def test_dry_run_parsing():
    args = ("-f", INI, "--users", "user[4]", "--reps", "2", "--dry-run")
    assert "publishes/rep=" in drive(*args, "--assign", "rr").stdout
    assert "publishes/rep=" in drive(*args, "--assign", "random").stdout
    assert "publishes/rep=" in drive(*args, "--assign", "random:7").stdout
    for bad, msg in ((("--assign", "lifo"), "rr or random"), (("--assign", "random:x"), "not an integer"),
                     (("--assign", "random:-1"), "SEED must be >= 0"),
                     (("--assign", "rr", "--policy", "EXT_LAT"), "not together with --policy")):
        p = drive(*args, *bad, check=False)
        assert p.returncode != 0 and msg in p.stderr, (bad, p.stderr)
    p = drive("-f", INI, "-c", "Example", "--nodes", "5", "--assign", "rr", "--dry-run", check=False)
    assert p.returncode != 0 and "BrokerBaseApp3 runs" in p.stderr  # the v2 broker
    assert "--assign rr|random[:SEED]" in drive("--help").stdout and "mt19937_64" in drive("--help").stdout


def scalars(text: str) -> dict:
    out = {}
    for m in re.finditer(r'^scalar \S+ \t("[^"]+"|\S+) \t(\S+)$', text, re.M):
        out.setdefault(m.group(1).strip('"'), m.group(2))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["rr", "random:7"])
def test_sca_totals_equal_a_python_replay(ctx, tmp_path, rule):
    from fognetsimpp_amd import formats
    sca, trc, vec = (str(tmp_path / n) for n in ("a.sca", "a.fogntrc", "a.vec"))
    R = 3
    out = drive("-f", INI, "--users", "user[6]", "--reps", str(R), "--assign", rule, "--sca", sca, "--trace-out", trc,
                "--vec", vec, "--node-stats", "--user-stats", "--vec-users").stdout
    tr = formats.load_trace(trc)
    T, N = tr["arrive"].shape[1], len(tr["mips"])
    if rule == "rr":
        assign = np.tile(np.arange(T) % N, (R, 1))
    else:
        gens = [Mt19937_64(7 + r) for r in range(R)]
        assign = np.array([[g() % N for _ in range(T)] for g in gens])
    want = ar.replay(tr, assign)
    assert (want["stats"]["status"] == 0).all()
    text = open(sca).read()
    assert re.search(r"^attr assign " + re.escape(rule) + "$", text, re.M) and text.count("version 2") == 1
    assert re.search(r"^attr assign " + re.escape(rule) + "$", open(vec).read(), re.M)
    s = scalars(text)
    assert int(s["replications"]) == R and int(s["failed replications"]) == 0
    assert int(s["decisions"]) == R * T == int(want["stats"]["n_tasks"].sum())
    assert int(s["FES events"]) == int(want["stats"]["events"].sum())
    assert int(s["tasks queued"]) == int((want["status"] == 4).sum())
    assert int(s["tasks started"]) == int((want["status"] == 5).sum())
    assert int(s["max pending"]) == int(want["stats"]["max_pending"].max())
    busy = sum(int(tr["req"][r, i]) // int(tr["mips"][assign[r, i]]) for r in range(R) for i in range(T))
    assert int(s["busy seconds"]) == busy
    assert f"policy=assign:{rule}" in out and f"max_pending={int(want['stats']['max_pending'].max())}" in out
    per = [int(x) for x in re.search(r"tasks_per_node=([\d,]+)", out).group(1).split(",")]
    assert per == np.bincount(assign.reshape(-1), minlength=N).tolist()
    assert f"makespan_ticks={int(want['done'].max())}" in out
    assert "fogNode[" in text and ".user[" in text  # --node-stats and --user-stats blocks follow


@pytest.mark.gpu
def test_refusals_return_nonzero_with_a_message(ctx):
    p = drive("-f", INI, "--users", "user[2]", "--assign", "rr", "--policy", "REF_V3", check=False)
    assert p.returncode != 0 and "not together with --policy" in p.stderr
    p = drive("-f", INI, "-c", "Example", "--nodes", "5", "--assign", "random:1", check=False)
    assert p.returncode != 0 and "BrokerBaseApp3 runs" in p.stderr
