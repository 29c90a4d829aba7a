"""tests/assigned_ref.py, the plain-Python restatement of the assigned replay, pinned on the CPU:
fed the oracle's own decisions it must reproduce the oracle's node model, and fed the reference's
recorded decisions it must reproduce what the reference's own handlers did."""
import numpy as np
import pytest

import assigned_ref as ar
import golden_io
import oracle_lib as ol
import tracegen as tg

TPS = 10**12


def oracle(tr, policy="REF_V3", **kw):
    return ol.run_batch(tr["arrive"], tr["req"], tr["mips"], tr["dl"], tr["ul"], tr["init"],
                        policy=ol.POLICIES[policy], down=tr.get("down"), **kw)


def tie_heavy(seed, R, N, T):
    from test_parity_gpu import tie_heavy as th  # the suite's generator
    return th(seed, R, N, T)


def with_crashes(tr, seed, grid=None):
    from test_parity_gpu import with_crashes as wc
    return wc(tr, seed=seed, frac=0.5, grid=grid)


def check(tr, policy="REF_V3", what=""):
    o = oracle(tr, policy)
    assert (o["stats"]["status"] == 0).all(), what
    ar.assert_equals_oracle(ar.replay(tr, o["node"]), o, what)
    return o


@pytest.mark.parametrize("N", [1, 3, 64, 300])
@pytest.mark.parametrize("policy", ["REF_V3", "EXT_LAT"])
def test_oracle_decisions_tracegen(N, policy):
    for T, rho in ((300, 0.9), (129, 3.0)):
        check(tg.make_batch(0x5EED0A00 + N, 3, N, T, rho=rho), policy, f"N={N} T={T}")


@pytest.mark.parametrize("N", [1, 3, 38, 300])
def test_oracle_decisions_tie_heavy(N):
    check(tie_heavy(11 + N, 4, N, 300), "REF_V3", f"tie N={N}")
    check(tie_heavy(12 + N, 2, N, 300), "EXT_LAT", f"tie ext N={N}")


@pytest.mark.parametrize("N", [1, 5, 64])
def test_oracle_decisions_with_down(N):
    tr = with_crashes(tg.make_batch(0x5EED0B00 + N, 4, N, 300, rho=0.9), seed=N)
    o = check(tr, what=f"down N={N}")
    assert (o["done"] < 0).any() and (o["status"] == 9).any()
    check(with_crashes(tie_heavy(300 + N, 4, N, 300), seed=N, grid=10**11), what=f"down tie N={N}")


def test_known_answers():
    for name, tr, _ in golden_io.replay_cases():
        check(tr, what=name)
    for name, tr, _ in golden_io.replay_down_cases():
        check(tr, what=name)
    for name, tr, _ in golden_io.qtime_cases():
        check(tr, what=name)


@pytest.mark.parametrize("case", golden_io.ref_v3_replay_cases(), ids=lambda c: c[0])
def test_recorded_decisions_give_the_recorded_node_model(case):
    """The reference's own handlers with the decision logic taken out: every task's status,
    start and release tick on the prefix the reference defines (what an aborted run never
    reached is 0 / -1 in the recording; its undecided tail is filled from the oracle)."""
    name, tr, _, _, rec = case
    node = np.array(rec["node"], np.int64)
    o = oracle({k: (v[None] if k in ("arrive", "req") else v) for k, v in tr.items()})
    if (node < 0).any():
        assert rec["abort"] is not None
        node = np.where(node < 0, o["node"][0], node)
    got = ar.replay(tr, node)
    assert got["stats"]["status"][0] == 0
    status, start, done = (np.array(rec[k], np.int64) for k in ("status", "start", "done"))
    m = status != 0
    np.testing.assert_array_equal(got["status"][0][m], status[m])
    for mine, theirs in ((got["start"][0], start), (got["done"][0], done)):
        np.testing.assert_array_equal(mine[theirs >= 0], theirs[theirs >= 0])
    if rec["abort"] is None:
        assert m.all() and (done >= 0).all()
    assert m.sum() + (start >= 0).sum() + (done >= 0).sum() >= 3


def test_recordings_are_fourteen():
    assert len(golden_io.ref_v3_replay_cases()) == 14


def test_tie_census():
    """Both outcomes of an arrival at the very tick its predecessor completes occur on these inputs."""
    arrival_first = completion_first = 0
    for N, seed in ((1, 12), (3, 14), (38, 49), (300, 311)):
        tr = tie_heavy(seed, 4, N, 300)
        o = oracle(tr)
        for r in range(4):
            node = o["node"][r]
            a = tr["arrive"][r] + tr["dl"][r][node]
            s = (tr["req"][r] // tr["mips"][r][node]).astype(np.int64) * TPS
            last = {}
            for i in range(300):
                k = int(node[i])
                if k in last and a[i] == o["done"][r][last[k]]:
                    if tr["dl"][r][k] >= s[last[k]]:
                        arrival_first += 1
                        assert o["status"][r][i] == 4
                    else:
                        completion_first += 1
                        assert o["status"][r][i] == 5
                last[k] = i
    assert arrival_first > 0 and completion_first > 0, (arrival_first, completion_first)


def test_refusals():
    tr = tg.make_batch(5, 1, 4, 50)
    one = {k: (v[0] if v.ndim == 2 else v) for k, v in tr.items()}
    node = np.arange(50) % 4

    def refused(**change):
        t = {k: np.array(v) for k, v in one.items()}
        assign = np.array(node)
        for k, (i, v) in change.items():
            (assign if k == "assign" else t[k])[i] = v
        rec = ar.replay_one(t["arrive"], t["req"], assign, t["mips"], t["dl"], t["ul"], t["init"], t.get("down"))[3]
        return int(rec["status"]) == ar.ERR_ARG and int(rec["n_tasks"]) == 0 and int(rec["events"]) == 0

    assert not refused()
    assert refused(assign=(7, 4)) and refused(assign=(0, -1)) and refused(req=(3, -1)) and refused(mips=(2, 0))
    assert refused(arrive=(10, int(one["arrive"][9]) - 1)) and refused(init=(1, int(one["arrive"][0])))
    assert refused(init=(1, int(one["ul"][1]) - 1)) and refused(arrive=(49, (1 << 61) + 1))
    assert refused(req=(5, 2**31 - 1), mips=(1, 1))  # node 1 serves task 5: 2^31 - 1 s


def test_zero_service_same_tick_and_pending():
    """Several zero-service tasks at one tick at one node: each starts on arrival; none has left the
    broker's count when the next is published."""
    z = np.zeros(4, np.int64)
    st, start, done, rec = ar.replay_one(z + 100, [0, 0, 0, 0], [0, 0, 0, 0], [1000], [5], [7], [50])
    assert st.tolist() == [5, 4, 4, 4] and start.tolist() == [105] * 4 and done.tolist() == [105] * 4
    assert int(rec["max_pending"]) == 4 and int(rec["events"]) == 2 + 16
