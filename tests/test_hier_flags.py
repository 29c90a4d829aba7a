"""EXT_HIER escalation flags, host side (no GPU): the flags hier_ref rebuilds from the
oracle's per-task outputs are the oracle's decisions (hier_ref.expected_flags asserts the
node of every publish), and with them the closed forms of the two statistics passes --
the hop hier_up_tick added to an escalated task's arrival at its node -- equal the
oracle's event-level records bit for bit; without them they do not.  The cases are the
ones test_hier_flags_gpu.py runs on the device."""
import numpy as np
import pytest

import hier_ref as hr
import node_stats_ref as ns
import user_stats_ref as us

REGION_NODES = hr.REGION_NODES


@pytest.mark.parametrize("name", list(hr.CASES))
def test_flags_are_the_oracles_decisions(name):
    tr, uu, ud, o, flags, thr, up = hr.case(name)
    assert (o["stats"]["status"] == 0).all()
    assert flags.shape == tr["arrive"].shape and set(np.unique(flags)) <= {0, 1}
    assert (flags[:2].sum(axis=1) >= 50).all(), flags.sum(axis=1)
    own = o["node"] // REGION_NODES == tr["region"]
    if name == "D":  # one region: every escalation lands inside it, the node does not give the flag away
        assert own.all() and not (flags == 0).all()
    else:
        assert (flags[2] == 0).all()  # the quiet replication
        # the first escalation lies past the first 64-publish chunk
        assert all(64 <= int(np.argmax(flags[r])) for r in range(2))
    if name == "B":
        assert ((flags == 1) & (o["status"] == 5)).any(), "no escalated task started on arrival"
    assert ((flags == 1) & (o["status"] == 4)).any()


@pytest.mark.parametrize("name", list(hr.CASES))
def test_user_signals_need_the_flags(name):
    tr, uu, ud, o, flags, thr, up = hr.case(name)
    us.assert_user_parity(hr.user_expected(tr, o, uu, ud, flags, up), o["user"])
    plain = hr.user_expected(tr, o, uu, ud, np.zeros_like(flags), up)
    assert plain.tobytes() == us.expected(tr, o, uu, ud).tobytes()  # (the restatement itself)
    for r in range(2):
        assert plain[r].tobytes() != o["user"][r].tobytes(), (name, r)
        for sig in ("delay", "taskTime"):  # only the node ack's term moves
            assert plain[r][sig].tobytes() == o["user"][r][sig].tobytes(), (name, r, sig)


@pytest.mark.parametrize("name", list(hr.CASES))
def test_node_records_need_the_flags(name):
    tr, uu, ud, o, flags, thr, up = hr.case(name)
    recs = hr.node_expected(tr, o, flags, up)
    plain = hr.node_expected(tr, o, np.zeros_like(flags), up)
    assert plain.tobytes() == ns.expected(tr, o).tobytes()  # (the restatement itself)
    for r in range(flags.shape[0]):
        ns.assert_merge_is_rep_record(recs[r], o["stats"][r])
    for r in range(2):
        with pytest.raises(AssertionError):
            ns.assert_merge_is_rep_record(plain[r], o["stats"][r])
