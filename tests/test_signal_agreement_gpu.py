"""The vectors are the rows the records count, on the device: fognet_node_stats_dev,
fognet_per_user_stats_dev and fognet_signal_vectors_dev run on one replay, and the values of
every vector are held to the record of the same signal (test_signal_agreement.py states the
comparison and shows on the oracle's outputs that these cases have rows of every kind).  Each
case runs with the default layouts and with every pass's accumulators and sort forced to HBM."""
from __future__ import annotations

import numpy as np
import pytest

import fognetsimpp_amd as fa
from fognetsimpp_amd import _abi
from test_per_user_stats import carry_case, draw_links, trace_case
from test_signal_agreement import SHAPES, TS, assert_vectors_are_the_records, trace_users
from test_signal_vectors_gpu import I32_MAX, device_replay, mixed_batch

pytestmark = pytest.mark.gpu

HBM = ("FOGNET_NODE_STATS", "FOGNET_USER_STATS", "FOGNET_VEC_SORT")


def three_passes(ctx, monkeypatch, d, out, who, uu, ud, policy="REF_V3", what=""):
    """The comparison in both layouts; the default layout's row counts."""
    R, N, U = d["arrive"].shape[0], d["mips"].shape[-1], np.shape(uu)[-1]
    counts = []
    for hbm in (False, True):
        for k in HBM:
            monkeypatch.setenv(k, "hbm") if hbm else monkeypatch.delenv(k, raising=False)
        nodes = fa.node_stats(ctx, d, out, policy=policy).cpu().numpy().view(_abi.NODE_STATS_DTYPE).reshape(R, N)
        recs, un = fa.per_user_stats(ctx, d, out, who, uu, ud)
        users = recs.cpu().numpy().view(_abi.USER_STATS_DTYPE).reshape(R, U)
        vec = fa.signal_vectors(ctx, d, out, who, uu, ud)
        assert (un.cpu().numpy() == 0).all() and (vec["n_unassigned"] == 0).all()
        counts.append(assert_vectors_are_the_records(vec, nodes, users, f"{what} {'hbm' if hbm else 'default'}"))
    assert counts[0] == counts[1]
    return counts[0]


@pytest.mark.parametrize("N,U", SHAPES)
@pytest.mark.parametrize("T", TS)
def test_vectors_are_the_rows_the_records_count(ctx, monkeypatch, T, N, U):
    tr = trace_case(N, T)[0]
    d, out = device_replay(ctx, ("trace", N, T), tr)
    assert (out.rep_stats()["status"] == 0).all()
    n = three_passes(ctx, monkeypatch, d, out, *trace_users(N, U, T), what=f"N={N} U={U} T={T}")
    assert n["delay"] == 3 * T and n["latencyH1"] >= 3 * T and n["lost user-side"] == 0
    if T >= 63:  # a row of every kind: nothing is lost, so latencyH1 holds every pubAck, and relayed acks beyond them
        assert n["queueTime"] > 0 and n["latency"] > 0 and n["taskTime"] > 0 and n["latencyH1"] > n["delay"], n


def test_ext_lat(ctx, monkeypatch):
    tr = trace_case(5, 129, "EXT_LAT")[0]
    d, out = device_replay(ctx, ("trace", 5, 129, "EXT_LAT"), tr, policy="EXT_LAT")
    n = three_passes(ctx, monkeypatch, d, out, *trace_users(5, 3, 129), policy="EXT_LAT", what="EXT_LAT")
    assert n["lost user-side"] == 0  # (so latencyH1 holds every pubAck, and relayed acks beyond them)
    assert n["queueTime"] > 0 and n["latency"] > 0 and n["taskTime"] > 0 and n["latencyH1"] > n["delay"] == 3 * 129


def test_lost_emissions_are_counted_and_have_no_row(ctx, monkeypatch):
    tr, who, uu, ud = carry_case()
    d, out = device_replay(ctx, None, tr)
    n = three_passes(ctx, monkeypatch, d, out, who, uu, ud, what="carry")
    assert n["lost user-side"] > 0 and n["delay"] == 96


def test_a_failed_replication_between_good_ones(ctx, monkeypatch):
    """[good, failed, REF_ABORTED, good]: all-zero offsets against empty records; nothing of the failed one is read."""
    tr = mixed_batch()
    who = np.array([[0, 1, 2, 0, 1]] * 4, np.int32)
    uu, ud = draw_links(3, 4, 3, True)
    who[1] = I32_MAX
    uu[1] = ud[1] = 0x5A5A5A5A5A5A5A5A
    d, out = device_replay(ctx, None, tr, ref_abort=True)
    st = [int(s) for s in out.rep_stats()["status"]]
    assert st[0] == st[3] == 0 and st[2] == _abi.FOGNET_REF_ABORTED and st[1] not in (0, _abi.FOGNET_REF_ABORTED)
    n = three_passes(ctx, monkeypatch, d, out, who, uu, ud, what="mixed")
    decided = out.rep_stats()["n_tasks"]
    assert n["delay"] == int(decided[0] + decided[2] + decided[3]) >= 11  # every decided publish but the failed one's
