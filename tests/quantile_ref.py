"""Expected quantiles (fognet_quantiles_dev, fognet_job_quantiles_dev) from a finished replay's
per-task outputs, in plain Python ints (test infrastructure for test_quantiles*.py; no GPU needed).

Worded as include/fognet_hip.h words them ("Quantiles"): a signal's population is the raw values
of its emissions as window_ref.replication_events lists them (a lost emission, raw None, is no
member), the rank rule is nearest rank on sorted(), and the job's population is the
concatenation over the replications whose status is OK.
"""
from __future__ import annotations

import numpy as np

import window_ref as wr
from fognetsimpp_amd import _abi

SIGNALS = _abi.WINDOW_SIGNALS  # queue, delay, latency, latencyH1, taskTime
I64_MAX = 2**63 - 1
PPM = 10**6


def rank_of(n: int, ppm: int) -> int:
    """k = max(1, ceil(n * ppm / 10^6)), 1-based, in integers."""
    assert n > 0 and 0 <= ppm <= PPM
    return max(1, -(-n * ppm // PPM))


def nearest_rank(values, ppm: int) -> int:
    """The quantile of a population of ints; INT64_MAX for an empty one."""
    if not len(values):
        return I64_MAX
    return sorted(int(v) for v in values)[rank_of(len(values), ppm) - 1]


def populations(points) -> dict:
    """{signal: [raw values]} of replication_events' points."""
    pop = {s: [] for s in SIGNALS}
    for what, _, raw in points:
        if what in pop and raw is not None:
            pop[what].append(int(raw))
    return pop


def replication_populations(tr, o, user_of, user_ul, user_dl, flags=None, up=0, statuses=None):
    """[R] of ({signal: values}, n_unassigned), None for a replication that is not read."""
    out = []
    for _, ev in wr._replications(tr, o, user_of, user_ul, user_dl, flags, up, statuses):
        out.append(None if ev is None else (populations(ev[0]), ev[2]))
    return out


def table(pops: dict, ppm) -> tuple:
    """([5, Q] values, [5] counts) of one population set."""
    value = np.array([[nearest_rank(pops[s], int(p)) for p in ppm] for s in SIGNALS], np.int64).reshape(len(SIGNALS), len(ppm))
    return value, np.array([len(pops[s]) for s in SIGNALS], np.int64)


def expected(tr, o, user_of, user_ul, user_dl, ppm, flags=None, up=0, statuses=None):
    """([R, 5, Q] values, [R, 5] counts, [R] n_unassigned) per replication; arguments as
    window_ref.expected."""
    reps = replication_populations(tr, o, user_of, user_ul, user_dl, flags, up, statuses)
    R, Q = len(reps), len(ppm)
    value = np.full((R, len(SIGNALS), Q), I64_MAX, np.int64)
    count, un = np.zeros((R, len(SIGNALS)), np.int64), np.zeros(R, np.int64)
    for r, rep in enumerate(reps):
        if rep is not None:
            value[r], count[r] = table(rep[0], ppm)
            un[r] = rep[1]
    return value, count, un


def expected_job(tr, o, user_of, user_ul, user_dl, ppm, flags=None, up=0, statuses=None):
    """([5, Q] values, [5] counts) of the job: the populations of the OK replications pooled."""
    st = np.asarray(o["stats"]["status"] if statuses is None else statuses)
    reps = replication_populations(tr, o, user_of, user_ul, user_dl, flags, up, statuses)
    pool = {s: [] for s in SIGNALS}
    for r, rep in enumerate(reps):
        if rep is not None and int(st[r]) == _abi.FOGNET_OK:
            for s in SIGNALS:
                pool[s] += rep[0][s]
    return table(pool, ppm)
