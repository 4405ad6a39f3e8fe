"""Inputs shared by tests/test_place_impact_cpu.py (the host statement ``to_graph.placement_impact`` and the definition
``infer.materialise_retest``, no GPU) and tests/test_gpu_place_impact.py (``LightpathPredictor.place_impact`` against
``predict`` over ``materialise_retest``'s samples, bit for bit).

The random inputs are ``place_cases.batch``'s: the dense 4 x 70 grid, a dozen lightpaths crowded into the slots 52 ... 69.
``batch()`` asserts two conditions on them at threshold 0.12: at least half of the candidates have two or more affected
lightpaths, and at least half of all affected lightpaths have a source other than the candidate -- a retest that lost the
lightpath's own neighbourhood, or found nobody, would pass otherwise.  The hand cases name what they pin in ``HAND``; each
is an ``Impact``: one candidate (conn 5) in sample 0 of ``ns``, with ``want`` the tuples ``to_graph.placement_impact`` must
return -- ``(conn, node_before, node_after, sources_before, sources_after)`` per affected lightpath -- stated by hand.  The
slots are 0.05 apart: at threshold 0.07 a slot meets its two neighbours, at 0.12 two slots either side."""
import functools
from collections import namedtuple

import numpy as np

import place_cases as PC
import status_infer_cases as SK
from gnn_qot_estimation_amd import to_graph as TG

FEATS, FI, LUT_COL = PC.FEATS, PC.FI, PC.LUT_COL
THRESHOLDS = PC.THRESHOLDS
CAND = 5                                                    # the candidate's conn in every hand case

# count: the flagged lightpaths of the sample plus the candidate (place's count)
Impact = namedtuple("Impact", "ns values cells thr want count")


def host_impact(b, k, thr):
    return TG.placement_impact(b.ns.data[b.samples[k]], b.ns.freq, FI, b.values[k], PC.candidate_cells(b, k), thr)


@functools.lru_cache(maxsize=None)
def batch(seed=0, K=8, S=2, flagged=False):
    """``place_cases.batch`` with the conditions a retest needs of its inputs."""
    b = PC.batch(seed, K, S, flagged)
    impacts = [host_impact(b, k, 0.12) for k in range(K)]
    assert 2 * sum(len(imp) >= 2 for imp in impacts) >= K, [len(imp) for imp in impacts]
    own = [len(t[3]) >= 1 for imp in impacts for t in imp]      # sources_before: a source other than the candidate
    assert own and 2 * sum(own) >= len(own), own
    return b


def as_batch(case):
    return PC.Batch(case.ns, [0], case.values[None, :], np.asarray(case.cells, dtype=np.int64), [0, np.asarray(case.cells).shape[1]])


def _candidate(freq, slot):
    return SK.vec(CAND, 8, 50000, 2, freq[slot], SK.UNDER_TEST)


# ------------------------------------------------------------------ hand cases: where the candidate's row is inserted
def _candidate_first():
    """The candidate on channel (0, 10) is seen before everything: it is the FIRST message of conn 8 (0, 11), whose own
    sources 7 and 9 sit either side of its second channel (2, 20)."""
    data, freq = PC.grid()
    data[0, :, 0, 11] = data[0, :, 2, 20] = SK.vec(8, 64, 70000, 9, freq[11])
    data[0, :, 2, 19] = SK.vec(7, 4, 30000, 1, freq[19])
    data[0, :, 2, 21] = SK.vec(9, 16, 90000, 5, freq[21])
    return Impact(SK.status(data, freq), _candidate(freq, 10), np.array([[0], [10]]), 0.07, [(8, 0, 1, [7, 9], [CAND, 7, 9])], 1)


def _candidate_last():
    """The candidate on (3, 40) is seen behind everything: the LAST message of conn 8."""
    data, freq = PC.grid()
    data[0, :, 1, 5] = data[0, :, 3, 41] = SK.vec(8, 64, 70000, 9, freq[5])
    data[0, :, 1, 4] = SK.vec(7, 4, 30000, 1, freq[4])
    data[0, :, 1, 6] = SK.vec(9, 16, 90000, 5, freq[6])
    return Impact(SK.status(data, freq), _candidate(freq, 40), np.array([[3], [40]]), 0.07, [(8, 1, 1, [7, 9], [7, 9, CAND])], 1)


def _candidate_between():
    """The candidate on (1, 30) is seen behind conn 7 (0, 4) and before conn 9 (2, 6): BETWEEN the two messages of conn 8."""
    data, freq = PC.grid()
    data[0, :, 0, 5] = data[0, :, 2, 5] = data[0, :, 1, 31] = SK.vec(8, 64, 70000, 9, freq[5])
    data[0, :, 0, 4] = SK.vec(7, 4, 30000, 1, freq[4])
    data[0, :, 2, 6] = SK.vec(9, 16, 90000, 5, freq[6])
    return Impact(SK.status(data, freq), _candidate(freq, 30), np.array([[1], [30]]), 0.07, [(8, 1, 1, [7, 9], [7, CAND, 9])], 1)


def _only_source():
    """The candidate is the only source of conn 8: ``before`` sums no message (na = 0), only the self loop."""
    data, freq = PC.grid()
    data[0, :, 1, 11] = SK.vec(8, 64, 70000, 9, freq[11])
    data[0, :, 3, 40] = SK.vec(9, 16, 90000, 5, freq[40])                     # far away: nobody's neighbour
    return Impact(SK.status(data, freq), _candidate(freq, 10), np.array([[1], [10]]), 0.07, [(8, 0, 1, [], [CAND])], 1)


def _wider_neighbourhood():
    """conn 8 runs over three links; the candidate meets it on link 0 only, and conn 8 has sources on the links 1 and 2,
    which the candidate does not touch: its neighbourhood is larger than the candidate's (which is conn 8 alone)."""
    data, freq = PC.grid()
    data[0, :, 0, 20] = data[0, :, 1, 20] = data[0, :, 2, 20] = SK.vec(8, 64, 70000, 9, freq[20])
    data[0, :, 1, 21] = SK.vec(6, 32, 40000, 3, freq[21])
    data[0, :, 2, 19] = SK.vec(7, 4, 30000, 1, freq[19])
    data[0, :, 2, 21] = SK.vec(9, 16, 90000, 5, freq[21])
    return Impact(SK.status(data, freq), _candidate(freq, 21), np.array([[0], [21]]), 0.07,
                  [(8, 0, 0, [6, 7, 9], [CAND, 6, 7, 9])], 1)


def _flagged_is_affected():
    """The sample's own lightpath under test, conn 8, is the affected one: flagging it again changes nothing."""
    data, freq = PC.grid()
    data[0, :, 1, 11] = SK.vec(8, 64, 70000, 9, freq[11], SK.UNDER_TEST)
    data[0, :, 1, 12] = SK.vec(7, 4, 30000, 1, freq[12])
    return Impact(SK.status(data, freq), _candidate(freq, 10), np.array([[1], [10]]), 0.07, [(8, 0, 1, [7], [CAND, 7])], 2)


def _flagged_is_a_source():
    """The sample's own lightpath under test, conn 7, is a source of the affected conn 8: it stays flagged in the retest
    sample, so ``is_lut = 1`` occurs inside a message."""
    data, freq = PC.grid()
    data[0, :, 1, 11] = SK.vec(8, 64, 70000, 9, freq[11])
    data[0, :, 1, 12] = SK.vec(7, 4, 30000, 1, freq[12], SK.UNDER_TEST)
    return Impact(SK.status(data, freq), _candidate(freq, 10), np.array([[1], [10]]), 0.07, [(8, 0, 1, [7], [CAND, 7])], 2)


def _no_interferer():
    data, freq = PC.grid()
    data[0, :, 0, 40] = SK.vec(9, 16, 90000, 5, freq[40])
    return Impact(SK.status(data, freq), _candidate(freq, 1), np.array([[0, 2], [1, 1]]), 0.12, [], 1)


def _crowd():
    """``place_cases.crowd(255)``: 255 single-channel lightpaths in scan order, the candidate on (3, 46).  The affected
    lightpath (slot 44 of link 3) has number 254, its sources the numbers 252 and 253, and the candidate is first seen at
    position 255: the staging loop's second and later passes of 64, on both sides of the insertion."""
    c = PC.crowd(255)
    near = 10 + 3 * PC.Q + 44
    return Impact(c.ns, c.values, c.cells, c.thr, [(near, 254, 254, [near - 2, near - 1], [near - 2, near - 1, CAND])], 1)


HAND = {
    "the candidate is seen before all sources of the lightpath": _candidate_first,
    "the candidate is seen after all sources of the lightpath": _candidate_last,
    "the candidate is seen between two sources of the lightpath": _candidate_between,
    "the candidate is the only source: before sums no message": _only_source,
    "an affected lightpath with sources on links the candidate does not touch": _wider_neighbourhood,
    "the sample's flagged lightpath is the affected one": _flagged_is_affected,
    "the sample's flagged lightpath is a source of the affected one": _flagged_is_a_source,
    "no interferer": _no_interferer,
    "a table beyond one wave": _crowd,
}
