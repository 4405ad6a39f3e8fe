"""Inputs shared by tests/test_retest_cpu.py (the host statement ``to_graph.retest_neighbourhood``, no GPU) and
tests/test_gpu_retest.py (``LightpathPredictor.retest`` against ``predict`` over ``infer.materialise_retest``'s samples, bit
for bit).

The random inputs are ``place_cases.batch``'s samples: the dense 4 x 70 grid, 10 - 12 lightpaths per sample crowded into
the slots 52 ... 69, two samples, without and with a flagged lightpath of their own.  ``samples()`` asserts two conditions
on them at threshold 0.12: at least half of all lightpaths have two or more sources, and at most a quarter have none -- a
retest that found nobody would pass otherwise.  The hand cases name what they pin in ``HAND``; each is a ``Case``: sample 0
of ``ns`` with ``want`` the tuples ``to_graph.retest_neighbourhood`` must return -- ``(conn, node, sources)`` per lightpath
-- stated by hand, and ``count`` the sample's own flagged lightpaths.  The slots are 0.05 apart: at threshold 0.07 a slot
meets its two neighbours, at 0.12 two slots either side."""
import functools
from collections import namedtuple

import place_cases as PC
import status_infer_cases as SK
from gnn_qot_estimation_amd import to_graph as TG

FEATS, FI, LUT_COL = PC.FEATS, PC.FI, PC.LUT_COL
THRESHOLDS = PC.THRESHOLDS                                  # (0.05, 0.12)

Case = namedtuple("Case", "ns thr want count")


def host(ns, s, thr):
    return TG.retest_neighbourhood(ns.data[s], ns.freq, FI, thr)


@functools.lru_cache(maxsize=None)
def samples(flagged=False):
    """The ``NetworkStatus`` of ``place_cases.batch(seed=0, S=2, flagged=flagged)`` with the conditions a retest needs."""
    ns = PC.batch(0, S=2, flagged=flagged).ns
    degrees = [len(t[2]) for s in range(2) for t in host(ns, s, 0.12)]
    assert 2 * sum(d >= 2 for d in degrees) >= len(degrees), degrees
    assert 4 * sum(d == 0 for d in degrees) <= len(degrees), degrees
    return ns


# ------------------------------------------------------------------ hand cases
def _no_source():
    """conn 8 and conn 9 far apart: both rows sum no message (na = 0), only the self loop."""
    data, freq = PC.grid()
    data[0, :, 1, 11] = SK.vec(8, 64, 70000, 9, freq[11])
    data[0, :, 3, 40] = SK.vec(9, 16, 90000, 5, freq[40])
    return Case(SK.status(data, freq), 0.07, [(8, 0, []), (9, 1, [])], 0)


def _three_links():
    """conn 8 runs over three links and has a source on each (two on link 2); the others meet conn 8 alone -- 7 and 9 are
    two slots apart."""
    data, freq = PC.grid()
    data[0, :, 0, 20] = data[0, :, 1, 20] = data[0, :, 2, 20] = SK.vec(8, 64, 70000, 9, freq[20])
    data[0, :, 0, 21] = SK.vec(5, 8, 50000, 2, freq[21])
    data[0, :, 1, 21] = SK.vec(6, 32, 40000, 3, freq[21])
    data[0, :, 2, 19] = SK.vec(7, 4, 30000, 1, freq[19])
    data[0, :, 2, 21] = SK.vec(9, 16, 90000, 5, freq[21])
    return Case(SK.status(data, freq), 0.07, [(8, 0, [5, 6, 7, 9]), (5, 1, [8]), (6, 2, [8]), (7, 3, [8]), (9, 4, [8])], 0)


def _flagged():
    """The sample's own lightpath under test, conn 8: retested itself (flagging it again changes nothing), and a source
    of conn 7 -- it stays flagged there, so ``is_lut = 1`` occurs inside a message."""
    data, freq = PC.grid()
    data[0, :, 1, 11] = SK.vec(8, 64, 70000, 9, freq[11], SK.UNDER_TEST)
    data[0, :, 1, 12] = SK.vec(7, 4, 30000, 1, freq[12])
    return Case(SK.status(data, freq), 0.07, [(8, 0, [7]), (7, 1, [8])], 1)


def _shared():
    """conn 8 and conn 5 share two links and meet on two slots of each: one message either way.  conn 9 is too far."""
    data, freq = PC.grid()
    for l in (0, 1):
        data[0, :, l, 1] = data[0, :, l, 4] = SK.vec(8, 64, 70000, 9, freq[1])
        data[0, :, l, 2] = data[0, :, l, 3] = SK.vec(5, 8, 50000, 2, freq[2])
    data[0, :, 1, 7] = SK.vec(9, 4, 30000, 1, freq[7])
    return Case(SK.status(data, freq), 0.07, [(8, 0, [5]), (5, 1, [8]), (9, 2, [])], 0)


def _empty():
    data, freq = PC.grid()
    return Case(SK.status(data, freq), 0.12, [], 0)


def _crowd():
    """``place_cases.crowd(255)``: 255 single-channel lightpaths in scan order, lightpath k (conn 10 + k) on link k // 70,
    slot k % 70.  At 0.12 its sources are the lightpaths up to two slots either side on its link: slots in every chunk,
    lightpath numbers beyond one wave."""
    ns, Q = PC.crowd(255).ns, PC.Q
    want = [(10 + k, k, [10 + j for j in range(k - 2, k + 3) if j != k and 0 <= j < 255 and j // Q == k // Q]) for k in range(255)]
    return Case(ns, 0.12, want, 0)


HAND = {
    "a lightpath without a source": _no_source,
    "a lightpath on three links with sources on each": _three_links,
    "the sample's flagged lightpath, retested itself and as a source": _flagged,
    "two lightpaths sharing two links and several slots": _shared,
    "an empty sample": _empty,
    "255 lightpaths": _crowd,
}
