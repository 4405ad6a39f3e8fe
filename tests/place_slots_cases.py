"""Inputs shared by tests/test_place_slots_cpu.py (the host statement ``to_graph.slot_sweep`` and the definition
``infer.materialise_slot_sweep``, no GPU) and tests/test_gpu_place_slots.py (``LightpathPredictor.place_slots`` against
``materialise_slot_sweep`` + ``place``, bit for bit).

The samples are ``place_cases.batch(seed)``'s DENSE ones -- L = 4 links, Q = 70 slots (ragged against the 64-lane slot walk,
against chunks of 5 and of 32, and above 64), a dozen lightpaths crowded into the slots 52 ... 69 -- with seeded routes of
1 - 3 links.  A sweep over an empty band alone would pass with a kernel that finds nobody, so ``batch()`` asserts a
condition on the inputs, computed with existing code only (raw occupancy ``np.any(sample != 0, axis=0)`` and
``to_graph.placement_neighbourhood``) over the start slots >= 50 of its routes, for ``width`` 1 and 2: at least a quarter
of the (route, slot) pairs are free, at least a quarter are not, and at least a third of the free ones have two or more
interferers at threshold 0.12."""
import functools
from collections import namedtuple

import numpy as np

import place_cases as PC
import status_infer_cases as SK
from gnn_qot_estimation_amd import to_graph as TG

FEATS, FI, LUT_COL = PC.FEATS, PC.FI, PC.LUT_COL
P, L, Q = PC.P, PC.L, PC.Q
BAND0 = 50                                                  # the condition on the inputs is taken from this start slot on
THRESHOLDS = PC.THRESHOLDS
WIDTHS = (1, 2)

# ns: the NetworkStatus; samples [R]; values [R, P]; links [M]; link_ptr [R + 1] (numpy / lists, all on the host)
Routes = namedtuple("Routes", "ns samples values links link_ptr")


def route_links(b, r):
    return b.links[b.link_ptr[r]:b.link_ptr[r + 1]]


def cells_of(links, q, width):
    """The cells of the candidate of a route that starts at slot ``q``: link by link, the ``width`` slots rising."""
    return np.array([[l, q + t] for l in list(links) for t in range(width)], dtype=np.int64).T


def condition(b):
    """The shares the module docstring names, from raw occupancy and ``placement_neighbourhood``: ``(free, crowded)`` as
    fractions of the pairs / of the free pairs."""
    pairs = free = crowded = 0
    for width in WIDTHS:
        for r, s in enumerate(b.samples):
            occupied = np.any(b.ns.data[s] != 0, axis=0)
            for q in range(BAND0, Q):
                cells = cells_of(route_links(b, r), q, width)
                pairs += 1
                if q + width > Q or occupied[cells[0], cells[1]].any():
                    continue
                free += 1
                crowded += len(TG.placement_neighbourhood(b.ns.data[s], b.ns.freq, FI, cells, 0.12)) >= 2
    return free / pairs, crowded / free


@functools.lru_cache(maxsize=None)
def batch(seed=0, R=6, flagged=False):
    """``R`` random routes of 1 - 3 links over ``place_cases.batch(seed)``'s two dense samples (sample numbers repeat)."""
    ns = PC.batch(seed, flagged=flagged).ns
    rng = np.random.default_rng(1000 + seed)
    S = ns.data.shape[0]
    samples = [int(rng.integers(0, S)) for _ in range(R)]
    links, ptr, values = [], [0], []
    for r in range(R):
        on = rng.choice(L, size=int(rng.integers(1, 4)), replace=False)
        links += [int(l) for l in on]
        ptr.append(len(links))
        values.append(PC.random_vec(rng, 900 + r, 0.0, SK.UNDER_TEST))        # (freq: the sweep's to fill in)
    b = Routes(ns, samples, np.stack(values), np.array(links, dtype=np.int64), ptr)
    free, crowded = condition(b)
    assert 0.25 <= free <= 0.75 and 3 * crowded >= 1, (free, crowded)         # a condition on the inputs
    return b


def single(ns, links, values=None, sample=0):
    """One route over sample ``sample`` of ``ns``."""
    v = SK.vec(905, quality=SK.UNDER_TEST) if values is None else values
    return Routes(ns, [sample], np.asarray(v)[None, :], np.asarray(links, dtype=np.int64), [0, len(links)])


def join(parts):
    """Several ``Routes`` over samples of one shape as one: the samples are concatenated, the sample numbers shifted."""
    data = np.concatenate([p.ns.data for p in parts])
    samples, links, ptr, base = [], [], [0], 0
    for p in parts:
        samples += [s + base for s in p.samples]
        base += p.ns.data.shape[0]
        for r in range(len(p.samples)):
            links += [int(l) for l in route_links(p, r)]
            ptr.append(len(links))
    return Routes(SK.status(data, parts[0].ns.freq), samples, np.concatenate([p.values for p in parts]),
                  np.array(links, dtype=np.int64), ptr)


# ------------------------------------------------------------------ hand cases
def blocked_in_parts():
    """Route (0, 2), ``width`` 2.  Slot 10 is blocked on link 2 only; slot 21 is occupied on link 0, so start slot 20 is
    blocked only by its second width-slot (and start 21 by its first); start slot 69 runs off the grid.  conn 8 on (1, 30)
    is off the route: slot 30 stays free."""
    data, freq = PC.grid()
    data[0, :, 2, 10] = SK.vec(8, 64, 70000, 9, freq[10])
    data[0, :, 0, 21] = SK.vec(9, 4, 30000, 1, freq[21])
    data[0, :, 1, 30] = SK.vec(7, 8, 50000, 2, freq[30])
    not_free = {9, 10, 20, 21, Q - 1}
    return single(SK.status(data, freq), [0, 2]), 2, not_free


def empty_sample():
    data, freq = PC.grid()
    return single(SK.status(data, freq), [1, 3])


def full_route():
    """Every slot of link 1 is occupied: the route (1, 2) has no free slot at all.  That is an answer, not an error."""
    data, freq = PC.grid()
    for q in range(Q):
        data[0, :, 1, q] = SK.vec(10 + q // 2, fval=freq[q])
    return single(SK.status(data, freq), [1, 2])


def crowded_link():
    """Link 0 filled with 69 single-channel lightpaths, slot 40 left free; at threshold 10.0 the one free slot of the route
    (0,) sums 69 messages: across the 64-message chunk of the staging and of the row routine."""
    rng = np.random.default_rng(69)
    data, freq = PC.grid()
    for q in range(Q):
        if q != 40:
            data[0, :, 0, q] = PC.random_vec(rng, 100 + q, freq[q])
    return single(SK.status(data, freq), [0]), 10.0, 40


def repeated_frequency():
    """A frequency table in which slots 11 and 12 carry the same value: ``df == 0`` names nobody, so the lightpath of
    slot 12 is no interferer of start slot 11, while that of slot 10 is."""
    data, freq = PC.grid()
    freq = freq.copy()
    freq[12] = freq[11]
    data[0, :, 1, 10] = SK.vec(8, 64, 70000, 9, freq[10])
    data[0, :, 1, 12] = SK.vec(9, 4, 30000, 1, freq[12])
    return single(SK.status(data, freq), [1]), 0.07


# ------------------------------------------------------------------ refused routes: {name: (bit's name, cause, Routes)}
def refusals():
    """One route with one thing wrong, over ``blocked_in_parts``' sample (the default shape, so it joins good routes).
    (A bad slice of a device ``link_ptr`` is the GPU test's own edit of a good batch.)"""
    good, _, _ = blocked_in_parts()
    out = {}

    def with_value(row, v):
        vals = good.values.copy()
        vals[0, FI[row]] = v
        return vals

    def add(name, bit, cause, **kw):
        out[name] = (bit, cause, good._replace(**kw))

    add("a sample number at S", "LP_STATUS_BAD_SAMPLE", "sample number", samples=[1])
    add("a negative sample number", "LP_STATUS_BAD_SAMPLE", "sample number", samples=[-1])
    add("a link index at L", "LP_PLACE_BAD_CELL", "outside the sample", links=np.array([0, L], dtype=np.int64))
    add("a negative link index", "LP_PLACE_BAD_CELL", "outside the sample", links=np.array([-1, 2], dtype=np.int64))
    add("a conn_id of the sample", "LP_PLACE_CONN_TAKEN", "conn_id is a lightpath of the sample", values=with_value("conn_id", 9.6))
    add("a measured osnr", "LP_PLACE_NOT_LUT", "without osnr == snr == ber == -1", values=with_value("osnr", 20.0))
    add("a NaN conn_id", "LP_STATUS_BAD_CONN", "conn_id is not finite", values=with_value("conn_id", np.nan))
    add("a conn_id beyond 2^53", "LP_STATUS_BAD_CONN", "conn_id is not finite", values=with_value("conn_id", 2.0 ** 60))
    add("a sample of 256 lightpaths", "LP_STATUS_TOO_MANY", f"more than {TG.MAX_LIGHTPATHS} lightpaths",
        ns=PC.crowd(256).ns)
    return out
