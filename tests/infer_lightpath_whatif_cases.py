"""Inputs shared by tests/test_infer_lightpath_whatif_cpu.py (the definition ``materialise_lightpath_what_if``, no GPU)
and tests/test_gpu_infer_lightpath_whatif.py (``LightpathPredictor.what_if`` against it, bit for bit): the mixed batch of
``lightpath_grad_cases.py`` (16 graphs, 405 nodes, 471 edges) and a hand-written list of candidates, all in one call with
``node`` given and K > L.  ``EXPECTED`` writes out, for a handful of them, the local edge list the candidate's graph must
have.

The layout of the base batch does not depend on F or on the LUT column (``PTR`` / ``EPTR`` below; the CPU file asserts
them): graph 3 is the one-node graph, 4 the LUT of in-degree 0, 5 the input self loop, 6 the triple edge, 7 - 9 the stars
of in-degree 63 / 64 / 65, 10 the 150-star with 40 interleaved back edges, 11 the two-LUT chain, 12 the LUT-less chain,
13 a chain whose last node is a LUT, 14 the adjacent LUTs, 15 the unrolled triple edge (the batch's last node, 404, is a
plain node of it)."""
import collections
import functools

import torch

import gnn_qot_estimation_amd as q
import lightpath_grad_cases as G
from lightpath_grad_cases import engine_model, lut_rows, oracle_model          # noqa: F401  (re-exported for the tests)

PTR = [0, 2, 17, 25, 26, 30, 33, 36, 100, 165, 231, 382, 387, 391, 394, 400, 405]
EPTR = [0, 2, 30, 44, 44, 47, 51, 56, 119, 183, 248, 438, 446, 452, 456, 466, 471]
LUT_ROWS = [0, 2, 17, 25, 26, 30, 33, 36, 100, 165, 231, 383, 385, 393, 396, 397, 400]
ONE_NODE, DEG0, SELF_LOOP, TRIPLE, STAR63, STAR64, STAR65, STAR150, TWO_LUT, NO_LUT, ADJACENT, LAST = \
    3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15
SHAPES = [(4, 2, 1, 0), (20, 5, 3, 4), (32, 5, 3, 1), (128, 16, 3, 15)]       # (C, F, O, LUT column): columns 0, 1, F - 1

# name, graph, the node (local), a fresh feature row?, drop offsets into the graph's slice, added sources (local)
Cand = collections.namedtuple("Cand", "name graph node fresh drop add")


def _n(g, local):
    return PTR[g] + local


def _e(g, offset):
    return EPTR[g] + offset


def _candidates():
    c = [Cand("no edit", g, n - PTR[g], False, [], [])
         for n in LUT_ROWS for g in [max(k for k in range(16) if PTR[k] <= n)]]
    hub = 0
    c += [
        # ---- features only
        Cand("features: chain", 0, 0, True, [], []),
        Cand("features: 150-star", STAR150, hub, True, [], []),
        Cand("features: first of two LUTs", TWO_LUT, 1, True, [], []),
        # ---- additions
        Cand("add: one source", DEG0, 0, False, [], [2]),
        Cand("add: the node itself", TRIPLE, 0, False, [], [0]),
        Cand("add: a sender again", TRIPLE, 0, False, [], [1]),
        Cand("add: 63 on the 150-star", STAR150, hub, False, [], [1 + (7 * j) % 150 for j in range(63)]),
        Cand("add: 64 on the 150-star", STAR150, hub, False, [], [1 + (11 * j) % 150 for j in range(64)]),
        Cand("add: 65 on the 150-star", STAR150, hub, False, [], [1 + (13 * j) % 150 for j in range(65)]),
        Cand("add: behind a slice of 63", STAR63, hub, False, [], [5, 63]),
        Cand("add: behind a slice of 64", STAR64, hub, False, [], [64]),
        Cand("add: behind a slice of 65", STAR65, hub, False, [], [1, 0, 2]),
        # ---- removals
        Cand("drop: a message", TRIPLE, 0, False, [1], []),
        Cand("drop: no message", TRIPLE, 0, False, [4], []),
        Cand("drop: a back edge", STAR150, hub, False, [1], []),
        Cand("drop: a repeat", SELF_LOOP, 0, False, [2, 2], []),
        Cand("drop: offset 0 of 64", STAR64, hub, False, [0], []),
        Cand("drop: offset 63 of 64", STAR64, hub, False, [63], []),
        Cand("drop: 32 on the 150-star", STAR150, hub, False, [(37 * j) % 190 for j in range(32)], []),
        Cand("drop: every message", TRIPLE, 0, False, [3, 0, 2, 1], []),
        # ---- combined, on each LUT node of the two-LUT and the adjacent-LUT graphs
        Cand("combined: two LUTs, first", TWO_LUT, 1, True, [0, 2], [4, 3]),
        Cand("combined: two LUTs, second", TWO_LUT, 3, True, [7], [0, 3, 2]),
        Cand("combined: adjacent, first", ADJACENT, 2, True, [7, 1], [5]),
        Cand("combined: adjacent, second", ADJACENT, 3, True, [2], [0, 0]),
        # ---- the one-node graph; nodes that only the candidate makes a LUT; the batch's last node
        Cand("one node: features", ONE_NODE, 0, True, [], []),
        Cand("a plain node of the LUT-less graph", NO_LUT, 1, True, [1], [3]),
        Cand("the batch's last node", LAST, 4, True, [3], [1]),
    ]
    return c


CANDIDATES = _candidates()

# the local (source, target) lists of some candidates' graphs, written out by hand: the base graph's edges less the
# dropped ones in their order, then (source, node) per addition
EXPECTED = {
    "add: one source": [(0, 1), (1, 2), (2, 3), (2, 0)],
    "add: the node itself": [(1, 0), (1, 0), (2, 0), (1, 0), (0, 1), (0, 0)],
    "add: a sender again": [(1, 0), (1, 0), (2, 0), (1, 0), (0, 1), (1, 0)],
    "drop: a message": [(1, 0), (2, 0), (1, 0), (0, 1)],
    "drop: no message": [(1, 0), (1, 0), (2, 0), (1, 0)],
    "drop: a repeat": [(1, 0), (0, 0), (0, 1)],
    "drop: every message": [(0, 1)],
    "combined: two LUTs, first": [(1, 2), (3, 4), (1, 0), (2, 1), (3, 2), (4, 3), (4, 1), (3, 1)],
    "combined: two LUTs, second": [(0, 1), (1, 2), (2, 3), (3, 4), (1, 0), (2, 1), (3, 2), (0, 3), (3, 3), (2, 3)],
    "combined: adjacent, first": [(0, 1), (2, 3), (3, 4), (4, 5), (1, 0), (2, 1), (4, 3), (5, 4), (5, 2)],
    "combined: adjacent, second": [(0, 1), (1, 2), (3, 4), (4, 5), (1, 0), (2, 1), (3, 2), (4, 3), (5, 4), (0, 3), (0, 3)],
    "one node: features": [],
    "the batch's last node": [(1, 0), (3, 0), (2, 0), (0, 1), (1, 4)],
}

# a call's arguments: the base batch (host), the candidates, and the six arrays (host tensors; the pointers as lists)
WhatIf = collections.namedtuple("WhatIf", "data cands node x_lut add_src add_ptr drop drop_ptr")


def fresh_rows(K, F, lut, seed=5):
    """``[K, F]`` seeded feature rows in [0, 1) with 1.0 in the LUT column."""
    x = torch.rand(K, F, generator=torch.Generator().manual_seed(seed))
    x[:, lut] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def build(F, lut):
    """The base batch and the whole candidate list as one call's arguments; shared, never modified.  ``x_lut[k]`` of a
    candidate without a fresh row is its node's own row (which is no edit)."""
    data = q.Batch.from_data_list(G.mixed(F, lut))
    cands = CANDIDATES
    node = torch.tensor([_n(c.graph, c.node) for c in cands])
    x_lut = data.x[node].clone()
    fresh = fresh_rows(len(cands), F, lut)
    for k, c in enumerate(cands):
        if c.fresh:
            x_lut[k] = fresh[k]
    add_ptr, drop_ptr, add, drop = [0], [0], [], []
    for c in cands:
        add += [_n(c.graph, s) for s in c.add]
        drop += [_e(c.graph, o) for o in c.drop]
        add_ptr.append(len(add))
        drop_ptr.append(len(drop))
    return WhatIf(data, cands, node, x_lut, torch.tensor(add, dtype=torch.long), add_ptr,
                  torch.tensor(drop, dtype=torch.long), drop_ptr)


def pick(w, ks, x_lut=True):
    """The candidates ``ks`` of ``w``, in that order, as a call of their own (``x_lut=False``: without feature rows)."""
    add_ptr, drop_ptr, add, drop = [0], [0], [], []
    for k in ks:
        add.append(w.add_src[w.add_ptr[k]:w.add_ptr[k + 1]])
        drop.append(w.drop[w.drop_ptr[k]:w.drop_ptr[k + 1]])
        add_ptr.append(add_ptr[-1] + add[-1].numel())
        drop_ptr.append(drop_ptr[-1] + drop[-1].numel())
    empty = [torch.zeros(0, dtype=torch.long)]
    return WhatIf(w.data, [w.cands[k] for k in ks], w.node[ks], w.x_lut[ks] if x_lut else None, torch.cat(add + empty),
                  add_ptr, torch.cat(drop + empty), drop_ptr)


def args(w, device=None, data=None):
    """``(data, kwargs)`` of ``predict.what_if`` / (with ``lut_col`` in between) ``materialise_lightpath_what_if``: the
    tensors on ``device``, the pointer arrays as they are (lists)."""
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    data = w.data if data is None else data
    return (data if device is None else data.to(device)), dict(
        x_lut=None if w.x_lut is None else to(w.x_lut), add_src=to(w.add_src), add_ptr=w.add_ptr, drop=to(w.drop),
        drop_ptr=w.drop_ptr, node=to(w.node))


def index(name):
    return [c.name for c in CANDIDATES].index(name)


def local_edges(batch, k):
    """The ``(source, target)`` pairs of graph ``k`` of ``batch`` in its own numbering, in order."""
    e0, e1, n0 = int(batch.edge_ptr[k]), int(batch.edge_ptr[k + 1]), int(batch.ptr[k])
    return [tuple(p) for p in (batch.edge_index[:, e0:e1] - n0).t().tolist()]


def oracle_rows(ref, batch, dtype=torch.float64):
    """``(out [L, O], lut_batch)`` of the oracle's eval forward of ``batch`` in ``dtype``."""
    import copy
    model = copy.deepcopy(ref).to(dtype).eval()
    b = copy.copy(batch)
    b.x = batch.x.detach().to(dtype)
    with torch.no_grad():
        out, lb = model(b)
    return out, lb
