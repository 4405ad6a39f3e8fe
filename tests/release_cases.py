"""Inputs shared by tests/test_place_release_cpu.py (the host statements with ``release=``, ``materialise_placement(release=)``,
no GPU) and the two GPU files tests/test_gpu_infer_lightpath_place_release.py / tests/test_gpu_infer_topological_place_release.py
(``place(..., release=, release_ptr=)`` against ``from_status`` / ``predict`` over the edited samples, bit for bit).

Seeded builders on the shapes of ``place_cases`` (L = 4, Q = 70, a dozen lightpaths crowded into the slots 52 ... 69) and
``topo_place_cases`` (the 6 x 12 chunk of ``status_topo_cases``).  Each builder asserts its own cover, so that no test
passes vacuously: ``lp_batch`` that at least half of its candidates release an interferer of the unreleased placement (at
threshold 0.12) and at least a third reuse a released cell; ``topo_batch`` that each outcome of ``TOPO_OUTCOMES`` occurs at
least twice.  ``edit`` is the numpy statement of the edited sample, independent of ``to_graph``'s."""
import functools
from collections import namedtuple

import numpy as np

import place_cases as PC
import status_topo_cases as TK
import topo_place_cases as TC
from gnn_qot_estimation_amd import to_graph as TG

FI = PC.FI
P = PC.P
MAX_RELEASE = 32

# place_cases.Batch / topo_place_cases.Batch plus release [R] and release_ptr [K + 1] (numpy / lists, all on the host)
Batch = namedtuple("Batch", "ns samples values cells cell_ptr release release_ptr")


def candidate_cells(b, k):
    return b.cells[:, b.cell_ptr[k]:b.cell_ptr[k + 1]]


def released(b, k):
    return [int(c) for c in b.release[b.release_ptr[k]:b.release_ptr[k + 1]]]


def plain(b):
    """The batch without its release lists: what ``place`` took before."""
    return PC.Batch(b.ns, b.samples, b.values, b.cells, b.cell_ptr)


def pack(ns, candidates):
    """``[(sample number, values row, cells [2, m], released conns), ...]`` as one batch over ``ns``."""
    cells = [np.asarray(c, dtype=np.int64).reshape(2, -1) for _, _, c, _ in candidates]
    ptr = np.cumsum([0] + [c.shape[1] for c in cells]).tolist()
    rptr = np.cumsum([0] + [len(r) for _, _, _, r in candidates]).tolist()
    rel = np.asarray([c for _, _, _, r in candidates for c in r], dtype=np.int64)
    return Batch(ns, [s for s, _, _, _ in candidates], np.stack([v for _, v, _, _ in candidates]),
                 np.concatenate(cells, axis=1), ptr, rel, rptr)


def join(batches):
    """One-sample batches over samples of one shape as one batch: the candidates of batch j go into sample j."""
    data = np.concatenate([b.ns.data[:1] for b in batches])
    cands = [(j, b.values[k], candidate_cells(b, k), released(b, k)) for j, b in enumerate(batches) for k in range(len(b.samples))]
    return pack(TK.status(data, batches[0].ns.freq), cands)


# ------------------------------------------------------------------ the edited sample in numpy
def lightpaths(sample):
    """``[(conn, first channel (l, q)), ...]`` of a sample in first-seen (scan) order."""
    occ = np.argwhere(np.any(sample != 0, axis=0))
    seen, out = set(), []
    for l, q in occ:
        c = int(sample[FI["conn_id"], l, q])
        if c not in seen:
            seen.add(c)
            out.append((c, (int(l), int(q))))
    return out


def edit(sample, values_row, cells, release):
    """The sample with every occupied channel of the conns ``release`` zeroed, then ``values_row`` in ``cells``."""
    occ = np.any(sample != 0, axis=0)
    conn = sample[FI["conn_id"]].astype(np.int64)
    out = sample.copy()
    out[:, occ & np.isin(conn, np.asarray(list(release), dtype=np.int64))] = 0.0
    cells = np.asarray(cells, dtype=np.int64)
    out[:, cells[0], cells[1]] = np.asarray(values_row)[:, None]
    return out


def edited(b, k):
    return edit(b.ns.data[b.samples[k]], b.values[k], candidate_cells(b, k), released(b, k))


# ------------------------------------------------------------------ lightpath model: random batches
def lp_cover(b, thr=0.12):
    """Per candidate ``(releases an interferer of the unreleased placement, reuses a released cell)``."""
    out = []
    for k, s in enumerate(b.samples):
        sample, cells, rel = b.ns.data[s], candidate_cells(b, k), set(released(b, k))
        occ = np.any(sample != 0, axis=0)
        conn = sample[FI["conn_id"]].astype(np.int64)
        free = cells[:, ~occ[cells[0], cells[1]]]                              # what the unreleased placement could take
        near = set(TG.placement_neighbourhood(sample, b.ns.freq, FI, free, thr)) if free.shape[1] else set()
        reuse = bool((occ[cells[0], cells[1]] & np.isin(conn[cells[0], cells[1]], list(rel))).any())
        out.append((bool(rel & near), reuse))
    return out


@functools.lru_cache(maxsize=None)
def lp_batch(seed=0, flagged=False):
    """``place_cases.batch(seed)``'s 8 candidates over 2 dense samples, each with a release list.  Candidate k, by k % 3:
    0 -- releases an interferer and takes one of its channels as one more cell; 1 -- releases an interferer and a
    lightpath that is none; 2 -- an empty slice (k even) or a non-interferer named twice (k odd)."""
    base = PC.batch(seed, flagged=flagged)
    rng = np.random.default_rng(1000 + seed)
    cands = []
    for k, s in enumerate(base.samples):
        sample, cells = base.ns.data[s], PC.candidate_cells(base, k)
        table = lightpaths(sample)
        near = TG.placement_neighbourhood(sample, base.ns.freq, FI, cells, 0.12)
        far = [c for c, _ in table if c not in near]
        if k % 3 == 0:
            target = near[0] if near else far[int(rng.integers(len(far)))]
            rel = [target]
            cells = np.concatenate([cells, np.array(dict(table)[target]).reshape(2, 1)], axis=1)
        elif k % 3 == 1:
            rel = ([near[-1]] if near else []) + [far[int(rng.integers(len(far)))]]
        else:
            rel = [] if k % 2 == 0 else [far[0], far[0]]
        cands.append((s, base.values[k], cells, rel))
    b = pack(base.ns, cands)
    cover = lp_cover(b)
    K = len(b.samples)
    assert 2 * sum(i for i, _ in cover) >= K and 3 * sum(r for _, r in cover) >= K, cover       # conditions on the inputs
    assert any(b.release_ptr[k] == b.release_ptr[k + 1] for k in range(K))                       # an empty slice among them
    return b


# ------------------------------------------------------------------ lightpath model: hand cases
# one candidate in sample 0: thr, the interferers' conn_ids in message order, count (flagged survivors + 1)
Case = namedtuple("Case", "ns values cells release thr interferers count")


def as_batch(case):
    return pack(case.ns, [(0, case.values, case.cells, case.release)])


def _reroute_sample():
    """conn 5 (flagged) on (1, 10) and (2, 10); conn 8 one slot below on link 1, conn 9 one slot above; conn 7 beside (2, 20)."""
    data, freq = PC.grid()
    data[0, :, 1, 10] = data[0, :, 2, 10] = PC.SK.vec(5, 8, 50000, 2, freq[10], PC.SK.UNDER_TEST)
    data[0, :, 1, 9] = PC.SK.vec(8, 64, 70000, 9, freq[9])
    data[0, :, 1, 11] = PC.SK.vec(9, 4, 30000, 1, freq[11])
    data[0, :, 2, 21] = PC.SK.vec(7, 8, 50000, 2, freq[21])
    return data, freq


def _reroute(cells, near, values_conn=5, release=(5,), count=1):
    data, freq = _reroute_sample()
    v = PC.SK.vec(values_conn, 16, 60000, 4, freq[cells[1][0]], PC.SK.UNDER_TEST)
    return Case(PC.SK.status(data, freq), v, np.array(cells), list(release), 0.07, near, count)


def _flagged_released():
    """The sample's flagged lightpath (conn 8, seen first) is released: count drops from 2 to 1 and the candidate is the
    first-seen flagged lightpath of the edited sample."""
    c = PC.HAND["behind a flagged lightpath of the sample"]()
    return Case(c.ns, c.values, c.cells, [8], c.thr, [7], 1)


def _crowd(n, n_release, near):
    """``place_cases.crowd(n)`` (single-channel lightpaths 10 ... 10 + n - 1, a candidate on (3, 46)) releasing the first
    ``n_release`` of them -- none is an interferer."""
    c = PC.crowd(n)
    return Case(c.ns, c.values, c.cells, list(range(10, 10 + n_release)), c.thr, near, 1)


LP_HAND = {
    "reroute with the same conn_id onto its own old cells": functools.partial(_reroute, [[1, 2], [10, 10]], [8, 9]),
    "reroute with the same conn_id onto other cells": functools.partial(_reroute, [[2, 2], [20, 22]], [7]),
    "reroute onto one old cell and a new one, the interferers released too":
        functools.partial(_reroute, [[1, 2], [10, 20]], [7], 5, (5, 8, 9)),
    "a new conn_id on a released lightpath's cells": functools.partial(_reroute, [[1], [9]], [5], 40, (8,), 2),
    "the released lightpath is the flagged one": _flagged_released,
    "a conn named twice": functools.partial(_reroute, [[1], [12]], [], 41, (9, 5, 9), 1),
    "32 releases": functools.partial(_crowd, 255, 32, [10 + 3 * PC.Q + 44]),
    "256 lightpaths, one released": functools.partial(_crowd, 256, 1, [10 + 3 * PC.Q + 44, 10 + 3 * PC.Q + 45]),
}


# ------------------------------------------------------------------ topological model
TOPO_OUTCOMES = ("a survivor takes the released winner's pair", "a sole owner released: two links fewer",
                 "the candidate takes the released winner's pair", "a self loop released")


def topo_table(sample):
    """``{unordered pair (u, v), 1-based: [(conn, first channel), ...] by descending conn}`` of a sample."""
    out = {}
    for c, (l, q) in lightpaths(sample):
        u, v = int(sample[FI["src_id"], l, q]), int(sample[FI["dst_id"], l, q])
        out.setdefault((min(u, v), max(u, v)), []).append((c, (l, q)))
    return {pair: sorted(v, reverse=True) for pair, v in out.items()}


def _tcand(conn, src, dst, freq, cell):
    return TK.vec(conn, src, dst, fval=freq[cell[1]], quality=TK.UNDER_TEST, **TC.CAND)


@functools.lru_cache(maxsize=None)
def topo_batch(chunk_seed=0):
    """Candidates over the 8 samples of ``status_topo_cases.random_chunk``: per sample one of each outcome it offers.
    Returns ``(batch, outcomes)`` with ``outcomes[k]`` the name in ``TOPO_OUTCOMES``.  Candidates of the third outcome
    alternately carry the released winner's own conn_id on its own first channel (a reroute) and a larger one in a free
    cell; the others sit on a node pair nobody uses (20 + k, 70), the second outcome's in the released lightpath's channel."""
    ns = TK.random_chunk(seed=chunk_seed)
    cands, outcomes = [], []
    for s in range(len(ns)):
        sample, table = ns.data[s], topo_table(ns.data[s])
        free = TC.free_cells(sample)
        k = len(cands)
        contested = [(p, v) for p, v in table.items() if len(v) >= 2]
        sole = [(p, v) for p, v in table.items() if len(v) == 1 and p[0] != p[1]]
        loops = [(p, v) for p, v in table.items() if p[0] == p[1]]
        if contested:
            (u, v), owners = contested[0]
            cands.append((s, _tcand(2000 + k, 20 + k, 70, ns.freq, free[:, 0]), free[:, :1], [owners[0][0]]))
            outcomes.append(TOPO_OUTCOMES[0])
        if sole:
            (u, v), owners = sole[-1]
            cell = np.array(owners[0][1]).reshape(2, 1)
            cands.append((s, _tcand(2100 + k, 20 + k, 70, ns.freq, cell[:, 0]), cell, [owners[0][0]] * (1 + s % 2)))
            outcomes.append(TOPO_OUTCOMES[1])
        if table:
            (u, v), owners = (contested[-1] if contested and s % 2 else sole[0] if sole else list(table.items())[0])
            conn, first = owners[0]
            if s % 2:
                cands.append((s, _tcand(conn + 0.5, v, u, ns.freq, first), np.array(first).reshape(2, 1), [conn]))
            else:
                cands.append((s, _tcand(conn + 5000, u, v, ns.freq, free[:, 1]), free[:, 1:2], [conn]))
            outcomes.append(TOPO_OUTCOMES[2])
        if loops:
            (u, _), owners = loops[0]
            others = [o[0][0] for p, o in table.items() if p != (u, u)][:s % 3]      # 0 - 2 more lightpaths go with it
            cands.append((s, _tcand(2300 + k, 20 + k, 70, ns.freq, free[:, 2]), free[:, 2:3],
                          [o[0] for o in owners] + others))
            outcomes.append(TOPO_OUTCOMES[3])
    b = pack(ns, cands)
    assert all(outcomes.count(name) >= 2 for name in TOPO_OUTCOMES), outcomes                   # conditions on the inputs
    for k, name in enumerate(outcomes):                                         # ... and each is what its name says
        sample, rel = ns.data[b.samples[k]], released(b, k)
        before_ei, before_conn = TG.topological_links(sample, FI)
        ei, conn = TG.topological_links(edited(b, k), FI)
        mine = int(b.values[k][FI["conn_id"]])
        assert not set(rel) & (set(conn.tolist()) - {mine}), (k, name)
        if name == TOPO_OUTCOMES[0]:
            lost = [i for i in range(before_conn.shape[0]) if before_conn[i] == rel[0]]
            assert lost and all(((ei[0] == before_ei[0, i]) & (ei[1] == before_ei[1, i])).any() for i in lost), (k, name)
            assert ei.shape[1] == before_ei.shape[1] + 2
        elif name == TOPO_OUTCOMES[1]:
            assert ei.shape[1] == before_ei.shape[1] - 2 + 2, (k, name)
            assert not any(((ei[0] == before_ei[0, i]) & (ei[1] == before_ei[1, i])).any()
                           for i in range(before_conn.shape[0]) if before_conn[i] == rel[0]), (k, name)
        elif name == TOPO_OUTCOMES[2]:
            assert ei.shape[1] == before_ei.shape[1] and np.array_equal(ei, before_ei), (k, name)
            assert sorted(conn[before_conn == rel[0]].tolist()) == [mine] * int((before_conn == rel[0]).sum()), (k, name)
        else:
            u = int(b.ns.data[b.samples[k]][FI["src_id"]][tuple(dict(lightpaths(sample))[rel[0]])]) - 1
            assert ((before_ei[0] == u) & (before_ei[1] == u)).any() and not ((ei[0] == u) & (ei[1] == u)).any(), (k, name)
    return b, outcomes


# one candidate in sample 0: the directed links of the edited sample's graph
TopoCase = namedtuple("TopoCase", "ns values cells release links")


def topo_as_batch(case):
    return pack(case.ns, [(0, case.values, case.cells, case.release)])


def _on_hand(conn, src, dst, cells, release, links):
    """``topo_place_cases._hand_sample``: conn 7 (1 -> 4) on (0, 1) and (2, 1); conn 9 (5 -> 2) on (1, 0); conn 3 (2 -> 5) on
    (3, 4); conn 0, the self loop of node 6, on (3, 5): 5 directed links."""
    ns = TC._hand_sample()
    return TopoCase(ns, TK.vec(conn, src, dst, fval=ns.freq[cells[1][0]], quality=TK.UNDER_TEST, **TC.CAND), np.array(cells),
                    list(release), links)


def _bad_endpoint_released():
    """A lightpath with src_id 0 -- ``place`` refuses the sample -- is released: nothing of it is looked at."""
    ns = TC._hand_sample()
    data = ns.data.copy()
    data[0, :, 4, 7] = TK.vec(21, 0, 3, fval=ns.freq[7])
    ns = TK.status(data, ns.freq)
    return TopoCase(ns, TK.vec(30, 10, 11, fval=ns.freq[7], quality=TK.UNDER_TEST, **TC.CAND), np.array([[4], [7]]), [21], 7)


def _cap(n_release):
    """``status_topo_cases._cap``: 256 lightpaths (conn 1000 + 7 k on channel k) on 256 pairs, 512 links; the first
    ``n_release`` released, the candidate on the first one's pair and channel."""
    ns, _ = TK._cap()
    first = ns.data[0][:, 0, 0]
    v = TK.vec(5, first[FI["dst_id"]], first[FI["src_id"]], fval=ns.freq[0], quality=TK.UNDER_TEST, **TC.CAND)
    return TopoCase(ns, v, np.array([[0], [0]]), [1000 + 7 * k for k in range(n_release)], 512 - 2 * n_release + 2)


TOPO_HAND = {
    "the winner released, the loser takes over": functools.partial(_on_hand, 40, 10, 20, [[5], [11]], [9], 7),
    "both lightpaths of a pair released: the pair disappears": functools.partial(_on_hand, 40, 10, 20, [[5], [11]], [9, 3], 5),
    "reroute with the same conn_id onto its own old cell": functools.partial(_on_hand, 9, 5, 2, [[1], [0]], [9], 5),
    "reroute with the same conn_id onto another cell, other end nodes": functools.partial(_on_hand, 7, 1, 5, [[5], [11]], [7], 5),
    "reroute onto one old cell of two": functools.partial(_on_hand, 7, 1, 4, [[2, 5], [1, 3]], [7], 5),
    "a smaller conn_id takes the pair once both owners are gone": functools.partial(_on_hand, 1, 2, 5, [[3], [4]], [3, 9], 5),
    "still loses the pair to the survivor": functools.partial(_on_hand, 1, 2, 5, [[1], [0]], [9], 5),
    "the self loop released and taken": functools.partial(_on_hand, -4, 6, 6, [[3], [5]], [0], 5),
    "everything released": functools.partial(_on_hand, 7, 30, 31, [[0], [1]], [7, 9, 3, 0], 2),
    "a conn named twice": functools.partial(_on_hand, 40, 10, 20, [[5], [11]], [3, 9, 3], 5),
    "a released lightpath with a bad end node": _bad_endpoint_released,
    "256 lightpaths, one released, the candidate in its table slot": functools.partial(_cap, 1),
    "256 lightpaths, 32 released": functools.partial(_cap, 32),
}


def take(b, ks):
    """The candidates ``ks`` of a batch, in that order, as a batch over the same samples."""
    return pack(b.ns, [(b.samples[k], b.values[k], candidate_cells(b, k), released(b, k)) for k in ks])
