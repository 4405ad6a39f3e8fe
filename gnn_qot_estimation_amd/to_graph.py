"""Graph construction: one network-status sample -> the reference's two graph representations.

Counterpart of ``to_graph.py`` and the loop of ``store_graphs.py:64-79``.  The reference reads
an xarray ``.nc`` file -- and re-opens it for every sample (``to_graph.py:124-129, 216-219``); xarray and the ``.nc``
data are not available here, and the rules only need plain arrays, so a sample source is a ``NetworkStatus``: the same
variables under the same names (``data [sample, lp_feat, link, freq]``, ``target [sample, metric]``, coordinate arrays
``lp_feat``, ``metric``, ``link``, ``freq``), held in memory or in an ``.npz`` file; an ``.nc`` path is accepted when
xarray is importable.

Rules restated (graph-for-graph, including node order, attribute values and adjacency insertion order, which is what
fixes the column order of ``edge_index`` downstream):

``create_topological_graph`` (``to_graph.py:62-182``): 75 featureless nodes ``1..75``; an occupied (link, freq)
channel is one whose feature vector is not all zero; lightpaths are the unique ``conn_id`` values (first occupied
channel in (link, freq) scan order supplies the features); one undirected edge ``src_id -- dst_id`` per lightpath, added
in ascending ``conn_id`` order, carrying the requested features -- parallel lightpaths between the same node pair
collapse to one edge whose attributes are the LAST one's (``nx.Graph.add_edge`` updates), its position the first one's.

``create_lightpath_graph`` (``to_graph.py:187-312``): one node ``"lightpath_<conn_id>"`` per lightpath in first-seen
order with the requested features + ``is_lut`` (1 iff osnr == snr == ber == -1 on the first-seen channel,
``:247-251``); two lightpaths are linked when, on some shared link, they occupy frequencies with
``0 < |f1 - f2| < freq_threshold`` (``:279-310``; a lightpath with two such slots on one link gets a self loop, as in
the reference).  The pair test is one vectorised comparison per link.

Both return ``networkx.Graph`` objects that pickle into the ``.gpickle`` files ``dataset.TopologicalDataset`` /
``LightpathDataset`` (and the reference's own dataset classes) read; ``store_graphs`` writes them, ``build_shard``
skips the files and packs ``Data`` objects straight into a ``PackedGraphs`` shard.

Device form: ``NetworkStatus.to_device`` keeps a chunk of samples in HBM (``DeviceStatus``);
``build_shard(..., device=...)`` / ``device_batch`` run ``csrc/status_graph.hip`` over it -- one workgroup per sample, no
``networkx`` -- and return a resident ``PackedGraphs`` / ``Batch``.  Its directed links are in the canonical order
(source, target) inside each graph; ``canonical_link_order`` brings a host-built shard into the same order.
``infer.LightpathPredictor.from_status`` predicts from a ``DeviceStatus`` without building the
graphs; ``lut_neighbourhood`` states on the host which lightpaths of a sample its row takes.
``infer.TopologicalPredictor.from_status`` does the same for the topological model;
``topological_links`` states on the host the directed links of a sample's graph, in canonical order, and the lightpath
that gives each its features.
"""
from __future__ import annotations

import os
import pickle
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

DEFAULT_FEATURES = ["mod_order", "path_len", "num_spans", "freq"]        # store_graphs.py:51-56
NUM_TOPOLOGY_NODES = 75                                                   # to_graph.py:134


@dataclass
class NetworkStatus:
    """The variables ``to_graph.py`` reads from the ``.nc`` dataset, as arrays (``to_graph.py:23-38,124-129``)."""
    data: np.ndarray        # [sample, lp_feat, link, freq]
    target: np.ndarray      # [sample, metric]
    lp_feat: Sequence[str]  # names along axis 1 of data
    metric: Sequence[str]   # names along axis 1 of target
    link: np.ndarray        # [link] identifiers
    freq: np.ndarray        # [freq] centre frequencies (THz)

    def __post_init__(self):
        self.lp_feat = [str(v) for v in self.lp_feat]
        self.metric = [str(v) for v in self.metric]
        self.feature_indexes = {f: i for i, f in enumerate(self.lp_feat)}       # to_graph.py:27
        if self.data.ndim != 4 or self.data.shape[1] != len(self.lp_feat):
            raise ValueError("data must be [sample, lp_feat, link, freq]")
        if self.data.shape[2] != len(self.link) or self.data.shape[3] != len(self.freq):
            raise ValueError("link / freq coordinates do not match data")

    def __len__(self) -> int:
        return self.data.shape[0]

    def save(self, path: str):
        np.savez_compressed(path, data=self.data, target=self.target, lp_feat=np.array(self.lp_feat),
                            metric=np.array(self.metric), link=np.asarray(self.link), freq=np.asarray(self.freq))

    @classmethod
    def load(cls, path: str) -> "NetworkStatus":
        if path.endswith(".nc"):
            try:
                import xarray as xr
            except ImportError as e:
                raise ImportError("reading .nc needs xarray; convert once to .npz with NetworkStatus.save") from e
            ds = xr.open_dataset(path)
            try:
                return cls(ds["data"].values, ds["target"].values, ds["lp_feat"].values, ds["metric"].values,
                           ds["link"].values, ds["freq"].values)
            finally:
                ds.close()
        z = np.load(path, allow_pickle=False)
        return cls(z["data"], z["target"], z["lp_feat"], z["metric"], z["link"], z["freq"])

    def to_device(self, device="cuda", samples: Optional[Sequence[int]] = None) -> "DeviceStatus":
        """The chosen samples (default: all) as fp64 tensors on ``device``, with the coordinate names: the input of the
        device builder.  The reference's whole dataset does not fit in HBM as a dense array, so a chunk is the unit."""
        import torch
        pick = slice(None) if samples is None else np.asarray(list(samples), dtype=np.int64)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        return DeviceStatus(up(np.asarray(self.data)[pick]), up(np.asarray(self.target)[pick]), up(self.freq),
                            self.lp_feat, self.metric, np.asarray(self.link))


class DeviceStatus:
    """A chunk of network-status samples resident on the GPU: ``data [sample, lp_feat, link, freq]``, ``target [sample,
    metric]`` and ``freq [freq]`` as contiguous fp64 tensors, plus the coordinate names (``NetworkStatus.to_device``)."""

    def __init__(self, data, target, freq, lp_feat: Sequence[str], metric: Sequence[str], link=None):
        import torch
        for name, t, nd in (("data", data, 4), ("target", target, 2), ("freq", freq, 1)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != nd:
                raise ValueError(f"{name} must be a {nd}-d float64 tensor")
        self.data, self.target, self.freq = data.contiguous(), target.contiguous(), freq.contiguous()
        self.lp_feat = [str(v) for v in lp_feat]
        self.metric = [str(v) for v in metric]
        self.link = link
        self.feature_indexes = {f: i for i, f in enumerate(self.lp_feat)}
        if data.shape[1] != len(self.lp_feat) or data.shape[3] != freq.shape[0]:
            raise ValueError("lp_feat / freq coordinates do not match data")
        if target.shape[0] != data.shape[0] or target.shape[1] != len(self.metric):
            raise ValueError("target must be [sample, metric]")
        self._tables: Dict[tuple, tuple] = {}

    def __len__(self) -> int:
        return self.data.shape[0]

    @property
    def device(self):
        return self.data.device


Source = Union[NetworkStatus, str]
_loaded: Dict[str, NetworkStatus] = {}


def _source(dataset: Source) -> NetworkStatus:
    if isinstance(dataset, NetworkStatus):
        return dataset
    if dataset not in _loaded:            # the reference caches only metadata and re-opens per sample
        _loaded[dataset] = NetworkStatus.load(dataset)
    return _loaded[dataset]


def _occupied(sample: np.ndarray):
    """(link index, freq index) of occupied channels in scan order and their feature vectors [lp_feat, n]
    (``to_graph.py:141-146,229-232``)."""
    occ = np.any(sample != 0, axis=0)
    idx = np.argwhere(occ)
    return idx[:, 0], idx[:, 1], sample[:, occ]


def create_topological_graph(sample_index: int, features_to_consider: Sequence[str], dataset: Source):
    import networkx as nx
    ds = _source(dataset)
    fi = ds.feature_indexes
    sample = np.asarray(ds.data[sample_index])
    G = nx.Graph()
    G.add_nodes_from(range(1, NUM_TOPOLOGY_NODES + 1))
    _, _, vec = _occupied(sample)
    conn = vec[fi["conn_id"], :].astype(int)
    src = vec[fi["src_id"], :].astype(int)
    dst = vec[fi["dst_id"], :].astype(int)
    _, first = np.unique(conn, return_index=True)            # ascending conn_id, first occupied channel of each
    rows = [fi[f] for f in features_to_consider]
    feats = vec[rows][:, first]                               # [feature, lightpath]
    for n, i in enumerate(first):
        G.add_edge(src[i], dst[i], **{f: feats[r, n] for r, f in enumerate(features_to_consider)})
    G.graph["labels"] = dict(zip(ds.metric, np.asarray(ds.target[sample_index])))
    return G


def lightpath_pairs(link_idx: np.ndarray, freq_val: np.ndarray, conn: np.ndarray, freq_threshold: float = 0.05):
    """All (conn_a, conn_b) with a shared link and ``0 < |f_a - f_b| < freq_threshold`` on it, as the reference finds
    them (``to_graph.py:279-310``) but with one vectorised comparison per link; returned in the reference's insertion
    order (links ascending; inside a link the (i, j) order of its frequency table).  The per-link tables are built from
    Python sets in the reference -- lightpaths per link and frequencies per (lightpath, link) -- and their iteration
    order decides the table order, so the same sets are built here."""
    out: List[tuple] = []
    order = np.argsort(link_idx, kind="stable")
    bounds = np.flatnonzero(np.diff(link_idx[order])) + 1
    for seg in np.split(order, bounds):
        if seg.size < 2:
            continue
        lps: set = set()
        per_lp: Dict[int, set] = {}
        for t in seg:                                   # scan order inside the link
            c = int(conn[t])
            lps.add(c)
            per_lp.setdefault(c, set()).add(freq_val[t])
        if len(lps) < 2:
            continue
        ids, fr = [], []
        for c in list(lps):
            for f in per_lp[c]:
                fr.append(f)
                ids.append(c)
        fr, ids = np.asarray(fr), np.asarray(ids)
        diff = np.abs(fr[:, None] - fr[None, :])
        ii, jj = np.where((diff < freq_threshold) & (diff > 0))
        seen = set()
        for a, b in zip(ids[ii].tolist(), ids[jj].tolist()):
            key = (a, b) if a <= b else (b, a)
            if key not in seen:
                seen.add(key)
                out.append((a, b))
    return out


def create_lightpath_graph(sample_index: int, features_to_consider: Sequence[str], dataset: Source,
                           freq_threshold: float = 0.05):
    import networkx as nx
    ds = _source(dataset)
    fi = ds.feature_indexes
    sample = np.asarray(ds.data[sample_index])
    G = nx.Graph()
    G.graph["labels"] = dict(zip(ds.metric, np.asarray(ds.target[sample_index])))
    link_idx, freq_idx, vec = _occupied(sample)
    conn = vec[fi["conn_id"], :].astype(np.int64)        # int(...) truncation, as the per-channel loop does
    uniq, first = np.unique(conn, return_index=True)
    seen_order = np.sort(first)                           # lightpaths in first-seen order (dict insertion order)
    is_lut = ((vec[fi["osnr"], :] == -1) & (vec[fi["snr"], :] == -1) & (vec[fi["ber"], :] == -1)).astype(int)
    rows = [fi[f] for f in features_to_consider]
    for i in seen_order:
        attrs = {f: vec[r, i] for r, f in zip(rows, features_to_consider)}
        attrs["is_lut"] = int(is_lut[i])
        G.add_node(f"lightpath_{int(conn[i])}", **attrs)
    freq_val = np.asarray(ds.freq)[freq_idx]
    for a, b in lightpath_pairs(link_idx, freq_val, conn, freq_threshold):
        G.add_edge(f"lightpath_{a}", f"lightpath_{b}")
    return G


def lut_neighbourhood(sample: np.ndarray, freq: np.ndarray, feature_indexes: Dict[str, int], freq_threshold: float = 0.05):
    """What ``LightpathPredictor.from_status`` takes of one sample ``[lp_feat, link, freq]``, stated on the host:
    ``(count, conn, interferers)``.  ``count``: the lightpaths whose first-seen channel carries ``osnr == snr == ber ==
    -1``; ``conn``: the ``conn_id`` of the first-seen one of them, ``None`` when there is none; ``interferers``: the
    ``conn_id`` values, in first-seen order, of the OTHER lightpaths that occupy, on some link the lightpath is routed
    over, a slot with ``0 < |f1 - f2| < freq_threshold`` to one of its own (fp64) -- each once, however many links and
    slots the pair shares; a pair of the lightpath's own slots names nobody.  These are the neighbours of the LUT node in
    ``create_lightpath_graph``'s graph without the node itself, and the messages of its row in their order."""
    fi = feature_indexes
    sample, freq = np.asarray(sample, dtype=np.float64), np.asarray(freq, dtype=np.float64)
    link_idx, freq_idx, vec = _occupied(sample)
    conn = vec[fi["conn_id"], :].astype(np.int64)
    _, first = np.unique(conn, return_index=True)
    seen_order = np.sort(first)
    flagged = [int(i) for i in seen_order
               if vec[fi["osnr"], i] == -1 and vec[fi["snr"], i] == -1 and vec[fi["ber"], i] == -1]
    if not flagged:
        return 0, None, []
    a = int(conn[flagged[0]])
    hit = set()
    for t in np.flatnonzero(conn == a):                       # every channel of the lightpath
        on_link = np.flatnonzero((link_idx == link_idx[t]) & (conn != a))
        diff = np.abs(freq[freq_idx[t]] - freq[freq_idx[on_link]])
        hit.update(conn[on_link[(diff > 0) & (diff < freq_threshold)]].tolist())
    return len(flagged), a, [int(conn[i]) for i in seen_order if int(conn[i]) in hit]


def _cells_of(cells, L: int, Q: int):
    cells = np.asarray(cells, dtype=np.int64)
    if cells.ndim != 2 or cells.shape[0] != 2 or cells.shape[1] < 1:
        raise ValueError(f"cells must be [2, m] (link index, frequency index) with m >= 1, got {tuple(cells.shape)}")
    if ((cells[0] < 0) | (cells[0] >= L) | (cells[1] < 0) | (cells[1] >= Q)).any():
        raise ValueError(f"a cell lies outside the {L} links x {Q} frequency slots of the sample")
    return cells


def _released(sample: np.ndarray, release, feature_indexes: Dict[str, int]):
    """``(copy of sample with every occupied channel of the lightpaths ``release`` zeroed, the released conns)``: what a
    candidate of ``place(..., release=)`` is placed into.  A channel is occupied when any of its values != 0, its conn is
    ``trunc(conn_id)``; a conn named twice is released once; ``ValueError`` for a conn the sample does not hold."""
    release = sorted({int(c) for c in np.asarray(release, dtype=np.int64).reshape(-1).tolist()})
    occupied = np.any(sample != 0, axis=0)
    conn = np.where(occupied, sample[feature_indexes["conn_id"]], 0.0).astype(np.int64)
    unknown = [c for c in release if not (occupied & (conn == c)).any()]
    if unknown:
        raise ValueError(f"released conn_id {unknown[0]} is no lightpath of the sample")
    out = sample.copy()
    out[:, occupied & np.isin(conn, release)] = 0.0
    return out, release


def place_lightpath(sample: np.ndarray, values_row: np.ndarray, cells, feature_indexes: Dict[str, int], release=()):
    """One candidate of ``LightpathPredictor.place``, stated on the host: ``(edited, node)``.  ``edited`` is a copy of
    ``sample [lp_feat, link, freq]`` with the raw ``lp_feat`` vector ``values_row`` written into every channel of ``cells
    [2, m]`` (link index, frequency index; a repeated cell is written once more); ``node`` is the candidate's number in
    the first-seen order of ``edited``: its node in ``create_lightpath_graph``'s graph.  ``ValueError`` for a cell outside
    the sample, a cell whose channel is occupied (any of its values != 0) and a ``conn_id`` that truncates to one the
    sample holds already.  The input is not modified.
    ``release``: conn ids of lightpaths that are released first (``place(..., release=)``): their channels are zeroed
    before anything else is looked at, so they are free for the cells and their conn ids for the candidate; a conn the
    sample does not hold is a ``ValueError``.  The survivors keep their channels, hence their relative first-seen order."""
    fi = feature_indexes
    sample = np.asarray(sample, dtype=np.float64)
    values_row = np.asarray(values_row, dtype=np.float64)
    if sample.ndim != 3 or values_row.shape != (sample.shape[0],):
        raise ValueError("sample must be [lp_feat, link, freq] and values_row [lp_feat]")
    cells = _cells_of(cells, sample.shape[1], sample.shape[2])
    sample, _ = _released(sample, release, fi)
    occupied = np.any(sample != 0, axis=0)
    if occupied[cells[0], cells[1]].any():
        l, q = cells[:, np.flatnonzero(occupied[cells[0], cells[1]])[0]]
        raise ValueError(f"the channel of cell (link {int(l)}, slot {int(q)}) is occupied in the sample")
    conn = int(values_row[fi["conn_id"]])
    if conn in set(sample[fi["conn_id"]][occupied].astype(np.int64).tolist()):
        raise ValueError(f"conn_id {conn} is a lightpath of the sample already")
    edited = sample.copy()
    edited[:, cells[0], cells[1]] = values_row[:, None]
    _, _, vec = _occupied(edited)
    seen = vec[fi["conn_id"], :].astype(np.int64)
    _, first = np.unique(seen, return_index=True)
    order = [int(seen[i]) for i in np.sort(first)]
    return edited, order.index(conn)


def placement_neighbourhood(sample: np.ndarray, freq: np.ndarray, feature_indexes: Dict[str, int], cells,
                            freq_threshold: float = 0.05, release=()):
    """Who sends a message into the row of a candidate of ``LightpathPredictor.place``, stated on the UNEDITED sample
    ``[lp_feat, link, freq]`` plus the candidate's ``cells [2, m]``: the ``conn_id`` values, in the sample's first-seen
    order, of the lightpaths that occupy, on the link of some cell, a slot with ``0 < |f1 - f2| < freq_threshold`` to that
    cell's (fp64) -- each once, however many links and slots are shared.  The candidate's own cells are free in the
    sample, so a pair of them names nobody.  For a candidate that is the first-seen flagged lightpath of its edited sample
    this is ``lut_neighbourhood(place_lightpath(...)[0], ...)[2]``: the candidate fills free channels only, so every other
    lightpath keeps its place in first-seen order.
    ``release``: conn ids of lightpaths released first (``place(..., release=)``; a conn the sample does not hold is a
    ``ValueError``).  Still stated on the UNEDITED sample: the walk and the first-seen order are the unedited sample's, and
    the released lightpaths are struck from the result.  That is the edited sample's neighbourhood in its message order,
    because releasing zeroes whole channels and the candidate fills channels that are free afterwards: a survivor keeps
    every channel it had, so who is near a cell, each survivor's first channel and the survivors' relative first-seen
    order are what they were."""
    fi = feature_indexes
    sample, freq = np.asarray(sample, dtype=np.float64), np.asarray(freq, dtype=np.float64)
    cells = _cells_of(cells, sample.shape[1], sample.shape[2])
    _, gone = _released(sample, release, fi)
    link_idx, freq_idx, vec = _occupied(sample)
    conn = vec[fi["conn_id"], :].astype(np.int64)
    _, first = np.unique(conn, return_index=True)
    hit = set()
    for l, q in cells.T:
        on_link = np.flatnonzero(link_idx == l)
        diff = np.abs(freq[q] - freq[freq_idx[on_link]])
        hit.update(conn[on_link[(diff > 0) & (diff < freq_threshold)]].tolist())
    hit -= set(gone)
    return [int(conn[i]) for i in np.sort(first) if int(conn[i]) in hit]


def slot_sweep(sample: np.ndarray, freq: np.ndarray, feature_indexes: Dict[str, int], links, freq_threshold: float = 0.05,
               width: int = 1):
    """One route of ``LightpathPredictor.place_slots``, stated on the host: ``(free [Q] bool, neighbours)``.  ``links``:
    the link indices of the route (non-empty; a duplicate link changes nothing).  The candidate that starts at slot ``q``
    takes the cells ``links x {q ... q + width - 1}``; ``free[q]``: every one of those channels of ``sample [lp_feat, link,
    freq]`` has all its values equal to 0, and ``q + width <= Q`` -- the start slots at which ``place_lightpath`` accepts
    the cells.  ``neighbours[q]``: ``placement_neighbourhood`` of those cells for a free ``q`` -- who sends a message into
    the candidate's row, in message order -- and ``None`` otherwise."""
    sample = np.asarray(sample, dtype=np.float64)
    L, Q = sample.shape[1], sample.shape[2]
    links = np.asarray(links, dtype=np.int64).reshape(-1)
    if links.size < 1 or ((links < 0) | (links >= L)).any():
        raise ValueError(f"links must hold at least one link index in 0 ... {L - 1}, got {links.tolist()}")
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or width < 1:
        raise ValueError(f"width must be a positive int, got {width!r}")
    clear = ~np.any(sample[:, links, :] != 0, axis=(0, 1))                       # [Q]: the slot is free on every link
    free = np.zeros(Q, dtype=bool)
    neighbours = [None] * Q
    for q in range(Q - width + 1):
        if clear[q:q + width].all():
            free[q] = True
            cells = np.array([[l, q + t] for l in links.tolist() for t in range(width)], dtype=np.int64).T
            neighbours[q] = placement_neighbourhood(sample, freq, feature_indexes, cells, freq_threshold)
    return free, neighbours


def _sources_of(sample: np.ndarray, freq: np.ndarray, feature_indexes: Dict[str, int], conn_a: int, freq_threshold: float):
    """``(node, sources)`` of the lightpath ``conn_a`` of ``sample``: its number in first-seen order, and the conn ids, in
    first-seen order, of the other lightpaths within the threshold of one of its channels on that channel's link
    (``lut_neighbourhood``'s rule for a lightpath the caller names)."""
    link_idx, freq_idx, vec = _occupied(sample)
    conn = vec[feature_indexes["conn_id"], :].astype(np.int64)
    _, first = np.unique(conn, return_index=True)
    order = [int(conn[i]) for i in np.sort(first)]
    hit = set()
    for t in np.flatnonzero(conn == conn_a):
        on_link = np.flatnonzero((link_idx == link_idx[t]) & (conn != conn_a))
        diff = np.abs(freq[freq_idx[t]] - freq[freq_idx[on_link]])
        hit.update(conn[on_link[(diff > 0) & (diff < freq_threshold)]].tolist())
    return order.index(conn_a), [c for c in order if c in hit]


def retest_neighbourhood(sample: np.ndarray, freq: np.ndarray, feature_indexes: Dict[str, int], freq_threshold: float = 0.05):
    """What ``LightpathPredictor.retest`` takes of one sample ``[lp_feat, link, freq]``, stated on the host: one tuple
    ``(conn, node, sources)`` per lightpath of the sample, in first-seen order -- so ``node`` counts 0, 1, ...: the
    lightpath's node in ``create_lightpath_graph``'s graph of the sample, with or without that lightpath flagged
    (``infer.materialise_retest`` changes ``osnr``, ``snr`` and ``ber`` only, hence nobody's channels).  ``sources``: the conn
    ids whose messages the lightpath's row sums when it is retested, in message order (first-seen order), by the rule of
    ``lut_neighbourhood`` for a lightpath the caller names.  An empty sample gives ``[]``."""
    fi = feature_indexes
    sample, freq = np.asarray(sample, dtype=np.float64), np.asarray(freq, dtype=np.float64)
    _, _, vec = _occupied(sample)
    conn = vec[fi["conn_id"], :].astype(np.int64)
    _, first = np.unique(conn, return_index=True)
    return [(int(conn[i]),) + _sources_of(sample, freq, fi, int(conn[i]), freq_threshold) for i in np.sort(first)]


def placement_impact(sample: np.ndarray, freq: np.ndarray, feature_indexes: Dict[str, int], values_row: np.ndarray, cells,
                     freq_threshold: float = 0.05):
    """Which established lightpaths a candidate of ``LightpathPredictor.place_impact`` disturbs and what their rows sum,
    stated on the host: one tuple ``(conn, node_before, node_after, sources_before, sources_after)`` per affected
    lightpath, in the sample's first-seen order -- the conns are ``placement_neighbourhood``'s list, because the
    interference rule is symmetric: the candidate's interferers are the lightpaths the candidate interferes with.
    ``node_before`` / ``node_after``: the lightpath's number in first-seen order of ``sample`` / of the sample with the
    candidate placed (``place_lightpath``; its refusals apply), i.e. its node in ``create_lightpath_graph``'s graph of the
    retest sample without / with the candidate.  ``sources_before`` / ``sources_after``: the conn ids whose messages its row
    sums there, in message order (first-seen order), each taken from its own sample by the rule of ``lut_neighbourhood``.
    The candidate fills free channels only, so ``sources_after`` is ``sources_before`` with the candidate's conn inserted
    at the candidate's first-seen position: behind the lightpaths whose first channel ``l * Q + q`` lies below the smallest
    of the candidate's cells."""
    fi = feature_indexes
    sample, freq = np.asarray(sample, dtype=np.float64), np.asarray(freq, dtype=np.float64)
    edited, _ = place_lightpath(sample, values_row, cells, fi)
    out = []
    for conn in placement_neighbourhood(sample, freq, fi, cells, freq_threshold):
        node_before, sources_before = _sources_of(sample, freq, fi, conn, freq_threshold)
        node_after, sources_after = _sources_of(edited, freq, fi, conn, freq_threshold)
        out.append((conn, node_before, node_after, sources_before, sources_after))
    return out


def reroute_impact(sample: np.ndarray, freq: np.ndarray, feature_indexes: Dict[str, int], values_row: np.ndarray, cells,
                   freq_threshold: float = 0.05, release=()):
    """Whom a candidate of ``LightpathPredictor.reroute_impact`` helps and whom it hurts, stated on the host: one tuple
    ``(conn, node_before, node_after, sources_before, sources_after, gains, lost)`` per affected lightpath, in the sample's
    first-seen order.  Affected are the SURVIVORS (the lightpaths not in ``release``) that interfere with the candidate --
    ``placement_neighbourhood(..., release=)``'s list -- or had, in the unedited ``sample``, at least one released
    lightpath among their sources; a released lightpath is never affected.  ``node_before`` / ``sources_before``: the
    lightpath's number and the conn ids whose messages its row sums in ``sample`` (``_sources_of``: the released
    lightpaths still send theirs); ``node_after`` / ``sources_after``: the same in the sample with ``release`` released and
    the candidate placed (``place_lightpath(..., release=)``; its refusals apply).  ``gains``: the candidate is one of
    ``sources_after``; ``lost``: the released lightpaths among ``sources_before``, each once.  With ``release=()`` the
    first five fields are ``placement_impact``'s tuples, ``gains`` is True and ``lost`` 0."""
    fi = feature_indexes
    sample, freq = np.asarray(sample, dtype=np.float64), np.asarray(freq, dtype=np.float64)
    values_row = np.asarray(values_row, dtype=np.float64)
    edited, _ = place_lightpath(sample, values_row, cells, fi, release)
    _, gone = _released(sample, release, fi)
    near = set(placement_neighbourhood(sample, freq, fi, cells, freq_threshold, release))
    own = int(values_row[fi["conn_id"]])
    _, _, vec = _occupied(sample)
    conn = vec[fi["conn_id"], :].astype(np.int64)
    _, first = np.unique(conn, return_index=True)
    out = []
    for c in [int(conn[i]) for i in np.sort(first)]:
        if c in gone:
            continue
        node_before, sources_before = _sources_of(sample, freq, fi, c, freq_threshold)
        lost = sum(s in gone for s in sources_before)
        if c not in near and not lost:
            continue
        node_after, sources_after = _sources_of(edited, freq, fi, c, freq_threshold)
        out.append((c, node_before, node_after, sources_before, sources_after, own in sources_after, lost))
    return out


def topological_links(sample: np.ndarray, feature_indexes: Dict[str, int]):
    """What ``TopologicalPredictor.from_status`` takes of one sample ``[lp_feat, link, freq]``, stated on the host:
    ``(edge_index [2, m] int64, conn [m] int64)``.  The lightpaths are the distinct ``trunc(conn_id)`` of the occupied
    channels, each with the ``src_id`` / ``dst_id`` of its first channel in scan order; among the lightpaths of one
    unordered node pair the one with the largest ``conn_id`` wins the pair; a winner between ``u != v`` gives the directed
    links ``(u, v)`` and ``(v, u)``, one with ``u == v`` the single self loop.  Nodes are 0-based (``src_id - 1``), the
    links ascending by ``(source, target)`` -- the canonical order -- and ``conn[e]`` is the winner whose features link ``e``
    carries.  These are the links of ``create_topological_graph``'s graph after ``canonical_link_order``."""
    fi = feature_indexes
    _, _, vec = _occupied(np.asarray(sample, dtype=np.float64))
    conn = vec[fi["conn_id"], :].astype(np.int64)
    uniq, first = np.unique(conn, return_index=True)
    winner: Dict[tuple, int] = {}
    for c, i in zip(uniq.tolist(), first.tolist()):           # ascending conn: the last one written is the largest
        u, v = int(vec[fi["src_id"], i]) - 1, int(vec[fi["dst_id"], i]) - 1
        winner[(min(u, v), max(u, v))] = c
    links = sorted({(a, b, c) for (u, v), c in winner.items() for a, b in ((u, v), (v, u))})
    if not links:
        return np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.int64)
    arr = np.asarray(links, dtype=np.int64)
    return np.ascontiguousarray(arr[:, :2].T), np.ascontiguousarray(arr[:, 2])


def placement_links(sample: np.ndarray, values_row: np.ndarray, cells, feature_indexes: Dict[str, int], release=()):
    """One candidate of ``TopologicalPredictor.place``, stated on the host: ``(edge_index [2, m] int64, conn [m] int64,
    outcome)``.  ``edge_index`` and ``conn`` are ``topological_links`` of the edited sample, ``place_lightpath(sample,
    values_row, cells, feature_indexes)[0]`` (its ``ValueError`` for an illegal placement as there).  ``outcome`` says what
    the candidate did to the graph of the unedited sample: ``"new pair"`` -- no lightpath of the sample joins its unordered
    node pair, the graph grows by two links (one for a self loop); ``"takes the pair"`` -- its ``trunc(conn_id)`` is larger
    than that of every lightpath of the sample on the pair, whose links now carry the candidate's features; ``"loses the
    pair"`` -- it is not, and the edited graph is the unedited one.  The cells decide only whether the placement is legal.
    ``release``: conn ids of lightpaths released first (``place(..., release=)``; a conn the sample does not hold is a
    ``ValueError``).  They take no part in the pair contest, and ``outcome`` is then stated against the graph of the
    survivors: a pair whose only lightpaths were released is new to the candidate."""
    fi = feature_indexes
    edited, _ = place_lightpath(sample, values_row, cells, fi, release)
    sample, _ = _released(np.asarray(sample, dtype=np.float64), release, fi)
    edge_index, conn = topological_links(edited, fi)
    values_row = np.asarray(values_row, dtype=np.float64)
    c = int(values_row[fi["conn_id"]])
    u, v = int(values_row[fi["src_id"]]) - 1, int(values_row[fi["dst_id"]]) - 1
    before, _ = topological_links(sample, fi)
    had_pair = bool(((before[0] == u) & (before[1] == v)).any())
    if not had_pair:
        return edge_index, conn, "new pair"
    return edge_index, conn, "takes the pair" if (conn == c).any() else "loses the pair"


# ------------------------------------------------------------------------------------------ store_graphs.py counterpart
def store_graphs(dataset: Source, representation: str = "lightpath", directory: Optional[str] = None,
                 features_to_consider: Sequence[str] = DEFAULT_FEATURES, storage_type: str = "pickle",
                 samples: Optional[Sequence[int]] = None) -> str:
    """The loop of ``store_graphs.py:58-79``: clear the directory, write ``graph_<i>.gpickle`` (or ``.gexf``)."""
    if representation not in ("lightpath", "topological"):
        raise ValueError("representation must be 'lightpath' or 'topological'")
    ds = _source(dataset)
    directory = directory or ("networkx_graphs_lightpath" if representation == "lightpath" else "networkx_graphs_topological")
    if os.path.exists(directory):
        for name in os.listdir(directory):
            os.remove(os.path.join(directory, name))
    os.makedirs(directory, exist_ok=True)
    make = create_lightpath_graph if representation == "lightpath" else create_topological_graph
    for i in (range(len(ds)) if samples is None else samples):
        G = make(i, list(features_to_consider), ds)
        if storage_type == "pickle":
            with open(os.path.join(directory, f"graph_{i}.gpickle"), "wb") as f:
                pickle.dump(G, f, protocol=pickle.HIGHEST_PROTOCOL)
        elif storage_type == "gexf":
            import networkx as nx
            nx.write_gexf(G, os.path.join(directory, f"graph_{i}.gexf"))
        else:
            raise ValueError("storage_type must be 'pickle' or 'gexf'")
    return directory


def build_shard(dataset, representation: str = "lightpath", features_to_consider: Sequence[str] = DEFAULT_FEATURES,
                samples: Optional[Sequence[int]] = None, device=None, freq_threshold: float = 0.05):
    """Samples -> graphs -> ``Data`` -> one ``PackedGraphs`` shard, without the per-graph files in between; the
    conversion rules are those of the dataset classes (``dataset.topological_data_from_graph`` / ``lightpath_...``).

    With a ``device`` (or a ``DeviceStatus`` as ``dataset``) the shard is built on the GPU and stays there, in the state
    ``PackedGraphs.to_device`` leaves one; its directed links are in canonical order (``canonical_link_order``)."""
    if isinstance(dataset, DeviceStatus):
        return _device_build(dataset, representation, features_to_consider, samples, freq_threshold)
    if device is not None:
        status = _source(dataset).to_device(device, samples)
        return _device_build(status, representation, features_to_consider, None, freq_threshold)
    from .dataset import lightpath_data_from_graph, topological_data_from_graph
    from .loader import PackedGraphs
    ds = _source(dataset)
    feats = sorted(features_to_consider)
    out = []
    for i in (range(len(ds)) if samples is None else samples):
        if representation == "lightpath":
            out.append(lightpath_data_from_graph(create_lightpath_graph(i, list(features_to_consider), ds, freq_threshold),
                                                 sorted(feats + ["is_lut"])))
        else:
            out.append(topological_data_from_graph(create_topological_graph(i, list(features_to_consider), ds), feats))
    return PackedGraphs.from_data_list(out)


# ------------------------------------------------------------------------------------------ device builder
# caps and status bits of csrc/status_graph.hip (include/qot_gnn.h: QOT_SG_*)
MAX_FREQS, MAX_LIGHTPATHS = 1024, 256
SG_BAD_CONN, SG_TOO_MANY, SG_BAD_ENDPOINT, SG_BAD_SAMPLE = 1, 2, 4, 8
_SG_CAUSES = (
    (SG_BAD_CONN, "a conn_id is not finite or lies beyond +-2^53"),
    (SG_TOO_MANY, f"a sample holds more than {MAX_LIGHTPATHS} lightpaths (the cap of the device builder)"),
    (SG_BAD_ENDPOINT, f"a src_id / dst_id is not an integer in 1 .. {NUM_TOPOLOGY_NODES}"),
    (SG_BAD_SAMPLE, "a sample number lies outside the status chunk"),
)


def _column_tables(st: DeviceStatus, representation: str, features_to_consider: Sequence[str]):
    """The two column tables of ``qot_status_graph_fill`` on the device: one row ``(lp_feat row, min, max - min,
    has_range)`` per output column in sorted name order (``is_lut``: row -1), and the same over ``target``."""
    import torch
    from .dataset import FEATURE_RANGES, TARGET_KEYS, TARGET_RANGES
    key = (representation, tuple(features_to_consider))
    if key not in st._tables:
        feats = sorted(features_to_consider)
        names = sorted(feats + ["is_lut"]) if representation == "lightpath" else feats
        fi = st.feature_indexes

        def row(index, r):
            if r is None:
                return [float(index), 0.0, 1.0, 0.0]
            return [float(index), float(r["min"]), float(r["max"] - r["min"]), 1.0]

        cols = [row(-1, None) if (n == "is_lut" and representation == "lightpath") else row(fi[n], FEATURE_RANGES.get(n))
                for n in names]
        tcols = [row(st.metric.index(k) if k in st.metric else -1, TARGET_RANGES[k]) for k in TARGET_KEYS]
        up = lambda rows: torch.tensor(rows, dtype=torch.float64).reshape(len(rows), 4).to(st.device)
        st._tables[key] = (up(cols), up(tcols), len(names))
    return st._tables[key]


def _device_build(st: DeviceStatus, representation: str, features_to_consider: Sequence[str],
                  samples: Optional[Sequence[int]], freq_threshold: float):
    """``csrc/status_graph.hip`` over the samples of a resident chunk: count launch, ONE host read (status word, self-loop
    flag, per-graph node and link counts), fill launch.  There is no CPU form of this path."""
    import torch
    from . import _lib
    from .loader import PackedGraphs
    if representation not in ("lightpath", "topological"):
        raise ValueError("representation must be 'lightpath' or 'topological'")
    _lib.load()
    if not st.data.is_cuda:
        raise _lib.QotError("the device graph builder needs a status chunk on the GPU, got CPU tensors: there is no CPU "
                            "form of it (the host path is build_shard(..., device=None))")
    dev = st.device
    S, P, L, Q = (int(v) for v in st.data.shape)
    fi = st.feature_indexes
    lightpath = representation == "lightpath"
    rep = 0 if lightpath else 1
    conn_row = fi["conn_id"]
    src_row, dst_row = (-1, -1) if lightpath else (fi["src_id"], fi["dst_id"])
    osnr_row, snr_row, ber_row = (fi["osnr"], fi["snr"], fi["ber"]) if lightpath else (-1, -1, -1)
    cols, tcols, ncol = _column_tables(st, representation, list(features_to_consider))
    if Q > MAX_FREQS:
        raise _lib.QotError(f"the device graph builder takes at most {MAX_FREQS} frequency slots per link, got {Q}")
    with torch.cuda.device(dev):
        if samples is None:
            G, picks = S, None
        else:
            picks = torch.tensor([int(v) for v in samples], dtype=torch.long).to(dev)
            G = int(picks.numel())
        info = torch.zeros(2 + 2 * G, dtype=torch.int32, device=dev)
        nbytes = int(_lib.load().qot_status_graph_scratch_bytes(G, L, Q, rep))
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        _lib.call("qot_status_graph_count", st.data, st.freq, picks, G, S, P, L, Q, conn_row, src_row, dst_row,
                  float(freq_threshold), rep, scratch, nbytes, info)
        host = info.cpu()                                    # the one device -> host read of the call
        code = int(host[0])
        if code:
            raise _lib.QotError("qot_status_graph: " + "; ".join(t for bit, t in _SG_CAUSES if code & bit) +
                                ": no graph was built")
        counts = host[2:].view(G, 2).to(torch.long)
        zero = torch.zeros(1, dtype=torch.long)
        node_ptr = torch.cat([zero, counts[:, 0].cumsum(0)])
        edge_ptr = torch.cat([zero, counts[:, 1].cumsum(0)])
        N, E = int(node_ptr[-1]), int(edge_ptr[-1])
        dcounts = info[2:].view(G, 2).to(torch.long)
        dzero = torch.zeros(1, dtype=torch.long, device=dev)
        node_ptr_dev = torch.cat([dzero, dcounts[:, 0].cumsum(0)])
        edge_ptr_dev = torch.cat([dzero, dcounts[:, 1].cumsum(0)])
        edge_index = torch.empty(2, E, dtype=torch.long, device=dev)
        feat = torch.empty(N if lightpath else E, ncol, dtype=torch.float32, device=dev)
        node_ids = None if lightpath else torch.empty(N, dtype=torch.long, device=dev)
        y = torch.empty(G, 3, dtype=torch.float32, device=dev)
        _lib.call("qot_status_graph_fill", st.data, st.target, picks, G, S, P, L, Q, int(st.target.shape[1]), osnr_row,
                  snr_row, ber_row, cols, ncol, tcols, rep, scratch, info, node_ptr_dev, edge_ptr_dev, N, E, edge_index,
                  feat, node_ids, y)
        if lightpath:
            out = PackedGraphs(node_ptr, edge_ptr, edge_index, None, None, feat, y, None)
        else:
            out = PackedGraphs(node_ptr, edge_ptr, edge_index, feat, node_ids, None, y.view(-1),
                               NUM_TOPOLOGY_NODES if G else None)
        out.has_self_loops = bool(host[1])
        out.graph_of_node = torch.repeat_interleave(torch.arange(G, device=dev), dcounts[:, 0], output_size=N)
        out.node_ptr_dev, out.edge_ptr_dev = node_ptr_dev, edge_ptr_dev
        out.device = dev
        out._batch_cache = {}
    return out


def device_batch(status: DeviceStatus, representation: str, features_to_consider: Sequence[str] = DEFAULT_FEATURES,
                 samples: Optional[Sequence[int]] = None, freq_threshold: float = 0.05):
    """The chosen samples of a resident chunk as one ``Batch`` on the device, with the fields ``PackedGraphs.device_batch``
    sets: what the models and the single-launch predictors take."""
    if not isinstance(status, DeviceStatus):
        raise TypeError("device_batch takes a DeviceStatus (NetworkStatus.to_device)")
    shard = _device_build(status, representation, features_to_consider, samples, freq_threshold)
    return shard.device_batch(0, len(shard))


def canonical_link_order(edge_index, edge_ptr, edge_attr=None):
    """The directed links of a shard in the device builder's order: graphs as they are, inside a graph ascending by
    ``(edge_index[0], edge_index[1])``.  The host builder's order inside a graph follows networkx's adjacency (grouped by
    source, targets in insertion order); this keeps the grouping by graph and by source.  Returns the reordered
    ``edge_index``, or ``(edge_index, edge_attr)`` when ``edge_attr`` is given (its rows follow their links).  Pure host
    function; the inputs are not modified."""
    import torch
    E = edge_index.shape[1]
    counts = (edge_ptr[1:] - edge_ptr[:-1]).to(torch.long)
    if int(edge_ptr[-1]) - int(edge_ptr[0]) != E:
        raise ValueError("edge_ptr does not cover edge_index")
    graph = torch.repeat_interleave(torch.arange(counts.numel()), counts)
    perm = torch.argsort(edge_index[1], stable=True)
    perm = perm[torch.argsort(edge_index[0][perm], stable=True)]
    perm = perm[torch.argsort(graph[perm], stable=True)]
    ei = edge_index[:, perm].contiguous()
    if edge_attr is None:
        return ei
    return ei, edge_attr[perm].contiguous()


def canonical_shard(shard):
    """A host shard with its links in canonical order (``canonical_link_order``); everything else is shared."""
    from .loader import PackedGraphs
    if shard.edge_attr is None:
        ei, ea = canonical_link_order(shard.edge_index, shard.edge_ptr), None
    else:
        ei, ea = canonical_link_order(shard.edge_index, shard.edge_ptr, shard.edge_attr)
    return PackedGraphs(shard.node_ptr, shard.edge_ptr, ei, ea, shard.node_ids, shard.x, shard.y, shard.uniform_node_ids)


# ------------------------------------------------------------------------------------------ .nc-free sample generator
LP_FEAT = ["conn_id", "src_id", "dst_id", "mod_order", "path_len", "num_spans", "freq", "osnr", "snr", "ber"]
METRICS = ["osnr", "snr", "ber", "class"]


def synthetic_network_status(num_samples: int, num_links: int = 60, num_freqs: int = 72, max_lightpaths: int = 24,
                             seed: int = 0) -> NetworkStatus:
    """Network-status samples with the dataset's structure (the real ``.nc`` is not shipped, ``.gitignore:2``): per
    sample up to ``max_lightpaths`` lightpaths, each routed over 1-6 links on one 50 GHz slot (occasionally two
    adjacent slots), feature values inside ``constants.FEATURE_RANGES``, established lightpaths carrying measured
    osnr/snr/ber and exactly one lightpath under test (osnr = snr = ber = -1)."""
    rng = np.random.default_rng(seed)
    freq = np.round(192.2 + 0.05 * np.arange(num_freqs), 6)
    data = np.zeros((num_samples, len(LP_FEAT), num_links, num_freqs), dtype=np.float64)
    target = np.zeros((num_samples, len(METRICS)), dtype=np.float64)
    fi = {f: i for i, f in enumerate(LP_FEAT)}
    for s in range(num_samples):
        n_lp = int(rng.integers(2, max_lightpaths + 1))
        lut = int(rng.integers(0, n_lp))
        conn_ids = rng.choice(np.arange(1, 10 * max_lightpaths), size=n_lp, replace=False)
        for k in range(n_lp):
            src, dst = rng.choice(np.arange(1, NUM_TOPOLOGY_NODES + 1), size=2, replace=False)
            links = rng.choice(num_links, size=int(rng.integers(1, 7)), replace=False)
            f0 = int(rng.integers(0, num_freqs - 1))
            slots = [f0] if rng.random() < 0.85 else [f0, f0 + 1]
            spans = int(rng.integers(1, 107))
            vec = np.zeros(len(LP_FEAT))
            vec[fi["conn_id"]], vec[fi["src_id"]], vec[fi["dst_id"]] = conn_ids[k], src, dst
            vec[fi["mod_order"]] = float(rng.choice([4, 8, 16, 32, 64]))
            vec[fi["num_spans"]] = spans
            vec[fi["path_len"]] = float(rng.integers(24214, 7834746))
            vec[fi["freq"]] = freq[f0]
            if k == lut:
                vec[fi["osnr"]] = vec[fi["snr"]] = vec[fi["ber"]] = -1.0
            else:
                vec[fi["osnr"]] = rng.uniform(12.47, 33.49)
                vec[fi["snr"]] = rng.uniform(8.96, 29.98)
                vec[fi["ber"]] = rng.uniform(1.7e-12, 1.98e-2)
            for l in links:
                for fslot in slots:
                    if not data[s, :, l, fslot].any():        # a slot on a link carries one lightpath
                        data[s, :, l, fslot] = vec
        target[s] = [rng.uniform(12.47, 33.49), rng.uniform(8.96, 29.98), rng.uniform(1.7e-12, 1.98e-2), float(rng.integers(0, 2))]
    return NetworkStatus(data, target, LP_FEAT, METRICS, np.arange(num_links), freq)


def main(argv=None):
    """``python -m gnn_qot_estimation_amd.to_graph --dataset x.npz --representation lightpath`` (store_graphs.py:8-36)."""
    import argparse
    ap = argparse.ArgumentParser(description="Store networkx graphs in a directory.")
    ap.add_argument("--dataset", required=True, help=".npz written by NetworkStatus.save (or .nc with xarray installed)")
    ap.add_argument("--representation", default="lightpath", choices=["lightpath", "topological"])
    ap.add_argument("--storage_type", default="pickle", choices=["pickle", "gexf"])
    ap.add_argument("--directory", default=None)
    ap.add_argument("--shard", default=None, help="write one PackedGraphs shard file (dataset.save_shard) instead of graph files")
    ap.add_argument("--device", default=None, help="with --shard: build the shard on this device (e.g. cuda)")
    args = ap.parse_args(argv)
    if args.shard is not None:
        from .dataset import save_shard
        shard = build_shard(args.dataset, args.representation, device=args.device)
        save_shard(args.shard, shard, {"representation": args.representation, "features": sorted(DEFAULT_FEATURES)})
        print(f"Shard of {len(shard)} graphs stored in {args.shard}")
        return
    d = store_graphs(args.dataset, args.representation, args.directory, storage_type=args.storage_type)
    print(f"Graphs stored in {d}")


if __name__ == "__main__":
    main()
