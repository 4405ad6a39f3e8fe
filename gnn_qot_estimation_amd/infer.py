"""Single-launch inference: ``TopologicalPredictor`` (``csrc/infer.hip``; its Monte-Carlo dropout
``sample``: ``csrc/infer_mc.hip``; its per-link ``sensitivity``: ``csrc/infer_grad.hip``, DESIGN.md
4.16; its ``what_if`` over edited graphs: ``csrc/infer_whatif.hip``; its ``from_status`` over network-status
samples: ``csrc/infer_topological_status.hip``; its ``place`` of candidate lightpaths into such samples:
``csrc/infer_topological_place.hip``) and ``LightpathPredictor`` (``csrc/infer_lightpath.hip``; its per-neighbour ``sensitivity``:
``csrc/infer_lightpath_grad.hip``; its ``what_if`` over candidate lightpaths:
``csrc/infer_lightpath_whatif.hip``; its ``from_status`` over network-status samples:
``csrc/infer_lightpath_status.hip``; its ``place`` of candidate lightpaths into such samples:
``csrc/infer_lightpath_place.hip``).  Both ``place`` calls take ``release=`` / ``release_ptr=`` for a reroute:
``csrc/infer_lightpath_place_release.hip``, ``csrc/infer_topological_place_release.hip``, DESIGN.md 4.24.

``model(data)`` in eval mode goes through the training machinery: a launch group, the prologue launch, the graph form of
TransformerConv, the NNConv forward and the read-out kernel (``LightpathGNN``: the self-looped graph index, the GAT walk
over all nodes, BatchNorm rows and the head), each behind an autograd wrapper.  That is host-bound for one graph or a
handful -- the case of a planning tool that scores one candidate after another.  A predictor runs the same function as ONE
kernel launch per call and touches autograd nowhere.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib, to_graph
from .functional import _f32c
from .graph import _cache

MAX_NODES = 128                 # csrc/infer.hip: kInferMaxN
WIDTHS = (16, 32, 64)
MAX_EDGE_DIM = 4
MAX_OUTPUTS = 8

_WCAT_IDX = {}


def wcat_index(h: int, k: int, device) -> torch.Tensor:
    """Gather index into ``cat([nn.2.weight.flatten(), nn.2.bias, lin.weight.flatten()])`` that lays the NNConv operand
    ``Wcat [(K + 2) H, H]`` out row-major, as ``functional.nnconv_wcat`` states it (``qot_gather3`` does the gather)."""
    key = (h, k, str(device))
    if key not in _WCAT_IDX:
        kk, a, o = torch.meshgrid(torch.arange(k), torch.arange(h), torch.arange(h), indexing="ij")
        a2, o2 = torch.meshgrid(torch.arange(h), torch.arange(h), indexing="ij")
        idx = torch.cat([((a * h + o) * k + kk).reshape(k * h, h), h * h * k + a2 * h + o2,
                         h * h * (k + 1) + o2 * h + a2], 0)
        _WCAT_IDX[key] = idx.reshape(-1).to(torch.int32).contiguous().to(device)
    return _WCAT_IDX[key]


# kind -> (the envelope's symbol, the edge cap's symbol, the word the error message puts before "edge cap")
_KINDS = {
    "eval": ("qot_topological_infer_supported", "qot_topological_infer_max_edges", ""),
    "mc": ("qot_topological_infer_mc_supported", "qot_topological_infer_mc_max_edges", "sampling "),
    "grad": ("qot_topological_infer_grad_supported", "qot_topological_infer_grad_max_edges", "sensitivity "),
    "whatif": ("qot_topological_infer_whatif_supported", "qot_topological_infer_whatif_max_edges", "what-if "),
}


def _edge_cap(kind, n_max, hidden, edge_dim):
    return int(getattr(_lib.load(), _KINDS[kind][1])(int(n_max), int(hidden), int(edge_dim)))


def edge_cap(n_max: int, hidden: int, edge_dim: int) -> int:
    """Most edges a graph may have beside ``n_max`` nodes (the kernel's LDS budget, asked of the library); -1: none."""
    return _edge_cap("eval", n_max, hidden, edge_dim)


def mc_edge_cap(n_max: int, hidden: int, edge_dim: int) -> int:
    """``edge_cap`` of the sampling kernel (``TopologicalPredictor.sample``): lower, its LDS image also holds the sample's
    masked copy of the first convolution's output; -1: none."""
    return _edge_cap("mc", n_max, hidden, edge_dim)


def grad_edge_cap(n_max: int, hidden: int, edge_dim: int) -> int:
    """``edge_cap`` of the sensitivity kernel (``TopologicalPredictor.sensitivity``): lower, its LDS image also holds the
    adjoint of the first convolution's output and ``2 * edge_dim`` more words per edge; -1: none."""
    return _edge_cap("grad", n_max, hidden, edge_dim)


def what_if_edge_cap(n_max: int, hidden: int, edge_dim: int) -> int:
    """``edge_cap`` of the what-if kernel (``TopologicalPredictor.what_if``): the eval kernel's, its LDS image is the same.
    It bounds ``edges of a candidate's base graph + the candidate's additions`` (removals are not credited); -1: none."""
    return _edge_cap("whatif", n_max, hidden, edge_dim)


def grad_outputs(outputs, num_outputs: int, who: str = "TopologicalPredictor.sensitivity"):
    """The ``outputs`` argument of ``TopologicalPredictor.sensitivity`` (and of ``LightpathPredictor.sensitivity``: ``who``
    names the caller in the message), checked without a device: ``None`` (every output, in order) or a non-empty list /
    tuple of distinct integers in ``0 ... num_outputs - 1``; returns the list or raises the named ``ValueError``."""
    O = int(num_outputs)
    if outputs is None:
        return list(range(O))
    if not isinstance(outputs, (list, tuple)) or len(outputs) == 0:
        raise ValueError(f"{who}: outputs must be None or a non-empty list of output indices, got {outputs!r}")
    for o in outputs:
        if isinstance(o, bool) or not isinstance(o, int) or not 0 <= o < O:
            raise ValueError(f"{who}: outputs must be integers in 0 ... {O - 1}, got {o!r}")
    if len(set(outputs)) != len(outputs):
        raise ValueError(f"{who}: outputs must be distinct, got {list(outputs)!r}")
    return list(outputs)


MC_MAX_SAMPLES = 4096           # csrc/infer_mc.hip: T


def mc_chunk(num_graphs: int, samples: int, compute_units: int) -> int:
    """Samples per workgroup of ``qot_topological_infer_mc``'s grid ``(B, ceil(T / chunk))``.  The grid is that of the
    largest chunk for which ``B * ceil(T / chunk)`` workgroups still reach the device's compute-unit count (a larger chunk
    shares phases 1 - 2 among more samples, but leaves units idle); the chunk returned is the smallest with that many
    workgroups, so that they carry equal shares (T = 32 over 4 workgroups: 8 each, not 10, 10, 10, 2).  1 when no chunk
    reaches the device.  Pure host arithmetic."""
    B, T, cus = int(num_graphs), int(samples), int(compute_units)
    if T < 1:
        raise ValueError(f"mc_chunk: samples must be >= 1, got {T}")
    if B < 1 or B * T < cus:
        return 1
    need = -(-cus // B)                                    # workgroups per graph that reach the device
    largest = T if need <= 1 else (T - 1) // (need - 1)    # largest chunk with ceil(T / chunk) >= need
    chunks = -(-T // largest)
    return -(-T // chunks)


def mc_args(samples, p, chunk, first_step, model_p=(0.0, 0.0)):
    """The argument checks of ``TopologicalPredictor.sample`` that need no device: returns ``(T, p_conv, p_head, chunk or
    None, first_step)`` or raises the named ``ValueError``.  ``model_p``: the model's ``(conv, head)`` probabilities, used
    when ``p`` is ``None``."""
    who = "TopologicalPredictor.sample"
    if isinstance(samples, bool) or not isinstance(samples, int) or not 2 <= samples <= MC_MAX_SAMPLES:
        raise ValueError(f"{who}: samples must be an integer in 2 ... {MC_MAX_SAMPLES}, got {samples!r}")
    if p is None:
        pc, ph = model_p
    elif isinstance(p, (tuple, list)):
        if len(p) != 2:
            raise ValueError(f"{who}: p must be a probability or a (conv, head) pair, got {p!r}")
        pc, ph = p
    else:
        pc = ph = p
    for name, v in (("the convolutions'", pc), ("the read-out's", ph)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) < 1.0:
            raise ValueError(f"{who}: p must lie in [0, 1), got {v!r} for {name} dropout")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk <= samples):
        raise ValueError(f"{who}: chunk must be an integer in 1 ... samples = {samples}, got {chunk!r}")
    if isinstance(first_step, bool) or not isinstance(first_step, int) or first_step < 0 or first_step + samples > 1 << 63:
        raise ValueError(f"{who}: first_step must be an integer >= 0 with first_step + samples <= 2^63, got {first_step!r}")
    return samples, float(pc), float(ph), chunk, first_step


def _i64(t, dev):
    if t.dtype != torch.int64 or t.device != dev:
        t = t.to(device=dev, dtype=torch.int64)
    return t.contiguous()


def graph_slices(data, ei, N, dev, who):
    """``(node_ptr, edge_ptr, B, n_max, max_e, exact)`` of a block-diagonal batch of ``N`` nodes with the int64
    ``edge_index`` ``ei`` on ``dev``.  A batch that carries ``ptr`` / ``edge_ptr`` / ``graph_sizes`` (ours do) costs no
    device read; otherwise the slices come from ``data.batch`` with device-side torch ops (and ``n_max`` / ``max_e`` with one
    read).  Edges not grouped by graph raise ``ValueError``.  ``exact()`` reads the true largest node / edge count (the
    carried sizes are bounds: a shard inherits its parent's).  ``who`` prefixes the error messages."""
    E = ei.shape[1]
    ptr, eptr, sizes = getattr(data, "ptr", None), getattr(data, "edge_ptr", None), getattr(data, "graph_sizes", None)
    if ptr is None:
        batch = _i64(data.batch, dev)
        B = getattr(data, "num_graphs", None)
        B = int(B) if B is not None else (int(batch.max()) + 1 if N else 0)
        ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.cumsum(torch.bincount(batch, minlength=B), 0)
        sizes = None
    ptr = _i64(ptr, dev)
    B = ptr.numel() - 1
    if eptr is None:
        # edges of a collated batch are grouped by graph: the slices follow from the graph of every edge's target
        batch = torch.repeat_interleave(torch.arange(B, device=dev), ptr[1:] - ptr[:-1])
        eb = batch[ei[1]]
        if E > 1 and not bool((eb[1:] >= eb[:-1]).all()):
            raise ValueError(f"{who}: the edges of the batch are not grouped by graph")
        eptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        eptr[1:] = torch.cumsum(torch.bincount(eb, minlength=B), 0)
        sizes = None
    eptr = _i64(eptr, dev)
    if eptr.numel() != B + 1:
        raise ValueError(f"{who}: ptr and edge_ptr disagree on the number of graphs")

    def exact():
        if B == 0:
            return 0, 0
        return int((ptr[1:] - ptr[:-1]).max()), int((eptr[1:] - eptr[:-1]).max())
    n_max, max_e = (int(sizes[0]), int(sizes[1])) if sizes is not None else exact()
    return ptr, eptr, B, n_max, max_e, exact


WHAT_IF_MAX_DROP = 32           # csrc/infer_whatif.hip: kWhatIfMaxDrop; csrc/infer_lightpath_dev.hpp: kLpMaxDrop


def _host_ptr(p, name, total, who):
    """A pointer array as an int64 host tensor, checked: non-decreasing from 0 to ``total``.  A device tensor costs one
    read; a list or a host tensor none."""
    try:
        t = torch.as_tensor(p)
    except (TypeError, ValueError, RuntimeError):
        t = None
    if t is None or t.dim() != 1 or t.numel() == 0 or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"{who}: {name} must be a non-empty 1-d sequence of integers, got {p!r}")
    t = t.to(device="cpu", dtype=torch.int64)
    if int(t[0]) != 0 or int(t[-1]) != total or (t.numel() > 1 and int(t.diff().min()) < 0):
        raise ValueError(f"{who}: {name} must be non-decreasing from 0 to {total}, got {t.tolist()!r}")
    return t


_WhatIf = namedtuple("_WhatIf", "K A R add_ptr drop_ptr max_add")


def what_if_args(edge_dim, add_edge_index, add_edge_attr, add_ptr, drop=None, drop_ptr=None, graph=None, num_graphs=None,
                 who="TopologicalPredictor.what_if"):
    """The argument checks of ``TopologicalPredictor.what_if`` (and of ``materialise_what_if``) that need no device:
    returns ``(K, A, R, add_ptr, drop_ptr, max_add)`` with the pointer arrays as int64 host tensors (``drop_ptr`` ``None``
    without removals), or raises the named ``ValueError``.  ``num_graphs``: the base batch's graph count when the caller
    knows it (``graph=None`` needs exactly one)."""
    if not isinstance(add_edge_index, torch.Tensor) or add_edge_index.dim() != 2 or add_edge_index.shape[0] != 2 \
            or add_edge_index.dtype.is_floating_point:
        raise ValueError(f"{who}: add_edge_index must be an integer tensor [2, A], got "
                         f"{tuple(add_edge_index.shape) if isinstance(add_edge_index, torch.Tensor) else add_edge_index!r}")
    A = add_edge_index.shape[1]
    if not isinstance(add_edge_attr, torch.Tensor) or tuple(add_edge_attr.shape) != (A, int(edge_dim)):
        raise ValueError(f"{who}: add_edge_attr must be [{A}, {int(edge_dim)}], got "
                         f"{tuple(add_edge_attr.shape) if isinstance(add_edge_attr, torch.Tensor) else add_edge_attr!r}")
    if (drop is None) != (drop_ptr is None):
        raise ValueError(f"{who}: drop and drop_ptr must be given together (got only "
                         f"{'drop_ptr' if drop is None else 'drop'})")
    ap = _host_ptr(add_ptr, "add_ptr", A, who)
    K = ap.numel() - 1
    R, dp = 0, None
    if drop is not None:
        if not isinstance(drop, torch.Tensor) or drop.dim() != 1 or drop.dtype.is_floating_point:
            raise ValueError(f"{who}: drop must be a 1-d integer tensor of positions into data.edge_index, got {drop!r}")
        R = drop.shape[0]
        dp = _host_ptr(drop_ptr, "drop_ptr", R, who)
        if dp.numel() != K + 1:
            raise ValueError(f"{who}: add_ptr names {K} candidates, drop_ptr {dp.numel() - 1}")
        worst = int(dp.diff().max()) if K else 0
        if worst > WHAT_IF_MAX_DROP:
            raise ValueError(f"{who}: a candidate removes {worst} edges; at most WHAT_IF_MAX_DROP = {WHAT_IF_MAX_DROP}")
    if graph is None:
        if num_graphs is not None and num_graphs != 1:
            raise ValueError(f"{who}: graph=None needs a base batch of exactly one graph, this one has {num_graphs}")
    elif not isinstance(graph, torch.Tensor) or tuple(graph.shape) != (K,) or graph.dtype.is_floating_point:
        raise ValueError(f"{who}: graph must be an integer tensor [{K}] (one base graph per candidate), got "
                         f"{tuple(graph.shape) if isinstance(graph, torch.Tensor) else graph!r}")
    return _WhatIf(K, A, R, ap, dp, int(ap.diff().max()) if K else 0)


def _num_graphs_hint(data):
    """The graph count of a batch where it can be told without a device read, else ``None``."""
    ptr = getattr(data, "ptr", None)
    if ptr is not None:
        return ptr.numel() - 1
    B = getattr(data, "num_graphs", None)
    return None if B is None else int(B)


def materialise_what_if(data, add_edge_index, add_edge_attr, add_ptr, drop=None, drop_ptr=None, graph=None):
    """The explicit batch of the K edited graphs that ``TopologicalPredictor.what_if`` scores: the DEFINITION of that call
    (``predict.what_if(...)[k]`` is row ``k`` of ``predict(materialise_what_if(...))`` bit for bit) and what it saves.
    Pure torch, no kernel of ours; works on CPU tensors as well.

    ``data``: the base batch of B graphs (table mode: ``node_ids``).  Candidate ``k`` names base graph ``graph[k]``
    (``None``: B == 1, all zeros), removes the edges at positions ``drop[drop_ptr[k]:drop_ptr[k + 1]]`` of
    ``data.edge_index`` (any order, a repeat counts once; they must lie in that graph's edge slice) and appends the edges
    ``add_edge_index[:, add_ptr[k]:add_ptr[k + 1]]`` -- ``(source, target)`` in the batch's node numbering, as
    ``data.edge_index`` -- with the rows of ``add_edge_attr``.  Graph ``k`` of the result holds the base graph's nodes
    (``node_ids`` copied, ``x`` as the base batch has it: ``None`` in table mode), its surviving edges in their order and
    the added edges behind them in the order given, node numbers renumbered to the candidate's own block.  The result
    carries ``batch``, ``ptr``, ``edge_ptr`` and ``graph_sizes``.  Bad arguments, a graph number outside ``0 ... B - 1``, a
    drop position outside its graph's slice or an added endpoint outside its graph raise ``ValueError``."""
    from .batch import Batch
    who = "materialise_what_if"
    ei = data.edge_index
    dev = ei.device
    ea = data.edge_attr
    if ea is None or ea.dim() != 2 or ea.shape[0] != ei.shape[1]:
        raise ValueError(f"{who}: data.edge_attr must be [{ei.shape[1]}, D]")
    ids = data.node_ids
    if ids is None:
        raise ValueError(f"{who}: data.node_ids is required (table mode)")
    N, E = ids.shape[0], ei.shape[1]
    ei = _i64(ei, dev)
    ptr, eptr, B, _, _, _ = graph_slices(data, ei, N, dev, who)
    w = what_if_args(ea.shape[1], add_edge_index, add_edge_attr, add_ptr, drop, drop_ptr, graph, B, who)
    K = w.K
    i64 = dict(dtype=torch.int64, device=dev)
    g = torch.zeros(K, **i64) if graph is None else _i64(graph, dev)
    if K and (int(g.min()) < 0 or int(g.max()) >= B):
        raise ValueError(f"{who}: graph must lie in 0 ... {B - 1}")
    ar = torch.arange(K, **i64)
    n_k, m_k = (ptr[1:] - ptr[:-1])[g], (eptr[1:] - eptr[:-1])[g]
    nptr = torch.zeros(K + 1, **i64)
    nptr[1:] = torch.cumsum(n_k, 0)
    bptr = torch.zeros(K + 1, **i64)                       # the base edges of every candidate, dropped ones included
    bptr[1:] = torch.cumsum(m_k, 0)
    # nodes: candidate c's block is its base graph's rows
    cn = torch.repeat_interleave(ar, n_k)
    rows = ptr[g][cn] + (torch.arange(cn.shape[0], **i64) - nptr[cn])
    shift = nptr[:-1] - ptr[g]                             # batch node number -> the candidate's block
    # base edges: every position of the base graph's slice, less the dropped ones
    ce = torch.repeat_interleave(ar, m_k)
    pos = eptr[g][ce] + (torch.arange(ce.shape[0], **i64) - bptr[ce])
    if w.R:
        dpos = _i64(drop, dev)
        cd = torch.repeat_interleave(ar, w.drop_ptr.to(dev).diff())
        if bool(((dpos < eptr[g][cd]) | (dpos >= eptr[g + 1][cd])).any()):
            raise ValueError(f"{who}: a drop position lies outside its candidate's base graph")
        keep = ~torch.isin(ce * max(E, 1) + pos, cd * max(E, 1) + dpos)
        ce, pos = ce[keep], pos[keep]
    # added edges
    ca = torch.repeat_interleave(ar, w.add_ptr.to(dev).diff())
    aei = _i64(add_edge_index, dev)
    if w.A and bool(((aei < ptr[g][ca]) | (aei >= ptr[g + 1][ca])).any()):
        raise ValueError(f"{who}: an added edge has an endpoint outside its candidate's base graph")
    cand = torch.cat([ce, ca])
    order = torch.argsort(cand, stable=True)               # per candidate: survivors in their order, then the additions
    new_ei = torch.cat([ei[:, pos] + shift[ce], aei + shift[ca]], 1)[:, order]
    new_ea = torch.cat([ea[pos], add_edge_attr.to(device=dev, dtype=ea.dtype)], 0)[order]
    out = Batch()
    out.num_graphs = K
    out._num_nodes = int(rows.shape[0])
    out.ptr, out.batch = nptr, cn
    out.node_ids = ids.to(dev)[rows]
    out.x = None if data.x is None else data.x.to(dev)[rows]
    out.uniform_node_ids = None
    out.edge_index, out.edge_attr = new_ei, new_ea
    counts = torch.bincount(cand, minlength=K)
    out.edge_ptr = torch.zeros(K + 1, **i64)
    out.edge_ptr[1:] = torch.cumsum(counts, 0)
    out.graph_sizes = (int(n_k.max()), int(counts.max())) if K else (0, 0)
    out.has_self_loops = None
    return out


# include/qot_gnn.h: QOT_TOPO_STATUS_*, the status bits of qot_topological_infer_status (above the other kernels' 1, 2, 4)
TOPO_STATUS_BAD_CONN, TOPO_STATUS_TOO_MANY, TOPO_STATUS_BAD_SAMPLE, TOPO_STATUS_BAD_ENDPOINT = 8, 16, 32, 64
TOPO_STATUS_MAX_FREQS = 1024    # include/qot_gnn.h: QOT_SG_MAX_FREQS
TOPO_STATUS_MAX_LINKS = 512     # csrc/infer_topological_status.hip: kTopoStatusLinks, two directed links per lightpath

_TopoStatus = namedtuple("_TopoStatus", "features S P L Q conn_row src_row dst_row")


def topological_status_args(status, edge_dim, features_to_consider=to_graph.DEFAULT_FEATURES, samples=None,
                            num_embeddings=None, model_device=None, who="TopologicalPredictor.from_status"):
    """The argument checks of ``TopologicalPredictor.from_status`` that need no device: returns a ``_TopoStatus`` (the
    feature list, the chunk's sizes, the ``lp_feat`` rows the kernel reads) or raises -- ``TypeError`` for a ``status`` that
    is no ``DeviceStatus``, ``IndexError`` for an embedding table (``num_embeddings`` rows) that does not hold the 75 nodes
    of the topology, ``ValueError`` naming the condition for everything else; a chunk on the CPU, then one on another
    device than ``model_device``, are named last."""
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    feats = list(features_to_consider)
    S, P, L, Q = (int(v) for v in status.data.shape)
    if Q > TOPO_STATUS_MAX_FREQS:
        raise ValueError(f"{who}: at most {TOPO_STATUS_MAX_FREQS} frequency slots per link, got {Q}")
    if L * Q >= 1 << 31:
        raise ValueError(f"{who}: links x frequency slots must stay below 2^31, got {L} x {Q}")
    if len(feats) != int(edge_dim):
        raise ValueError(f"{who}: {len(feats)} features, the model takes edge_dim = {edge_dim}")
    fi = status.feature_indexes
    missing = [n for n in feats + ["conn_id", "src_id", "dst_id"] if n not in fi]
    if missing:
        raise ValueError(f"{who}: the status has no lp_feat row named {', '.join(repr(n) for n in missing)}")
    if isinstance(samples, torch.Tensor) and (samples.dim() != 1 or samples.dtype != torch.int64):
        raise ValueError(f"{who}: samples must be a sequence or a 1-d int64 tensor, got {samples.dtype} "
                         f"{tuple(samples.shape)}")
    if num_embeddings is not None and int(num_embeddings) < to_graph.NUM_TOPOLOGY_NODES:
        raise IndexError("index out of range in self")
    if not status.data.is_cuda:
        raise ValueError(f"{who}: the status chunk is on the CPU; there is no CPU form of this call "
                         f"(NetworkStatus.to_device)")
    if model_device is not None and status.device != model_device:
        raise ValueError(f"{who}: the status chunk is on {status.device}, the model on {model_device}")
    return _TopoStatus(feats, S, P, L, Q, fi["conn_id"], fi["src_id"], fi["dst_id"])


# include/qot_gnn.h: QOT_TOPO_PLACE_*, the status bits qot_topological_infer_place adds beside QOT_TOPO_STATUS_*
TOPO_PLACE_BAD_CELL, TOPO_PLACE_OCCUPIED, TOPO_PLACE_CONN_TAKEN = 128, 256, 512
_TOPO_PLACE_CAUSES = (
    (TOPO_PLACE_BAD_CELL, "place: a link or frequency index outside the sample, or a cell_ptr slice that is empty, descending "
                          "or beyond the cells"),
    (TOPO_PLACE_OCCUPIED, "place: a cell whose channel is occupied in the sample"),
    (TOPO_PLACE_CONN_TAKEN, "place: a candidate's conn_id is a lightpath of the sample already"),
)

PLACE_MAX_RELEASE = 32          # include/qot_gnn.h: QOT_PLACE_MAX_RELEASE, released lightpaths per candidate
# include/qot_gnn.h: the status bits the two *_place_release entries (place with release=) add, the same two in both
TOPO_PLACE_NO_SUCH_CONN, TOPO_PLACE_BAD_RELEASE = 1024, 2048
LP_PLACE_NO_SUCH_CONN, LP_PLACE_BAD_RELEASE = 1024, 2048
_TOPO_RELEASE_CAUSES = (
    (TOPO_PLACE_NO_SUCH_CONN, "place: a released conn_id is no lightpath of the sample"),
    (TOPO_PLACE_BAD_RELEASE, f"place: a release_ptr slice that is descending, beyond the released conns or longer than "
                             f"{PLACE_MAX_RELEASE}"),
)
_LP_RELEASE_CAUSES = tuple((lp, text) for lp, (_, text) in zip((LP_PLACE_NO_SUCH_CONN, LP_PLACE_BAD_RELEASE),
                                                               _TOPO_RELEASE_CAUSES))

# release: the caller's int64 tensor; release_ptr: an int64 tensor, on the host checked and to be uploaded, or on the
# device and used in place
_PlaceRelease = namedtuple("_PlaceRelease", "R release release_ptr")


def place_release_args(status, K, release, release_ptr, who="place"):
    """The checks of ``release`` / ``release_ptr`` of both ``place`` methods and of ``materialise_placement`` that need no
    device, beside ``lightpath_place_args`` / ``topological_place_args`` (which give ``K``): returns ``None`` when both are
    ``None``, else a ``_PlaceRelease`` (``R``; ``release``; ``release_ptr`` as a 1-d int64 tensor, the caller's own where
    one was given) or raises ``ValueError`` naming the argument -- only one of the two given; ``release`` not a 1-d int64
    tensor on the chunk's device; ``release_ptr`` of the wrong length or dtype; a host ``release_ptr`` that is not
    non-decreasing from 0 to ``R`` or has a slice longer than ``PLACE_MAX_RELEASE`` (one on the device is checked by the
    kernel)."""
    def got(t):
        return f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__

    if release is None and release_ptr is None:
        return None
    if release is None or release_ptr is None:
        raise ValueError(f"{who}: release and release_ptr go together, got only "
                         f"{'release_ptr' if release is None else 'release'}")
    if not isinstance(release, torch.Tensor) or release.dim() != 1 or release.dtype != torch.int64:
        raise ValueError(f"{who}: release must be a 1-d int64 tensor of conn_id values, got {got(release)}")
    if release.device != status.data.device:
        raise ValueError(f"{who}: release is on {release.device}, the status chunk on {status.data.device}")
    R = int(release.shape[0])
    if isinstance(release_ptr, torch.Tensor):
        if release_ptr.dim() != 1 or release_ptr.dtype != torch.int64 or release_ptr.shape[0] != K + 1:
            raise ValueError(f"{who}: release_ptr must be a sequence or a 1-d int64 tensor of K + 1 = {K + 1} offsets into "
                             f"release, got {got(release_ptr)}")
    else:
        release_ptr = torch.tensor([int(v) for v in release_ptr], dtype=torch.int64).reshape(-1)
        if release_ptr.shape[0] != K + 1:
            raise ValueError(f"{who}: release_ptr must hold K + 1 = {K + 1} offsets into release, got {release_ptr.shape[0]}")
    if not release_ptr.is_cuda:                            # on the host: checked here; on the device: by the kernel
        if int(release_ptr[0]) != 0 or int(release_ptr[-1]) != R or (K and int(release_ptr.diff().min()) < 0):
            raise ValueError(f"{who}: release_ptr must be non-decreasing from 0 to R = {R}, got {release_ptr.tolist()}")
        if K and int(release_ptr.diff().max()) > PLACE_MAX_RELEASE:
            raise ValueError(f"{who}: candidate {int(release_ptr.diff().argmax())} releases "
                             f"{int(release_ptr.diff().max())} lightpaths, at most {PLACE_MAX_RELEASE}")
    return _PlaceRelease(R, release, release_ptr)


def _status_picks(samples, S, dev, who):
    """``samples`` of both ``from_status`` calls and of ``retest`` as ``(picks, G)``: ``None`` (all ``S``, in order), the
    caller's 1-d int64 tensor (used in place when it is on ``dev``) or a sequence (uploaded)."""
    if samples is None:
        return None, S
    if isinstance(samples, torch.Tensor):
        if samples.dim() != 1 or samples.dtype != torch.int64:
            raise ValueError(f"{who}: samples must be a sequence or a 1-d int64 tensor, got {samples.dtype} "
                             f"{tuple(samples.shape)}")
        picks = _i64(samples, dev)
    else:
        picks = torch.tensor([int(v) for v in samples], dtype=torch.int64).to(dev)
    return picks, int(picks.shape[0])


def _place_index_lists(dev, *lists):
    """The int64 index lists of a ``place`` call on ``dev``: those on the host go up in ONE copy, those on the device
    stay the caller's tensors."""
    host = [t for t in lists if not t.is_cuda]
    if host:
        up = iter(torch.cat(host).to(dev).split([int(t.shape[0]) for t in host]))
    return [_i64(t, dev) if t.is_cuda else next(up) for t in lists]


# samples / cell_ptr: int64 tensors, on the host checked (cell_ptr) and to be uploaded, or on the device and used in place
_TopoPlace = namedtuple("_TopoPlace", "status K M samples cell_ptr")


def topological_place_args(status, edge_dim, samples, values, cells, cell_ptr,
                           features_to_consider=to_graph.DEFAULT_FEATURES, num_embeddings=None, model_device=None,
                           who="TopologicalPredictor.place"):
    """The argument checks of ``TopologicalPredictor.place`` that need no device: returns a ``_TopoPlace`` (``status``:
    the ``_TopoStatus`` of ``topological_status_args``; ``K``, ``M``; ``samples`` and ``cell_ptr`` as 1-d int64 tensors) or
    raises -- ``TypeError`` for a ``status`` that is no ``DeviceStatus``; ``ValueError`` naming the argument for ``values``
    not float64 ``[K, P]``, ``cells`` not int64 ``[2, M]``, either on another device than the chunk, ``samples`` or
    ``cell_ptr`` of the wrong length or dtype, a host ``cell_ptr`` that is not non-decreasing from 0 to ``M`` or has an
    empty slice (one on the device is checked by the kernel); then everything ``topological_status_args`` refuses, a
    chunk on the CPU last."""
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    K, M, samples, cell_ptr = _place_lists(status, samples, values, cells, cell_ptr, who)
    sa = topological_status_args(status, edge_dim, features_to_consider, None, num_embeddings, model_device, who)
    return _TopoPlace(sa, K, M, samples, cell_ptr)


class _DeviceState:
    """What both predictors keep on the device beside the model: the status word their kernels flag a batch in and the
    ``outputs`` selections of ``sensitivity``.  ``_FLAGS`` of a predictor: its kernel's name, the meaning of the status bits."""

    def __init__(self):
        self._status = None
        self._outputs_dev = {}

    def _status_on(self, dev):
        if self._status is None or self._status.device != dev:
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)

    def _outputs(self, sel, dev):
        """``sel`` as a device int32 tensor: one upload per selection and device, none in later calls."""
        t = self._outputs_dev.get((tuple(sel), dev))
        if t is None:
            t = self._outputs_dev[(tuple(sel), dev)] = torch.tensor(sel, dtype=torch.int32, device=dev)
        return t

    def check_status(self):
        """Reads the kernels' status word (one device synchronisation): raises when a batch since the last check had an
        edge outside its graph's node range or indices / slices that disagree with its arrays (such rows are NaN)."""
        if self._status is None:
            return
        code = int(self._status.item())
        self._status.zero_()
        if code:
            causes = (tuple(getattr(self, "_CAUSES", ())) + tuple(getattr(self, "_PLACE_CAUSES", ()))
                      + tuple(getattr(self, "_RELEASE_CAUSES", ())) + tuple(getattr(self, "_RETEST_CAUSES", ())))
            named = "; ".join(text for bit, text in causes if code & bit)
            raise _lib.QotError("%s flagged the batch (status %d): %s%s" % (self._FLAGS[0], code, self._FLAGS[1],
                                                                           named and " -- here: " + named))


# what TopologicalPredictor._prepare hands to _launch: the model's shape, the batch on dev, its size bounds, the tables
_Prepared = namedtuple("_Prepared", "H D O dev ids ei ea ptr eptr n_max max_e B tables")


class TopologicalPredictor(_DeviceState):
    """``predictor(data) -> out [B, O]``: the EVAL-MODE forward of a two-layer ``TopologicalGNN`` as one kernel launch.

    ``model.training`` does not matter: the predictor always computes the eval-mode function (no dropout).  The result
    is a plain tensor without ``grad_fn`` on the model's device, bitwise reproducible, and a graph's row does not depend
    on the other graphs of the batch.  Against ``model.eval()(data)`` it agrees to fp32 rounding, not bit for bit (the
    sums run in another order).

    What depends on the parameters only (the projected embedding table, the score matrices of TransformerConv's graph
    form, the NNConv operand) is kept in the predictor and rebuilt, in one launch, when a parameter's storage or version
    counter has changed: an in-place optimizer step or ``load_state_dict`` is picked up by the next call.

    Envelope -- anything else raises ``ValueError`` naming the condition, there is no fallback: a model on the GPU with
    ``num_layers == 2``, hidden width 16 / 32 / 64 (not a zero-padded one), ``edge_dim <= 4``, at most 8 outputs; a batch
    in table mode (``data.x`` ``None`` or empty) whose graphs have at most 128 nodes and at most ``edge_cap(n_max,
    hidden, edge_dim)`` edges each.  ``node_ids`` outside the embedding table raise ``IndexError`` as the model does.

    ``predictor.sample(data, samples)``: Monte-Carlo dropout, ``samples`` stochastic forwards in one launch (see there).
    ``predictor.sensitivity(data)``: the output together with its Jacobian wrt the edge features, in one launch.
    ``predictor.what_if(data, ...)``: K small edits of the batch's graphs (edges added / removed), scored in one launch.
    ``predictor.from_status(status)``: ``__call__``'s rows straight from network-status samples, no graph in between, one
    launch and no host read (see there).
    ``predictor.place(status, samples, values, cells, cell_ptr)``: K candidate lightpaths, each placed into a status sample
    that does not hold it yet, scored in one launch without the edited samples (see there).
    """

    _FLAGS = ("qot_topological_infer", "bit 0 an edge leaves its graph's node range, bit 1 slices outside the arrays, "
                                       "bit 2 a node id outside the table (what_if: bit 0 also an added edge, bit 1 also a "
                                       "graph number or a drop position out of range; from_status: bit 3 a bad conn_id, "
                                       "bit 4 too many lightpaths, bit 5 a sample number out of range, bit 6 a bad "
                                       "src_id / dst_id; place: those, the candidate's values included, bit 7 a bad cell or "
                                       "cell_ptr slice, bit 8 an occupied cell, bit 9 a conn_id of the sample)")
    # the bits of qot_topological_infer_status, named when check_status() finds them: the device builder's own words
    _CAUSES = tuple((bit, next(t for b, t in to_graph._SG_CAUSES if b == sg)) for bit, sg in (
        (TOPO_STATUS_BAD_CONN, to_graph.SG_BAD_CONN), (TOPO_STATUS_TOO_MANY, to_graph.SG_TOO_MANY),
        (TOPO_STATUS_BAD_SAMPLE, to_graph.SG_BAD_SAMPLE), (TOPO_STATUS_BAD_ENDPOINT, to_graph.SG_BAD_ENDPOINT)))
    # ... and the bits qot_topological_infer_place adds, named by check_status() behind them
    _PLACE_CAUSES = _TOPO_PLACE_CAUSES
    # ... and the two of qot_topological_infer_place_release (place with release=), behind those
    _RELEASE_CAUSES = _TOPO_RELEASE_CAUSES

    def __init__(self, model):
        super().__init__()
        self.model = model
        self._tables = None
        self._tag = None
        self._topology = None           # from_status: (device, arange(75), an empty edge_index)
        self._check_model()

    # ------------------------------------------------------------------ envelope
    def _check_model(self, on_gpu=True):
        m = self.model
        if getattr(m, "num_layers", None) != 2 or not hasattr(m, "conv2") or not hasattr(m, "node_embeddings"):
            raise ValueError(f"TopologicalPredictor: num_layers must be 2 (TransformerConv + NNConv), got "
                             f"{getattr(m, 'num_layers', None)}")
        H = m.node_embeddings.embedding_dim
        if getattr(m, "_qot_hp", None) is not None:
            raise ValueError(f"TopologicalPredictor: a model that runs zero-padded (hidden width {H}) is not supported; "
                             f"hidden width must be one of {WIDTHS}")
        if H not in WIDTHS:
            raise ValueError(f"TopologicalPredictor: hidden width {H} is not supported; it must be one of {WIDTHS}")
        D = m.conv1.edge_dim
        if not 1 <= D <= MAX_EDGE_DIM:
            raise ValueError(f"TopologicalPredictor: edge_dim {D} is not supported; it must be 1 ... {MAX_EDGE_DIM}")
        O = m.mlp[3].out_features
        if not 1 <= O <= MAX_OUTPUTS or m.mlp[0].out_features != H:
            raise ValueError(f"TopologicalPredictor: out_channels {O} is not supported; it must be 1 ... {MAX_OUTPUTS}")
        if on_gpu and not m.node_embeddings.weight.is_cuda:
            raise ValueError("TopologicalPredictor: the model is on the CPU; move it to the GPU first (model.to('cuda'))")
        return H, D, O

    # ------------------------------------------------------------------ parameter-only tables
    def _params(self):
        m = self.model
        c1, c2 = m.conv1, m.conv2
        w1, b1, w2, b2 = c2._edge_mlp()
        return (m.node_embeddings.weight, c1.lin_query.weight, c1.lin_query.bias, c1.lin_key.weight, c1.lin_key.bias,
                c1.lin_value.weight, c1.lin_value.bias, c1.lin_skip.weight, c1.lin_skip.bias, c1.lin_edge.weight,
                w1, b1, w2, b2, c2.lin.weight, c2.bias, m.mlp[0].weight, m.mlp[0].bias, m.mlp[3].weight, m.mlp[3].bias)

    def _refresh(self, H, D):
        params = self._params()
        tag = tuple((p.data_ptr(), p._version) for p in params)
        if tag == self._tag:
            return self._tables
        (emb, wq, bq, wk, bk, wv, bv, ws, bs, we, w1, b1, w2, b2, wroot, bias2, w0, b0, w3, b3) = \
            (_f32c(p.detach()) for p in params)
        V, K = emb.shape[0], 2 * D
        if tuple(w1.shape) != (K, D):
            raise ValueError(f"TopologicalPredictor: the edge network's hidden layer must have 2 * edge_dim = {K} units")
        dev = emb.device
        lib = _lib.load()
        t4 = torch.empty(V, 4 * H, dtype=torch.float32, device=dev)
        ldm = int(lib.qot_tconv_graph_ldm(V))
        M = torch.empty(V, ldm, dtype=torch.float32, device=dev)
        Pm = torch.empty(V, D, dtype=torch.float32, device=dev)
        idx = wcat_index(H, K, dev)
        wcat = torch.empty(idx.numel(), dtype=torch.float32, device=dev)
        # three independent jobs of the existing kernels, one multi-role launch
        _lib.run_roles([
            _lib.make_role(_lib.ROLE_TABLE_PROJECT_FWD, (emb, wq, bq, wk, bk, wv, bv, ws, bs, t4, None, None), (V, H)),
            _lib.make_role(_lib.ROLE_TABLE_SCORES, (emb, wq, bq, wk, bk, we, M, Pm), (V, H, D)),
            _lib.make_role(_lib.ROLE_GATHER3, (w2, b2, wroot, idx, wcat), (w2.numel(), b2.numel(), idx.numel())),
        ])
        # the kernel reads the remaining parameters in place: the (contiguous fp32 views of the) tensors are held here
        self._tables = dict(t4=t4, M=M, ldm=ldm, P=Pm, V=V, wcat=wcat, we=we, w1=w1, b1=b1, bias2=bias2, w0=w0, b0=b0,
                            w3=w3, b3=b3)
        self._tag = tag
        return self._tables

    # ------------------------------------------------------------------ the batch
    def _slices(self, data, dev):
        """``(node_ids, edge_index, node_ptr, edge_ptr, n_max, max_e, B)``, remembered on the batch object.  A batch that
        carries ``ptr`` / ``edge_ptr`` / ``graph_sizes`` (ours do) costs no device read; otherwise the slices come from
        ``data.batch`` once per batch object."""
        ids, ei = data.node_ids, data.edge_index
        if ids is None:
            raise ValueError("TopologicalPredictor: data.node_ids is required (table mode)")
        tag = (ids.data_ptr(), ids._version, tuple(ids.shape), ei.data_ptr(), ei._version, tuple(ei.shape))
        c = _cache(data)
        if c is not None and "infer" in c and c["infer"][0] == tag:
            return c["infer"][1]
        ids, ei = _i64(ids, dev), _i64(ei, dev)
        ptr, eptr, B, n_max, max_e, exact = graph_slices(data, ei, ids.shape[0], dev, "TopologicalPredictor")
        res = (ids, ei, ptr, eptr, n_max, max_e, B, exact)
        if c is not None:
            c["infer"] = (tag, res)
        return res

    def _check_ids(self, data, ids, V, n_max):
        """The model's ``IndexError`` for an id outside the embedding table (``TopologicalGNN._check_node_ids``)."""
        if getattr(data, "uniform_node_ids", None):
            if n_max > V:
                raise IndexError("index out of range in self")
            return
        c = _cache(data)
        tag = (ids.data_ptr(), ids._version, tuple(ids.shape), V)
        if c is not None and c.get("infer_ids_ok") == tag:
            return
        if ids.numel() and not torch.cuda.is_current_stream_capturing():
            lo, hi = torch.aminmax(ids)
            if int(lo) < 0 or int(hi) >= V:
                raise IndexError("index out of range in self")
        if c is not None:
            c["infer_ids_ok"] = tag

    # ------------------------------------------------------------------ the call
    def _prepare(self, data, kind="eval"):
        """Everything a launch needs, checked, as a ``_Prepared``.  ``kind``: whose envelope holds -- the eval kernel's, the
        sampling kernel's (``"mc"``) or the sensitivity kernel's (``"grad"``); see ``_KINDS``."""
        H, D, O = self._check_model()
        m = self.model
        if data.x is not None and data.x.numel():
            raise ValueError("TopologicalPredictor: data.x is given; only table mode (node_ids into the embedding "
                             "table) is supported")
        dev = m.node_embeddings.weight.device
        ids, ei, ptr, eptr, n_max, max_e, B, exact = self._slices(data, dev)
        supported, _, which = _KINDS[kind]
        if n_max > MAX_NODES or not getattr(_lib.load(), supported)(n_max, max_e, H, D, O):
            n_max, max_e = exact()          # the carried sizes are bounds (a shard inherits its parent's): look once
            if n_max > MAX_NODES:
                raise ValueError(f"TopologicalPredictor: a graph of {n_max} nodes; at most {MAX_NODES} nodes per graph")
            cap = _edge_cap(kind, n_max, H, D)
            if max_e > cap:
                raise ValueError(f"TopologicalPredictor: a graph of {max_e} edges is above the {which}"
                                 f"edge cap {cap} for graphs of up to {n_max} nodes at hidden width {H}, edge_dim {D}")
        ea = data.edge_attr
        E = ei.shape[1]
        if ea is None or tuple(ea.shape) != (E, D):
            raise ValueError(f"TopologicalPredictor: edge_attr must be [{E}, {D}], got "
                             f"{None if ea is None else tuple(ea.shape)}")
        ea = _f32c(ea if ea.device == dev else ea.to(dev))
        t = self._refresh(H, D)
        self._check_ids(data, ids, t["V"], n_max)
        self._status_on(dev)
        return _Prepared(H, D, O, dev, ids, ei, ea, ptr, eptr, n_max, max_e, B, t)

    def _launch(self, name, p, out, *extra):
        """One launch of entry point ``name``: the arguments the three kernels share (``out`` among them), then ``extra``."""
        t = p.tables
        _lib.call(name, p.ids, p.ei, p.ea, p.ptr, p.eptr, p.ids.shape[0], p.ei.shape[1], p.B, p.n_max, p.max_e, t["t4"],
                  4 * p.H, t["M"], t["ldm"], t["P"], t["V"], t["we"], t["w1"], t["b1"], t["wcat"], t["bias2"], t["w0"], t["b0"],
                  t["w3"], t["b3"], 0.01, float(self.model.mlp[1].negative_slope), out, p.H, p.D, p.O, self._status, *extra)

    @torch.no_grad()
    def __call__(self, data):
        p = self._prepare(data)
        out = torch.empty(p.B, p.O, dtype=torch.float32, device=p.dev)
        self._launch("qot_topological_infer", p, out)
        return out

    @torch.no_grad()
    def sample(self, data, samples, *, p=None, seed=None, first_step=0, chunk=None, return_samples=False):
        """Monte-Carlo dropout: ``samples`` (T) stochastic forwards of the batch in ONE kernel launch; returns ``(mean [B,
        O], std [B, O])`` over the draws (``std`` unbiased), with ``return_samples=True`` also ``draws [T, B, O]``.

        Draw ``t`` is, by construction, the output of a train-mode forward of the engine on this batch at dropout step
        ``first_step + t`` with base seed ``seed``: the masks are the engine's pure function of ``(site seed, step, flat
        element index)`` (``include/qot_gnn.h``; ``oracle/dropout.py`` restates it), nothing is drawn from a generator.  A
        given ``(batch, seed, first_step, t)`` is therefore bitwise reproducible and does not depend on ``samples`` or
        ``chunk``.  The element index runs over the BATCH's activations, so a graph's draws depend on its row offset in the
        batch, as in training: ``__call__``'s batch independence does NOT extend to ``sample``.  With ``p == 0`` every draw
        equals ``self(data)`` bit for bit.

        ``p``: dropout probability of all three sites, or a ``(convolutions, read-out)`` pair; ``None`` takes
        ``model.dropout.p`` and ``model.mlp[2].p`` (a model built for testing has 0 there).  ``seed``: ``None`` takes the
        model's base seed.  ``chunk``: samples per workgroup (grid ``(B, ceil(T / chunk))``); ``None`` asks ``mc_chunk`` with
        the device's compute-unit count.

        Pure: ``model.training``, the model's dropout counter, its parameters and the tables ``__call__`` relies on are not
        touched; parameter updates are followed as ``__call__`` follows them.  Refusals (``ValueError`` naming the condition):
        everything ``__call__`` refuses, ``p`` outside ``[0, 1)``, ``samples`` outside ``2 ... 4096``, ``chunk`` outside ``1 ...
        samples``, ``first_step < 0`` or ``first_step + samples > 2^63``, a graph above ``mc_edge_cap`` (lower than the eval
        kernel's: DESIGN.md 4.15).  ``IndexError`` and ``check_status()`` as ``__call__``."""
        m = self.model
        T, p_conv, p_head, chunk, first_step = mc_args(samples, p, chunk, first_step,
                                                        (getattr(getattr(m, "dropout", None), "p", 0.0),
                                                         getattr(m.mlp[2], "p", 0.0) if hasattr(m, "mlp") else 0.0))
        prep = self._prepare(data, "mc")
        base = (m._seed() if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        if chunk is None:
            chunk = mc_chunk(prep.B, T, torch.cuda.get_device_properties(prep.dev).multi_processor_count)
        draws = torch.empty(T, prep.B, prep.O, dtype=torch.float32, device=prep.dev)
        self._launch("qot_topological_infer_mc", prep, draws, T, first_step, base, p_conv, p_head, chunk)
        mean, std = draws.mean(0), draws.std(0, unbiased=True)
        return (mean, std, draws) if return_samples else (mean, std)

    @torch.no_grad()
    def sensitivity(self, data, outputs=None, *, return_attention_weights=False):
        """The per-link sensitivity of the prediction in ONE kernel launch: returns ``(out [B, O], jac [Q, E, D])`` with
        ``jac[q, e, :] = d out[graph(e), outputs[q]] / d edge_attr[e, :]`` of the EVAL-MODE function -- what
        ``model.eval()(data)[:, o].sum().backward()`` leaves in ``edge_attr.grad``, for every requested output at once
        (graphs are block-diagonal: this is the whole Jacobian).  ``out`` is ``self(data)`` bit for bit.

        ``outputs``: ``None`` (all, in order) or a non-empty list of distinct integers in ``0 ... O - 1``.
        ``return_attention_weights=True``: also ``(edge_index, alpha [E, 1])``, conv1's softmax weights in the order of
        ``data.edge_index`` -- what ``model(data, return_attention_weights=True)`` returns.

        Plain tensors without ``grad_fn``, bitwise reproducible; a graph's slices of ``jac`` and ``alpha`` do not depend on
        the other graphs of the batch (no atomics: every sum has one owner and a fixed order).  The derivative of
        ``leaky_relu`` / ``relu`` at 0 is torch's.  Pure: no model state is touched; parameter updates are followed as
        ``__call__`` follows them.  Refusals, ``IndexError`` and ``check_status()`` as ``__call__`` (a flagged graph has NaN in
        its ``out`` row, its ``jac`` slice and its ``alpha`` slice), with a lower edge cap: ``grad_edge_cap`` (DESIGN.md
        4.16)."""
        # the model's shape, then the argument, are named before the model's device and the batch are looked at
        sel = grad_outputs(outputs, self._check_model(on_gpu=False)[2])
        p = self._prepare(data, "grad")
        E, Q, dev = p.ei.shape[1], len(sel), p.dev
        out = torch.empty(p.B, p.O, dtype=torch.float32, device=dev)
        jac = torch.empty(Q, E, p.D, dtype=torch.float32, device=dev)
        alpha = torch.empty(E, 1, dtype=torch.float32, device=dev) if return_attention_weights else None
        self._launch("qot_topological_infer_grad", p, out, self._outputs(sel, dev), Q, jac, alpha)
        if return_attention_weights:
            return out, jac, (data.edge_index, alpha)
        return out, jac

    @torch.no_grad()
    def what_if(self, data, add_edge_index, add_edge_attr, add_ptr, drop=None, drop_ptr=None, graph=None):
        """"What if": scores K small edits of the batch's graphs in ONE kernel launch, ``out [K, O]``, without building
        the edited graphs.  ``out[k]`` is, bit for bit, row ``k`` of ``self(materialise_what_if(data, ...))`` -- see there
        for the definition: candidate ``k`` names base graph ``graph[k]``, removes the edges at positions
        ``drop[drop_ptr[k]:drop_ptr[k + 1]]`` of ``data.edge_index`` and appends ``add_edge_index[:, add_ptr[k]:add_ptr[k +
        1]]`` (batch node numbering) with the rows of ``add_edge_attr``; the edited graph holds the base graph's nodes, its
        surviving edges in their order and the added edges behind them.  A candidate's row does not depend on the other
        candidates, and one without an edit equals ``self(data)[graph[k]]``.  The graphs are directed: a candidate
        lightpath of an undirected network graph is its TWO directed edges (set-up: add both; tear-down: drop both; re-route:
        both).

        ``add_edge_index [2, A]`` int64, ``add_edge_attr [A, D]``, ``add_ptr [K + 1]`` (an empty slice is legal); ``drop [R]``
        int64 with ``drop_ptr [K + 1]``, both or neither (any order within a candidate, a repeat counts once, at most
        ``WHAT_IF_MAX_DROP`` = 32 per candidate); ``graph [K]`` int64, ``None`` only for a base batch of one graph.  Hand
        ``add_ptr`` / ``drop_ptr`` over as lists or host tensors: they are checked on the host, a device tensor costs one read
        each.  Nothing else is read back from the device.

        Plain tensor without ``grad_fn``; pure (no model state is touched); parameter updates are followed as ``__call__``
        follows them.  Refusals (``ValueError`` naming the condition, before any launch): everything ``__call__`` refuses,
        pointer arrays not non-decreasing from 0 to A (R), ``add_edge_attr`` not ``[A, D]``, ``drop`` without ``drop_ptr`` or the
        reverse, ``graph=None`` with B != 1, more than 32 removals in one candidate, a candidate whose ``edges of its graph +
        its additions`` exceed ``what_if_edge_cap(n_max, hidden, edge_dim)`` (the eval kernel's cap; removals are not
        credited.  The bound ``largest graph + most additions`` is tried first; only when that fails are the candidates'
        own sums read, once).  On the device: an added edge with an endpoint outside its graph (status bit 0), a ``graph[k]``
        outside ``0 ... B - 1`` or a drop position outside that graph's edge slice (bit 1) give NaN in that candidate's row
        only, and ``check_status()`` raises."""
        who = "TopologicalPredictor.what_if"
        # the arguments are named before the model's device and the batch are looked at
        H, D, O = self._check_model(on_gpu=False)
        w = what_if_args(D, add_edge_index, add_edge_attr, add_ptr, drop, drop_ptr, graph, _num_graphs_hint(data), who)
        p = self._prepare(data)
        if graph is None and p.B != 1:
            raise ValueError(f"{who}: graph=None needs a base batch of exactly one graph, this one has {p.B}")
        dev, K = p.dev, w.K
        out = torch.empty(K, O, dtype=torch.float32, device=dev)
        if K == 0:
            return out
        if p.B == 0:
            raise ValueError(f"{who}: {K} candidates, but the base batch has no graph")

        def on_dev(given, host):
            if isinstance(given, torch.Tensor) and given.device == dev:
                return _i64(given, dev)
            return host.to(dev)
        add_ptr_d = on_dev(add_ptr, w.add_ptr)
        g = None if graph is None else _i64(graph, dev)
        max_e, cap = p.max_e, _edge_cap("whatif", p.n_max, H, D)
        if max_e + w.max_add > cap:
            # the bound fails: look at the candidates' own sums (one read); a graph number out of range is the kernel's to flag
            m = p.eptr[1:] - p.eptr[:-1]
            worst = int((m[g.clamp(0, p.B - 1)] if g is not None else m[:1]).add(add_ptr_d.diff()).max())
            if worst > cap:
                raise ValueError(f"{who}: a candidate of {worst} edges (its graph's and its additions; removals are not "
                                 f"credited) is above the what-if edge cap {cap} for graphs of up to {p.n_max} nodes at "
                                 f"hidden width {H}, edge_dim {D}")
            max_e = worst - w.max_add
        aei = _i64(add_edge_index, dev)
        aea = _f32c(add_edge_attr if add_edge_attr.device == dev else add_edge_attr.to(dev))
        dpos = dptr = None
        if w.R:
            dpos, dptr = _i64(drop, dev), on_dev(drop_ptr, w.drop_ptr)
        self._launch("qot_topological_infer_whatif", p._replace(max_e=max_e), out, aei, aea, add_ptr_d, w.A, dpos, dptr, w.R,
                     g, K, w.max_add)
        return out

    @torch.no_grad()
    def from_status(self, status, samples=None, features_to_consider=to_graph.DEFAULT_FEATURES):
        """The QoT of network-status samples, straight from the samples: ``(out [G, O] float32, links [G] int64)`` in ONE
        kernel launch (``csrc/infer_topological_status.hip``), without the graphs in between, with nothing read back, legal
        inside ``torch.cuda.graph`` capture.

        ``status``: a ``to_graph.DeviceStatus`` on the model's device.  ``samples``: ``None`` (all, in order), a sequence
        of sample numbers (uploaded) or a 1-d int64 device tensor (used in place: the form to capture); a repeated number
        is allowed and gives equal rows.  ``features_to_consider`` as ``to_graph.device_batch``.

        The definition is what the tree computes already: with ``batch = to_graph.device_batch(status, "topological",
        features_to_consider, samples)``, ``out`` is ``self(batch)`` bit for bit and ``links[g]`` is ``batch.edge_ptr[g + 1] -
        batch.edge_ptr[g]``, the directed links of sample ``g``'s graph: 75 nodes, one link pair per unordered node pair
        that some lightpath joins (a lightpath from a node to itself: one self loop), with the features of the pair's
        lightpath of largest ``conn_id``.  ``to_graph.topological_links`` states the selection on the host.  A sample's row
        depends on that sample alone; ``model.training`` does not matter; parameter updates are followed as ``__call__``
        follows them.

        Refusals before any launch: ``TypeError`` for a ``status`` that is no ``DeviceStatus``; ``ValueError`` naming the
        condition for everything ``_check_model`` refuses, ``len(features_to_consider) != edge_dim``, a feature or
        ``conn_id`` / ``src_id`` / ``dst_id`` missing from ``lp_feat``, more than 1024 frequency slots, ``L * Q >= 2^31``, a
        ``samples`` tensor that is not 1-d int64, a chunk on the CPU or on another device than the model; ``IndexError``
        when the embedding table has fewer than 75 rows, as the model raises.  ``G == 0`` gives empty tensors without a
        launch.  On the device, since nothing is read back: a ``conn_id`` that is not finite or beyond +-2^53, more than
        256 lightpaths in a sample, a sample number outside the chunk, a ``src_id`` / ``dst_id`` that is no integer in
        1 ... 75 -- that sample's row is NaN and its ``links`` 0, the other rows are untouched, and ``check_status()``
        raises naming the cause.  (The column table of a feature list, ``arange(75)`` and the parameter tables are uploaded
        by the first call with a chunk: make that call before capturing.)"""
        who = "TopologicalPredictor.from_status"
        H, D, O = self._check_model()
        emb = self.model.node_embeddings.weight
        dev = emb.device
        sa = topological_status_args(status, D, features_to_consider, samples, emb.shape[0], dev, who)
        picks, G = _status_picks(samples, sa.S, dev, who)          # (a tensor's dtype: topological_status_args has refused)
        out = torch.empty(G, O, dtype=torch.float32, device=dev)
        links = torch.empty(G, dtype=torch.int64, device=dev)
        if G == 0:
            return out, links
        self._launch_status("qot_topological_infer_status", status, sa, (H, D, O), out, links, picks)
        return out, links

    def _launch_status(self, name, status, sa, shape, out, links, picks, *extra):
        """One launch of a status entry point (``from_status``, ``place``): the 75 nodes of the topology in place of a
        batch, ``out.shape[0]`` rows, the sample arguments of ``sa``, then ``extra``."""
        H, D, O = shape
        dev = out.device
        if self._topology is None or self._topology[0] != dev:
            self._topology = (dev, torch.arange(to_graph.NUM_TOPOLOGY_NODES, dtype=torch.int64, device=dev),
                              torch.empty(2, 0, dtype=torch.int64, device=dev))
        _, ids, no_edges = self._topology
        t = self._refresh(H, D)
        self._status_on(dev)
        cols, _, ncol = to_graph._column_tables(status, "topological", sa.features)
        p = _Prepared(H, D, O, dev, ids, no_edges, None, None, None, to_graph.NUM_TOPOLOGY_NODES, TOPO_STATUS_MAX_LINKS,
                      int(out.shape[0]), t)
        self._launch(name, p, out, links, status.data, picks, sa.S, sa.P, sa.L, sa.Q, sa.conn_row, sa.src_row, sa.dst_row,
                     cols, ncol, *extra)

    @torch.no_grad()
    def place(self, status, samples, values, cells, cell_ptr, features_to_consider=to_graph.DEFAULT_FEATURES, *,
              release=None, release_ptr=None):
        """Routing and spectrum assignment with the topological model: scores K candidate assignments of a NEW lightpath
        against the status samples of the established ones, ``(out [K, O] float32, links [K] int64)`` in ONE kernel
        launch (``csrc/infer_topological_place.hip``), without the edited samples or their graphs, with nothing read
        back, legal inside ``torch.cuda.graph`` capture.

        ``status``, ``samples``, ``values [K, P]`` float64, ``cells [2, M]`` int64 and ``cell_ptr`` have the meaning and
        the accepted forms they have in ``LightpathPredictor.place``: candidate ``k`` is the raw ``lp_feat`` vector
        ``values[k]`` (``conn_id``, ``src_id``, ``dst_id``, the features, in status units) written into the channels
        ``cells[:, cell_ptr[k]:cell_ptr[k + 1]]`` of sample ``samples[k]``; ``status.data`` is never written.  There is no
        ``freq_threshold`` (the topological graph has no interference rule) and ``osnr`` / ``snr`` / ``ber`` are not read.

        ``materialise_placement`` is the definition: with ``edited`` its K samples, ``out`` is
        ``self.from_status(edited, features_to_consider=...)[0]`` bit for bit and ``links`` that call's ``links`` -- hence
        both equal ``self(to_graph.device_batch(edited, "topological", ...))`` as well.  The candidate joins the pair
        contest: when its ``trunc(conn_id)`` is larger than the conn of every lightpath of the sample on the same
        unordered node pair, or the pair is new (``links`` grows by 2, by 1 for a self loop), the pair's links carry the
        candidate's scaled features; otherwise the edited graph is the unedited one and the row is
        ``self.from_status(status, samples)[0][k]``.  The cells do not enter the graph: they decide only whether the
        placement is legal.  ``to_graph.placement_links`` states the links and the outcome on the host.  A candidate's
        row depends on its sample and itself alone; every candidate rescans its sample, O(L Q + cells): candidates of
        one sample do not share the scan.

        Refusals before any launch (``topological_place_args``): ``TypeError`` for a ``status`` that is no
        ``DeviceStatus``; ``ValueError`` for ``values`` not float64 ``[K, P]``, ``cells`` not int64 ``[2, M]``, ``samples``
        or ``cell_ptr`` of the wrong length or dtype, a host ``cell_ptr`` that is not non-decreasing from 0 to M or has an
        empty slice, then everything ``from_status`` refuses.  ``K == 0`` gives empty tensors without a launch.  On the
        device, since nothing is read back: a cell outside the sample or a bad ``cell_ptr`` slice, an occupied cell, a
        ``conn_id`` the sample holds already, a ``conn_id`` that is not finite or beyond +-2^53, a ``src_id`` / ``dst_id``
        that is no integer in 1 ... 75 (an all-zero ``values`` row falls here), a sample that holds 256 lightpaths
        already, a sample number outside the chunk -- that candidate's row is NaN and its ``links`` 0, the other rows are
        untouched, and ``check_status()`` raises naming the cause.  (The column table of a feature list, ``arange(75)``
        and the parameter tables are uploaded by the first call with a chunk: make that call before capturing.)

        ``release [R]`` (int64, on the chunk's device) with ``release_ptr`` (K + 1 offsets, a host sequence or an int64
        device tensor, as ``cell_ptr``): a REROUTE, or an admission together with a tear-down, in the same launch
        (``csrc/infer_topological_place_release.hip``).  Candidate ``k`` first releases the lightpaths of
        its sample whose ``trunc(conn_id)`` is in ``release[release_ptr[k]:release_ptr[k + 1]]`` -- an empty slice and a conn
        named twice are allowed, at most ``PLACE_MAX_RELEASE = 32`` -- and is then placed;
        ``materialise_placement(..., release=, release_ptr=)`` is the definition as above.  A released lightpath contests
        no pair (the pair goes to the largest surviving conn, to the candidate, or disappears), frees its channels for the
        candidate's cells, may have any ``src_id`` / ``dst_id``, and the candidate may carry its ``conn_id``; a sample of
        256 lightpaths is accepted when at least one is released.  ``to_graph.placement_links(release=)`` states the
        links on the host.  More refusals: before any launch (``place_release_args``) only one of the two given,
        ``release`` not a 1-d int64 tensor on the chunk's device, ``release_ptr`` of the wrong length or dtype, a host
        ``release_ptr`` not non-decreasing from 0 to R or with a slice longer than 32; on the device a released conn the
        sample does not hold and a bad slice of a device ``release_ptr``.  Without the two keywords the call is the one
        above, through the same C entry."""
        who = "TopologicalPredictor.place"
        H, D, O = self._check_model()
        emb = self.model.node_embeddings.weight
        dev = emb.device
        pa = topological_place_args(status, D, samples, values, cells, cell_ptr, features_to_consider, emb.shape[0], dev, who)
        ra = place_release_args(status, pa.K, release, release_ptr, who)
        out = torch.empty(pa.K, O, dtype=torch.float32, device=dev)
        links = torch.empty(pa.K, dtype=torch.int64, device=dev)
        if pa.K == 0:
            return out, links
        picks, ptr, *rptr = _place_index_lists(dev, pa.samples, pa.cell_ptr, *(() if ra is None else (ra.release_ptr,)))
        name, extra = "qot_topological_infer_place", ()
        if ra is not None:
            name, extra = "qot_topological_infer_place_release", (ra.release.contiguous(), rptr[0], ra.R)
        self._launch_status(name, status, pa.status, (H, D, O), out, links, picks, values.contiguous(), cells.contiguous(), ptr,
                            pa.M, *extra)
        return out, links


# ====================================================================== LightpathGNN
LP_MAX_FEATURES = 16            # csrc/infer_lightpath_dev.hpp: kLpMaxF (all three kernels)
LP_MAX_HIDDEN = 256             # kLpMaxC
LP_MAX_OUTPUTS = 8              # kLpMaxO; also the most outputs one sensitivity call differentiates (Q <= O)
LP_HEADS = 4                    # kLpHeads: the columns of alpha_self / alpha_edge


class EnvelopeError(ValueError):
    """A model or a batch outside what ``LightpathPredictor`` runs; there is no other path behind it.  (A LUT-less batch is
    NOT one: that is the model's own ``ValueError``.)"""


_LpWhatIf = namedtuple("_LpWhatIf", "K A R add_ptr drop_ptr")


def lightpath_what_if_args(num_features, x_lut=None, add_src=None, add_ptr=None, drop=None, drop_ptr=None, node=None,
                           who="LightpathPredictor.what_if"):
    """The argument checks of ``LightpathPredictor.what_if`` (and of ``materialise_lightpath_what_if``) that need no
    device: returns ``(K, A, R, add_ptr, drop_ptr)`` with the pointer arrays as int64 host tensors (``None`` where the
    list is not given), or raises the named ``ValueError``.  ``K`` is the candidate count the arguments agree on, ``None``
    when none of them states one (the caller takes the number of LUT rows)."""
    F = int(num_features)

    def shape_of(t):
        return tuple(t.shape) if isinstance(t, torch.Tensor) else t

    def index_list(t, name, what):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype.is_floating_point or t.dtype.is_complex \
                or t.dtype == torch.bool:
            raise ValueError(f"{who}: {name} must be a 1-d integer tensor of {what}, got {shape_of(t)!r}"
                             f"{' of ' + str(t.dtype) if isinstance(t, torch.Tensor) else ''}")

    counts = []                                            # (the argument that states a candidate count, the count)
    if x_lut is not None:
        if not isinstance(x_lut, torch.Tensor) or x_lut.dim() != 2 or x_lut.shape[1] != F or x_lut.dtype != torch.float32:
            raise ValueError(f"{who}: x_lut must be a float32 tensor [K, {F}] (one feature row per candidate), got "
                             f"{shape_of(x_lut)!r}{' of ' + str(x_lut.dtype) if isinstance(x_lut, torch.Tensor) else ''}")
        counts.append(("x_lut", x_lut.shape[0]))
    if node is not None:
        index_list(node, "node", "node numbers of the batch, one per candidate")
        counts.append(("node", node.shape[0]))
    if (add_src is None) != (add_ptr is None):
        raise ValueError(f"{who}: add_src and add_ptr must be given together (got only "
                         f"{'add_ptr' if add_src is None else 'add_src'})")
    if (drop is None) != (drop_ptr is None):
        raise ValueError(f"{who}: drop and drop_ptr must be given together (got only "
                         f"{'drop_ptr' if drop is None else 'drop'})")
    A, ap, R, dp = 0, None, 0, None
    if add_src is not None:
        index_list(add_src, "add_src", "source node numbers of the batch")
        A = add_src.shape[0]
        ap = _host_ptr(add_ptr, "add_ptr", A, who)
        counts.append(("add_ptr", ap.numel() - 1))
    if drop is not None:
        index_list(drop, "drop", "positions into data.edge_index")
        R = drop.shape[0]
        dp = _host_ptr(drop_ptr, "drop_ptr", R, who)
        counts.append(("drop_ptr", dp.numel() - 1))
    K = counts[0][1] if counts else None
    for name, k in counts[1:]:
        if k != K:
            raise ValueError(f"{who}: {counts[0][0]} names {K} candidates, {name} {k}")
    if dp is not None and dp.numel() > 1:
        worst = int(dp.diff().max())
        if worst > WHAT_IF_MAX_DROP:
            raise ValueError(f"{who}: a candidate removes {worst} edges; at most WHAT_IF_MAX_DROP = {WHAT_IF_MAX_DROP}")
    return _LpWhatIf(K, A, R, ap, dp)


def materialise_lightpath_what_if(data, lut_col, x_lut=None, add_src=None, add_ptr=None, drop=None, drop_ptr=None, node=None):
    """The explicit batch of the K candidate graphs that ``LightpathPredictor.what_if`` scores: the DEFINITION of that call
    and what it saves.  Returns ``(batch, node_new)``; ``predict.what_if(...)[0][k]`` is, bit for bit, the row of
    ``predict(batch)`` that belongs to node ``node_new[k]`` (``torch.searchsorted(model._lut_rows(batch), node_new)`` finds
    it).  Pure torch, no kernel of ours; works on CPU tensors as well.

    ``data``: the base batch (``x [N, F]``); ``lut_col``: the model's ``is_lut_index``.  Candidate ``k`` is about node
    ``node[k]`` of the batch (``None``: the LUT rows ``x[:, lut_col] == 1.0`` in node order, candidate ``k`` is row ``k``) and
    its graph ``batch[node[k]]``.  Graph ``k`` of the result is a copy of that graph's nodes with the node's feature row
    replaced by ``x_lut[k]`` (``None``: kept), its edges less those at the positions ``drop[drop_ptr[k]:drop_ptr[k + 1]]`` of
    ``data.edge_index`` (any order, a repeat counts once; they must lie in that graph's edge slice) in their order, and
    behind them the edges ``(add_src[j], node[k])`` for ``j`` in ``add_ptr[k] ... add_ptr[k + 1]`` in the order given (sources
    in the batch's node numbering, inside that graph), all renumbered to the candidate's own block.  ``node_new[k]`` is the
    candidate's node in the new numbering.  The result carries ``x``, ``batch``, ``ptr`` and ``edge_ptr``.  Bad arguments,
    a node outside ``0 ... N - 1``, a drop position outside its graph's slice, an added source outside its graph or an
    effective feature row without ``1.0`` in column ``lut_col`` raise ``ValueError``."""
    from .batch import Batch
    who = "materialise_lightpath_what_if"
    x = getattr(data, "x", None)
    if x is None or x.dim() != 2:
        raise ValueError(f"{who}: data.x must be [N, F]")
    N, F = x.shape
    lut_col = int(lut_col)
    if not 0 <= lut_col < F:
        raise ValueError(f"{who}: lut_col {lut_col} is not a column of {F} features")
    w = lightpath_what_if_args(F, x_lut, add_src, add_ptr, drop, drop_ptr, node, who)
    dev = x.device
    ei = _i64(data.edge_index, dev)
    E = ei.shape[1]
    ptr, eptr, B, _, _, _ = graph_slices(data, ei, N, dev, who)
    i64 = dict(dtype=torch.int64, device=dev)
    if node is None:
        nd = (x[:, lut_col] == 1.0).nonzero().squeeze(1)
        if w.K is not None and w.K != nd.shape[0]:
            raise ValueError(f"{who}: the arguments name {w.K} candidates, the batch has {nd.shape[0]} LUT rows "
                             f"(node=None: candidate k is LUT row k)")
    else:
        nd = _i64(node, dev)
        if nd.numel() and (int(nd.min()) < 0 or int(nd.max()) >= N):
            raise ValueError(f"{who}: node must lie in 0 ... {N - 1}")
    K = nd.shape[0]
    g = torch.bucketize(nd, ptr[1:], right=True)           # the graph of every candidate's node
    ar = torch.arange(K, **i64)
    n_k, m_k = (ptr[1:] - ptr[:-1])[g], (eptr[1:] - eptr[:-1])[g]
    nptr = torch.zeros(K + 1, **i64)
    nptr[1:] = torch.cumsum(n_k, 0)
    bptr = torch.zeros(K + 1, **i64)                       # the base edges of every candidate, dropped ones included
    bptr[1:] = torch.cumsum(m_k, 0)
    # nodes: candidate c's block is its base graph's rows, its own row replaced
    cn = torch.repeat_interleave(ar, n_k)
    rows = ptr[g][cn] + (torch.arange(cn.shape[0], **i64) - nptr[cn])
    shift = nptr[:-1] - ptr[g]                             # batch node number -> the candidate's block
    node_new = nd + shift
    new_x = x[rows].clone()
    if x_lut is not None:
        new_x[node_new] = x_lut.to(device=dev, dtype=x.dtype)
    if K and not bool((new_x[node_new, lut_col] == 1.0).all()):
        raise ValueError(f"{who}: a candidate's feature row does not hold 1.0 in the LUT column {lut_col}")
    # base edges: every position of the base graph's slice, less the dropped ones
    ce = torch.repeat_interleave(ar, m_k)
    pos = eptr[g][ce] + (torch.arange(ce.shape[0], **i64) - bptr[ce])
    if w.R:
        dpos = _i64(drop, dev)
        cd = torch.repeat_interleave(ar, w.drop_ptr.to(dev).diff())
        if bool(((dpos < eptr[g][cd]) | (dpos >= eptr[g + 1][cd])).any()):
            raise ValueError(f"{who}: a drop position lies outside its candidate's base graph")
        keep = ~torch.isin(ce * max(E, 1) + pos, cd * max(E, 1) + dpos)
        ce, pos = ce[keep], pos[keep]
    # added edges: (source, the candidate's node)
    ca = torch.zeros(0, **i64)
    aei = torch.zeros(2, 0, **i64)
    if w.A:
        ca = torch.repeat_interleave(ar, w.add_ptr.to(dev).diff())
        src = _i64(add_src, dev)
        if bool(((src < ptr[g][ca]) | (src >= ptr[g + 1][ca])).any()):
            raise ValueError(f"{who}: an added source lies outside its candidate's base graph")
        aei = torch.stack([src + shift[ca], node_new[ca]])
    cand = torch.cat([ce, ca])
    order = torch.argsort(cand, stable=True)               # per candidate: survivors in their order, then the additions
    out = Batch()
    out.num_graphs = K
    out._num_nodes = int(rows.shape[0])
    out.ptr, out.batch = nptr, cn
    out.x = new_x
    out.uniform_node_ids = None
    out.edge_index = torch.cat([ei[:, pos] + shift[ce], aei], 1)[:, order]
    counts = torch.bincount(cand, minlength=K)
    out.edge_ptr = torch.zeros(K + 1, **i64)
    out.edge_ptr[1:] = torch.cumsum(counts, 0)
    out.graph_sizes = (int(n_k.max()), int(counts.max())) if K else (0, 0)
    out.has_self_loops = None
    return out, node_new


LP_STATUS_MAX_FREQS = 1024      # include/qot_gnn.h: QOT_SG_MAX_FREQS
# include/qot_gnn.h: QOT_LP_STATUS_*, the status bits of qot_lightpath_infer_status (above the other kernels' 1, 2, 4)
LP_STATUS_BAD_CONN, LP_STATUS_TOO_MANY, LP_STATUS_BAD_SAMPLE = 8, 16, 32

_LpStatus = namedtuple("_LpStatus", "features S P L Q conn_row osnr_row snr_row ber_row freq_threshold")


def lightpath_status_args(status, in_channels, is_lut_index, features_to_consider=to_graph.DEFAULT_FEATURES,
                          freq_threshold=0.05, who="LightpathPredictor.from_status"):
    """The argument checks of ``LightpathPredictor.from_status`` that need no device: returns an ``_LpStatus`` (the feature
    list, the chunk's sizes, the ``lp_feat`` rows the kernel reads, the threshold as a float) or raises -- ``TypeError`` for
    a ``status`` that is no ``DeviceStatus``, ``ValueError`` for a threshold that is no finite positive number,
    ``EnvelopeError`` naming the condition for everything else; a chunk on the CPU is named last."""
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    thr = freq_threshold
    if isinstance(thr, bool) or not isinstance(thr, (int, float)) or not 0.0 < float(thr) < float("inf"):
        raise ValueError(f"{who}: freq_threshold must be a finite positive number, got {thr!r}")
    feats = list(features_to_consider)
    S, P, L, Q = (int(v) for v in status.data.shape)
    if Q > LP_STATUS_MAX_FREQS:
        raise EnvelopeError(f"{who}: at most {LP_STATUS_MAX_FREQS} frequency slots per link, got {Q}")
    if L * Q >= 1 << 31:
        raise EnvelopeError(f"{who}: links x frequency slots must stay below 2^31, got {L} x {Q}")
    if len(feats) + 1 != int(in_channels):
        raise EnvelopeError(f"{who}: {len(feats)} features + is_lut are {len(feats) + 1} columns, the model takes "
                            f"in_channels = {in_channels}")
    if "is_lut" in feats:
        raise EnvelopeError(f"{who}: is_lut is not a feature of the status; the column is added to features_to_consider")
    col = sorted(feats + ["is_lut"]).index("is_lut")
    if col != int(is_lut_index):
        raise EnvelopeError(f"{who}: is_lut is column {col} of the sorted feature names, the model's is_lut_index is "
                            f"{is_lut_index}")
    fi = status.feature_indexes
    missing = [n for n in feats + ["conn_id", "osnr", "snr", "ber"] if n not in fi]
    if missing:
        raise EnvelopeError(f"{who}: the status has no lp_feat row named {', '.join(repr(n) for n in missing)}")
    if not status.data.is_cuda:
        raise EnvelopeError(f"{who}: the status chunk is on the CPU; there is no CPU form of this call "
                            f"(NetworkStatus.to_device)")
    return _LpStatus(feats, S, P, L, Q, fi["conn_id"], fi["osnr"], fi["snr"], fi["ber"], float(thr))


# include/qot_gnn.h: QOT_LP_PLACE_*, the status bits qot_lightpath_infer_place adds beside QOT_LP_STATUS_*
LP_PLACE_BAD_CELL, LP_PLACE_OCCUPIED, LP_PLACE_CONN_TAKEN, LP_PLACE_NOT_LUT = 64, 128, 256, 512
_LP_PLACE_CAUSES = (
    (LP_PLACE_BAD_CELL, "place: a link or frequency index outside the sample, or a cell_ptr slice that is empty, descending "
                        "or beyond the cells"),
    (LP_PLACE_OCCUPIED, "place: a cell whose channel is occupied in the sample"),
    (LP_PLACE_CONN_TAKEN, "place: a candidate's conn_id is a lightpath of the sample already"),
    (LP_PLACE_NOT_LUT, "place: a candidate's values without osnr == snr == ber == -1"),
)

# samples / cell_ptr: int64 tensors, on the host checked (cell_ptr) and to be uploaded, or on the device and used in place
_LpPlace = namedtuple("_LpPlace", "status K M samples cell_ptr")


def _place_lists(status, samples, values, cells, cell_ptr, who, routes=False):
    """The checks of the candidate lists that ``lightpath_place_args`` and ``materialise_placement`` share: returns ``(K,
    M, samples, cell_ptr)`` with the last two as 1-d int64 tensors -- the caller's own tensor where one was given -- or
    raises the named ``ValueError``.  ``routes`` (``lightpath_place_slots_args`` and ``materialise_slot_sweep``): the same
    checks of ``R`` routes, with ``links [M]`` in the place of ``cells`` and ``link_ptr`` in the place of ``cell_ptr``."""
    def got(t):
        return f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__

    one, K_, cells_, ptr_ = ("route", "R", "links", "link_ptr") if routes else ("candidate", "K", "cells", "cell_ptr")
    P = int(status.data.shape[1])
    if not isinstance(values, torch.Tensor) or values.dim() != 2 or values.dtype != torch.float64 or values.shape[1] != P:
        raise ValueError(f"{who}: values must be a float64 tensor [{K_}, {P}] (one raw lp_feat vector per {one}), got "
                         f"{got(values)}")
    K = int(values.shape[0])
    if routes:
        if not isinstance(cells, torch.Tensor) or cells.dim() != 1 or cells.dtype != torch.int64:
            raise ValueError(f"{who}: links must be a 1-d int64 tensor [M] of link indices, got {got(cells)}")
        M = int(cells.shape[0])
    else:
        if not isinstance(cells, torch.Tensor) or cells.dim() != 2 or cells.dtype != torch.int64 or cells.shape[0] != 2:
            raise ValueError(f"{who}: cells must be an int64 tensor [2, M] (link index, frequency index), got {got(cells)}")
        M = int(cells.shape[1])
    for name, t in (("values", values), (cells_, cells)):
        if t.device != status.data.device:
            raise ValueError(f"{who}: {name} is on {t.device}, the status chunk on {status.data.device}")
    if isinstance(samples, torch.Tensor):
        if samples.dim() != 1 or samples.dtype != torch.int64 or samples.shape[0] != K:
            raise ValueError(f"{who}: samples must be an int, a sequence or a 1-d int64 tensor of {K} sample numbers (one "
                             f"per row of values), got {got(samples)}")
    elif isinstance(samples, bool) or samples is None:
        raise ValueError(f"{who}: samples must be an int, a sequence or a 1-d int64 tensor, got {got(samples)}")
    elif isinstance(samples, int):
        samples = torch.full((K,), samples, dtype=torch.int64)
    else:
        samples = torch.tensor([int(v) for v in samples], dtype=torch.int64).reshape(-1)
        if samples.shape[0] != K:
            raise ValueError(f"{who}: samples names {samples.shape[0]} {one}s, values has {K} rows")
    if isinstance(cell_ptr, torch.Tensor):
        if cell_ptr.dim() != 1 or cell_ptr.dtype != torch.int64 or cell_ptr.shape[0] != K + 1:
            raise ValueError(f"{who}: {ptr_} must be a sequence or a 1-d int64 tensor of {K_} + 1 = {K + 1} offsets into "
                             f"{cells_}, got {got(cell_ptr)}")
    else:
        cell_ptr = torch.tensor([int(v) for v in cell_ptr], dtype=torch.int64).reshape(-1)
        if cell_ptr.shape[0] != K + 1:
            raise ValueError(f"{who}: {ptr_} must hold {K_} + 1 = {K + 1} offsets into {cells_}, got {cell_ptr.shape[0]}")
    if not cell_ptr.is_cuda:                               # on the host: checked here; on the device: by the kernel
        if int(cell_ptr[0]) != 0 or int(cell_ptr[-1]) != M or (K and int(cell_ptr.diff().min()) < 0):
            raise ValueError(f"{who}: {ptr_} must be non-decreasing from 0 to M = {M}, got {cell_ptr.tolist()}")
        if K and int(cell_ptr.diff().min()) == 0:
            raise ValueError(f"{who}: {one} {int(cell_ptr.diff().argmin())} has an empty slice of {cells_}")
    return K, M, samples, cell_ptr


def lightpath_place_args(status, in_channels, is_lut_index, samples, values, cells, cell_ptr,
                         features_to_consider=to_graph.DEFAULT_FEATURES, freq_threshold=0.05,
                         who="LightpathPredictor.place"):
    """The argument checks of ``LightpathPredictor.place`` that need no device: returns an ``_LpPlace`` (``status``: the
    ``_LpStatus`` of ``lightpath_status_args``; ``K``, ``M``; ``samples`` and ``cell_ptr`` as 1-d int64 tensors) or raises
    -- ``TypeError`` for a ``status`` that is no ``DeviceStatus``; ``ValueError`` naming the argument for ``values`` not
    float64 ``[K, P]``, ``cells`` not int64 ``[2, M]``, either on another device than the chunk, ``samples`` or ``cell_ptr``
    of the wrong length or dtype, a host ``cell_ptr`` that is not non-decreasing from 0 to ``M`` or has an empty slice
    (one on the device is checked by the kernel), a bad ``freq_threshold``; then ``EnvelopeError`` for everything
    ``lightpath_status_args`` refuses, a chunk on the CPU last."""
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    K, M, samples, cell_ptr = _place_lists(status, samples, values, cells, cell_ptr, who)
    sa = lightpath_status_args(status, in_channels, is_lut_index, features_to_consider, freq_threshold, who)
    return _LpPlace(sa, K, M, samples, cell_ptr)


def _release_in_place(edited, conn_row, ra):
    """The release of ``materialise_placement`` and ``materialise_retest``: sample ``k`` of ``edited [K, P, L, Q]`` has all P
    rows zeroed in every occupied channel whose ``trunc(conn_id)`` is in ``ra.release[ra.release_ptr[k]:ra.release_ptr[k +
    1]]`` (``ra``: ``place_release_args``' answer; ``None`` or no conn: nothing happens)."""
    if ra is None or not ra.R:
        return
    K, dev = edited.shape[0], edited.device
    who_k = torch.repeat_interleave(torch.arange(K, device=dev), ra.release_ptr.to(dev).diff(), output_size=ra.R)
    cv = edited[:, conn_row]                                                      # [K, L, Q]
    named = (edited != 0).any(1) & (cv.abs() <= 2.0 ** 53)                       # occupied, with a conn to compare
    conn = torch.where(named, cv, torch.zeros_like(cv)).trunc().to(torch.int64)
    hit = (conn.index_select(0, who_k) == ra.release[:, None, None]) & named.index_select(0, who_k)       # [R, L, Q]
    gone = torch.zeros(K, *hit.shape[1:], dtype=torch.int32, device=dev).index_add_(0, who_k, hit.int())
    edited.masked_fill_((gone > 0)[:, None], 0.0)


def materialise_placement(status, samples, values, cells, cell_ptr, release=None, release_ptr=None):
    """The K edited samples that ``LightpathPredictor.place`` and ``TopologicalPredictor.place`` score without building
    them: the DEFINITION of both calls and what they save.  Returns a ``DeviceStatus`` of K samples; sample ``k`` is
    ``status.data[samples[k]]`` with ``values[k]`` written into each of the channels ``cells[:, cell_ptr[k]:cell_ptr[k +
    1]]`` (``target`` rows follow their samples).  For a ``LightpathPredictor``, ``predict.place(...)[0][k]`` is, bit for
    bit, the row ``predict(to_graph.device_batch(edited, "lightpath", ...))`` gives the candidate's node of graph ``k``,
    and -- the candidate being the first-seen flagged lightpath of its edited sample --
    ``predict.from_status(edited)[0][k]``.  For a ``TopologicalPredictor``, ``predict.place(...)`` is
    ``predict.from_status(edited)``, rows and link counts, bit for bit.  Pure torch on the status' device (CPU tensors as
    well), no kernel of ours; ``status`` is not modified.  Arguments as ``place``; occupied cells are overwritten, not
    refused.

    ``release [R]`` with ``release_ptr`` (as ``place``; ``place_release_args`` checks them): sample ``k`` first has all P
    rows zeroed in every occupied channel whose ``trunc(conn_id)`` is in ``release[release_ptr[k]:release_ptr[k + 1]]``,
    then gets ``values[k]`` in its cells.  Occupancy and conn are the kernels' rule: a channel is occupied when any of its
    values != 0; its conn is ``trunc(conn_id)``, and a ``conn_id`` that is NaN, infinite or beyond +-2^53 matches nothing.
    A conn that names no lightpath of the sample releases nothing here (``place`` refuses it on the device)."""
    who = "materialise_placement"
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    K, M, samples, cell_ptr = _place_lists(status, samples, values, cells, cell_ptr, who)
    ra = place_release_args(status, K, release, release_ptr, who)
    dev = status.data.device
    samples, cell_ptr = samples.to(dev), cell_ptr.to(dev)
    edited = status.data.index_select(0, samples)
    _release_in_place(edited, status.feature_indexes["conn_id"], ra)
    cand = torch.repeat_interleave(torch.arange(K, device=dev), cell_ptr.diff(), output_size=M)
    edited[cand, :, cells[0], cells[1]] = values.index_select(0, cand)
    return to_graph.DeviceStatus(edited, status.target.index_select(0, samples), status.freq, status.lp_feat, status.metric,
                                 status.link)


PLACE_SLOTS_MAX_CHUNK = 32      # include/qot_gnn.h: QOT_LP_PLACE_SLOTS_MAX_CHUNK, start slots one workgroup runs one after the other
PLACE_SLOTS_MAX_WIDTH = 8       # include/qot_gnn.h: QOT_LP_PLACE_SLOTS_MAX_WIDTH, slots a candidate occupies on every link

# what LightpathPredictor.place_slots returns: out [R, Q, O] float32, the row of the candidate of route r that starts at
# slot q, NaN where it is not free; free [R, Q] bool; count [R] int64, place's count (the same at every slot)
PlaceSlots = namedtuple("PlaceSlots", "out free count")
# what materialise_slot_sweep returns: place's argument lists of the K free (route, start slot) pairs -- samples [K],
# values [K, P], cells [2, Mc], cell_ptr [K + 1] -- which pair each is, route [K] and slot [K], and free [R, Q] bool
SlotSweep = namedtuple("SlotSweep", "samples values cells cell_ptr route slot free")

# samples / link_ptr: int64 tensors, on the host checked (link_ptr) and to be uploaded, or on the device and used in place;
# slot_row: the lp_feat row that carries the start slot's frequency, -1 for none; chunk: None or the caller's int
_LpPlaceSlots = namedtuple("_LpPlaceSlots", "status R M samples link_ptr slot_row width chunk")


def place_slots_chunk(num_routes: int, num_slots: int, compute_units: int) -> int:
    """Start slots per workgroup of ``qot_lightpath_infer_place_slots``'s grid ``R * ceil(Q / chunk)``, ``1 ...
    PLACE_SLOTS_MAX_CHUNK``, by ``retest_chunk``'s reasoning with the ``Q`` start slots of a route in the place of the
    ``M`` slots of a sample: the grid is that of the largest chunk for which ``R * ceil(Q / chunk)`` workgroups still reach
    the device's compute-unit count (a larger chunk shares the discovery of the sample among more start slots, but leaves
    units idle and runs more rows one after the other on one wave); the chunk returned is the smallest with that many
    workgroups, so that they carry equal shares.  Once ``R`` alone fills the device that is the grid of chunk 32.  1 when
    no chunk reaches the device.  Pure host arithmetic; no result of ``place_slots`` depends on it."""
    R, Q, cus = int(num_routes), int(num_slots), int(compute_units)
    if not 1 <= Q <= LP_STATUS_MAX_FREQS:
        raise ValueError(f"place_slots_chunk: num_slots must be in 1 ... {LP_STATUS_MAX_FREQS}, got {Q}")
    if R < 1 or R * Q < cus:
        return 1
    need = max(-(-cus // R), 1)                            # workgroups per route that reach the device
    largest = Q if need <= 1 else (Q - 1) // (need - 1)    # largest chunk with ceil(Q / chunk) >= need
    blocks = -(-Q // min(largest, PLACE_SLOTS_MAX_CHUNK))
    return -(-Q // blocks)


def _slot_sweep_options(status, width, slot_feature, who):
    """``width`` and ``slot_feature`` of ``place_slots`` and ``materialise_slot_sweep``: returns the ``lp_feat`` row that
    carries the start slot's frequency, -1 for ``None``, or raises the named ``ValueError``."""
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= PLACE_SLOTS_MAX_WIDTH:
        raise ValueError(f"{who}: width must be an int in 1 ... {PLACE_SLOTS_MAX_WIDTH}, got {width!r}")
    if slot_feature is None:
        return -1
    if slot_feature not in status.feature_indexes:
        raise ValueError(f"{who}: slot_feature {slot_feature!r} is no lp_feat row of the status (None: values unchanged at "
                         f"every slot)")
    if slot_feature in ("conn_id",) + _LABEL_ROWS:
        raise ValueError(f"{who}: slot_feature cannot be {slot_feature!r}: the candidate's conn_id and its osnr = snr = ber = "
                         f"-1 are what place tests")
    return int(status.feature_indexes[slot_feature])


def lightpath_place_slots_args(status, in_channels, is_lut_index, samples, values, links, link_ptr,
                               features_to_consider=to_graph.DEFAULT_FEATURES, freq_threshold=0.05, width=1,
                               slot_feature="freq", chunk=None, who="LightpathPredictor.place_slots"):
    """The argument checks of ``LightpathPredictor.place_slots`` that need no device: returns an ``_LpPlaceSlots``
    (``status``: the ``_LpStatus`` of ``lightpath_status_args``; ``R``, ``M``; ``samples`` and ``link_ptr`` as 1-d int64
    tensors; ``slot_row``, ``width``, ``chunk``) or raises -- ``TypeError`` for a ``status`` that is no ``DeviceStatus``;
    ``ValueError`` naming the argument for what ``_place_lists`` refuses of ``values`` (float64 ``[R, P]``), ``links``
    (int64 ``[M]``), ``samples`` and ``link_ptr`` (a host ``link_ptr`` not non-decreasing from 0 to ``M`` or with an empty
    slice; one on the device is checked by the kernel), a ``width`` that is no int in ``1 ... PLACE_SLOTS_MAX_WIDTH``, a
    ``slot_feature`` that is no row of ``lp_feat`` or one of ``conn_id``, ``osnr``, ``snr``, ``ber``, a ``chunk`` that is
    neither ``None`` nor an int in ``1 ... PLACE_SLOTS_MAX_CHUNK``, a bad ``freq_threshold``; then ``EnvelopeError`` for
    everything ``lightpath_status_args`` refuses, a chunk on the CPU last."""
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    R, M, samples, link_ptr = _place_lists(status, samples, values, links, link_ptr, who, routes=True)
    slot_row = _slot_sweep_options(status, width, slot_feature, who)
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk <= PLACE_SLOTS_MAX_CHUNK):
        raise ValueError(f"{who}: chunk must be None or an int in 1 ... {PLACE_SLOTS_MAX_CHUNK}, got {chunk!r}")
    sa = lightpath_status_args(status, in_channels, is_lut_index, features_to_consider, freq_threshold, who)
    return _LpPlaceSlots(sa, R, M, samples, link_ptr, slot_row, width, chunk)


def materialise_slot_sweep(status, samples, values, links, link_ptr, *, width=1, slot_feature="freq"):
    """The explicit ``place`` argument lists of every FREE (route, start slot) pair that ``LightpathPredictor.place_slots``
    scores without building them: the DEFINITION of that call and what it saves -- the occupancy pass, the host read of
    the free slots and the list building.  Arguments as ``place_slots`` (``_place_lists`` and the same ``width`` /
    ``slot_feature`` checks).  Returns ``SlotSweep(samples [K], values [K, P], cells [2, Mc], cell_ptr [K + 1], route [K],
    slot [K], free [R, Q])``, routes rising and start slots rising inside a route.  ``free[r, q]``: every channel of
    ``route x {q ... q + width - 1}`` of sample ``samples[r]`` has all P values equal to 0, and ``q + width <= Q``.
    Candidate ``k`` is route ``route[k]`` started at ``slot[k]``: sample ``samples[route[k]]``; ``values[route[k]]`` with
    -- unless ``slot_feature`` is ``None`` -- ``status.freq[slot[k]]`` in the ``slot_feature`` row; its cells link by link
    in the route's order (a duplicate link gives duplicate cells), the ``width`` slots rising inside a link.  With those
    lists ``place_slots(...).out[route[k], slot[k]]`` is, bit for bit, ``place(status, samples, values, cells,
    cell_ptr)[0][k]``.  Pure torch on the status' device (CPU tensors as well), no kernel of ours; it reads the free pairs
    back to the host (``nonzero``); ``status`` is not modified."""
    who = "materialise_slot_sweep"
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    R, M, samples, link_ptr = _place_lists(status, samples, values, links, link_ptr, who, routes=True)
    slot_row = _slot_sweep_options(status, width, slot_feature, who)
    dev = status.data.device
    Q = int(status.data.shape[3])
    samples, link_ptr = samples.to(dev), link_ptr.to(dev)
    length = link_ptr.diff()                                                      # [R] links per route
    of_route = torch.repeat_interleave(torch.arange(R, device=dev), length, output_size=M)
    occupied = (status.data != 0).any(1)                                          # [S, L, Q]
    blocked = torch.zeros(R, Q, dtype=torch.int32, device=dev)
    blocked.index_add_(0, of_route, occupied[samples.index_select(0, of_route), links].int())
    free = torch.zeros(R, Q, dtype=torch.bool, device=dev)
    if width <= Q:
        clear = blocked == 0
        run = clear[:, :Q - width + 1].clone()
        for t in range(1, width):
            run &= clear[:, t:Q - width + 1 + t]
        free[:, :Q - width + 1] = run
    route, slot = free.nonzero(as_tuple=True)                                     # (the host read)
    K = int(route.shape[0])
    per = length.index_select(0, route) * width                                   # [K] cells per candidate
    cell_ptr = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    cell_ptr[1:] = per.cumsum(0)
    Mc = int(cell_ptr[-1])
    cand = torch.repeat_interleave(torch.arange(K, device=dev), per, output_size=Mc)
    pos = torch.arange(Mc, device=dev) - cell_ptr.index_select(0, cand)
    link = links.index_select(0, link_ptr.index_select(0, route.index_select(0, cand)) + pos // width)
    cells = torch.stack([link, slot.index_select(0, cand) + pos % width])
    vals = values.index_select(0, route)
    if slot_row >= 0:
        vals[:, slot_row] = status.freq.index_select(0, slot)
    return SlotSweep(samples.index_select(0, route), vals, cells, cell_ptr, route, slot, free)


PLACE_MAX_AFFECTED = 32         # include/qot_gnn.h: QOT_PLACE_MAX_AFFECTED, retested lightpaths per candidate
_LABEL_ROWS = ("osnr", "snr", "ber")

# what LightpathPredictor.place_impact returns: place(...)'s out [K, O] and count [K]; affected [K, A] int64 conn ids, -1
# padded, and n_affected [K] int64, their true number; before / after [K, A, O] float32, NaN padded
PlaceImpact = namedtuple("PlaceImpact", "out count affected n_affected before after")
# what LightpathPredictor.reroute_impact returns: PlaceImpact's six for place(..., release=); gains [K, A] bool, the
# candidate is a source of after (False padded); lost [K, A] int64, the released sources of before (-1 padded)
RerouteImpact = namedtuple("RerouteImpact", "out count affected n_affected before after gains lost")


def lightpath_place_impact_args(status, in_channels, is_lut_index, samples, values, cells, cell_ptr,
                                features_to_consider=to_graph.DEFAULT_FEATURES, freq_threshold=0.05, max_affected=8,
                                who="LightpathPredictor.place_impact"):
    """The argument checks of ``LightpathPredictor.place_impact`` that need no device: ``ValueError`` for a
    ``max_affected`` that is no int in ``1 ... PLACE_MAX_AFFECTED``; ``EnvelopeError`` for a feature list that holds
    ``osnr``, ``snr`` or ``ber`` (the retest rewrites those rows, so they must not be features); then everything
    ``lightpath_place_args`` refuses, whose ``_LpPlace`` is returned."""
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    if isinstance(max_affected, bool) or not isinstance(max_affected, int) or not 1 <= max_affected <= PLACE_MAX_AFFECTED:
        raise ValueError(f"{who}: max_affected must be an int in 1 ... {PLACE_MAX_AFFECTED}, got {max_affected!r}")
    labels = [n for n in features_to_consider if n in _LABEL_ROWS]
    if labels:
        raise EnvelopeError(f"{who}: {', '.join(repr(n) for n in labels)} cannot be a feature: retesting a lightpath rewrites "
                            f"its osnr, snr and ber")
    return lightpath_place_args(status, in_channels, is_lut_index, samples, values, cells, cell_ptr, features_to_consider,
                                freq_threshold, who)


def materialise_retest(status, samples, conns, values=None, cells=None, cell_ptr=None, *, release=None, release_ptr=None):
    """The samples in which an ESTABLISHED lightpath is the lightpath under test, without or with a candidate established
    next to it: the DEFINITION of ``LightpathPredictor.place_impact``'s ``before`` and ``after`` -- and, with ``release``
    and ``release_ptr`` (keyword-only; as ``place`` takes them, T slices, checked by ``place_release_args``), of
    ``LightpathPredictor.reroute_impact``'s ``after``: then one edit runs before the two below, with or without
    ``values`` -- (0) sample ``t`` has all P rows zeroed in every occupied channel whose ``trunc(conn_id)`` is in
    ``release[release_ptr[t]:release_ptr[t + 1]]``, ``materialise_placement``'s rule exactly: a conn that names no
    lightpath of the sample releases nothing.  Without the two keywords nothing changes.  Returns a
    ``DeviceStatus`` of T samples; sample ``t`` is ``status.data[samples[t]]`` with two edits, in this order.  (1) Only
    when ``values`` is given (then ``cells`` and ``cell_ptr`` too, all as ``place`` takes them, T candidates): ``values[t]``
    is written into each of the channels ``cells[:, cell_ptr[t]:cell_ptr[t + 1]]`` with its ``osnr``, ``snr`` and ``ber``
    entries replaced by 0.0 -- the candidate as an established neighbour, unflagged, ``is_lut`` 0: how every neighbour of
    a lightpath under test looks in the training data.  (2) Every occupied channel whose ``trunc(conn_id)`` is
    ``conns[t]`` gets ``osnr = snr = ber = -1``.  Occupancy and conn follow the rule of ``materialise_placement``.  A
    flagged lightpath the sample holds already stays flagged.

    ``before[k, i]`` is, bit for bit, the row ``predict(to_graph.device_batch(materialise_retest(status, [samples[k]],
    [affected[k, i]]), "lightpath", ...))`` gives the node of conn ``affected[k, i]`` (``to_graph.placement_impact`` states
    its number) -- ``predict.from_status(...)[0][0]`` where that lightpath is the sample's first flagged one -- and
    ``after[k, i]`` the same with ``values[k:k + 1]``, candidate ``k``'s cells and ``[0, m]`` passed in as well.  Pure
    torch on the status' device (CPU tensors as well), no kernel of ours; ``status`` is not modified."""
    who = "materialise_retest"
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    dev = status.data.device
    fi = status.feature_indexes
    conns = torch.as_tensor(conns, dtype=torch.int64).reshape(-1).to(dev)
    T = int(conns.shape[0])
    if values is None:
        if cells is not None or cell_ptr is not None:
            raise ValueError(f"{who}: cells and cell_ptr go with values")
        if isinstance(samples, int) and not isinstance(samples, bool):
            samples = [samples] * T
        samples = torch.as_tensor(samples, dtype=torch.int64).reshape(-1).to(dev)
        if samples.shape[0] != T:
            raise ValueError(f"{who}: samples names {samples.shape[0]} samples, conns {T} lightpaths")
        edited = status.data.index_select(0, samples)
        _release_in_place(edited, fi["conn_id"], place_release_args(status, T, release, release_ptr, who))
    else:
        K, M, samples, cell_ptr = _place_lists(status, samples, values, cells, cell_ptr, who)
        if K != T:
            raise ValueError(f"{who}: values has {K} rows, conns names {T} lightpaths")
        samples, cell_ptr = samples.to(dev), cell_ptr.to(dev)
        edited = status.data.index_select(0, samples)
        _release_in_place(edited, fi["conn_id"], place_release_args(status, T, release, release_ptr, who))
        established = values.clone()
        established[:, [fi[n] for n in _LABEL_ROWS]] = 0.0
        cand = torch.repeat_interleave(torch.arange(K, device=dev), cell_ptr.diff(), output_size=M)
        edited[cand, :, cells[0], cells[1]] = established.index_select(0, cand)
    cv = edited[:, fi["conn_id"]]                                                 # [T, L, Q]
    named = (edited != 0).any(1) & (cv.abs() <= 2.0 ** 53)                       # occupied, with a conn to compare
    conn = torch.where(named, cv, torch.zeros_like(cv)).trunc().to(torch.int64)
    under_test = named & (conn == conns[:, None, None])
    for n in _LABEL_ROWS:
        edited[:, fi[n]].masked_fill_(under_test, -1.0)
    return to_graph.DeviceStatus(edited, status.target.index_select(0, samples), status.freq, status.lp_feat, status.metric,
                                 status.link)


RETEST_MAX_LIGHTPATHS = 256     # include/qot_gnn.h: QOT_SG_MAX_LIGHTPATHS, slots per sample of LightpathPredictor.retest
RETEST_MAX_CHUNK = 32           # include/qot_gnn.h: QOT_LP_RETEST_MAX_CHUNK, slots one workgroup runs one after the other
LP_RETEST_NO_SUCH_CONN = 4096   # include/qot_gnn.h: QOT_LP_RETEST_NO_SUCH_CONN, the one status bit qot_lightpath_infer_retest adds
_RETEST_CAUSES = (
    (LP_RETEST_NO_SUCH_CONN, "retest: a named conn_id is no lightpath of the sample"),
)

# what LightpathPredictor.retest returns: out [G, M, O] float32, NaN padded; conn [G, M] int64 conn ids, -1 padded; n [G]
# int64, the lightpaths of each sample (may exceed M); count [G] int64, from_status's count
Retest = namedtuple("Retest", "out conn n count")

# M; conns: None or the caller's int64 [G, M] tensor; chunk: None (retest_chunk decides) or the caller's int
_LpRetest = namedtuple("_LpRetest", "status M conns chunk")


def retest_chunk(num_samples: int, max_lightpaths: int, compute_units: int) -> int:
    """Slots per workgroup of ``qot_lightpath_infer_retest``'s grid ``G * ceil(M / chunk)``, ``1 ... RETEST_MAX_CHUNK``, in
    the manner of ``mc_chunk``.  The grid is that of the largest chunk for which ``G * ceil(M / chunk)`` workgroups still
    reach the device's compute-unit count (a larger chunk shares the discovery and the rescan of the sample among more
    slots, but leaves units idle and runs more rows one after the other); the chunk returned is the smallest with that
    many workgroups, so that they carry equal shares.  Once ``G`` alone fills the device that is the grid of chunk 32
    (M = 256: 32).  1 when no chunk reaches the device.  Pure host arithmetic; no result of ``retest`` depends on it."""
    G, M, cus = int(num_samples), int(max_lightpaths), int(compute_units)
    if not 1 <= M <= RETEST_MAX_LIGHTPATHS:
        raise ValueError(f"retest_chunk: max_lightpaths must be in 1 ... {RETEST_MAX_LIGHTPATHS}, got {M}")
    if G < 1 or G * M < cus:
        return 1
    need = max(-(-cus // G), 1)                            # workgroups per sample that reach the device
    largest = M if need <= 1 else (M - 1) // (need - 1)    # largest chunk with ceil(M / chunk) >= need
    blocks = -(-M // min(largest, RETEST_MAX_CHUNK))
    return -(-M // blocks)


def lightpath_retest_args(status, in_channels, is_lut_index, conns=None, features_to_consider=to_graph.DEFAULT_FEATURES,
                          freq_threshold=0.05, max_lightpaths=RETEST_MAX_LIGHTPATHS, chunk=None,
                          who="LightpathPredictor.retest"):
    """The argument checks of ``LightpathPredictor.retest`` that need no device: returns an ``_LpRetest`` (``status``: the
    ``_LpStatus`` of ``lightpath_status_args``; ``M``; ``conns``; ``chunk``) or raises -- ``TypeError`` for a ``status``
    that is no ``DeviceStatus``; ``ValueError`` for a ``chunk`` that is neither ``None`` nor an int in ``1 ...
    RETEST_MAX_CHUNK``, for ``conns`` that is not an int64 tensor ``[G, M]`` with ``M`` in ``1 ... RETEST_MAX_LIGHTPATHS``
    on the chunk's device (the call itself compares ``G`` with ``samples``), or -- without ``conns`` -- a ``max_lightpaths``
    that is no int in that range (with ``conns`` it is ignored); ``EnvelopeError`` for a feature list that holds ``osnr``, ``snr`` or
    ``ber`` (the retest rewrites those rows); then everything ``lightpath_status_args`` refuses, a chunk on the CPU last."""
    if not isinstance(status, to_graph.DeviceStatus):
        raise TypeError(f"{who} takes a DeviceStatus (NetworkStatus.to_device), got {type(status).__name__}")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk <= RETEST_MAX_CHUNK):
        raise ValueError(f"{who}: chunk must be None or an int in 1 ... {RETEST_MAX_CHUNK}, got {chunk!r}")
    if conns is None:
        M = max_lightpaths
        if isinstance(M, bool) or not isinstance(M, int) or not 1 <= M <= RETEST_MAX_LIGHTPATHS:
            raise ValueError(f"{who}: max_lightpaths must be an int in 1 ... {RETEST_MAX_LIGHTPATHS}, got {M!r}")
    else:
        got = f"{conns.dtype} {tuple(conns.shape)}" if isinstance(conns, torch.Tensor) else type(conns).__name__
        if (not isinstance(conns, torch.Tensor) or conns.dim() != 2 or conns.dtype != torch.int64
                or not 1 <= conns.shape[1] <= RETEST_MAX_LIGHTPATHS):
            raise ValueError(f"{who}: conns must be an int64 tensor [G, M] of conn_id values (-1: an empty slot) with M "
                             f"in 1 ... {RETEST_MAX_LIGHTPATHS}, got {got}")
        if conns.device != status.data.device:
            raise ValueError(f"{who}: conns is on {conns.device}, the status chunk on {status.data.device}")
        M = int(conns.shape[1])
    labels = [n for n in features_to_consider if n in _LABEL_ROWS]
    if labels:
        raise EnvelopeError(f"{who}: {', '.join(repr(n) for n in labels)} cannot be a feature: retesting a lightpath rewrites "
                            f"its osnr, snr and ber")
    sa = lightpath_status_args(status, in_channels, is_lut_index, features_to_consider, freq_threshold, who)
    return _LpRetest(sa, M, conns, chunk)


# what LightpathPredictor._prepare hands to _launch: the model's shape, the batch on dev, which rows (rows mode: batch,
# idx; graphs mode: a fresh count) and how many
_LpPrepared = namedtuple("_LpPrepared", "F C O dev x ei batch ptr eptr idx B rows count")


class LightpathPredictor(_DeviceState):
    """``predict = LightpathPredictor(model)``: the EVAL-MODE forward of a one-layer ``LightpathGNN`` as one kernel launch
    that computes the LUT rows only (one wavefront per row, no graph index, no other node's row).

    ``predict(data) -> (out [L, O], lut_batch [L])``: the contract of ``model.eval()(data)``.  The LUT rows are the model's
    (``model._lut_rows``: cached on the batch object, one host read on the first visit of a batch); a LUT-less batch raises
    the model's ``ValueError("No LUT node found in the batch.")``, or gives zero rows when ``model.allow_empty_lut`` is set.

    ``predict.per_graph(data) -> (out [B, O], count [B] int32)``: one row per GRAPH, found on the device: ``count[g]`` LUT
    nodes in graph ``g``, ``out[g]`` the row of the lowest-numbered one, NaN when there is none.  No host synchronisation;
    legal inside ``torch.cuda.graph`` capture when the batch carries ``ptr`` / ``edge_ptr`` (ours do) or has been through
    one call before (the derived slices are remembered on the batch object).

    Both: ``model.training`` does not matter (eval-mode function: running statistics, no dropout), buffers are never
    written, the result carries no ``grad_fn``.  Parameters and buffers are read by the kernel at call time, in place: an
    in-place optimizer step, ``load_state_dict`` or running statistics moved by a train-mode forward are seen by the next
    call with no bookkeeping.  A row is bitwise reproducible, independent of the other graphs of the batch and the same
    from either call; against ``model.eval()(data)`` it agrees to fp32 rounding.  A model whose width the engine runs
    zero-padded (e.g. C = 20) is supported: the kernel reads its real parameters.

    ``predict.sensitivity(data)``: the rows together with their Jacobian wrt the node features of each row's one-hop
    in-neighbourhood, in one launch (see there).
    ``predict.what_if(data, ...)``: K candidate lightpaths -- another feature row for a LUT node, interferers removed and
    added -- scored in one launch (see there).
    ``predict.from_status(status)``: ``per_graph``'s rows straight from network-status samples, no graph in between, one
    launch and no host read (see there).
    ``predict.place(status, samples, values, cells, cell_ptr)``: K candidate (route, slot) assignments of a NEW lightpath,
    each placed into a status sample that does not hold it yet -- the interferers are found by the kernel -- one launch and
    no host read (see there).
    ``predict.place_slots(status, samples, values, links, link_ptr)``: the step before ``place`` -- R routes, each swept over
    every start slot of the grid; an occupied slot is an answer (``free``), not an error -- one launch and no host read
    (see there).
    ``predict.place_impact(status, samples, values, cells, cell_ptr)``: ``place``'s rows together with the retest of the
    established lightpaths each candidate disturbs -- their rows as the lightpath under test before and after the candidate
    is lit -- one launch and no host read (see there).
    ``predict.reroute_impact(status, samples, values, cells, cell_ptr, release=, release_ptr=)``: ``place_impact`` with
    established lightpaths released in the same launch -- the lightpaths beside the new route gain an interferer, those
    beside the old route lose one; both are retested (see there).
    ``predict.retest(status)``: every ESTABLISHED lightpath of the status samples, or a named subset (``conns=``), retested
    as the lightpath under test -- the standing question about a network state, a margin audit -- one launch and no host
    read (see there).

    Envelope -- ``EnvelopeError`` naming the condition otherwise: a model on the GPU with ``num_layers == 1``, 1 ... 16 input
    features, hidden width 1 ... 256, 1 ... 8 outputs; ``data.x`` of shape ``[N, F]``.  No cap on in-degree, graph size or
    batch size.  Edges must be grouped by graph (``ValueError`` otherwise); an edge that leaves its graph's node range makes
    the rows of that graph NaN and ``check_status()`` raise.
    """

    _FLAGS = ("qot_lightpath_infer", "bit 0 an edge leaves its graph's node range, bit 1 a LUT index, graph number or slice "
                                     "outside the arrays (what_if: bit 0 also an added source, bit 1 also a candidate's "
                                     "node or a drop position out of range, bit 2 a candidate's feature row without 1.0 "
                                     "in the LUT column; from_status: bit 3 a bad conn_id, bit 4 too many lightpaths, bit 5 "
                                     "a sample number out of range; place: those, bit 6 a bad cell, bit 7 an occupied "
                                     "cell, bit 8 a conn_id taken, bit 9 values not under test; place_slots: place's "
                                     "without bit 7, bit 6 a bad link or link_ptr slice; retest: from_status's, bit "
                                     "12 a named conn_id the sample does not hold)")
    # the bits of qot_lightpath_infer_status, named when check_status() finds them: the device builder's own words
    _CAUSES = tuple((bit, next(t for b, t in to_graph._SG_CAUSES if b == sg)) for bit, sg in (
        (LP_STATUS_BAD_CONN, to_graph.SG_BAD_CONN), (LP_STATUS_TOO_MANY, to_graph.SG_TOO_MANY),
        (LP_STATUS_BAD_SAMPLE, to_graph.SG_BAD_SAMPLE)))
    # ... and the bits qot_lightpath_infer_place adds, named by check_status() behind them
    _PLACE_CAUSES = _LP_PLACE_CAUSES
    # ... and the two of qot_lightpath_infer_place_release (place with release=), behind those
    _RELEASE_CAUSES = _LP_RELEASE_CAUSES
    # ... and the one of qot_lightpath_infer_retest (retest with conns=), behind those
    _RETEST_CAUSES = _RETEST_CAUSES

    def __init__(self, model):
        super().__init__()
        self.model = model
        F, C, O = self._check_model()
        self._outputs(list(range(O)), self._device())               # the default selection is uploaded here, not in a call

    def _check_model(self):
        m = self.model
        if getattr(m, "num_layers", None) != 1 or not hasattr(m, "conv1") or not hasattr(m, "norm1"):
            raise EnvelopeError(f"LightpathPredictor: num_layers must be 1 (the reference architecture: one GATConv), got "
                                f"{getattr(m, 'num_layers', None)}")
        conv = m.conv1
        F, C, O = conv.in_channels, conv.out_channels, m.mlp[3].out_features
        if conv.heads != 4:
            raise EnvelopeError(f"LightpathPredictor: heads {conv.heads} is not supported; it must be 4")
        if not 1 <= F <= LP_MAX_FEATURES:
            raise EnvelopeError(f"LightpathPredictor: in_channels {F} is not supported; it must be 1 ... {LP_MAX_FEATURES}")
        if not 1 <= C <= LP_MAX_HIDDEN:
            raise EnvelopeError(f"LightpathPredictor: hidden_channels {C} is not supported; it must be 1 ... {LP_MAX_HIDDEN}")
        if not 1 <= O <= LP_MAX_OUTPUTS:
            raise EnvelopeError(f"LightpathPredictor: output_dim {O} is not supported; it must be 1 ... {LP_MAX_OUTPUTS}")
        if not 0 <= int(m.is_lut_index) < F:
            raise EnvelopeError(f"LightpathPredictor: is_lut_index {m.is_lut_index} is not a column of {F} features")
        return F, C, O

    def _device(self):
        bias = self.model.conv1.bias
        if not bias.is_cuda:
            raise EnvelopeError("LightpathPredictor: the model is on the CPU; move it to the GPU first (model.to('cuda'))")
        return bias.device

    def _batch(self, data, F, dev):
        """``(x, edge_index, node_ptr, edge_ptr, B)`` on ``dev``; the slices are remembered on the batch object."""
        x = getattr(data, "x", None)
        if x is None or x.dim() != 2 or x.shape[1] != F:
            raise EnvelopeError(f"LightpathPredictor: data.x must be [N, {F}], got "
                                f"{None if x is None else tuple(x.shape)}")
        x = _f32c(x if x.device == dev else x.to(dev))
        ei = data.edge_index
        tag = (x.shape[0], ei.data_ptr(), ei._version, tuple(ei.shape))
        c = _cache(data)
        if c is not None and "infer_lp" in c and c["infer_lp"][0] == tag:
            return (x,) + c["infer_lp"][1]
        ei = _i64(ei, dev)
        ptr, eptr, B, _, _, _ = graph_slices(data, ei, x.shape[0], dev, "LightpathPredictor")
        res = (ei, ptr, eptr, B)
        if c is not None:
            c["infer_lp"] = (tag, res)
        return (x,) + res

    def _prepare(self, data, per_graph, shape=None, nodes=None, samples=None):
        """Everything a launch needs, checked, as an ``_LpPrepared``.  ``per_graph``: one row per graph, found on the device,
        instead of the model's LUT rows.  ``shape``: ``_check_model()``'s answer, when the caller has asked already.
        ``nodes``: the nodes whose rows are computed, in the place of the model's LUT rows (``what_if``).  ``data=None``
        (``from_status``): there is no batch, one row for each of ``samples`` status samples and an int64 ``count``."""
        F, C, O = shape or self._check_model()
        dev = self._device()
        if data is None:
            x = ei = ptr = eptr = idx = batch = None
            B = rows = samples
            count = torch.empty(B, dtype=torch.int64, device=dev)
            self._status_on(dev)
            return _LpPrepared(F, C, O, dev, x, ei, batch, ptr, eptr, idx, B, rows, count)
        x, ei, ptr, eptr, B = self._batch(data, F, dev)
        if per_graph:
            idx = batch = None
            rows, count = B, torch.empty(B, dtype=torch.int32, device=dev)
        else:
            idx = self.model._lut_rows(data) if nodes is None else nodes    # the model's ValueError for a LUT-less batch
            batch, idx = _i64(data.batch, dev), _i64(idx, dev)
            rows, count = idx.shape[0], None
        self._status_on(dev)
        return _LpPrepared(F, C, O, dev, x, ei, batch, ptr, eptr, idx, B, rows, count)

    def _launch(self, name, p, out, *extra, inside=True):
        """One launch of entry point ``name``: the arguments the three kernels share (``out`` among them), then ``extra``;
        none for 0 rows (only with ``allow_empty_lut``, an empty batch or no candidate).  Returns what the call hands back
        beside its rows: ``count``, or ``lut_batch`` -- gathered behind the launch, so that the kernel is not queued after
        it.  ``inside=False``: the rows' nodes are the caller's and unchecked (``what_if``); one outside ``0 ... N - 1`` has
        -1 in ``lut_batch``."""
        F, C, O, _, x, ei, batch, ptr, eptr, idx, B, rows, count = p
        if rows:
            m = self.model
            conv, bn, l0, l3 = m.conv1, m.norm1.module, m.mlp[0], m.mlp[3]
            w = [_f32c(t.detach()) for t in (conv.lin.weight, conv.att_src, conv.att_dst, conv.bias, bn.weight, bn.bias,
                                             bn.running_mean, bn.running_var, l0.weight, l0.bias, l3.weight, l3.bias)]
            N, E = (0, 0) if x is None else (x.shape[0], ei.shape[1])       # (no batch: from_status)
            _lib.call(name, x, ei, batch, ptr, eptr, idx, 0 if idx is None else rows, N, E, B, *w[:4],
                      float(conv.negative_slope), *w[4:8], float(bn.eps), *w[8:], float(m.mlp[1].negative_slope), out, count,
                      F, C, O, int(conv.heads), int(m.is_lut_index), self._status, *extra)
        if idx is None:
            return count
        if not rows:
            return batch[:0]
        if inside:
            return batch.index_select(0, idx)
        N = x.shape[0]
        if N == 0:
            return torch.full_like(idx, -1)
        inside = idx.clamp(0, N - 1)
        return batch.index_select(0, inside).masked_fill_(inside != idx, -1)

    @torch.no_grad()
    def __call__(self, data):
        p = self._prepare(data, False)
        out = torch.empty(p.rows, p.O, dtype=torch.float32, device=p.dev)
        return out, self._launch("qot_lightpath_infer", p, out)

    @torch.no_grad()
    def per_graph(self, data):
        p = self._prepare(data, True)
        out = torch.empty(p.rows, p.O, dtype=torch.float32, device=p.dev)
        return out, self._launch("qot_lightpath_infer", p, out)

    @torch.no_grad()
    def from_status(self, status, samples=None, features_to_consider=to_graph.DEFAULT_FEATURES, freq_threshold=0.05):
        """The QoT of the lightpath under test of network-status samples, straight from the samples: ``(out [G, O] float32,
        count [G] int64)`` in ONE kernel launch (``csrc/infer_lightpath_status.hip``), without the graphs in between, with
        nothing read back, legal inside ``torch.cuda.graph`` capture.

        ``status``: a ``to_graph.DeviceStatus`` on the model's device.  ``samples``: ``None`` (all, in order), a sequence
        of sample numbers (uploaded) or an int64 device tensor (used in place: the form to capture); a repeated number is
        allowed and gives equal rows.  ``features_to_consider`` and
        ``freq_threshold`` as ``to_graph.device_batch``.

        The definition is what the tree computes already: with ``batch = to_graph.device_batch(status, "lightpath",
        features_to_consider, samples, freq_threshold)``, ``out`` is ``self.per_graph(batch)[0]`` bit for bit (NaN rows as
        NaN) and ``count`` its count as int64: ``count[g]`` lightpaths of sample ``g`` carry ``osnr == snr == ber == -1``
        on their first channel, ``out[g]`` is the row of the first-seen one, NaN when there is none.
        ``to_graph.lut_neighbourhood`` states on the host which lightpaths send a message into that row.  A sample's row
        depends on that sample alone; parameters and running statistics are read at call time.

        Refusals before any launch: ``TypeError`` for a ``status`` that is no ``DeviceStatus``; ``ValueError`` for a
        ``freq_threshold`` that is no finite positive number or a ``samples`` tensor that is not 1-d int64;
        ``EnvelopeError`` for everything ``__call__`` refuses, a chunk on the CPU or on another device than the model, more
        than 1024 frequency slots, ``len(features_to_consider) + 1 != in_channels``, ``is_lut`` sorting to another column
        than ``model.is_lut_index``, a feature or ``conn_id`` / ``osnr`` / ``snr`` / ``ber`` missing from ``lp_feat``.
        ``G == 0`` gives empty tensors without a launch.  On the device, since nothing is read back: a ``conn_id`` that is
        not finite or beyond +-2^53, more than 256 lightpaths in a sample, a sample number outside the chunk -- that
        sample's row is NaN and its count 0, the other rows are untouched, and ``check_status()`` raises naming the cause.
        (The column table of a feature list is uploaded on its first call with a chunk: make that call before capturing.)"""
        who = "LightpathPredictor.from_status"
        shape = self._check_model()
        sa = lightpath_status_args(status, shape[0], self.model.is_lut_index, features_to_consider, freq_threshold, who)
        dev = self._status_device(status, who)
        picks, G = _status_picks(samples, sa.S, dev, who)
        out = torch.empty(G, shape[2], dtype=torch.float32, device=dev)
        if G == 0:
            return out, self._empty_count(shape)
        return out, self._launch_status("qot_lightpath_infer_status", status, sa, shape, G, picks, out)

    def _status_device(self, status, who):
        """The model's device, which a status call's chunk must be on."""
        dev = self._device()
        if status.device != dev:
            raise EnvelopeError(f"{who}: the status chunk is on {status.device}, the model on {dev}")
        return dev

    def _empty_count(self, shape):
        """``count`` of a status call without rows: nothing is uploaded, nothing launched."""
        return self._prepare(None, True, shape, samples=0).count

    def _launch_status(self, name, status, sa, shape, rows, picks, out, *extra):
        """One launch of a status entry point (``from_status``, ``retest``, ``place``, ``place_impact``, ``reroute_impact``): no batch, ``rows``
        rows, the sample arguments of ``sa`` (an ``_LpStatus``) with the column table of its feature list, then ``extra``.
        Returns ``count``.  (Not for ``rows == 0``: the column table is an upload; see ``_empty_count``.)"""
        p = self._prepare(None, True, shape, samples=rows)
        cols, _, ncol = to_graph._column_tables(status, "lightpath", sa.features)
        return self._launch(name, p, out, status.data, status.freq, picks, sa.S, sa.P, sa.L, sa.Q, sa.conn_row, sa.osnr_row,
                            sa.snr_row, sa.ber_row, cols, ncol, sa.freq_threshold, *extra)

    @torch.no_grad()
    def retest(self, status, samples=None, conns=None, features_to_consider=to_graph.DEFAULT_FEATURES, freq_threshold=0.05,
               max_lightpaths=RETEST_MAX_LIGHTPATHS, *, chunk=None):
        """The standing question about a network state: the predicted QoT of every lightpath that is already lit, each
        RETESTED as the lightpath under test, as ``Retest(out [G, M, O] float32, conn [G, M] int64, n [G] int64, count [G]
        int64)`` in ONE kernel launch (``csrc/infer_lightpath_retest.hip``), with nothing read back and
        ``status.data`` never written; legal inside ``torch.cuda.graph`` capture under the conditions of ``from_status``
        (index arguments as int64 device tensors, one call made first).  Margin audits, finding the lightpaths nearest
        their threshold before admitting more traffic, ranking reroute candidates: one call instead of one edited sample
        and one graph per lightpath.

        ``status``, ``samples``, ``features_to_consider`` and ``freq_threshold`` are ``from_status``'s, checked by the same
        routines.  ``n[g]``: the lightpaths of sample ``samples[g]``; ``count[g]``: ``from_status``'s count, the sample's
        own flagged lightpaths.

        ``conns=None``: every lightpath, ``M = max_lightpaths`` (an int in ``1 ... 256``) slots per sample.  ``conn[g,
        :min(n, M)]`` are the ``trunc(conn_id)`` values in first-seen order -- the node order of ``to_graph.device_batch(
        status, "lightpath")`` -- and ``out[g, i]`` the eval-mode row of lightpath ``conn[g, i]``.  The slots behind hold
        -1 / NaN; ``n[g] > M`` is no error: the first ``M`` are written.  A sample without a lightpath gives ``n = 0``.
        (Every workgroup of the grid ``G * ceil(M / chunk)`` scans its sample before it knows whether its slots hold a
        lightpath: with many samples pass a bound on the lightpaths per sample, e.g. ``n.max()`` of an earlier call,
        rather than 256 -- DESIGN.md 4.26 has the figures.)

        ``conns [G, M]`` (int64, on the chunk's device, used in place; ``M`` in ``1 ... 256``; ``max_lightpaths`` is
        ignored): a named subset.  Slot ``(g, i)`` retests the lightpath whose ``trunc(conn_id)`` is ``conns[g, i]``; -1
        marks an empty slot (NaN row, ``conn`` -1, no error); a conn named twice gives equal rows; a conn the sample does
        not hold gives NaN in that slot only, ``conn[g, i] = -1``, and ``check_status()`` raises naming the cause (status
        bit ``LP_RETEST_NO_SUCH_CONN = 4096``).

        ``infer.materialise_retest`` is the definition, as for ``place_impact``'s ``before``: ``out[g, i]`` is, bit for
        bit, the row ``self(to_graph.device_batch(materialise_retest(status, [samples[g]], [conn[g, i]]), "lightpath",
        ...))`` gives the node of that conn; ``to_graph.retest_neighbourhood`` states the nodes and the messages on the
        host.  The sample's own flagged lightpath stays flagged: it is retested like the others, and it carries ``is_lut =
        1`` where it is a message source.

        ``chunk``: the slots one workgroup runs one after the other, ``1 ... 32``; ``None``: ``retest_chunk(G, M,
        compute_units)``.  Every result is bitwise independent of it.

        Refusals before any launch (``lightpath_retest_args``): ``from_status``'s; ``ValueError`` for a bad
        ``max_lightpaths``, ``chunk`` or ``conns`` (a bool is no int); ``EnvelopeError`` for a feature list that holds
        ``osnr``, ``snr`` or ``ber`` -- the retest rewrites those rows.  ``G == 0`` gives empty tensors without a launch.
        On the device ``from_status``'s three refusals apply (a bad ``conn_id``, more than 256 lightpaths, a sample number
        outside the chunk): all ``M`` rows of that sample are NaN, its ``conn`` -1, ``n = count = 0``, the other samples
        are untouched, and ``check_status()`` raises naming the cause.  There is no ``release=``, no retest for the
        topological model (it has no per-lightpath row), and the rows of one workgroup are computed by one wave."""
        who = "LightpathPredictor.retest"
        shape = self._check_model()
        ra = lightpath_retest_args(status, shape[0], self.model.is_lut_index, conns, features_to_consider, freq_threshold,
                                   max_lightpaths, chunk, who)
        sa, M = ra.status, ra.M
        dev = self._status_device(status, who)
        picks, G = _status_picks(samples, sa.S, dev, who)
        if conns is not None and int(conns.shape[0]) != G:
            raise ValueError(f"{who}: conns has {int(conns.shape[0])} rows, samples names {G} samples")
        out = torch.empty(G, M, shape[2], dtype=torch.float32, device=dev)
        conn = torch.empty(G, M, dtype=torch.int64, device=dev)
        n = torch.empty(G, dtype=torch.int64, device=dev)
        if G == 0:
            return Retest(out, conn, n, self._empty_count(shape))
        if chunk is None:
            chunk = retest_chunk(G, M, torch.cuda.get_device_properties(dev).multi_processor_count)
        count = self._launch_status("qot_lightpath_infer_retest", status, sa, shape, G, picks, out,
                                    None if conns is None else conns.contiguous(), conn, n, M, chunk)
        return Retest(out, conn, n, count)

    @torch.no_grad()
    def place(self, status, samples, values, cells, cell_ptr, features_to_consider=to_graph.DEFAULT_FEATURES,
              freq_threshold=0.05, *, release=None, release_ptr=None):
        """Routing and spectrum assignment: scores K candidate (route, slot) assignments of a NEW lightpath against the
        status samples of the established ones, ``(out [K, O] float32, count [K] int64)`` in ONE kernel launch
        (``csrc/infer_lightpath_place.hip``), without the edited samples or their graphs, with nothing read back, legal
        inside ``torch.cuda.graph`` capture.  The caller does not name the interferers: the kernel finds them by the rule
        of the graph builder (same link, ``0 < |f1 - f2| < freq_threshold``).

        ``status``: a ``to_graph.DeviceStatus`` on the model's device; never written.  ``samples``: the sample each
        candidate is placed into -- an int (all K), a sequence, or a 1-d int64 device tensor (used in place: the form to
        capture); repeated numbers are the normal case.  ``values [K, P]`` float64 on the device: row ``k`` is the raw
        ``lp_feat`` vector the candidate writes into each of its channels (``conn_id``, ``src_id``, ``dst_id``, the features,
        ``osnr = snr = ber = -1``), in status units: the kernel scales it with the column table ``from_status`` uses.
        ``cells [2, M]`` int64 on the device: (link index, frequency index) pairs; candidate ``k`` occupies
        ``cells[:, cell_ptr[k]:cell_ptr[k + 1]]`` -- no cap on their number, duplicates allowed.  ``cell_ptr``: K + 1 offsets;
        a host sequence is checked here and uploaded, an int64 device tensor is used in place and checked by the kernel.

        ``materialise_placement`` is the definition: with ``edited`` its K samples and ``batch =
        to_graph.device_batch(edited, "lightpath", ...)``, ``out[k]`` is, bit for bit, the row ``self(batch)`` gives the
        candidate's node of graph ``k`` (``to_graph.place_lightpath`` states its number), and ``count[k]`` the flagged
        lightpaths of ``edited[k]``: the sample's own plus one.  When the candidate is the only or the first-seen flagged
        one, that is ``self.from_status(edited)[0][k]``.  ``to_graph.placement_neighbourhood`` states on the host which
        lightpaths send a message into the row.  A candidate's row depends on its sample and itself alone; every
        candidate rescans its sample, O(L Q + cells Q): candidates of one sample do not share the scan.

        Refusals before any launch (``lightpath_place_args``): ``TypeError`` for a ``status`` that is no ``DeviceStatus``;
        ``ValueError`` for a bad ``freq_threshold``, ``values`` not float64 ``[K, P]``, ``cells`` not int64 ``[2, M]``,
        ``samples`` or ``cell_ptr`` of the wrong length or dtype, a host ``cell_ptr`` that is not non-decreasing from 0 to M
        or has an empty slice; ``EnvelopeError`` for everything ``from_status`` refuses.  ``K == 0`` gives empty tensors
        without a launch.  On the device, since nothing is read back: a cell outside the sample or a bad ``cell_ptr``
        slice, an occupied cell, a ``conn_id`` the sample holds already, ``values[k]`` without ``osnr == snr == ber == -1``,
        a ``conn_id`` that is not finite or beyond +-2^53, a sample that holds 256 lightpaths already, a sample number
        outside the chunk -- that candidate's row is NaN and its count 0, the other rows are untouched, and
        ``check_status()`` raises naming the cause.  (The column table of a feature list is uploaded on its first call
        with a chunk: make that call before capturing.)

        ``release [R]`` (int64, on the chunk's device) with ``release_ptr`` (K + 1 offsets, a host sequence or an int64
        device tensor, as ``cell_ptr``): a REROUTE, or an admission together with a tear-down, in the same launch
        (``csrc/infer_lightpath_place_release.hip``).  Candidate ``k`` first releases the lightpaths of
        its sample whose ``trunc(conn_id)`` is in ``release[release_ptr[k]:release_ptr[k + 1]]`` -- an empty slice and a conn
        named twice are allowed, at most ``PLACE_MAX_RELEASE = 32`` -- and is then placed;
        ``materialise_placement(..., release=, release_ptr=)`` is the definition as above, and ``count[k]`` the flagged
        survivors plus one.  A released lightpath sends no message, frees its channels for the candidate's cells, and
        the candidate may carry its ``conn_id``; a sample of 256 lightpaths is accepted when at least one is released.
        ``to_graph.placement_neighbourhood(release=)`` states the messages on the host.  More refusals: before any launch
        (``place_release_args``) only one of the two given, ``release`` not a 1-d int64 tensor on the chunk's device,
        ``release_ptr`` of the wrong length or dtype, a host ``release_ptr`` not non-decreasing from 0 to R or with a
        slice longer than 32; on the device a released conn the sample does not hold and a bad slice of a device
        ``release_ptr``.  Without the two keywords the call is the one above, through the same C entry."""
        who = "LightpathPredictor.place"
        shape = self._check_model()
        pa = lightpath_place_args(status, shape[0], self.model.is_lut_index, samples, values, cells, cell_ptr,
                                  features_to_consider, freq_threshold, who)
        ra = place_release_args(status, pa.K, release, release_ptr, who)
        sa = pa.status
        dev = self._status_device(status, who)
        out = torch.empty(pa.K, shape[2], dtype=torch.float32, device=dev)
        if pa.K == 0:
            return out, self._empty_count(shape)
        picks, ptr, *rptr = _place_index_lists(dev, pa.samples, pa.cell_ptr, *(() if ra is None else (ra.release_ptr,)))
        name, extra = "qot_lightpath_infer_place", ()
        if ra is not None:
            name, extra = "qot_lightpath_infer_place_release", (ra.release.contiguous(), rptr[0], ra.R)
        return out, self._launch_status(name, status, sa, shape, pa.K, picks, out, values.contiguous(), cells.contiguous(), ptr,
                                        pa.M, *extra)

    @torch.no_grad()
    def place_slots(self, status, samples, values, links, link_ptr, features_to_consider=to_graph.DEFAULT_FEATURES,
                    freq_threshold=0.05, *, width=1, slot_feature="freq", chunk=None):
        """The step before ``place``: given a route, which frequency slot?  Sweeps each of R routes over EVERY start slot
        of the grid, ``PlaceSlots(out [R, Q, O] float32, free [R, Q] bool, count [R] int64)`` in ONE kernel launch
        (``csrc/infer_lightpath_place_slots.hip``), with nothing read back and ``status.data`` never
        written; legal inside ``torch.cuda.graph`` capture under the conditions of ``place`` (index arguments as device
        tensors, one call made first).  First-fit is ``free.int().argmax(1)``, best predicted OSNR ``out[..., 0]
        .masked_fill(~free, -inf).argmax(1)``: neither needs the free slots on the host, nor K candidate lists that
        differ in one feature.  An occupied slot is an answer (``free == False``, a NaN row), NOT an error: it sets no
        status bit.

        ``status``, ``samples`` and ``values [R, P]`` (float64, on the device) are ``place``'s, one row per route.
        ``links [M]`` int64 on the device: link indices; route ``r`` is ``links[link_ptr[r]:link_ptr[r + 1]]`` -- non-empty,
        a duplicate link allowed, no cap on its length.  ``link_ptr``: R + 1 offsets, by ``cell_ptr``'s rules: a host
        sequence is checked here and uploaded, an int64 device tensor is used in place and checked by the kernel.
        ``width``: an int in ``1 ... 8``, the same for the whole call: the candidate that starts at slot ``q`` occupies the
        slots ``q ... q + width - 1`` on every link of its route (spectrum continuity and contiguity); a start slot ``q >
        Q - width`` is never free.  ``slot_feature``: the name of an ``lp_feat`` row, or ``None``.  With a name the
        candidate at start slot ``q`` carries ``status.freq[q]`` in that row in the place of ``values[r]``'s entry -- what
        ``synthetic_network_status`` writes for a lightpath; with ``None`` ``values[r]`` is used unchanged at every slot.

        ``infer.materialise_slot_sweep`` is the definition: with ``sw`` its answer, ``out[sw.route[k], sw.slot[k]]`` is,
        bit for bit, ``self.place(status, sw.samples, sw.values, sw.cells, sw.cell_ptr, ...)[0][k]``, every other row of
        ``out`` is NaN, ``free`` equals ``sw.free``, and ``count[r]`` is ``place``'s count -- the flagged lightpaths of the
        sample plus one, the same at every slot.  ``to_graph.slot_sweep`` states the free slots and each one's message
        sources on the host.  A route's rows depend on its sample and itself alone.

        ``chunk``: the start slots one workgroup runs one after the other, ``1 ... 32``; ``None``:
        ``place_slots_chunk(R, Q, compute_units)``.  Every result is bitwise independent of it.

        Refusals before any launch (``lightpath_place_slots_args``): ``TypeError`` for a ``status`` that is no
        ``DeviceStatus``; ``ValueError`` for ``values``, ``links``, ``samples`` or ``link_ptr`` of the wrong dtype, shape
        or device, a host ``link_ptr`` that is not non-decreasing from 0 to M or has an empty slice, a ``width`` outside
        ``1 ... 8``, a ``slot_feature`` that is no row of ``status.lp_feat`` or one of ``conn_id``, ``osnr``, ``snr``,
        ``ber``, a bad ``chunk`` or ``freq_threshold``; ``EnvelopeError`` for everything ``from_status`` refuses and for
        ``R * Q >= 2^31``.  ``R == 0`` or ``Q == 0`` gives empty tensors without a launch.  On the device, per route since
        nothing is read back: a sample number outside the chunk, a bad slice of a device ``link_ptr`` or a link index
        outside ``[0, L)``, a ``conn_id`` that is not finite or beyond +-2^53 in ``values[r]`` or in the sample,
        ``values[r]`` without ``osnr == snr == ber == -1``, a ``conn_id`` the sample holds already, a sample of 256
        lightpaths -- all Q rows of that route are NaN, all of ``free[r]`` False, ``count[r]`` 0, the other routes are
        untouched, and ``check_status()`` raises naming the cause with ``place``'s bits.

        Out of scope: ``release=``, a ``width`` per route, a sub-range of the slots, a sweep for
        ``TopologicalPredictor``, and spreading the rows of one workgroup over its four waves (the row routine's barriers
        depend on the message count, so a workgroup's rows are computed by one wave, as in ``retest``)."""
        who = "LightpathPredictor.place_slots"
        shape = self._check_model()
        pa = lightpath_place_slots_args(status, shape[0], self.model.is_lut_index, samples, values, links, link_ptr,
                                        features_to_consider, freq_threshold, width, slot_feature, chunk, who)
        sa = pa.status
        dev = self._status_device(status, who)
        R, Q, O = pa.R, sa.Q, shape[2]
        if R * Q >= 1 << 31:
            raise EnvelopeError(f"{who}: routes x frequency slots must stay below 2^31, got {R} x {Q}")
        out = torch.empty(R, Q, O, dtype=torch.float32, device=dev)
        free = torch.empty(R, Q, dtype=torch.bool, device=dev)
        if R == 0 or Q == 0:                                   # (Q == 0: no slot to count a sample's lightpaths at)
            return PlaceSlots(out, free, torch.zeros(R, dtype=torch.int64, device=dev))
        if chunk is None:
            chunk = place_slots_chunk(R, Q, torch.cuda.get_device_properties(dev).multi_processor_count)
        picks, ptr = _place_index_lists(dev, pa.samples, pa.link_ptr)
        count = self._launch_status("qot_lightpath_infer_place_slots", status, sa, shape, R, picks, out, values.contiguous(),
                                    links.contiguous(), ptr, pa.M, pa.slot_row, width, chunk, free)
        return PlaceSlots(out, free, count)

    @torch.no_grad()
    def place_impact(self, status, samples, values, cells, cell_ptr, features_to_consider=to_graph.DEFAULT_FEATURES,
                     freq_threshold=0.05, max_affected=8):
        """The admission decision's second half: ``place``'s rows together with a RETEST of the established lightpaths
        each candidate lands next to -- do they stay above their thresholds once it is lit? -- as ``PlaceImpact(out [K, O]
        float32, count [K] int64, affected [K, A] int64, n_affected [K] int64, before [K, A, O] float32, after [K, A, O]
        float32)`` with ``A = max_affected``, in ONE kernel launch (``csrc/infer_lightpath_place_impact.hip``, DESIGN.md
        4.25), with nothing read back and ``status.data`` never written; legal inside ``torch.cuda.graph`` capture under
        the conditions of ``place`` (index arguments as device tensors, one call made first).

        ``samples``, ``values``, ``cells``, ``cell_ptr``, ``features_to_consider`` and ``freq_threshold`` are ``place``'s,
        checked by the same routines.  ``out`` and ``count`` are ``place(...)``'s, bit for bit.  ``affected[k, :n]``, ``n =
        min(n_affected[k], A)``: the ``conn_id`` values of the lightpaths of sample ``samples[k]`` that interfere with
        candidate ``k``, in the sample's first-seen order -- ``to_graph.placement_neighbourhood``'s list, the message order
        of the candidate's row; the interference rule is symmetric, so they are the only lightpaths whose own
        neighbourhood the candidate changes.  ``n_affected[k]`` is their true number: more than ``A`` is no error, the
        first ``A`` are written.  ``before[k, i]``: the eval-mode row of lightpath ``affected[k, i]`` retested as the
        lightpath under test of the unedited sample; ``after[k, i]``: the same row once the candidate is established next
        to it (unflagged, ``is_lut`` 0).  The slots behind ``n`` hold -1 / NaN.

        ``materialise_retest`` is the definition: ``before[k, i]`` is, bit for bit, the row ``self(to_graph.device_batch(
        materialise_retest(status, [samples[k]], [affected[k, i]]), "lightpath", ...))`` gives the node of that conn, and
        ``after[k, i]`` the same with ``values[k:k + 1]``, the candidate's cells and ``[0, m]`` passed in as well;
        ``to_graph.placement_impact`` states the nodes and the messages on the host.  The sample's own flagged lightpath,
        if it has one, stays flagged: it may be one of the affected, and it carries ``is_lut = 1`` where it is a message
        source.

        Refusals before any launch (``lightpath_place_impact_args``): ``place``'s; ``ValueError`` for a ``max_affected``
        that is no int in ``1 ... PLACE_MAX_AFFECTED = 32``; ``EnvelopeError`` for a feature list that holds ``osnr``,
        ``snr`` or ``ber`` -- the retest rewrites those rows.  ``K == 0`` gives empty tensors without a launch.  On the
        device every refusal of ``place`` applies, with the same status bits: the refused candidate has a NaN ``out`` row,
        ``count`` 0, ``n_affected`` 0, ``affected`` all -1, ``before`` and ``after`` all NaN; the other candidates are
        untouched, and ``check_status()`` raises naming the cause.  There is no ``release=`` here: a reroute, or an
        admission together with a tear-down, is ``reroute_impact``'s."""
        who = "LightpathPredictor.place_impact"
        shape = self._check_model()
        pa = lightpath_place_impact_args(status, shape[0], self.model.is_lut_index, samples, values, cells, cell_ptr,
                                         features_to_consider, freq_threshold, max_affected, who)
        sa = pa.status
        dev = self._status_device(status, who)
        K, A, O = pa.K, max_affected, shape[2]
        out = torch.empty(K, O, dtype=torch.float32, device=dev)
        affected = torch.empty(K, A, dtype=torch.int64, device=dev)
        n_affected = torch.empty(K, dtype=torch.int64, device=dev)
        before = torch.empty(K, A, O, dtype=torch.float32, device=dev)
        after = torch.empty(K, A, O, dtype=torch.float32, device=dev)
        if K == 0:
            return PlaceImpact(out, self._empty_count(shape), affected, n_affected, before, after)
        picks, ptr = _place_index_lists(dev, pa.samples, pa.cell_ptr)
        count = self._launch_status("qot_lightpath_infer_place_impact", status, sa, shape, K, picks, out, values.contiguous(),
                                    cells.contiguous(), ptr, pa.M, affected, n_affected, before, after, A)
        return PlaceImpact(out, count, affected, n_affected, before, after)

    @torch.no_grad()
    def reroute_impact(self, status, samples, values, cells, cell_ptr, features_to_consider=to_graph.DEFAULT_FEATURES,
                       freq_threshold=0.05, max_affected=8, *, release=None, release_ptr=None):
        """``place_impact`` for a REROUTE, or an admission together with a tear-down: whom the move helps and whom it
        hurts, as ``RerouteImpact(out [K, O] float32, count [K] int64, affected [K, A] int64, n_affected [K] int64, before
        [K, A, O] float32, after [K, A, O] float32, gains [K, A] bool, lost [K, A] int64)`` with ``A = max_affected``, in
        ONE kernel launch (``csrc/infer_lightpath_reroute_impact.hip``), with nothing read back and
        ``status.data`` never written; legal inside ``torch.cuda.graph`` capture under the conditions of ``place`` (index
        arguments as device tensors, one call made first).  Restoration after a link failure, defragmentation, "admit A
        by tearing down B": the lightpaths beside the new route gain an interferer, those beside the old route lose one.

        The arguments are ``place(..., release=, release_ptr=)``'s, checked by the same routines, plus ``max_affected``
        (``place_impact``'s).  ``release=None``: no candidate releases anything.  ``out`` and ``count`` are ``place(...,
        release=, release_ptr=)``'s, bit for bit.  The affected lightpaths of candidate ``k`` are the SURVIVORS of its
        sample (the lightpaths it does not release) that (a) interfere with the candidate --
        ``to_graph.placement_neighbourhood(..., release=)``'s list -- or (b) interfere, in the unedited sample, with a
        released lightpath; a released lightpath is never affected.  ``affected[k, :n]``, ``n = min(n_affected[k], A)``:
        their ``conn_id`` values in the sample's first-seen order; ``n_affected[k]`` is their true number, more than ``A``
        is no error.  ``before[k, i]``: the eval-mode row of lightpath ``affected[k, i]`` retested in the unedited sample
        (``place_impact``'s ``before``: the released lightpaths still send their messages).  ``after[k, i]``: the same row
        in the sample with the release applied and the candidate established (unflagged, ``is_lut`` 0): the surviving
        sources in the survivors' order, the candidate's row at its first-seen position among them where the lightpath
        gains the candidate.  ``gains[k, i]``: the candidate is a source of ``after``.  ``lost[k, i]``: the released
        lightpaths that were sources of ``before`` (a conn named twice counts once).  The slots behind ``n`` hold -1
        (``affected``, ``lost``), NaN and False.

        ``materialise_retest`` is the definition: ``before[k, i]`` is, bit for bit, the row ``self(to_graph.device_batch(
        materialise_retest(status, [samples[k]], [affected[k, i]]), "lightpath", ...))`` gives the node of that conn, and
        ``after[k, i]`` the same with ``values[k:k + 1]``, the candidate's cells, ``[0, m]`` and its release slice
        (``release=, release_ptr=[0, r]``) passed in as well; ``to_graph.reroute_impact`` states the nodes, the messages,
        ``gains`` and ``lost`` on the host.

        Refusals before any launch: ``place_impact``'s (``lightpath_place_impact_args``) and those of ``place``'s
        release lists (``place_release_args``).  ``K == 0`` gives empty tensors without a launch.  On the device every
        refusal of ``place(release=)`` applies, with the same status bits: the refused candidate has a NaN ``out`` row,
        ``count`` 0, ``n_affected`` 0, ``affected`` and ``lost`` all -1, ``gains`` False, ``before`` and ``after`` all
        NaN; the other candidates are untouched, and ``check_status()`` raises naming the cause.  There is no pure
        tear-down (a candidate needs a cell), and the rows of one candidate are computed by one wave."""
        who = "LightpathPredictor.reroute_impact"
        shape = self._check_model()
        pa = lightpath_place_impact_args(status, shape[0], self.model.is_lut_index, samples, values, cells, cell_ptr,
                                         features_to_consider, freq_threshold, max_affected, who)
        ra = place_release_args(status, pa.K, release, release_ptr, who)
        sa = pa.status
        dev = self._status_device(status, who)
        K, A, O = pa.K, max_affected, shape[2]
        out = torch.empty(K, O, dtype=torch.float32, device=dev)
        affected = torch.empty(K, A, dtype=torch.int64, device=dev)
        n_affected = torch.empty(K, dtype=torch.int64, device=dev)
        before = torch.empty(K, A, O, dtype=torch.float32, device=dev)
        after = torch.empty(K, A, O, dtype=torch.float32, device=dev)
        gains = torch.empty(K, A, dtype=torch.bool, device=dev)
        lost = torch.empty(K, A, dtype=torch.int64, device=dev)
        if K == 0:
            return RerouteImpact(out, self._empty_count(shape), affected, n_affected, before, after, gains, lost)
        picks, ptr, *rptr = _place_index_lists(dev, pa.samples, pa.cell_ptr, *(() if ra is None else (ra.release_ptr,)))
        rel = (None, None, 0) if ra is None else (ra.release.contiguous(), rptr[0], ra.R)
        count = self._launch_status("qot_lightpath_infer_reroute_impact", status, sa, shape, K, picks, out, values.contiguous(),
                                    cells.contiguous(), ptr, pa.M, *rel, affected, n_affected, before, after, gains, lost, A)
        return RerouteImpact(out, count, affected, n_affected, before, after, gains, lost)

    @torch.no_grad()
    def sensitivity(self, data, outputs=None, *, per_graph=False, return_attention_weights=False):
        """The rows of ``predict(data)`` together with their Jacobian wrt the node features of each row's one-hop
        in-neighbourhood, in ONE kernel launch: returns ``(out [L, O], lut_batch [L], jac_self [Q, L, F], jac_edge [Q, E,
        F])``; with ``per_graph=True`` ``(out [B, O], count [B], jac_self [Q, B, F], jac_edge)`` -- the rows of
        ``predict.per_graph(data)``.  ``out`` and ``lut_batch`` / ``count`` are those calls' results bit for bit.

        ``jac_edge[q, e, :]``, in the order of ``data.edge_index``: for an edge ``e`` that is a message into a computed row
        ``r`` (``dst(e)`` is the row's node and ``src(e) != dst(e)``), ``d out[r, outputs[q]] / d x[src(e), :]`` through that
        message; repeated edges are separate messages with a share each.  Every other edge holds exactly 0: input self
        loops (PyG removes them), edges into non-LUT nodes and, with ``per_graph=True``, edges into the LUT nodes behind a
        graph's first.  ``jac_self[q, r, :]``: the derivative wrt the row's own features -- the appended self loop's
        message and logit, and the destination term of every message's logit.  Together they are ``x.grad``: with
        ``J = zeros(N, F)``, ``J.index_add_(0, edge_index[0], jac_edge[q]); J[lut_idx] += jac_self[q]`` is what
        ``model.eval()(data)[0][:, outputs[q]].sum().backward()`` leaves in ``data.x.grad`` (the LUT selection is a
        constant: the ``is_lut`` column gets its plain derivative; ``leaky_relu`` / ``relu`` at 0 as torch).

        ``outputs``: ``None`` (all, in order) or a non-empty list of distinct integers in ``0 ... O - 1``; ``Q`` of them.
        ``return_attention_weights=True``: also ``(alpha_self [L or B, 4], alpha_edge [E, 4])``, conv1's softmax weights of
        each row's self loop and of the message edges (0 on every other edge): the values ``model(data,
        return_attention_weights=True)`` gives those ``(source, target)`` pairs.

        Plain tensors without ``grad_fn``; pure (no model state is touched); parameters and running statistics are read
        at call time.  No atomics: every element has one owning wave and every sum a fixed order, so the result is
        bitwise reproducible and a row's slices do not depend on the other graphs of the batch or on the mode.  The
        kernel writes only the message edges: the zeros elsewhere are ``torch.zeros`` allocations of ``jac_edge`` (and
        ``alpha_edge``), ONE FILL EACH in front of the one kernel launch.  With ``per_graph=True`` there is no host read,
        and the call is legal inside ``torch.cuda.graph`` capture under ``per_graph``'s condition (single stream); a graph
        without a LUT node has ``count == 0``, NaN in its ``out`` and ``jac_self`` rows and zeros in its ``jac_edge``
        slice.  (A selection other than ``None`` is uploaded once, on its first call: make that call before capturing.)

        Refusals as ``__call__`` (``EnvelopeError``; the LUT-less ``ValueError`` / ``allow_empty_lut`` in rows mode).  A
        flagged row (``check_status()`` raises) has NaN in its ``out`` and ``jac_self`` rows and, its graph's edge slice
        being valid, over that slice of ``jac_edge`` / ``alpha_edge``."""
        # the model's shape, then the argument, are named before the model's device and the batch are looked at
        shape = self._check_model()
        sel = grad_outputs(outputs, shape[2], "LightpathPredictor.sensitivity")
        p = self._prepare(data, per_graph, shape)
        E, Q, rows, dev = p.ei.shape[1], len(sel), p.rows, p.dev
        out = torch.empty(rows, p.O, dtype=torch.float32, device=dev)
        jac_self = torch.empty(Q, rows, p.F, dtype=torch.float32, device=dev)
        jac_edge = torch.zeros(Q, E, p.F, dtype=torch.float32, device=dev)
        alpha = (None, None)
        if return_attention_weights:
            alpha = (torch.empty(rows, LP_HEADS, dtype=torch.float32, device=dev),
                     torch.zeros(E, LP_HEADS, dtype=torch.float32, device=dev))
        second = self._launch("qot_lightpath_infer_grad", p, out, self._outputs(sel, dev), Q, jac_self, jac_edge, *alpha)
        res = (out, second, jac_self, jac_edge)
        return res + (alpha,) if return_attention_weights else res

    @torch.no_grad()
    def what_if(self, data, x_lut=None, add_src=None, add_ptr=None, drop=None, drop_ptr=None, node=None):
        """"What if": scores K candidate lightpaths in ONE kernel launch, ``(out [K, O], lut_batch [K])``, without building
        the candidates' graphs.  Setting up a lightpath means choosing among K (route, spectrum slot) assignments; each
        changes the LUT node's own features and the set of established lightpaths it interferes with (its in-neighbours).

        Candidate ``k`` is about node ``node[k]`` (int64 ``[K]``, the batch's node numbering; several candidates may name
        the same node) and that node's graph.  ``node=None``: the model's LUT rows, ``K == L`` and candidate ``k`` is row
        ``k`` (with the model's LUT-less ``ValueError`` / ``allow_empty_lut``).  It replaces the node's feature row by
        ``x_lut[k]`` (``[K, F]`` float32; ``None`` keeps it; the effective row must hold ``1.0`` in column ``is_lut_index``),
        removes the edges at positions ``drop[drop_ptr[k]:drop_ptr[k + 1]]`` of ``data.edge_index`` (any order, a repeat
        counts once, at most ``WHAT_IF_MAX_DROP`` = 32 per candidate; inside the graph's edge slice; an edge that is no
        message into the node changes nothing) and appends the messages ``add_src[add_ptr[k]:add_ptr[k + 1]] -> node[k]``
        behind the surviving edges in the order given (int64 node numbers of the batch, inside the graph; the node itself
        is an input self loop and no message; a source that sends already sends once more; no cap on their number).

        ``materialise_lightpath_what_if`` is the definition: ``out[k]`` is, bit for bit, the row of ``self(batch)`` that
        belongs to node ``node_new[k]`` of the batch it builds; ``lut_batch`` is ``data.batch[node]``.  A candidate's row
        does not depend on the other candidates, and one without an edit is ``self(data)``'s row of that node.  Every
        candidate rescans its graph's edge slice: O(m) per candidate, candidates of one node do not share the scan.

        ``add_src`` with ``add_ptr``, ``drop`` with ``drop_ptr``: both or neither.  Hand the pointer arrays over as lists or
        host tensors: they are checked on the host, a device tensor costs one read each.  With neither list, K comes
        from ``x_lut``, ``node`` or L.

        Plain tensor without ``grad_fn``; pure (no model state is touched); parameters and running statistics are read at
        call time.  ``K == 0`` gives ``[0, O]`` without a launch.  Capture inside ``torch.cuda.graph`` is not claimed.
        Refusals, before any launch: ``EnvelopeError`` for everything ``__call__`` refuses; ``ValueError`` naming the
        condition for a bad shape or dtype of ``x_lut``, ``add_src``, ``drop`` or ``node``, pointer arrays not non-decreasing
        from 0 to A (R), candidate counts that disagree between the arguments, more than 32 removals in one candidate.
        On the device: an added source outside the candidate's graph (status bit 0), a ``node[k]`` outside ``0 ... N - 1``
        (``lut_batch[k]`` is -1 then) or a drop position outside the graph's slice (bit 1), an effective feature row whose
        LUT column is not exactly ``1.0`` (bit 2) give NaN in that candidate's row only, and ``check_status()`` raises."""
        who = "LightpathPredictor.what_if"
        # the model's shape, then the arguments, are named before the model's device and the batch are looked at
        shape = self._check_model()
        w = lightpath_what_if_args(shape[0], x_lut, add_src, add_ptr, drop, drop_ptr, node, who)
        p = self._prepare(data, False, shape, node)
        dev, K = p.dev, p.rows
        if w.K is not None and w.K != K:
            raise ValueError(f"{who}: the arguments name {w.K} candidates, the batch has {K} LUT rows (node=None: "
                             f"candidate k is LUT row k)")
        out = torch.empty(K, p.O, dtype=torch.float32, device=dev)

        def on_dev(given):
            return _i64(given, dev) if isinstance(given, torch.Tensor) and given.device == dev else None
        xl = None if x_lut is None else _f32c(x_lut if x_lut.device == dev else x_lut.to(dev))
        src = aptr = dpos = dptr = None
        if w.A:
            src, aptr = _i64(add_src, dev), on_dev(add_ptr)
        if w.R:
            dpos, dptr = _i64(drop, dev), on_dev(drop_ptr)
        if w.A and w.R and aptr is None and dptr is None:   # both pointer arrays are on the host: one upload for the two
            both = torch.cat([w.add_ptr, w.drop_ptr]).to(dev)
            aptr, dptr = both[:K + 1], both[K + 1:]
        elif w.A and aptr is None:
            aptr = w.add_ptr.to(dev)
        elif w.R and dptr is None:
            dptr = w.drop_ptr.to(dev)
        return out, self._launch("qot_lightpath_infer_whatif", p, out, xl, src, aptr, w.A, dpos, dptr, w.R, K,
                                 inside=node is None)
