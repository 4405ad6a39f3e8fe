"""Train / evaluate loops with the behaviour of the reference scripts, driving the HIP models.

Counterpart of ``topological_training/train.py``, ``lightpath_training/train.py`` and the two
``test.py``.  What is kept from the reference: the 70/15/15 split without
shuffling (train.py:29-36), one 10 % chunk of the training range per epoch (train.py:79-90),
SGD(lr=0.1, momentum=0.9) with StepLR(step_size=10, gamma=0.5) (train.py:66-67), SmoothL1 loss
(train.py:69), sample-weighted epoch loss and uniform-average R2 (train.py:119-131), early stopping on
validation R2 with patience 10 and a best-model file (train.py:168-178), the checkpoint dictionary
(train.py:196-209), LUT target selection and batch skipping for LightpathGNN
(lightpath_training/train.py:112-135), min-max descaling and per-output R2 / MSE at test time
(topological_training/test.py:88-108).

What is different, because the device is an MI355X and not a laptop CPU: batches come from
``GraphLoader`` (pinned, prefetched), nothing in the batch loop reads a value back to the host -- the
loss sum and the R2 sufficient statistics accumulate on the device and are fetched once per epoch --
and the optimizer is one fused kernel over the flat parameter buffer.  With ``torch.distributed``
initialised every rank takes its share of each batch range and the statistics are summed over ranks.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from .dp import FlatModel, FusedSGD, graph_range, loss_scale
from .loader import GraphLoader, PackedGraphs, StageSlot, check_stage_status, uniform_node_count

# data constants of the reference's label scaling (constants.py:8-12), used at test.py:95-99
TARGET_RANGES = {
    "osnr": {"min": 12.47, "max": 33.49},
    "snr": {"min": 8.96, "max": 29.98},
    "ber": {"min": 1.70e-12, "max": 1.98e-2},
}


def split_ranges(total: int) -> Tuple[range, range, range]:
    """70 / 15 / 15 split in dataset order (train.py:29-36)."""
    tr = int(total * 0.7)
    va = int(total * 0.15)
    return range(0, tr), range(tr, tr + va), range(tr + va, total)


def epoch_chunk(epoch: int, train_len: int, fraction: float = 0.10) -> range:
    """The slice of the training range epoch ``epoch`` sees (train.py:79-90)."""
    num_chunks = int(1 / fraction)
    size = train_len // num_chunks
    start = (epoch % num_chunks) * size
    return range(start, min(start + size, train_len))


def step_lr(base_lr: float, epoch: int, step_size: int = 10, gamma: float = 0.5) -> float:
    """Learning rate in effect during ``epoch`` under StepLR stepped once per epoch (train.py:67,181)."""
    return base_lr * gamma ** (epoch // step_size)


class RegressionStats:
    """Streaming sufficient statistics for R2 and MSE, held on the device.

    ``sklearn.metrics.r2_score(..., multioutput=...)`` (train.py:127, test.py:106) needs only
    n, sum(y), sum(y^2) and sum((y - yhat)^2) per output; fp64 accumulators, one host read at the end.
    """

    def __init__(self, outputs: int, device):
        self.buf = torch.zeros(3 * outputs + 2, dtype=torch.float64, device=device)   # sy | syy | sse | n | loss*n
        self.o = outputs

    def update(self, y: torch.Tensor, yhat: torch.Tensor, loss: Optional[torch.Tensor] = None):
        y = y.detach().to(torch.float64)
        d = y - yhat.detach().to(torch.float64)
        n = y.shape[0]
        o = self.o
        self.buf[:o] += y.sum(0)
        self.buf[o:2 * o] += (y * y).sum(0)
        self.buf[2 * o:3 * o] += (d * d).sum(0)
        self.buf[3 * o] += n
        if loss is not None:
            self.buf[3 * o + 1] += loss.detach().to(torch.float64) * n

    def all_reduce(self):
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.buf, op=dist.ReduceOp.SUM)

    def result(self, scale: Optional[torch.Tensor] = None) -> Dict[str, object]:
        """``scale`` (per-output max-min) reports MSE in descaled units (test.py:93-108); R2 is invariant."""
        b = self.buf.cpu()
        o = self.o
        n = float(b[3 * o])
        if n == 0:
            nan = float("nan")
            return {"n": 0, "r2_raw": [nan] * o, "r2": nan, "mse_raw": [nan] * o, "loss_sum": 0.0}
        sy, syy, sse = b[:o], b[o:2 * o], b[2 * o:3 * o]
        sst = syy - sy * sy / n
        # sklearn: constant target -> 1.0 if perfect else 0.0
        r2 = torch.where(sst > 0, 1.0 - sse / sst.clamp_min(1e-300),
                         torch.where(sse == 0, torch.ones_like(sse), torch.zeros_like(sse)))
        mse = sse / n
        if scale is not None:
            mse = mse * scale.to(torch.float64).cpu() ** 2
        return {"n": int(n), "r2_raw": r2.tolist(), "r2": float(r2.mean()), "mse_raw": mse.tolist(),
                "loss_sum": float(b[3 * o + 1])}


def _targets_topological(model, data, out_dim):
    out = model(data)
    return out, data.y.view(-1, out_dim)


def _targets_lightpath(model, data, out_dim):
    out, lut_batch = model(data)            # ValueError when the batch has no LUT node (models.py:35-36)
    return out, data.y.view(-1, out_dim)[lut_batch]


_KINDS = {"topological": _targets_topological, "lightpath": _targets_lightpath}


@dataclass
class History:
    loss: List[float] = field(default_factory=list)
    val_loss: List[float] = field(default_factory=list)
    r2: List[float] = field(default_factory=list)
    val_r2: List[float] = field(default_factory=list)
    skipped_graphs: int = 0
    stopped_early: bool = False
    best_val_r2: float = float("-inf")
    epochs_run: int = 0
    # how the steps of a replayed run were issued (``StepReplayer.counts``): visits run eagerly / captured (and replayed
    # once) / replayed, and the number of captured graphs the run holds at its end; empty without a replayer
    replay_counts: Dict[str, int] = field(default_factory=dict)

    def dump(self, directory: str):
        """loss_history.json etc. as the reference writes them (train.py:213-226)."""
        os.makedirs(directory, exist_ok=True)
        for name, vals in (("loss_history", self.loss), ("val_loss_history", self.val_loss),
                           ("r2_history", self.r2), ("val_r2_history", self.val_r2)):
            with open(os.path.join(directory, name + ".json"), "w") as f:
                json.dump(vals, f)


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _graph_costs(dataset, idx: Sequence[int]):
    """Per-graph edge counts of ``idx`` when the dataset is a pre-tensorised shard (else None: split by count)."""
    if isinstance(dataset, PackedGraphs) and len(idx):
        e = (dataset.edge_ptr[1:] - dataset.edge_ptr[:-1])
        return e[torch.as_tensor(list(idx), dtype=torch.long)].to(torch.float64)
    return None


def _local_batches(idx: Sequence[int], batch_size: int, rank: int, world: int, costs=None) -> List[List[int]]:
    """One entry per GLOBAL batch of ``batch_size`` graphs: this rank's contiguous share of it (possibly empty
    when a trailing batch holds fewer graphs than there are ranks).  Every rank gets the same number of
    entries, so every rank issues the same sequence of collectives, and a step is the single-process step
    over the same global batch.  ``costs`` (per-graph edge counts, aligned with ``idx``): the cut inside each global
    batch evens out edges instead of graph counts."""
    out: List[List[int]] = []
    for b0 in range(0, len(idx), batch_size):
        n = min(batch_size, len(idx) - b0)
        lo, hi = graph_range(n, rank, world, costs=None if costs is None or world == 1 else costs[b0:b0 + n])
        out.append(list(idx[b0 + lo:b0 + hi]))
    return out


def batch_ranges(indices: range, batch_size: int) -> List[Tuple[int, int]]:
    """``[lo, hi)`` of every batch of ``batch_size`` consecutive graphs of ``indices`` (a ``range`` with step 1), in order."""
    if not isinstance(indices, range) or indices.step != 1:
        raise ValueError("streamed replay walks consecutive graphs: indices must be a range with step 1")
    return [(b0, min(b0 + batch_size, indices.stop)) for b0 in range(indices.start, indices.stop, batch_size)]


def batch_shape(node_ptr: torch.Tensor, edge_ptr: torch.Tensor, lo: int, hi: int) -> Tuple[int, int, int]:
    """``(B, N, E)`` of graphs ``[lo, hi)``: what decides which static slot (and which captured graph) runs them."""
    return hi - lo, int(node_ptr[hi]) - int(node_ptr[lo]), int(edge_ptr[hi]) - int(edge_ptr[lo])


def stream_schedule(node_ptr: torch.Tensor, edge_ptr: torch.Tensor, ranges: Sequence[Tuple[int, int]]
                    ) -> Dict[Tuple[int, int, int], List[int]]:
    """The batches of one epoch grouped by shape: ``{(B, N, E): [lo, ...]}``, every list in visiting order (pure host
    arithmetic on the shard's offsets).  One static slot and one captured graph serve each key."""
    out: Dict[Tuple[int, int, int], List[int]] = {}
    for lo, hi in ranges:
        out.setdefault(batch_shape(node_ptr, edge_ptr, lo, hi), []).append(lo)
    return out


def _plan_of_totals(totals: Dict[int, List[int]], n: int, max_m: int, option: str) -> Dict[int, Dict[str, object]]:
    """The plan of ``stream_pad_plan`` from the edge totals of every batch, per graph count: ``{B: [edge totals]}`` of graphs
    of ``n`` nodes and at most ``max_m`` edges; ``option`` names the caller's option in the refusal."""
    plan: Dict[int, Dict[str, object]] = {}
    for B, es in totals.items():
        e_cap, e_min = max(es), min(es)
        P = 0 if e_cap == e_min else -(-(e_cap - e_min) // max_m)
        if P and n < 2:
            raise ValueError(f"{option} needs graphs of at least 2 nodes (a pad graph is a ring without self loops)")
        plan[B] = {"E_cap": e_cap, "E_min": e_min, "P": P, "shape": (B + P, (B + P) * n, e_cap)}
    return plan


def stream_pad_plan(node_ptr: torch.Tensor, edge_ptr: torch.Tensor, ranges: Sequence[Tuple[int, int]],
                    graph_sizes: Tuple[int, int]) -> Dict[int, Dict[str, object]]:
    """Padded slots for the batches ``ranges`` of a shard whose graphs all have ``n`` nodes, per graph count ``B``:
    ``{B: {"E_cap", "E_min", "P", "shape"}}`` -- ``E_cap`` / ``E_min`` the largest / smallest edge total of a batch of
    ``B`` graphs, ``P = ceil((E_cap - E_min) / max_m)`` pad graphs (``max_m = graph_sizes[1]``, the shard's largest
    per-graph edge count: a pad graph never exceeds it), ``shape = (B + P, (B + P) n, E_cap)`` the one slot that takes
    them all.  Equal totals give ``P = 0`` and the exact shape.  Pure host arithmetic on the offsets; ``ValueError`` for
    mixed node counts (the pad graphs, ``node_ids`` in table mode and the graph form of TransformerConv take one ``n``)."""
    n = uniform_node_count(node_ptr)
    if n is None:
        raise ValueError("pad_edges=True needs a shard whose graphs all have the same node count (mixed node counts keep "
                         "stream=True with exact-shape slots)")
    totals: Dict[int, List[int]] = {}
    for lo, hi in ranges:
        totals.setdefault(hi - lo, []).append(int(edge_ptr[hi]) - int(edge_ptr[lo]))
    return _plan_of_totals(totals, n, int(graph_sizes[1]), "pad_edges=True")


def epoch_order(indices: range, seed: int, epoch: int) -> List[int]:
    """The order in which a shuffled epoch ``epoch`` visits the graphs ``indices``: a permutation of them drawn from a CPU
    generator seeded from ``(seed, epoch)`` alone.  A pure host function, so the padding plan, the streamed run and the
    eager loop of a host dataset all see the same orders."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed((int(seed) * 1000003 + int(epoch)) % (1 << 63))
    idx = list(indices)
    return [idx[i] for i in torch.randperm(len(idx), generator=gen).tolist()]


def fit_train_chunks(total: int, chunk_fraction: float, num_epochs: int) -> List[range]:
    """The graphs each of the ``num_epochs`` epochs of ``fit`` trains on, as ranges of dataset indices."""
    tr, _, _ = split_ranges(total)
    out = []
    for epoch in range(num_epochs):
        chunk = epoch_chunk(epoch, len(tr), chunk_fraction)
        out.append(range(tr[0] + chunk[0], tr[0] + chunk[-1] + 1) if len(chunk) else range(0))
    return out


def stream_shuffle_plan(node_ptr: torch.Tensor, edge_ptr: torch.Tensor, chunks: Sequence[range], batch_size: int, seed: int,
                        graph_sizes: Tuple[int, int]) -> Dict[int, Dict[str, object]]:
    """Gather slots for the shuffled training batches of a run, per graph count ``B``, in the format of
    ``stream_pad_plan``.  ``chunks[e]`` are the graphs epoch ``e`` trains on; its batches are consecutive pieces of
    ``epoch_order(chunks[e], seed, e)``.  ``E_cap`` / ``E_min`` are the largest / smallest edge total over EVERY batch of
    EVERY epoch -- the orders are known up front, so this is host arithmetic on the edge counts -- and
    ``P = ceil((E_cap - E_min) / max_m)``.  The totals of random subsets concentrate around ``B`` times the mean edge count, so
    ``P`` stays far below the worst case (the ``B`` largest graphs against the ``B`` smallest), which is not used."""
    n = uniform_node_count(node_ptr)
    if n is None:
        raise ValueError("shuffle=True on a resident shard needs graphs that all have the same node count")
    counts = (edge_ptr[1:] - edge_ptr[:-1]).tolist()
    totals: Dict[int, List[int]] = {}
    for epoch, chunk in enumerate(chunks):
        order = epoch_order(chunk, seed, epoch)
        for b0 in range(0, len(order), batch_size):
            ids = order[b0:b0 + batch_size]
            totals.setdefault(len(ids), []).append(sum(counts[g] for g in ids))
    return _plan_of_totals(totals, n, int(graph_sizes[1]), "shuffle=True")


def check_shuffle(dataset, kind: str, world: int, stream, pad_edges) -> None:
    """``shuffle=True``: a single process; on an HBM-resident shard the batches are gathered on the device, which needs
    ``stream=True, pad_edges=True`` and everything those need.  A host dataset takes the eager loop."""
    if world != 1:
        raise ValueError("shuffle=True needs a single process: every rank would have to gather its share of every batch")
    if not (isinstance(dataset, PackedGraphs) and dataset.device is not None):
        if stream or pad_edges:
            raise ValueError("stream=True needs an HBM-resident shard (PackedGraphs.to_device); shuffle=True on a host "
                             "dataset runs the eager loop")
        return
    if kind != "topological":
        raise ValueError("shuffle=True on a resident shard needs kind='topological' (streamed replay does)")
    if not stream or not pad_edges:
        raise ValueError("shuffle=True on a resident shard needs stream=True, pad_edges=True: shuffled batches are gathered "
                         "on the device into padded slots (or keep the shard on the host: PackedGraphs.pin)")
    if uniform_node_count(dataset.node_ptr) is None:
        raise ValueError("shuffle=True on a resident shard needs graphs that all have the same node count")


def fit_batch_ranges(total: int, batch_size: int, chunk_fraction: float) -> List[Tuple[int, int]]:
    """Every batch ``fit`` can ever run on a dataset of ``total`` graphs: all training chunks, then the validation range."""
    tr, va, _ = split_ranges(total)
    out: List[Tuple[int, int]] = []
    for epoch in range(int(1 / chunk_fraction)):
        chunk = epoch_chunk(epoch, len(tr), chunk_fraction)
        if len(chunk):
            out += batch_ranges(range(tr[0] + chunk[0], tr[0] + chunk[-1] + 1), batch_size)
    return out + batch_ranges(va, batch_size)


def check_pad_edges(dataset, kind: str, world: int, stream) -> None:
    """``pad_edges=True`` needs ``stream=True``, everything ``stream=True`` needs, and graphs of one node count."""
    if not stream:
        raise ValueError("pad_edges=True needs stream=True: the padding belongs to the static slots of streamed replay")
    check_stream(dataset, kind, world)
    if uniform_node_count(dataset.node_ptr) is None:
        raise ValueError("pad_edges=True needs a shard whose graphs all have the same node count (mixed node counts keep "
                         "stream=True with exact-shape slots)")


def check_stream(dataset, kind: str, world: int) -> None:
    """``stream=True`` needs a TopologicalGNN run on an HBM-resident shard in a single process."""
    if kind != "topological":
        raise ValueError("stream=True needs kind='topological': LightpathGNN's LUT row count is data-dependent and its "
                         "skip rule is decided on the host per batch (it keeps the per-batch replay)")
    if not isinstance(dataset, PackedGraphs) or dataset.device is None:
        raise ValueError("stream=True needs an HBM-resident shard (PackedGraphs.to_device): batches are staged on the "
                         "device from the shard's flat tensors")
    if world != 1:
        raise ValueError("stream=True needs a single process: a data-parallel rank's share and loss scale are per "
                         "batch (it keeps the per-batch replay)")


def _check_options(dataset, kind: str, world: int, stream, pad_edges, shuffle) -> None:
    """The option checks of ``fit``, ``run_epoch`` and ``StepReplayer``, in their one order: shuffle, then pad_edges (which
    checks what ``stream=True`` needs itself), else stream."""
    if shuffle:
        check_shuffle(dataset, kind, world, stream, pad_edges)
    if pad_edges:
        check_pad_edges(dataset, kind, world, stream)
    elif stream:
        check_stream(dataset, kind, world)


class StepReplayer:
    """HIP-graph replay of whole steps over the cached batches of an HBM-resident shard.

    The reference revisits the same unshuffled chunks for 35 epochs (``train.py:79-95``).  With the shard in
    HBM and the batch objects cached, a step's inputs are the SAME device tensors on every visit, so the
    whole step (forward, loss, backward, optimizer update, statistics) is captured once per batch and
    replayed afterwards: no Python, no launches, no allocation on later visits.  First visit of a key -- a batch
    object here, a slot under streamed replay -- runs eagerly (it also builds and caches the graph index), the second
    is captured, later ones replay (``_cycle``, the one state machine of both).
    All captures share one memory pool (steps never overlap), the learning rate lives in device memory
    (``FusedSGD(device_lr=True)``), dropout draws come from the device-side counter.  Batches whose
    forward raises (``ValueError``: no LUT node) are remembered and skipped; on later visits of such a training batch only
    its train-mode forward runs (eagerly), because that forward moves the BatchNorm running statistics before it raises.
    Data parallel (r04): RCCL takes part in stream capture, so with ``collective=True`` (set by ``fit`` for a TopologicalGNN
    run on more than one rank over the nccl backend) the captured step holds forward, backward, the pack of the gradients,
    ONE all-reduce of the flat gradient and the update -- the N > 1 step is the N = 1 step plus that exchange.  Every rank
    must visit the same sequence of batches (``_local_batches`` guarantees it).  LightpathGNN under data parallelism keeps
    the eager loop: its BatchNorm exchange and the LUT skip are decided per global batch on the host.

    Streamed replay (``stream=True`` with the resident ``shard``; TopologicalGNN, single process): one captured graph per
    batch SHAPE and direction instead of one per batch object.  ``run`` then takes a range ``(lo, hi)``; every batch goes
    through the static slot of its ``(B, N, E, training)`` (``loader.StageSlot``): the captured graph is ``stage + step``,
    the stage launch takes its ``lo`` from the slot's device-side schedule (``begin_epoch`` writes it once per epoch), so
    every batch of a shape -- first visits and single-epoch runs included -- replays the same graph, and the run holds
    as many graphs, cached indices and pool blocks as it has distinct shapes.  CACHE RULE: the stage launch rewrites the
    slot's tensors through raw pointers, their ``_version`` never moves, and every per-batch cache of ``graph.py`` (``graph_index_for``, ``batch_ptr_for``,
    ``cached_i32``, ``table_maps_for``, the checked node ids) is keyed by ``(data_ptr, _version, shape)``: left alone
    they would serve the PREVIOUS batch's index.  So the slot's ``_qot_cache`` is emptied before the eager visit and
    before the capture; the index build, the int32 narrowing and the table maps are then recorded inside the graph and
    run again on every replay.  No staged batch goes through host-side checks: the stage launch validates on the device
    and ``end_epoch`` raises from its status word (and from the index build's) once per epoch.

    Padded slots (``pad_edges=True`` on top of ``stream=True``; graphs of one node count): batches of ``B`` graphs whose
    edge totals differ share ONE slot and one captured graph per ``(B, training)``.  ``plan_padding(ranges)`` -- once,
    over every batch the run will ever see -- fixes ``E_cap`` and the number ``P`` of pad graphs per ``B``
    (``stream_pad_plan``); the slot (``loader.PaddedStageSlot``) holds ``B + P`` graphs and the staging launch appends pad
    graphs that take the spare edges.  The graphs of a batch are independent, the step takes ``out[:B]`` before the
    loss, its gradient and the statistics, so the pad rows of the output's gradient are zero and with them everything
    the pad graphs add to a parameter gradient.

    Shuffled epochs (``shuffle=True`` on top of ``stream=True, pad_edges=True``): the training slots are gather slots
    (``loader.GatherStageSlot``), whose schedule is the epoch's ORDER of graph ids instead of offsets;
    ``begin_epoch(ranges, True, order=...)`` writes it, ``plan_shuffle(chunks, batch_size)`` fixes ``E_cap`` and ``P`` over
    every batch of every epoch (``stream_shuffle_plan``).  Batches of arbitrary graphs never repeat, and still every
    step replays the one graph of its ``(graph count, direction)``.  A gathered batch is block-diagonal with graphs of
    ``n`` nodes and at most ``max_m`` edges, as a consecutive one: the model needs nothing new.  Validation stays
    consecutive on padded slots.
    """

    def __init__(self, model, kind: str, out_dim: int, device, flat: Optional[FlatModel], opt: Optional[FusedSGD],
                 collective: bool = False, stream: Optional[bool] = None, shard: Optional[PackedGraphs] = None,
                 pad_edges: Optional[bool] = None, shuffle: Optional[bool] = None, seed: int = 0):
        self.model, self.kind, self.out_dim, self.device = model, kind, out_dim, device
        self.stream = bool(stream)
        self.pad_edges = bool(pad_edges)
        self.shuffle, self.seed = bool(shuffle), int(seed)
        self.shuffle_plan: Dict[int, Dict[str, object]] = {}   # per graph count B of the training batches (plan_shuffle)
        _check_options(shard, kind, 2 if collective else 1, self.stream, self.pad_edges, self.shuffle)
        if self.shuffle and (shard is None or shard.device is None):
            raise ValueError("a StepReplayer shuffles on an HBM-resident shard (a host dataset takes the eager loop)")
        self.shard = shard
        self.pad_plan: Dict[int, Dict[str, object]] = {}       # per graph count B (plan_padding)
        self.slots: Dict[Tuple[int, int, int, bool], StageSlot] = {}
        self._stage_status = torch.zeros(1, dtype=torch.int32, device=device) if self.stream else None
        self.schedule_capacity: Optional[int] = None   # batches of one shape per epoch (default: one pass over the shard)
        self.counts = {"eager": 0, "captured": 0, "replayed": 0}
        self.flat, self.opt = flat, opt
        self.collective = bool(collective)
        self._scale: Dict[int, torch.Tensor] = {}      # per batch object: this rank's share of the global mean loss
        self.pool = torch.cuda.graph_pool_handle()
        self.graphs: Dict[Tuple[int, bool], object] = {}
        self.visits: Dict[Tuple[int, bool], int] = {}
        self.skip: set = set()
        self.stats = {True: RegressionStats(out_dim, device), False: RegressionStats(out_dim, device)}
        self._loss = torch.zeros((), dtype=torch.float32, device=device)
        self._keep: List[object] = []          # batch objects whose ids key the tables

    def _step(self, data, training: bool):
        from . import functional as QF
        fwd = _KINDS[self.kind]
        real = getattr(data, "real_graphs", None)
        if training:
            # The step differentiates with respect to fresh leaves that alias the parameters
            # (functional_call), not the Parameters themselves: a Parameter's gradient accumulator has the
            # stream affinity of whoever created it, and one that user code keeps alive (any earlier
            # forward whose output is still referenced) would drag a cross-stream sync into the capture
            # (observed as a crash in capture_end).
            names = [n for n, p in self.model.named_parameters() if p.requires_grad]
            leaves = {n: p.detach().requires_grad_(True) for n, p in zip(names, self.flat.params)}
            functional = lambda d: torch.func.functional_call(self.model, leaves, (d,))
            out, y = fwd(functional, data, self.out_dim)
            if real is not None:
                out = out[:real]                 # a padded slot: the pad graphs' rows take no part (zero gradient)
            _, g = QF.smooth_l1_loss_and_grad(out, y, loss_out=self._loss)
            if self.collective:
                # this rank's share of the global mean loss (dp.loss_scale: one host-built scalar per batch object, made
                # on the batch's first -- eager -- visit; a capture must not copy from pageable host memory)
                sc = self._scale.get(id(data))
                if sc is None:
                    sc = self._scale[id(data)] = loss_scale(y.shape[0], self.device)
                g = g * sc
            grads = torch.autograd.grad(out, list(leaves.values()), g, allow_unused=True)
            if self.collective:
                torch.cat([(gr if gr is not None else torch.zeros_like(p)).reshape(-1)
                           for gr, p in zip(grads, self.flat.params)], out=self.flat.flat_grad)
                self.flat.all_reduce_grads(force=True)
                self.opt.step()
            else:
                self.opt.step(grads=list(grads))     # the pack into the flat gradient rides in the update kernel
        else:
            with torch.no_grad():
                out, y = fwd(self.model, data, self.out_dim)
                if real is not None:
                    out = out[:real]
                QF.smooth_l1_loss_and_grad(out, y, loss_out=self._loss)
        self.stats[training].update(y, out, self._loss)

    def run(self, data, training: bool) -> bool:
        """One step on ``data`` (streamed replay: on graphs ``data = (lo, hi)`` of the shard); returns False when the
        batch is (remembered as) skipped."""
        if self.stream:
            return self._run_streamed(data, training)
        key = (id(data), training)
        if key in self.skip:
            if training:
                # The forward raises AFTER its layers ran in train mode (models.py:30-36), so in the eager loop -- and in
                # the reference -- the BatchNorm running statistics move on EVERY visit of such a batch, not only on the
                # one that found it out.  Nothing else moves: no optimizer step, no dropout draw, no statistics row.
                self.model.train(True)
                with torch.no_grad():
                    try:
                        _KINDS[self.kind](self.model, data, self.out_dim)
                    except ValueError:
                        pass
            return False
        # (a captured collective: thread-local capture mode -- the process group's watchdog thread polls its events meanwhile)
        mode = dict(capture_error_mode="thread_local") if self.collective else {}
        how = self._cycle(key, training, lambda: self._step(data, training), skip_on=ValueError, **mode)
        if how in ("eager", "skipped"):
            self._keep.append(data)
        if how == "skipped":
            self.skip.add(key)
        return how != "skipped"

    def _cycle(self, key, training: bool, step: Callable[[], None], prepare: Optional[Callable[[], None]] = None,
               skip_on=(), **capture_mode) -> str:
        """The eager -> capture -> replay cycle of the graph ``key``, ``step`` performing the visit: a replay when the graph
        exists; else ``prepare()`` and an eager ``step()`` on the first visit (and while the optimizer has not stepped), a
        capture of ``step()`` replayed once on the next.  Returns "replayed", "eager", "captured", or "skipped" when the
        eager ``step()`` raised ``skip_on``."""
        g = self.graphs.get(key)
        if g is not None:
            g.replay()
            self.counts["replayed"] += 1
            return "replayed"
        self.model.train(training)
        if prepare is not None:
            prepare()
        if self.visits.get(key, 0) == 0 or (training and self.opt.steps == 0):
            try:
                step()
            except skip_on:
                return "skipped"
            self.visits[key] = 1
            self.counts["eager"] += 1
            return "eager"
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self.pool, **capture_mode):
            step()
        self.graphs[key] = g
        g.replay()                      # capture records, it does not execute
        self.counts["captured"] += 1
        return "captured"

    # ---- streamed replay ------------------------------------------------------------------------------------------
    def replay_counts(self) -> Dict[str, int]:
        return dict(self.counts, graphs=len(self.graphs))

    def _slot_key(self, lo: int, hi: int, training: bool) -> tuple:
        """What keys the slot (and the captured graph) of graphs ``[lo, hi)``: the graph count under ``pad_edges``, else
        the exact shape."""
        if self.pad_edges:
            return (hi - lo, bool(training))
        return batch_shape(self.shard.node_ptr, self.shard.edge_ptr, lo, hi) + (bool(training),)

    def _slot(self, key: tuple) -> StageSlot:
        """The slot of ``key``, made on first use: an exact slot for ``(B, N, E, training)``; for ``(B, training)`` the
        padded slot of ``pad_plan`` or, for the training batches of a shuffled run, the gather slot of ``shuffle_plan``."""
        slot = self.slots.get(key)
        if slot is None:
            *shape, training = key
            emb = getattr(self.model, "node_embeddings", None)
            kw = dict(status=self._stage_status, num_embeddings=0 if emb is None else emb.num_embeddings,
                      capacity=self.schedule_capacity)
            if len(shape) == 3:
                slot = self.shard.stage_slot(*shape, **kw)
            else:
                gather = self.shuffle and training
                plan = (self.shuffle_plan if gather else self.pad_plan)[shape[0]]
                make = self.shard.gather_stage_slot if gather else self.shard.padded_stage_slot
                slot = make(shape[0], plan["E_cap"], plan["P"], **kw)
            self.slots[key] = slot
        return slot

    def plan_padding(self, ranges: Sequence[Tuple[int, int]]) -> Dict[int, Dict[str, object]]:
        """Fix the padded slots (``stream_pad_plan``) for every batch the run will ever stage.  Called once, before the
        first slot exists: a slot's buffers are part of its captured graph and never grow."""
        if not self.pad_edges:
            raise ValueError("plan_padding belongs to a StepReplayer(stream=True, pad_edges=True)")
        if self.slots:
            raise ValueError("the padding plan is fixed before the first batch is staged: slots never grow")
        self.pad_plan = stream_pad_plan(self.shard.node_ptr, self.shard.edge_ptr, ranges, self.shard.graph_sizes)
        return self.pad_plan

    def plan_shuffle(self, chunks: Sequence[range], batch_size: int) -> Dict[int, Dict[str, object]]:
        """Fix the gather slots of the training batches (``stream_shuffle_plan``): ``chunks[e]`` are the graphs epoch ``e``
        trains on.  Called once, before the first slot exists."""
        if not self.shuffle:
            raise ValueError("plan_shuffle belongs to a StepReplayer(stream=True, pad_edges=True, shuffle=True)")
        if self.slots:
            raise ValueError("the padding plan is fixed before the first batch is staged: slots never grow")
        self.shuffle_plan = stream_shuffle_plan(self.shard.node_ptr, self.shard.edge_ptr, chunks, batch_size, self.seed,
                                                self.shard.graph_sizes)
        return self.shuffle_plan

    def begin_epoch(self, ranges: Sequence[Tuple[int, int]], training: bool, order: Optional[Sequence[int]] = None) -> None:
        """Write this epoch's schedules: per shape (padded slots: per graph count), the ``lo`` of its batches in visiting
        order.  ``run`` must then be called with exactly ``ranges``, in order.  ``order`` (a shuffled training epoch):
        the graphs to visit instead, batch ``k`` taking as many of them as ``ranges[k]`` holds."""
        G = len(self.shard)
        gather = self.shuffle and training
        if order is not None:
            if not gather:
                raise ValueError("an epoch order belongs to the training epochs of a StepReplayer(shuffle=True)")
            order = [int(g) for g in order]
            if len(order) != sum(hi - lo for lo, hi in ranges):
                raise ValueError(f"an order of {len(order)} graphs for batches of {sum(hi - lo for lo, hi in ranges)}")
            if any(not 0 <= g < G for g in order):
                raise IndexError(f"the epoch order names graphs outside a shard of {G} graphs")
        else:
            if gather:
                raise ValueError("a training epoch of a StepReplayer(shuffle=True) needs its order")
            for lo, hi in ranges:
                if not 0 <= lo < hi <= G:
                    raise IndexError(f"graphs [{lo}, {hi}) lie outside a shard of {G} graphs")
        edge_ptr = self.shard.edge_ptr
        if not self.pad_edges:
            schedules = {shape + (bool(training),): los
                         for shape, los in stream_schedule(self.shard.node_ptr, edge_ptr, ranges).items()}
        else:
            plans = self.shuffle_plan if gather else self.pad_plan
            max_m = int(self.shard.graph_sizes[1])
            counts = edge_ptr[1:] - edge_ptr[:-1] if gather else None
            schedules: Dict[tuple, List[int]] = {}
            at = 0
            for lo, hi in ranges:
                B = hi - lo
                if gather:
                    entry = order[at:at + B]
                    at += B
                    e = int(counts[torch.as_tensor(entry, dtype=torch.long)].sum())
                else:
                    entry = [lo]
                    e = int(edge_ptr[hi]) - int(edge_ptr[lo])
                plan = plans.get(B)
                if plan is None or not 0 <= plan["E_cap"] - e <= plan["P"] * max_m:
                    what = f"a shuffled batch of {B} graphs ({e} edges) is" if gather else f"graphs [{lo}, {hi}) ({e} edges) are"
                    raise ValueError(f"{what} not covered by the padding plan "
                                     f"({'no slot for this graph count' if plan is None else plan}): "
                                     + ("plan_shuffle takes every epoch of the run" if gather else
                                        "plan_padding takes every batch of the run"))
                schedules.setdefault(self._slot_key(lo, hi, training), []).extend(entry)
        for key, entries in schedules.items():
            self._slot(key).set_schedule(entries)

    def end_epoch(self) -> None:
        """Raise what the epoch's device-side checks flagged (two 4-byte reads behind the epoch's host synchronisation)."""
        from .graph import check_index_status
        check_stage_status(self._stage_status)
        check_index_status(self.device)

    def _run_streamed(self, rng: Tuple[int, int], training: bool) -> bool:
        key = self._slot_key(rng[0], rng[1], training)

        def reset():
            # the stage launch rewrites the slot's tensors behind torch's back: nothing cached on the batch object may survive
            # into this visit (class docstring, CACHE RULE)
            self._slot(key).batch._qot_cache = {}

        def step():
            slot = self._slot(key)
            slot.stage()                # the schedule's next entry
            self._step(slot.batch, training)

        if self._cycle(key, training, step, prepare=reset) == "captured":
            reset()                     # what the capture cached lives in the graph's pool: only the graph may use it
        return True


def run_epoch(model, dataset, indices: range, *, kind: str, batch_size: int, out_dim: int, device,
              criterion, flat: Optional[FlatModel] = None, opt: Optional[FusedSGD] = None,
              replayer: Optional[StepReplayer] = None, stream: Optional[bool] = None,
              pad_edges: Optional[bool] = None, shuffle: Optional[bool] = None, seed: int = 0,
              epoch: int = 0) -> Dict[str, object]:
    """One pass over ``indices``; trains when ``opt`` is given, else evaluates under ``no_grad``.  ``stream=True``
    (with a ``StepReplayer(stream=True)``): every batch is staged on the device into the static slot of its shape and
    run by that shape's one captured graph.  ``pad_edges=True`` (with a ``StepReplayer(stream=True, pad_edges=True)``
    whose ``plan_padding`` covered these batches): one padded slot per graph count instead.  ``shuffle=True`` (training
    passes only): the graphs are visited in ``epoch_order(indices, seed, epoch)`` -- gathered on the device by a
    ``StepReplayer(..., shuffle=True)`` whose ``plan_shuffle`` covered the epoch, or, on a host dataset, collated by the
    eager loop."""
    fwd = _KINDS[kind]
    rank, world = _rank_world()
    shuffle = bool(shuffle)
    _check_options(dataset, kind, world, stream, pad_edges, shuffle)
    order = epoch_order(indices, seed, epoch) if shuffle and opt is not None else None
    if stream:
        if replayer is None or not replayer.stream or replayer.shard is not dataset:
            raise ValueError("stream=True needs a StepReplayer(stream=True, shard=dataset)")
        if bool(pad_edges) != replayer.pad_edges:
            raise ValueError("pad_edges must be what the StepReplayer was built with")
        training = opt is not None
        if training and (shuffle != replayer.shuffle or (shuffle and int(seed) != replayer.seed)):
            raise ValueError("shuffle and seed of a training pass must be what the StepReplayer was built with")
        ranges = batch_ranges(indices, batch_size)
        if order is not None:
            replayer.begin_epoch(ranges, training, order=order)
        else:
            replayer.begin_epoch(ranges, training)
        st = replayer.stats[training]
        st.buf.zero_()
        for r in ranges:
            replayer.run(r, training)
        res = st.result()               # the epoch's host synchronisation
        replayer.end_epoch()            # device-side checks of the staged batches: raises before the results are used
        res["avg_loss"] = res["loss_sum"] / max(len(indices), 1)
        res["skipped"] = 0
        return res
    # an HBM-resident shard keeps its batch objects (and the graph index the model attaches to them):
    # the chunks repeat every few epochs, so later visits do no graph preparation at all
    resident = isinstance(dataset, PackedGraphs) and dataset.device is not None
    if order is not None:
        # a shuffled epoch of a host dataset: the same loop over collated batches of arbitrary graphs (nothing to cache)
        loader = GraphLoader(dataset, batch_size, shuffle=False, device=device,
                             batches=[order[b0:b0 + batch_size] for b0 in range(0, len(order), batch_size)])
    else:
        loader = GraphLoader(dataset, batch_size, shuffle=False, device=device, cache_batches=resident,
                             batches=_local_batches(indices, batch_size, rank, world, _graph_costs(dataset, indices)))
    stats = RegressionStats(out_dim, device)
    skipped = 0
    training = opt is not None
    model.train(training)
    shares_ok = True
    if world > 1 and replayer is not None and replayer.collective:
        # a replayed step holds the collective: every rank must hold graphs of every global batch (the split is a pure
        # function of the indices, so every rank reaches the same verdict without talking)
        costs = _graph_costs(dataset, indices)
        for b0 in range(0, len(indices), batch_size):
            nb = min(batch_size, len(indices) - b0)
            for r in range(world):
                lo, hi = graph_range(nb, r, world, costs=None if costs is None else costs[b0:b0 + nb])
                shares_ok = shares_ok and hi > lo
    if replayer is not None and resident and (world == 1 or (replayer.collective and training and shares_ok)):
        st = replayer.stats[training]
        st.buf.zero_()
        for data in loader:
            if not replayer.run(data, training):
                skipped += data.num_graphs
        res = st.result()
        res["avg_loss"] = res["loss_sum"] / max(len(indices), 1)
        res["skipped"] = skipped
        return res
    coupled = world > 1 and training          # ranks meet in collectives inside every step
    with torch.set_grad_enabled(training):
        for data in loader:
            if training:
                flat.zero_grad()
            if data is None and not coupled:
                continue
            if coupled and kind == "lightpath":
                # Ranks are coupled inside forward/backward (global BatchNorm statistics), and whether a batch
                # is skipped is a property of the GLOBAL batch, as in the single-process reference: skipped only
                # when NO rank holds a LUT node.  One flag all-reduce (one host read) per batch.
                has = 0
                if data is not None:
                    has = int(bool((data.x[:, getattr(model, "is_lut_index", None)] == 1.0).any()))
                flags = torch.tensor([has, int(data is None)], dtype=torch.int32, device=device)
                dist.all_reduce(flags, op=dist.ReduceOp.MAX)
                any_lut, any_empty = (int(v) for v in flags.tolist())
                if any_empty:
                    # fewer graphs than ranks in a trailing batch: a rank without nodes cannot take part in the
                    # BatchNorm exchange; all ranks skip it (documented deviation, at most world-1 graphs per epoch)
                    skipped += 0 if data is None else data.num_graphs
                    continue
                model.allow_empty_lut = True
                try:
                    if not any_lut:
                        # the reference raises AFTER conv1/norm1 ran (models.py:30-36): running statistics move
                        with torch.no_grad():
                            fwd(model, data, out_dim)
                        skipped += data.num_graphs
                        continue
                    out, y = fwd(model, data, out_dim)
                finally:
                    model.allow_empty_lut = False
                loss = criterion(out, y) if y.shape[0] else out.sum() * 0.0
                (loss * loss_scale(y.shape[0], device)).backward()
                flat.all_reduce_grads()
                opt.step()
                if y.shape[0]:
                    stats.update(y, out, loss)
                continue
            if data is None:
                # empty share of a trailing batch: zero contribution, same collectives as the other ranks
                loss_scale(0, device)
                flat.all_reduce_grads()
                opt.step()
                continue
            try:
                out, y = fwd(model, data, out_dim)
            except ValueError:
                skipped += data.num_graphs          # lightpath_training/train.py:118-121
                continue
            loss = criterion(out, y)
            if training:
                if world > 1:
                    # this rank's share of the global mean loss, then a plain average of gradients
                    (loss * loss_scale(y.shape[0], device)).backward()
                    flat.all_reduce_grads()
                else:
                    loss.backward()
                opt.step()
            stats.update(y, out, loss)
    stats.all_reduce()
    res = stats.result()
    # the reference divides by len(loader.dataset), skipped graphs included (train.py:119)
    res["avg_loss"] = res["loss_sum"] / max(len(indices), 1)
    if world > 1:
        sk = torch.tensor([skipped], dtype=torch.int64, device=device)
        dist.all_reduce(sk, op=dist.ReduceOp.SUM)
        skipped = int(sk.item())
    res["skipped"] = skipped
    return res


def fit(model, dataset, *, kind: str = "topological", batch_size: int = 512, num_epochs: int = 35,
        patience: int = 10, lr: float = 0.1, momentum: float = 0.9, step_size: int = 10, gamma: float = 0.5,
        chunk_fraction: float = 0.10, output_dim: int = 3, device="cuda", best_path: Optional[str] = None,
        log: Callable[[str], None] = print, replay: Optional[bool] = None, stream: Optional[bool] = None,
        pad_edges: Optional[bool] = None, shuffle: Optional[bool] = None, seed: int = 0) -> History:
    """The training script's main loop (train.py:24-182) on a dataset object indexable by graph.

    ``replay`` (default: on for an HBM-resident shard in a single process): steps over cached batches are
    captured as HIP graphs on their second visit and replayed afterwards (``StepReplayer``).
    ``stream`` (default off; needs an HBM-resident shard, ``kind="topological"`` and a single process, else
    ``ValueError``): streamed replay -- one captured graph per batch shape, every batch staged into that shape's static
    buffers on the device, so first visits and single-epoch runs replay too.  ``History.replay_counts`` tells which
    path the steps took.
    ``pad_edges`` (default off; needs ``stream=True`` and graphs of one node count, else ``ValueError``): batches whose
    edge totals differ -- one edge per distinct connection of a sample, as the reference builds its graphs -- share one
    slot and one captured graph per graph count; pad graphs appended on the device bring every batch to the slot's edge
    count and take no part in the loss (``StepReplayer``, ``stream_pad_plan``).
    ``shuffle`` (default off): every epoch trains on its chunk in a fresh random order, ``epoch_order(chunk, seed,
    epoch)``; validation is unchanged.  On an HBM-resident shard it needs ``stream=True, pad_edges=True`` (and what they
    need, else ``ValueError``): the batches are gathered on the device into one slot per graph count
    (``loader.GatherStageSlot``, ``stream_shuffle_plan``), every step replays.  On a host dataset the eager loop collates
    the same batches."""
    device = torch.device(device)
    stream = bool(stream)
    pad_edges = bool(pad_edges)
    shuffle = bool(shuffle)
    _check_options(dataset, kind, _rank_world()[1], stream, pad_edges, shuffle)
    model.to(device)
    tr, va, _ = split_ranges(len(dataset))
    flat = FlatModel(model)
    flat.broadcast_params()
    rank, world = _rank_world()
    resident = isinstance(dataset, PackedGraphs) and dataset.device is not None
    # more than one rank: replayed steps hold the RCCL all-reduce (nccl backend, TopologicalGNN; StepReplayer docstring)
    dp_ok = world == 1 or (kind == "topological" and dist.get_backend() == "nccl")
    use_replay = stream or ((resident and dp_ok) if replay is None else (bool(replay) and resident and dp_ok))
    opt = FusedSGD(flat, lr=lr, momentum=momentum, device_lr=use_replay)
    replayer = None
    if use_replay:
        replayer = StepReplayer(model, kind, output_dim, device, flat, opt, collective=world > 1, stream=stream,
                                shard=dataset if stream else None, pad_edges=pad_edges,
                                **(dict(shuffle=True, seed=seed) if shuffle else {}))
        if pad_edges:
            # every batch the run can ever stage, so that no slot has to grow
            replayer.plan_padding(fit_batch_ranges(len(dataset), batch_size, chunk_fraction))
        if shuffle:
            replayer.plan_shuffle(fit_train_chunks(len(dataset), chunk_fraction, num_epochs), batch_size)
    criterion = torch.nn.SmoothL1Loss()
    hist = History()
    counter = 0
    for epoch in range(num_epochs):
        chunk = epoch_chunk(epoch, len(tr), chunk_fraction)
        if epoch == 0:
            log(f"Training model with {len(chunk)} samples and validating with {len(va)} samples.")
        opt.lr = step_lr(lr, epoch, step_size, gamma)
        t = run_epoch(model, dataset, range(tr[0] + chunk[0], tr[0] + chunk[-1] + 1) if len(chunk) else range(0),
                      kind=kind, batch_size=batch_size, out_dim=output_dim, device=device, criterion=criterion,
                      flat=flat, opt=opt, replayer=replayer, stream=stream, pad_edges=pad_edges,
                      **(dict(shuffle=True, seed=seed, epoch=epoch) if shuffle else {}))
        v = run_epoch(model, dataset, va, kind=kind, batch_size=batch_size, out_dim=output_dim, device=device,
                      criterion=criterion, replayer=replayer, stream=stream, pad_edges=pad_edges)
        if replayer is not None:
            hist.replay_counts = replayer.replay_counts()
        hist.loss.append(t["avg_loss"]); hist.r2.append(t["r2"])
        hist.val_loss.append(v["avg_loss"]); hist.val_r2.append(v["r2"])
        hist.skipped_graphs += t["skipped"]
        hist.epochs_run = epoch + 1
        log(f"Epoch {epoch + 1}, Loss: {t['avg_loss']:.4f}, R2 Score: {t['r2']:.4f}, "
            f"Val Loss: {v['avg_loss']:.4f}, Val R2 Score: {v['r2']:.4f}")
        if v["r2"] > hist.best_val_r2:
            hist.best_val_r2 = v["r2"]
            counter = 0
            if best_path and rank == 0:
                torch.save(model.state_dict(), best_path)
        else:
            counter += 1
            if counter >= patience:
                log("Early stopping triggered.")
                hist.stopped_early = True
                break
    return hist


def evaluate(model, dataset, indices: Optional[Sequence[int]] = None, *, kind: str = "topological",
             batch_size: int = 512, output_dim: int = 3, device="cuda",
             output_keys: Sequence[str] = ("osnr", "snr", "ber"),
             target_ranges: Dict[str, Dict[str, float]] = TARGET_RANGES, return_predictions: bool = False,
             fused: bool = False, predictor: Optional[Callable] = None, mc_samples: Optional[int] = None,
             mc_p=None, mc_seed: Optional[int] = None):
    """test.py's metric block: per-output R2 and MSE on min-max descaled values (test.py:76-121).

    ``fused=True`` (opt-in, ``kind="topological"`` on one process; ``ValueError`` otherwise or when the model or a batch
    is outside ``TopologicalPredictor``'s envelope): every batch runs as the single-launch inference kernel
    (``infer.TopologicalPredictor``) instead of ``model(data)``.  Same function to fp32 rounding.  Meant for the
    latency-bound regime -- one graph or a handful per call, up to batches of the reference's scale (hidden 16, 512
    graphs); at hidden 64 with a thousand graphs per batch the default path's MFMA NNConv kernel is expected to have the
    advantage (fp32 FMA here).  Neither side of that has been measured on an MI355X yet: DESIGN.md 4.12.

    ``predictor`` (opt-in, one process; ``ValueError`` in a larger world): a callable used in place of ``model(data)`` for
    the given ``kind`` -- for ``kind="lightpath"`` an ``infer.LightpathPredictor(model)``, whose ``(out, lut_batch)`` has the
    model's contract.  Its ``infer.EnvelopeError`` propagates; the LUT-less ``ValueError`` still skips the batch.

    ``return_predictions``: also return ``(y_true_descaled, y_pred_descaled, skipped_graphs)`` -- the arrays test.py
    writes to ``y_true_descaled.json`` / ``y_pred_descaled.json`` (test.py:92-103,129-136), in dataset order; they stay
    on the device until the loop is over (one host copy).

    ``mc_samples=T`` (with ``fused=True`` only, ``ValueError`` otherwise): every batch additionally runs
    ``TopologicalPredictor.sample(data, T, p=mc_p, seed=mc_seed)`` (Monte-Carlo dropout) and the result
    gains a LAST element ``y_pred_std_descaled [graphs, outputs]``: the per-graph standard deviation of the draws times
    ``max - min`` of the output (a spread: no offset), in dataset order.  The predictions and metrics stay the eval-mode
    ones.  ``mc_p=None``: the model's own dropout probabilities (a model rebuilt for testing has 0: say 0.5)."""
    rank, world = _rank_world()
    if mc_samples is not None and not fused:
        raise ValueError("evaluate(mc_samples=...) needs fused=True (TopologicalPredictor.sample)")
    if fused and kind != "topological":
        raise ValueError(f"evaluate(fused=True) is for kind='topological' only, got kind={kind!r}")
    if fused and world > 1:
        raise ValueError(f"evaluate(fused=True) runs on one process, got a world of {world}")
    if predictor is not None and world > 1:
        raise ValueError(f"evaluate(predictor=...) runs on one process, got a world of {world}")
    if predictor is not None and fused:
        raise ValueError("evaluate: give either fused=True or predictor=..., not both")
    device = torch.device(device)
    model.to(device)
    idx = range(len(dataset)) if indices is None else indices
    fwd = _KINDS[kind]
    stats = RegressionStats(output_dim, device)
    model.eval()
    if fused:
        from .infer import TopologicalPredictor
        predictor = TopologicalPredictor(model)
        fwd = lambda _model, data, out_dim: (predictor(data), data.y.view(-1, out_dim))      # noqa: E731
        sampler = predictor
    elif predictor is not None:
        kind_fwd, call = _KINDS[kind], predictor
        fwd = lambda _model, data, out_dim: kind_fwd(call, data, out_dim)                   # noqa: E731
    loader = GraphLoader(dataset, batch_size, shuffle=False, device=device,
                         batches=_local_batches(idx, batch_size, rank, world, _graph_costs(dataset, idx)))
    kept, skipped, stds = [], 0, []
    # Under data parallelism a rank sees only its share of every global batch.  The reference decides "no LUT node in the
    # batch" (lightpath_training/test.py:82-85) on the WHOLE batch, so a share without LUT rows contributes zero rows
    # (allow_empty_lut) and the skip is decided afterwards from the row counts of all ranks, per global batch.
    sharded_lut = world > 1 and kind == "lightpath" and hasattr(model, "allow_empty_lut")
    shares = []                                        # (global batch, rows this rank produced, graphs in its share)
    with torch.no_grad():
        for b, data in enumerate(loader):
            if data is None:
                continue
            if sharded_lut:
                model.allow_empty_lut = True
                try:
                    out, y = fwd(model, data, output_dim)
                finally:
                    model.allow_empty_lut = False
                shares.append((b, int(y.shape[0]), int(data.num_graphs)))
                if y.shape[0] == 0:
                    continue
                stats.update(y, out)
                if return_predictions:
                    kept.append((b, y.detach().clone(), out.detach().clone()))
                continue
            try:
                out, y = fwd(model, data, output_dim)
            except ValueError as err:
                from .infer import EnvelopeError
                if fused or isinstance(err, EnvelopeError):     # outside a predictor's envelope: not a LUT-less batch
                    raise
                skipped += data.num_graphs            # lightpath_training/test.py:82-85
                continue
            stats.update(y, out)
            if return_predictions:
                kept.append((b, y.detach().clone(), out.detach().clone()))
            if mc_samples is not None:
                stds.append(sampler.sample(data, mc_samples, p=mc_p, seed=mc_seed)[1])
    if sharded_lut:
        everyone = [None] * world
        dist.all_gather_object(everyone, shares)
        rows, graphs = {}, {}
        for per_rank in everyone:
            for b, r, g in per_rank:
                rows[b] = rows.get(b, 0) + r
                graphs[b] = graphs.get(b, 0) + g
        dead = {b for b, r in rows.items() if r == 0}  # global batches without any LUT node: skipped as a whole
        skipped = sum(g for b, r, g in shares if b in dead)
    stats.all_reduce()
    keys = list(output_keys)[:output_dim]
    scale = torch.tensor([target_ranges[k]["max"] - target_ranges[k]["min"] for k in keys], dtype=torch.float64)
    res = stats.result(scale)
    metrics = {k.upper(): {"R2": res["r2_raw"][i], "Test_MSE": res["mse_raw"][i]} for i, k in enumerate(keys)}
    extra = ()
    if mc_samples is not None:
        std = torch.cat([t.cpu().double() for t in stds]) if stds else torch.zeros(0, output_dim, dtype=torch.float64)
        extra = (std * scale,)                            # a spread descales by the range alone
    if not return_predictions:
        return (metrics,) + extra if extra else metrics
    parts = [(b, rank, y.cpu(), o.cpu()) for b, y, o in kept]
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, (parts, skipped))
        parts = sorted((p for ps, _ in gathered for p in ps), key=lambda t: (t[0], t[1]))
        skipped = sum(sk for _, sk in gathered)
    lo = torch.tensor([target_ranges[k]["min"] for k in keys], dtype=torch.float64)
    cat = lambda j: (torch.cat([p[j].double() for p in parts]) if parts else torch.zeros(0, output_dim, dtype=torch.float64))
    y_true = cat(2) * scale + lo                      # min_max_descale (test.py:12-13)
    y_pred = cat(3) * scale + lo
    return (metrics, y_true, y_pred, skipped) + extra


def next_model_path(root_dir: str) -> Tuple[str, int]:
    """``model_<k>.pth`` with k = 1 + the largest index present (train.py:185-195)."""
    os.makedirs(root_dir, exist_ok=True)
    idx = [int(n.split("_")[1].split(".")[0]) for n in os.listdir(root_dir) if n.startswith("model_")]
    k = max(idx) + 1 if idx else 0
    return os.path.join(root_dir, f"model_{k}.pth"), k


def save_checkpoint(path: str, model, model_params: Dict[str, object]):
    """The dictionary the reference test scripts expect (train.py:196-209, test.py:47-70)."""
    torch.save({"model_state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                "model_params": dict(model_params)}, path)


def load_checkpoint(path: str):
    """Reads a checkpoint written by this module or by the reference (tensors + plain containers only)."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    return ck["model_state_dict"], ck["model_params"]
