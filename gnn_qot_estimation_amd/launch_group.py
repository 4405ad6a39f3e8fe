"""Host side of the multi-role launch (``qot_run_roles``, ``csrc/roles.hip``): independent small jobs of a train step
share ONE kernel launch instead of costing 4-9 us of launch latency each.

Two users:

* ``LaunchGroup`` -- an explicit group for the FORWARD prologue of ``TopologicalGNN`` (graph index of the batch +
  embedding-table projection + NNConv operand packing: none reads what another writes).  Callers register jobs whose
  outputs they have already allocated and call ``run()`` before the first consumer.
* the BACKWARD epilogue queue (``defer`` / ``flush``): the second-stage sums that autograd Functions used to launch one by
  one from inside their ``backward`` (read-out partials, NNConv slabs, ``lin_edge`` partials, table-gradient row sum) are
  registered instead, with their outputs allocated but not yet filled, and launched together -- by
  ``TableProjectFn.backward`` (table mode: it is the last node and the only in-graph consumer of a deferred result) or
  by an end-of-backward callback of the autograd engine.  Stage-2 jobs run in a second launch behind stage 1 (a job may
  read what stage 1 wrote).  Deferred outputs are leaf gradients (or feed ``TableProjectFn``), so nothing reads them
  before the flush; what is returned to autograd are VIEWS of buffers the queue keeps alive, so ``AccumulateGrad``
  still takes them without a copy.

Hosted sums (``defer_gradh``): the H = 64 NNConv backward also queues its grad-h LAUNCH.  The grad-h kernel's persistent tile
walk ends in a ragged round that leaves three quarters of its workgroup slots idle for a tile time, and nothing of the pass
reads its output before the epilogue anyway; so the flush launches it behind the last backward kernel with the stage-1 sums
as tail workgroups of its own launch (``qot_nnconv_gradh_host_roles``), and the sum of its own partials -- the one stage-1
job it cannot carry -- rides with stage 2: the epilogue is {grad-h + stage-1 sums, stage 2} instead of {grad-h, stage 1,
stage 2}.  ``QOT_NO_HOSTED_SUMS=1`` (read on every call) restores that schedule exactly; ``QOT_HOSTED_SUMS_EARLY=1`` launches
grad-h where it always was, carrying only the sums already queued by then (measurements).

``QOT_NO_LAUNCH_GROUPS=1`` restores one launch per job (A/B measurements, bisecting).

Threading: the backward queue is ONE module-level object armed through an autograd-engine callback -- right for the
single-threaded step the reference runs (``topological_training/train.py:107-116``), NOT for two backward passes in flight
on different host threads (their jobs would share a queue and a stream).  Such callers set ``QOT_NO_LAUNCH_GROUPS=1``
("Threads").  A deferred gradient is only handed out when nothing can read it before the flush:
``can_defer`` refuses receivers with an existing ``.grad``, tensor hooks, post-accumulate hooks, a non-contiguous layout, or
one Parameter appearing twice.
"""
from __future__ import annotations

import os

import torch

from . import _lib


def enabled() -> bool:
    return os.environ.get("QOT_NO_LAUNCH_GROUPS", "0") != "1"


def hosted_sums() -> bool:
    return os.environ.get("QOT_NO_HOSTED_SUMS", "0") != "1"


def can_defer(*receivers) -> bool:
    """A backward-epilogue job may be deferred only if nothing reads its output before the flush.  Its outputs are
    gradients handed to autograd: for a LEAF whose ``.grad`` is ``None`` the engine just keeps the tensor (no kernel),
    but an existing ``.grad`` is accumulated into AT ONCE (an add kernel that would read the still unfilled buffer),
    and a non-leaf input (``F.pad`` of a parameter, a view, ...) hands the gradient to the next backward node at once.
    ``receivers``: the forward inputs that receive the deferred gradients (``None`` entries are ignored)."""
    if not enabled():
        return False
    for t in receivers:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_leaf or t.grad is not None:
            return False
        # a tensor hook / post-accumulate-grad hook runs on the gradient AT ONCE (on the still unfilled buffer), and a
        # receiver that is not contiguous makes AccumulateGrad clone the buffer at once (gradient layout contract)
        if getattr(t, "_backward_hooks", None) or getattr(t, "_post_accumulate_grad_hooks", None) or not t.is_contiguous():
            return False
    # one Parameter used by two nodes (tied weights): the engine's InputBuffer ADDS the two gradients as they arrive
    ids = [id(t) for t in receivers if t is not None]
    if len(ids) != len(set(ids)):
        return False
    return not torch.is_grad_enabled()   # create_graph=True: AccumulateGrad clones what it is given


class LaunchGroup:
    """Jobs launched together by ``run()``; ``post`` callables run after the launch (e.g. a status read-back)."""

    def __init__(self):
        self.roles, self.keep, self.post = [], [], []
        self.on_success = []         # run after the launch AND the post checks went through (e.g. cache insertions)

    def add(self, kind: int, ptrs, ints, keep=()):
        self.roles.append(_lib.make_role(kind, ptrs, ints))
        self.keep.extend(t for t in ptrs if isinstance(t, torch.Tensor))
        self.keep.extend(keep)

    def run(self):
        roles, post, done = self.roles, self.post, self.on_success
        self.roles, self.post, self.on_success = [], [], []
        try:
            _lib.run_roles(roles)
        finally:
            self.keep = []
        for fn in post:
            fn()                     # may raise (status read-back): nothing below runs then
        for fn in done:
            fn()


class _BackwardQueue:
    def __init__(self):
        self.clear()

    def pending(self) -> bool:
        return bool(self.stages[0] or self.stages[1] or self.gradh)

    def clear(self):
        self.stages = ([], [])
        self.gradh = []              # queued grad-h launches: (entry point, arguments, role of its partial sum)
        self.keep = []
        self.stream = None           # raw handle of the stream the backward nodes run on
        self.armed = False


_Q = _BackwardQueue()


def _arm():
    q = _Q
    if not q.armed:
        q.clear()                        # anything left over belongs to a backward pass that died: its buffers are gone
        q.stream = _lib.stream()         # node execution runs on the forward's stream; the callback may not
        torch.autograd.Variable._execution_engine.queue_callback(flush)
        q.armed = True
    return q


def defer(kind: int, ptrs, ints, stage: int = 1, keep=()):
    """Register a backward-epilogue job (``stage`` 1 or 2).  Only valid inside an autograd backward pass: the first job
    of a pass installs the engine's end-of-backward callback that launches whatever is still pending."""
    q = _arm()
    q.stages[stage - 1].append(_lib.make_role(kind, ptrs, ints))
    q.keep.extend(t for t in ptrs if isinstance(t, torch.Tensor))
    q.keep.extend(keep)


def _take_hostable(s1):
    """Splits stage 1 into what a grad-h launch can carry (light sums, at most ``MAX_ROLES``) and the rest, order kept."""
    hosted, rest = [], []
    for r in s1:
        (hosted if r.kind in _lib.HOSTABLE_ROLES and len(hosted) < _lib.MAX_ROLES else rest).append(r)
    return hosted, rest


def defer_gradh(fn: str, args, partial_sum, keep=()):
    """Queue the H = 64 grad-h launch ``fn(*args, stream)`` of an NNConv backward whose second-stage sums are deferred.
    ``partial_sum``: ``(kind, ptrs, ints)`` of the sum of the launch's own partials.  ``args`` are raw values: ``keep`` holds
    the tensors behind them.  Only valid inside an autograd backward pass, like ``defer``."""
    q = _arm()
    q.keep.extend(keep)
    q.keep.extend(t for t in partial_sum[1] if isinstance(t, torch.Tensor))
    role = _lib.make_role(*partial_sum)
    if os.environ.get("QOT_HOSTED_SUMS_EARLY", "0") == "1":
        hosted, q.stages[0][:] = _take_hostable(q.stages[0])
        _lib.host_roles(hosted)
        with _lib.on_stream(q.stream):
            _lib.call(fn, *args)
        q.stages[0].append(role)
    else:
        q.gradh.append((fn, args, role))


def plan(s1, s2, gradh):
    """The launches of a flush, in order: ``("gradh", fn, args, hosted roles)`` and ``("roles", roles)`` entries.
    Without a queued grad-h launch: stage 1, stage 2.  With one: grad-h carrying every stage-1 job it can host (NEVER the
    sum of its own partials: that one reads what the launch writes), then one launch of stage 2 plus the partial sums, which
    no stage-2 job reads or writes.  Stage-1 jobs it cannot carry (another kind, more than ``MAX_ROLES``) keep a launch of
    their own, with the partial sums, in front of stage 2.  Further queued grad-h launches (a second NNConv layer) carry nothing."""
    if not gradh:
        return [("roles", r) for r in (s1, s2) if r]
    hosted, rest = _take_hostable(s1)
    out = [("gradh", fn, args, hosted if k == 0 else []) for k, (fn, args, _) in enumerate(gradh)]
    sums = [role for _, _, role in gradh]
    if rest:
        out += [("roles", rest + sums)] + ([("roles", s2)] if s2 else [])
    else:
        out.append(("roles", s2 + sums))
    return out


def flush():
    """Launch the pending jobs: one launch for stage 1, one for stage 2 (if any); with a queued grad-h launch, see ``plan``."""
    q = _Q
    if not q.pending():
        q.armed = False
        return
    s1, s2 = q.stages
    gradh, stream = q.gradh, q.stream
    q.stages, q.gradh = ([], []), []
    try:
        for step in plan(s1, s2, gradh):
            if step[0] == "gradh":
                _, fn, args, hosted = step
                if hosted:
                    _lib.host_roles(hosted)
                with _lib.on_stream(stream):
                    _lib.call(fn, *args)
            else:
                _lib.run_roles(step[1], stream)
    finally:
        q.keep = []
        q.armed = False
        q.stream = None


def drop_stale():
    """Called where no backward can be in flight (start of a forward): jobs still queued were registered by a backward
    pass that raised before its callback ran; their buffers may be gone -- forget them."""
    if _Q.pending() or _Q.armed:
        gid = getattr(torch._C, "_current_graph_task_id", None)
        if gid is not None and gid() != -1:
            return                       # a forward recomputed INSIDE a backward pass (checkpointing): the queue is live
        _Q.clear()
