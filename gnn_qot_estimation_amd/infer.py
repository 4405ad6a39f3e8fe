"""Single-launch inference for ``TopologicalGNN``: ``TopologicalPredictor`` (``csrc/infer.hip``).

``model(data)`` in eval mode goes through the training machinery: a launch group, the prologue launch, the graph form of
TransformerConv, the NNConv forward and the read-out kernel, each behind an autograd wrapper.  That is host-bound for one
graph or a handful -- the case of a planning tool that scores one candidate after another.  The predictor runs the same
function as ONE kernel launch per call, one workgroup per graph, and touches autograd nowhere.
"""
from __future__ import annotations

import torch

from . import _lib
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


def edge_cap(n_max: int, hidden: int, edge_dim: int) -> int:
    """Most edges a graph may have beside ``n_max`` nodes (the kernel's LDS budget, asked of the library); -1: none."""
    return int(_lib.load().qot_topological_infer_max_edges(int(n_max), int(hidden), int(edge_dim)))


class TopologicalPredictor:
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
    """

    def __init__(self, model):
        self.model = model
        self._tables = None
        self._tag = None
        self._status = None
        self._check_model()

    # ------------------------------------------------------------------ envelope
    def _check_model(self):
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
        if not m.node_embeddings.weight.is_cuda:
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
    @staticmethod
    def _i64(t, dev):
        if t.dtype != torch.int64 or t.device != dev:
            t = t.to(device=dev, dtype=torch.int64)
        return t.contiguous()

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
        ids, ei = self._i64(ids, dev), self._i64(ei, dev)
        N, E = ids.shape[0], ei.shape[1]
        ptr, eptr, sizes = getattr(data, "ptr", None), getattr(data, "edge_ptr", None), getattr(data, "graph_sizes", None)
        if ptr is None:
            batch = self._i64(data.batch, dev)
            B = getattr(data, "num_graphs", None)
            B = int(B) if B is not None else (int(batch.max()) + 1 if N else 0)
            ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            ptr[1:] = torch.cumsum(torch.bincount(batch, minlength=B), 0)
            sizes = None
        ptr = self._i64(ptr, dev)
        B = ptr.numel() - 1
        if eptr is None:
            # edges of a collated batch are grouped by graph: the slices follow from the graph of every edge's target
            batch = torch.repeat_interleave(torch.arange(B, device=dev), ptr[1:] - ptr[:-1])
            eb = batch[ei[1]]
            if E > 1 and not bool((eb[1:] >= eb[:-1]).all()):
                raise ValueError("TopologicalPredictor: the edges of the batch are not grouped by graph")
            eptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            eptr[1:] = torch.cumsum(torch.bincount(eb, minlength=B), 0)
            sizes = None
        eptr = self._i64(eptr, dev)
        if eptr.numel() != B + 1:
            raise ValueError("TopologicalPredictor: ptr and edge_ptr disagree on the number of graphs")

        def exact():
            if B == 0:
                return 0, 0
            return int((ptr[1:] - ptr[:-1]).max()), int((eptr[1:] - eptr[:-1]).max())
        n_max, max_e = (int(sizes[0]), int(sizes[1])) if sizes is not None else exact()
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
    @torch.no_grad()
    def __call__(self, data):
        H, D, O = self._check_model()
        m = self.model
        if data.x is not None and data.x.numel():
            raise ValueError("TopologicalPredictor: data.x is given; only table mode (node_ids into the embedding "
                             "table) is supported")
        dev = m.node_embeddings.weight.device
        ids, ei, ptr, eptr, n_max, max_e, B, exact = self._slices(data, dev)
        lib = _lib.load()
        if n_max > MAX_NODES or not lib.qot_topological_infer_supported(n_max, max_e, H, D, O):
            n_max, max_e = exact()          # the carried sizes are bounds (a shard inherits its parent's): look once
            if n_max > MAX_NODES:
                raise ValueError(f"TopologicalPredictor: a graph of {n_max} nodes; at most {MAX_NODES} nodes per graph")
            cap = edge_cap(n_max, H, D)
            if max_e > cap:
                raise ValueError(f"TopologicalPredictor: a graph of {max_e} edges is above the edge cap {cap} for graphs of "
                                 f"up to {n_max} nodes at hidden width {H}, edge_dim {D}")
        ea = data.edge_attr
        E = ei.shape[1]
        if ea is None or tuple(ea.shape) != (E, D):
            raise ValueError(f"TopologicalPredictor: edge_attr must be [{E}, {D}], got "
                             f"{None if ea is None else tuple(ea.shape)}")
        ea = _f32c(ea if ea.device == dev else ea.to(dev))
        t = self._refresh(H, D)
        self._check_ids(data, ids, t["V"], n_max)
        if self._status is None or self._status.device != dev:
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.empty(B, O, dtype=torch.float32, device=dev)
        _lib.call("qot_topological_infer", ids, ei, ea, ptr, eptr, ids.shape[0], E, B, n_max, max_e, t["t4"], 4 * H, t["M"],
                  t["ldm"], t["P"], t["V"], t["we"], t["w1"], t["b1"], t["wcat"], t["bias2"], t["w0"], t["b0"], t["w3"],
                  t["b3"], 0.01, float(m.mlp[1].negative_slope), out, H, D, O, self._status)
        return out

    def check_status(self):
        """Reads the kernel's status word (one device synchronisation): raises when a batch since the last check had an
        edge outside its graph's node range or slices that disagree with its arrays (such graphs' rows are NaN)."""
        if self._status is None:
            return
        code = int(self._status.item())
        self._status.zero_()
        if code:
            raise _lib.QotError(f"qot_topological_infer flagged the batch (status {code}): bit 0 an edge leaves its "
                                "graph's node range, bit 1 slices outside the arrays, bit 2 a node id outside the table")
