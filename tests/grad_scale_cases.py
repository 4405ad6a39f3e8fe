"""Case tables and fp64 references of tests/test_gpu_grad_scale.py: every backward form of the package, fed a gradient
``c * g`` for ``c`` in ``SCALES`` (one fixed seeded ``g`` of unit scale).  Training does not run at ``c = 1``: the loss is
a mean over ``B * 3`` outputs (2^-10 .. 2^-12 at the flagship batch), shrinks late in training and under data-parallel
global batches, and grows under loss scaling.

Backward is linear in the incoming gradient, so one fp64 reference at ``c = 1`` serves every scale (``c * ref`` is exact),
and an fp32 kernel with a fixed summation order must return ``grads(c g) == c * grads(g)`` bit for bit.  The tensors that
are exempt from that (check 3) are the ones summed with fp32 atomics; each is named here with the atomic's place.

Nothing here touches the GPU: inputs, oracle modules and references live on the host, each built once and shared."""
import copy
import functools

import torch
import torch.nn.functional as F

import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import synthetic as S

SCALES = tuple(2.0 ** k for k in (-30, -15, 0, 15, 30))
# additive floors of the sibling rule (tests/test_gpu_nnconv_split_bf16.py): errors are taken relative to max|ref| after the
# kernel's result is divided by c, which is the rule's floor scaled by c
SIBLING_MAX, SIBLING_RMS, FLOOR_MAX, FLOOR_RMS = 2.0, 1.5, 1e-7, 1e-8
SLOPE = 0.01                     # leaky_relu behind conv1 (topological_training/models.py:54)

# fp32 atomics in backward kernels (global or LDS): the sums they feed have no fixed order
ATOMIC_EMBED = "csrc/misc.hip:65-72 (embed_bwd: table rows summed with atomicAdd, LDS image and global)"
ATOMIC_NNCONV_W1 = "csrc/nnconv.hip:140-147 (qot_nnconv_bwd_edge: w1 / b1 sums with LDS and global atomicAdd)"
ATOMIC_GRAPH_GM = "csrc/tconv_graph.hip:550 (graph form: ds_e added into the fp32 LDS image of grad M with atomicAdd)"
# what the grad M image of the graph form feeds: grad T_q and grad T_k, hence these parameters and the table behind them
_GM_CONSUMERS = ("lin_query.weight", "lin_query.bias", "lin_key.weight", "lin_key.bias")

# an analytically zero gradient (a constant added to every key of a destination leaves its softmax alone; a bias in front
# of a train-mode BatchNorm) is rounding noise on both sides: measured on the scale of the named tensor, as
# tests/test_gpu_tconv_rows.py and helpers.grad_compare do
ZERO_TCONV = {"lin_key.bias": "lin_key.weight"}
ZERO_TOPO = {"conv1.lin_key.bias": "conv1.lin_key.weight"}
ZERO_LIGHTPATH = {"conv1.bias": "conv1.lin.weight"}


# ------------------------------------------------------------------ TransformerConv, operator level
# conv(table[node_ids], edge_index, edge_attr) followed by leaky_relu (the fused epilogue the model uses), against
# oracle.sparse.TransformerConv in fp64.  ``form``: which backward must run (asserted from the recorded _lib.call names);
# ``env``: switches set through monkeypatch; ``sibling``: the switches of the implementation check 2 compares with.
# Row form: table mode, n % 4 == 0, N >= 4 n, n above the tile-form threshold (2 * rows_per_block * max(2, E / N): 96 at
# H = 64), npad = 32 * ceil(n / 32) != n.
TCONV_CASES = {
    # parts = 8, per = ceil(9 / 8) = 2: slices 5, 6, 7 are empty, slice 4 holds one graph
    "rows_h64_d4_b9": dict(form="rows", cfg=4, n=260, e=780, H=64, D=4, B=9, sibling={"QOT_NO_TCONV_SCORES": "1"}),
    # power-law degrees (cfg 5 generator: the hubs sit at the same rows of every graph, so many threads meet on one entry of
    # the LDS image); edge_dim > 4
    "rows_h128_d6_b13_powerlaw": dict(form="rows", cfg=5, n=264, e=0, H=128, D=6, B=13,
                                      sibling={"QOT_NO_TCONV_SCORES": "1"}),
    "rows_h256_d1_b5": dict(form="rows", cfg=4, n=260, e=780, H=256, D=1, B=5, sibling={"QOT_NO_TCONV_SCORES": "1"}),
    # the image pass shares a slice's in-edges evenly among its 256 threads (scan of the in-edge counts, binary search): 20
    # graphs per slice of power-law graphs put more than two rounds of 256 edges on the hub rows and fewer than 256 on every
    # other row (``min_slice_edges``, checked on the host)
    "rows_h64_d1_b160_powerlaw_hubs": dict(form="rows", cfg=5, n=264, e=0, H=64, D=1, B=160, min_slice_edges=513,
                                           sibling={"QOT_NO_TCONV_SCORES": "1"}),
    # the image pass takes a slice's destinations 256 at a time: ONE slice of 300 graphs (QOT_TCONV_ROWS_PARTS=1; with the
    # usual 8 slices that needs more than 2048 graphs) gives a full chunk and one of 44; trees only (e = 0 asks for no extra
    # links), n = 132 is the smallest n % 4 == 0 above the graph form's 128
    "rows_h64_d1_b300_one_slice": dict(form="rows", cfg=2, n=132, e=0, H=64, D=1, B=300, env={"QOT_TCONV_ROWS_PARTS": "1"},
                                       sibling={"QOT_NO_TCONV_SCORES": "1"}),
    # graph form (cfg2's shape, and a small one at H = 128, D = 3) and the per-destination kernels in table mode on the
    # same batches
    "graph_h64_b8": dict(form="graph", cfg=2, n=100, e=400, H=64, D=4, B=8, sibling={"QOT_NO_TCONV_GRAPH": "1"},
                         inhomogeneous={k: ATOMIC_GRAPH_GM for k in _GM_CONSUMERS + ("table",)}),
    "graph_h128_d3_b3": dict(form="graph", cfg=2, n=30, e=80, H=128, D=3, B=3, sibling={"QOT_NO_TCONV_GRAPH": "1"},
                             inhomogeneous={k: ATOMIC_GRAPH_GM for k in _GM_CONSUMERS + ("table",)}),
    "dst_table_h64_b8": dict(form="dst_table", cfg=2, n=100, e=400, H=64, D=4, B=8, env={"QOT_NO_TCONV_GRAPH": "1"}),
    "dst_table_h128_d3_b3": dict(form="dst_table", cfg=2, n=30, e=80, H=128, D=3, B=3, env={"QOT_NO_TCONV_GRAPH": "1"}),
    # node mode: graphs of 8 / 10 / 12 nodes (no uniform node_ids): EmbedFn, the node-level projection GEMM and the
    # per-destination kernels without a table
    "node_h32_mixed": dict(form="node", cfg=2, n=(8, 10, 12), e=None, H=32, D=4, B=9,
                           inhomogeneous={"table": ATOMIC_EMBED}),
}
TCONV_KERNELS = {"rows": ("qot_tconv_bwd_dst_rows", "qot_tconv_bwd_src_rows"), "graph": ("qot_tconv_bwd_graph",),
                 "dst_table": ("qot_tconv_bwd_dst", "qot_tconv_bwd_src", "qot_table_project_fwd"),
                 "node": ("qot_tconv_bwd_dst", "qot_tconv_bwd_src", "qot_embed_bwd")}
TCONV_NAMES = ("table", "lin_query.weight", "lin_query.bias", "lin_key.weight", "lin_key.bias", "lin_value.weight",
               "lin_value.bias", "lin_skip.weight", "lin_skip.bias", "lin_edge.weight")


def _topo_batch(c):
    if isinstance(c["n"], tuple):
        graphs = []
        for g in range(c["B"]):
            n = c["n"][g % len(c["n"])]
            b = S.topological_batch(c["cfg"], 1, n=n, e=2 * n + 6, edge_dim=c["D"], first_graph=g)
            graphs.append(q.Data(edge_index=b.edge_index, edge_attr=b.edge_attr, node_ids=b.node_ids,
                                 y=b.y.view(1, 3), num_nodes=n))
        return q.Batch.from_data_list(graphs)
    return S.topological_batch(c["cfg"], c["B"], n=c["n"], e=c["e"], edge_dim=c["D"])


def _nonzero_biases(module):
    with torch.no_grad():
        for p in module.parameters():
            if p.dim() == 1 and p.abs().max() == 0:
                p.uniform_(-0.1, 0.1)


def poison_node(batch):
    """A node with in-edges and out-edges that is not in the last graph: the destination of the batch's first edge."""
    ei = batch.edge_index
    i = int(ei[1, 0])
    assert bool((ei[0] == i).any()) and bool((ei[1] == i).any()) and i < int(batch.ptr[-2])
    return i


def poisoned(g, node):
    """``g`` with row ``node`` NaN, and ``g`` with one element of that row +inf (check 4)."""
    a, b = g.clone(), g.clone()
    a[node] = float("nan")
    b[node, 5 % g.shape[1]] = float("inf")
    return {"nan_row": a, "inf_element": b}


def _backward_all(out, params, g, extra):
    """``{tag: {name: grad}}`` for ``g`` (tag 1.0) and every gradient of ``extra``, through one retained graph."""
    res = {}
    for tag, gg in [(1.0, g)] + list(extra.items()):
        for p in params.values():
            p.grad = None
        out.backward(gg.to(out.dtype), retain_graph=True)
        res[tag] = {k: p.grad.detach().clone() for k, p in params.items()}
    return res


@functools.lru_cache(maxsize=None)
def tconv_case(name):
    """Batch, fp32 parameters, the unit gradient ``g [N, H]``, its poisoned versions and the fp64 gradients of all three."""
    from oracle import sparse as O
    c = TCONV_CASES[name]
    batch = _topo_batch(c)
    H, D = c["H"], c["D"]
    V = max(c["n"]) if isinstance(c["n"], tuple) else c["n"]
    if "min_slice_edges" in c:
        # in-edges of table row r over one slice of the graphs (8 slices of ceil(B / 8) graphs: functional._tconv_backward_rows)
        per = -(-c["B"] // 8)
        indeg = torch.bincount(batch.edge_index[1], minlength=batch.num_nodes).view(c["B"], V)
        heaviest = max(int(indeg[s:s + per].sum(0).max()) for s in range(0, c["B"], per))
        lightest = min(int(indeg[s:s + per].sum(0).min()) for s in range(0, c["B"], per))
        assert heaviest >= c["min_slice_edges"] > lightest, (heaviest, lightest)
    torch.manual_seed(20 + H + D)
    ref = O.TransformerConv(H, H, edge_dim=D)
    table = torch.randn(V, H)
    gen = torch.Generator().manual_seed(1000 + H)
    g = torch.randn(batch.num_nodes, H, generator=gen)
    bad = poisoned(g, poison_node(batch))
    ref64 = copy.deepcopy(ref).double()
    t64 = table.double().requires_grad_(True)
    out = F.leaky_relu(ref64(t64[batch.node_ids], batch.edge_index, batch.edge_attr.double()), SLOPE)
    params = dict([("table", t64)] + list(ref64.named_parameters()))
    assert sorted(params) == sorted(TCONV_NAMES)
    return dict(cfg=c, batch=batch, state=ref.state_dict(), table=table, g=g, bad=bad,
                ref=_backward_all(out, params, g.double(), {k: v.double() for k, v in bad.items()}))


# ------------------------------------------------------------------ NNConv at H = 64, operator level
# the ``ragged`` graph of tests/test_gpu_nnconv_split_bf16.py (1013 nodes: not a multiple of the 32-row tile) and the ``hub``
# graph of tests/test_gpu_nnconv_adjoint_split.py (40 out-edges of node 3, source nodes without out-edges), restated
NNCONV_H = 64
NNCONV_NAMES = ("x", "w1", "b1", "w2", "b2", "wroot", "bias")


def _nnconv_graph(kind, gen):
    if kind == "hub":
        N = 70
        srcs = torch.tensor([j for j in range(N) if j % 3 != 2])
        src = torch.cat([torch.full((40,), 3, dtype=torch.int64), srcs[torch.randint(0, len(srcs), (150,), generator=gen)]])
        return N, torch.stack([src, torch.randint(0, N, (190,), generator=gen)])
    N = 1000 + 13
    return N, torch.randint(0, N, (2, 4 * N), generator=gen)


@functools.lru_cache(maxsize=None)
def nnconv_case(kind):
    H, D = NNCONV_H, 4
    K = 2 * D
    gen = torch.Generator().manual_seed(7)
    N, ei = _nnconv_graph(kind, gen)
    E = ei.shape[1]
    p = dict(x=torch.randn(N, H, generator=gen), ea=torch.rand(E, D, generator=gen),
             w1=torch.randn(K, D, generator=gen) * 0.5, b1=torch.randn(K, generator=gen) * 0.5,
             w2=torch.randn(H * H, K, generator=gen) / 16, b2=torch.randn(H * H, generator=gen) / 16,
             wroot=torch.randn(H, H, generator=gen) / 8, bias=torch.randn(H, generator=gen))
    g = torch.randn(N, H, generator=gen)
    # a node with in-edges and out-edges (there is one graph: "not in the last graph" has no meaning here)
    node = next(i for i in ei[1].tolist() if bool((ei[0] == i).any()))
    bad = poisoned(g, node)
    t = {k: v.double().clone().requires_grad_(k != "ea") for k, v in p.items()}
    src, dst = ei[0], ei[1]
    h = torch.relu(t["ea"] @ t["w1"].t() + t["b1"])
    We = (h @ t["w2"].t() + t["b2"]).view(-1, H, H)
    msg = torch.einsum("ea,eao->eo", t["x"][src], We)
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, dst, torch.ones(E, dtype=torch.float64))
    agg = torch.zeros(N, H, dtype=torch.float64).index_add_(0, dst, msg) / deg.clamp(min=1)[:, None]
    out = agg + t["x"] @ t["wroot"].t() + t["bias"]
    params = {k: t[k] for k in NNCONV_NAMES}
    return dict(N=N, ei=ei, p=p, g=g, bad=bad,
                ref=_backward_all(out, params, g.double(), {k: v.double() for k, v in bad.items()}))


# ------------------------------------------------------------------ whole models
# out.backward(c * g) with g [rows, 3]: the read-out's backward with an explicit gradient (HeadFn; the folded-loss path forms
# its own gradient and is out of scope), the NNConv layers at every width, and TransformerConv in the form the batch takes.
# Training mode, dropout 0.  ``sibling``: as above.  ``kernels``: _lib.call names or role kinds that must have run.
_BN_BWD = ("qot_bn_bwd_reduce_rows", "qot_bn_bwd_reduce")          # (a tuple inside ``kernels``: any one of them)
_LP_WALK = ("qot_gat_bwd_dst", "qot_gat_bwd_src", _BN_BWD)
_LP_THIN = ("qot_gat_bwd_dst_thin", "qot_gat_bwd_src", _BN_BWD)
MODEL_CASES = {
    # H = 64: split-bf16 NNConv (default) against the fp32-MFMA kernels; graph-form TransformerConv; fused head
    "topo_h64_b8": dict(kind="topo", cfg=2, n=100, e=400, H=64, D=4, B=8, sibling={"QOT_NNCONV_F32_MFMA": "1"},
                        kernels=("qot_nnconv_gradh_split", "qot_nnconv_adjoint_dw", "qot_tconv_bwd_graph", "qot_head_bwd"),
                        inhomogeneous={"conv1." + k: ATOMIC_GRAPH_GM for k in _GM_CONSUMERS} |
                                      {"node_embeddings.weight": ATOMIC_GRAPH_GM}),
    "topo_h64_b8_f32_mfma": dict(kind="topo", cfg=2, n=100, e=400, H=64, D=4, B=8, env={"QOT_NNCONV_F32_MFMA": "1"},
                                 kernels=("qot_nnconv_gradh_fused", "qot_nnconv_adjoint_dw"),
                                 inhomogeneous={"conv1." + k: ATOMIC_GRAPH_GM for k in _GM_CONSUMERS} |
                                               {"node_embeddings.weight": ATOMIC_GRAPH_GM}),
    # H = 128 and H = 32: csrc/nnconv_gen.hip
    "topo_h128_d3_b3": dict(kind="topo", cfg=2, n=30, e=80, H=128, D=3, B=3,
                            kernels=("qot_nnconv_dw", "qot_nnconv_gradh_fused", "qot_tconv_bwd_graph"),
                            inhomogeneous={"conv1." + k: ATOMIC_GRAPH_GM for k in _GM_CONSUMERS} |
                                          {"node_embeddings.weight": ATOMIC_GRAPH_GM}),
    "topo_h32_mixed_nodes": dict(kind="topo", cfg=2, n=(8, 10, 12), e=None, H=32, D=4, B=9,
                                 kernels=("qot_nnconv_dw", "qot_nnconv_gradh_fused", "qot_tconv_bwd_dst", "qot_embed_bwd"),
                                 inhomogeneous={"node_embeddings.weight": ATOMIC_EMBED}),
    # edge_dim = 6: the materialised-operand NNConv (csrc/nnconv.hip), whose first-layer sums use atomics
    "topo_h64_d6_b7": dict(kind="topo", cfg=2, n=25, e=90, H=64, D=6, B=7,
                           kernels=("qot_nnconv_bwd_edge", "qot_nnconv_agg", "qot_tconv_bwd_graph"),
                           inhomogeneous={"conv1." + k: ATOMIC_GRAPH_GM for k in _GM_CONSUMERS} |
                                         {"node_embeddings.weight": ATOMIC_GRAPH_GM,
                                          "conv2.nn.0.weight": ATOMIC_NNCONV_W1, "conv2.nn.0.bias": ATOMIC_NNCONV_W1}),
    # LightpathGNN in training mode (BatchNorm backward, the skinny / small projections, the GAT walk), the first layer thin
    # and not thin (forced as tests/test_gpu_parity.py::test_lightpath_fwd_bwd does); C = 32 and C = 8 (not a multiple of 32)
    "lp_c32_b64": dict(kind="lp", C=32, B=64, env={"QOT_GAT_THIN_MIN_ROWS": "1000000000"}, kernels=_LP_WALK),
    "lp_c32_b64_thin": dict(kind="lp", C=32, B=64, env={"QOT_GAT_THIN_MIN_ROWS": "1"}, kernels=_LP_THIN,
                            sibling={"QOT_GAT_THIN_MIN_ROWS": "1000000000"}),
    "lp_c8_b5": dict(kind="lp", C=8, B=5, env={"QOT_GAT_THIN_MIN_ROWS": "1000000000"}, kernels=_LP_WALK),
    "lp_c8_b5_thin": dict(kind="lp", C=8, B=5, env={"QOT_GAT_THIN_MIN_ROWS": "1"}, kernels=_LP_THIN,
                          sibling={"QOT_GAT_THIN_MIN_ROWS": "1000000000"}),
}


def _double_batch(batch):
    b = copy.copy(batch)
    for f in ("x", "edge_attr"):
        v = getattr(b, f, None)
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            setattr(b, f, v.double())
    return b


def model_kwargs(c):
    if c["kind"] == "topo":
        V = max(c["n"]) if isinstance(c["n"], tuple) else c["n"]
        return dict(num_nodes=V, hidden_channels=c["H"], out_channels=3, edge_dim=c["D"], dropout_p=0.0)
    return dict(in_channels=5, hidden_channels=c["C"], output_dim=3, is_lut_index=1, dropout_p=0.0)


def _model_inputs(c):
    return tuple(sorted((k, v) for k, v in c.items() if k in ("kind", "cfg", "n", "e", "H", "D", "B", "C")))


@functools.lru_cache(maxsize=None)
def _model_reference(key):
    from oracle import sparse as O
    c = dict(key)
    batch = _topo_batch(c) if c["kind"] == "topo" else S.lightpath_batch(c["B"])
    torch.manual_seed(0)
    ref = (O.TopologicalGNN if c["kind"] == "topo" else O.LightpathGNN)(**model_kwargs(c))
    _nonzero_biases(ref)
    state = copy.deepcopy(ref.state_dict())
    ref64 = copy.deepcopy(ref).double().train()
    res = ref64(_double_batch(batch))
    out = res if c["kind"] == "topo" else res[0]
    gen = torch.Generator().manual_seed(77)
    g = torch.randn(out.shape, generator=gen)
    params = dict(ref64.named_parameters())
    return dict(batch=batch, state=state, g=g, out=out.detach(), ref=_backward_all(out, params, g.double(), {}))


def model_case(name):
    """Batch, the oracle's fp32 state, the unit gradient ``g [rows, 3]`` and the fp64 output and gradients; cases that
    differ only in their switches share one reference."""
    c = MODEL_CASES[name]
    return dict(_model_reference(_model_inputs(c)), cfg=c)


# ------------------------------------------------------------------ figures
def tensor_errors(got, ref, scale_ref=None):
    """``got`` (already divided by c, fp64) against ``ref``: max and RMS error over ``max|scale_ref|`` (the tensor's own
    reference unless it is analytically zero), and the worst per-element figure ``|d| / (|ref| + 1e-6 max|ref|)``."""
    d = (got - ref).abs()
    m = float((ref if scale_ref is None else scale_ref).abs().max())
    m = m if m > 0 else 1.0
    return dict(max=float(d.max()) / m, rms=float(d.pow(2).mean().sqrt()) / m,
                elem=float((d / (ref.abs() + 1e-6 * m)).max()))
