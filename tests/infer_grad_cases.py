"""Inputs and references shared by tests/test_infer_grad_cpu.py (fixture soundness, no GPU) and
tests/test_gpu_infer_grad.py (``TopologicalPredictor.sensitivity`` against them): seeded ``synthetic.py`` graphs, the model
pair, and the oracle's Jacobian wrt the edge features by plain autograd, one backward per output.

A gradient is discontinuous at a leaky_relu / relu kink: inputs on which the oracle's own fp32 and fp64 runs disagree
cannot judge a kernel, so the CPU file asserts that they agree to ``TOL / 10`` on every batch built here."""
import copy
import functools
import math

import torch

import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import infer, synthetic as S

PARITY = [(H, D, O) for H in (16, 32, 64) for D in (1, 4) for O in (1, 3)]
DEGENERATE_WIDTHS = (16, 64)
PARITY_SEED = 1         # (seed 0: the oracle's fp32 and fp64 Jacobians of the one-edge graph differ by 2.6e-5 at H = 64, D = 1)


def oracle_model(V, H, O=3, D=4, seed=0):
    """``oracle.sparse.TopologicalGNN`` in eval mode, seeded, zero-initialised biases made to matter."""
    from oracle import sparse as Osp
    torch.manual_seed(seed)
    ref = Osp.TopologicalGNN(V, H, O, D, dropout_p=0.0).eval()
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1 and p.abs().max() == 0:
                p.uniform_(-0.1, 0.1)
    return ref


def engine_model(ref, device):
    """The engine's model with ``ref``'s parameters, on ``device``, eval mode, parameters frozen."""
    m = ref
    hip = q.TopologicalGNN(m.node_embeddings.num_embeddings, m.node_embeddings.embedding_dim, m.mlp[3].out_features,
                           m.conv1.edge_dim, dropout_p=0.0)
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip = hip.to(device).eval()
    for p in hip.parameters():
        p.requires_grad_(False)
    return hip


def graph(n, e, D=4, g=0, edges=None):
    """One seeded synthetic graph of ``n`` nodes and ``e`` directed edges (both directions of e / 2 links); ``edges`` keeps
    only its first so many directed edges (odd counts, a single edge)."""
    b = S.topological_batch(2, 1, n=n, e=e, edge_dim=D, first_graph=g)
    ei, ea = b.edge_index, b.edge_attr
    if edges is not None:
        assert edges <= ei.shape[1], (edges, ei.shape[1])
        ei, ea = ei[:, :edges].contiguous(), ea[:edges].contiguous()
    return q.Data(edge_index=ei, edge_attr=ea, node_ids=torch.arange(n), num_nodes=n)


def custom(n, src, dst, D=4, seed=0):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)
    return q.Data(edge_index=ei, edge_attr=torch.rand(ei.shape[1], D, generator=gen), node_ids=torch.arange(n),
                  num_nodes=n)


def parity_graphs(H, D):
    """The mixed batch of the parity test: node counts on both sides of the row tile (16 or 32) at all three widths, one
    graph exactly at the sensitivity edge cap of the batch's largest node count (128)."""
    cap = infer.grad_edge_cap(128, H, D)
    e75 = min(600, cap)
    return [graph(2, 2, D, 0, edges=1),                   # a single directed edge
            graph(7, 12, D, 1),
            graph(33, 90, D, 5),
            graph(75, e75 + e75 % 2, D, 2, edges=e75),
            graph(100, cap + 1 + (cap + 1) % 2, D, 3, edges=cap),        # exactly at the cap
            graph(128, 400, D, 4)], cap


def degenerate(D=4):
    """``test_gpu_infer.py``'s degenerate set, restated."""
    half = graph(20, 60, D, 7)
    keep = half.edge_index[1] < 10                        # nodes 10..19: in-degree 0
    half = q.Data(edge_index=half.edge_index[:, keep], edge_attr=half.edge_attr[keep], node_ids=torch.arange(20),
                  num_nodes=20)
    return [
        q.Data(edge_index=torch.zeros(2, 0, dtype=torch.long), edge_attr=torch.zeros(0, D), node_ids=torch.arange(9),
               num_nodes=9),                                                     # no edges at all
        half,
        custom(6, [0, 1, 2, 2, 3, 5, 4], [0, 1, 2, 3, 2, 5, 0], D, 1),           # self loops (one node: only a loop)
        custom(5, [0, 1, 1, 1, 2, 3, 1], [1, 2, 2, 2, 3, 4, 0], D, 2),           # 1 -> 2 three times, different features
        custom(1, [], [], D, 3),                                                 # a single node
        custom(1, [0, 0], [0, 0], D, 4),                                         # ... and one with a repeated loop
    ]


FD_STEP = 1e-2
# (edge, feature) pairs of the central-difference test.  With a step this large a leaky_relu kink can lie inside [x - h,
# x + h], where the difference quotient is no derivative ((19, 3) and (14, 3) are such: the oracle's own autograd and its
# own difference quotient disagree by 1e-3 ... 9e-3 of the Jacobian's largest entry there); the CPU file asserts that on
# these three they agree to 1e-4 of the entry itself.
FD_POINTS = ((0, 0), (7, 1), (23, 2))


def fd_graph():
    """The 12-node / 30-edge graph of the central-difference test."""
    return graph(12, 30, 4, 40)


def fd_slopes(ref, batch):
    """``{(e, d): slope [O]}``: central differences of the fp64 oracle's output wrt ``edge_attr[e, d]``, step FD_STEP."""
    ref64 = copy.deepcopy(ref).double().eval()
    res = {}
    for e, d in FD_POINTS:
        outs = []
        for sign in (1.0, -1.0):
            b = copy.copy(batch)
            b.edge_attr = batch.edge_attr.double().clone()
            b.edge_attr[e, d] += sign * FD_STEP
            with torch.no_grad():
                outs.append(ref64(b)[0])
        res[(e, d)] = (outs[0] - outs[1]) / (2 * FD_STEP)
    return res


def oracle_jacobian(ref, batch, outputs=None, dtype=torch.float64):
    """``(out [B, O], jac [Q, E, D])`` of ``ref`` in ``dtype``: plain autograd, one backward per requested output."""
    model = copy.deepcopy(ref).to(dtype).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    b = copy.copy(batch)
    b.edge_attr = batch.edge_attr.detach().to(dtype).clone().requires_grad_()
    out = model(b)
    sel = list(range(out.shape[1])) if outputs is None else list(outputs)
    jac = []
    for o in sel:
        b.edge_attr.grad = None
        out[:, o].sum().backward(retain_graph=True)
        g = b.edge_attr.grad
        jac.append(torch.zeros_like(b.edge_attr) if g is None else g.detach().clone())
    jac = torch.stack(jac) if jac else torch.zeros(0, *b.edge_attr.shape, dtype=dtype)
    return out.detach(), jac


def oracle_alpha(ref, batch):
    """``oracle.sparse.TransformerConv.forward``'s softmax in fp64, ``[E, 1]`` in edge order."""
    from oracle import sparse as Osp
    c = copy.deepcopy(ref.conv1).double()
    x = ref.node_embeddings.weight.detach().double()[batch.node_ids]
    ea = batch.edge_attr.detach().double()
    src, dst = batch.edge_index
    with torch.no_grad():
        k = c.lin_key(x)[src] + c.lin_edge(ea)
        s = (c.lin_query(x)[dst] * k).sum(-1) / math.sqrt(c.out_channels)
        return Osp.segment_softmax(s, dst, x.shape[0]).unsqueeze(1)


TRACK_LR = 0.5


@functools.lru_cache(maxsize=None)
def tracking_case():
    """``(batch, refs, grads)`` of the parameter-tracking test: three 30-node / 100-edge graphs; ``refs`` the oracle model
    at its three stages -- seeded, after ONE in-place SGD step (lr ``TRACK_LR``) along ``grads`` (its own smooth-L1
    gradients against a seeded target), and with the parameters of another seed loaded."""
    batch = q.Batch.from_data_list([graph(30, 100, 4, 20 + k) for k in range(3)])
    first = oracle_model(30, 32)
    stepped = copy.deepcopy(first)
    target = torch.rand(3, 3, generator=torch.Generator().manual_seed(7)) + 1.0
    torch.nn.functional.smooth_l1_loss(stepped(batch), target).backward()
    grads = {name: p.grad.detach().clone() for name, p in stepped.named_parameters()}
    with torch.no_grad():
        for name, p in stepped.named_parameters():
            p.sub_(TRACK_LR * grads[name])
            p.grad = None
    return batch, (first, stepped, oracle_model(30, 32, seed=5)), grads


def edge_slices(batch):
    """``[(e0, e1)]`` per graph of the batch."""
    ep = [int(v) for v in batch.edge_ptr]
    return list(zip(ep[:-1], ep[1:]))


@functools.lru_cache(maxsize=None)
def parity_case(H, D, O):
    """``(ref, batch, cap, out64, jac64, alpha64)`` of one parity case: computed once, shared, never modified."""
    graphs, cap = parity_graphs(H, D)
    batch = q.Batch.from_data_list(graphs)
    ref = oracle_model(128, H, O, D, PARITY_SEED)
    out64, jac64 = oracle_jacobian(ref, batch)
    return ref, batch, cap, out64, jac64, oracle_alpha(ref, batch)


@functools.lru_cache(maxsize=None)
def degenerate_case(H):
    """``(ref, graphs, batch, out64, jac64, alpha64)`` of the degenerate set as one batch."""
    graphs = degenerate()
    batch = q.Batch.from_data_list(graphs)
    ref = oracle_model(20, H)
    out64, jac64 = oracle_jacobian(ref, batch)
    return ref, graphs, batch, out64, jac64, oracle_alpha(ref, batch)
