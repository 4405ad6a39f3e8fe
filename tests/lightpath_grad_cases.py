"""Inputs and references shared by tests/test_infer_lightpath_grad_cpu.py (fixture soundness, no GPU) and
tests/test_gpu_infer_lightpath_grad.py (``LightpathPredictor.sensitivity`` against them): the mixed batch of
``test_gpu_infer_lightpath.py`` with two graphs added, the model pair, and the oracle's ``x.grad`` per output by plain
autograd, one backward per output.

A gradient is discontinuous at a leaky_relu / relu kink: inputs on which the oracle's own fp32 and fp64 runs disagree
cannot judge a kernel, so the CPU file asserts that they agree to ``TOL / 10`` on every batch built here."""
import copy
import functools

import torch

import gnn_qot_estimation_amd as q
from test_gpu_infer_lightpath import _chain_edges, _chains, _graph, _mixed, _star

WIDTHS, FEATURES, OUTPUTS = (4, 20, 32, 128), (2, 5, 16), (1, 3)
PARITY = [(C, F, O) for C in WIDTHS for F in FEATURES for O in OUTPUTS]
TRIPLE, SELF_LOOP = 6, 5            # graphs of the mixed batch: 1 -> 0 three times; an input self loop (its second edge)
TRIPLE_EDGES = (0, 1, 3)            # the three 1 -> 0 edges inside TRIPLE's slice ...
UNROLLED_NODES = (1, 3, 4)          # ... and the node of the unrolled copy (the batch's last graph) that sends each
ADJACENT_SEED, UNROLLED_SEED = 21, 13


def lut_columns(F):
    return sorted({0, 1, F - 1})


def oracle_model(F=5, C=32, O=3, lut=1, seed=0):
    """``oracle.sparse.LightpathGNN`` in eval mode with the parameter perturbation of ``test_gpu_infer_lightpath._models``
    (the same draws in the same order: the same model)."""
    from oracle import sparse as Osp
    torch.manual_seed(seed)
    ref = Osp.LightpathGNN(F, C, O, lut, dropout_p=0.0).eval()
    with torch.no_grad():
        ref.conv1.bias.uniform_(-0.5, 0.5)
        bn = ref.norm1.module
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
    return ref


def engine_model(ref, device):
    """The engine's model with ``ref``'s parameters and statistics, on ``device``, eval mode, parameters frozen."""
    conv = ref.conv1
    hip = q.LightpathGNN(conv.in_channels, conv.out_channels, ref.mlp[3].out_features, ref.is_lut_index, dropout_p=0.0)
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip = hip.to(device).eval()
    for p in hip.parameters():
        p.requires_grad_(False)
    return hip


def adjacent(F, lut):
    """A chain of 6 nodes whose LUT nodes 2 and 3 are adjacent: row 2's self term and row 3's edge term land on node 2."""
    return _graph(6, *_chain_edges(6), (2, 3), F, lut, ADJACENT_SEED)


def unrolled(F, lut):
    """The triple-edge graph of the mixed batch with its source node 1 split into three feature-identical nodes 1, 3, 4
    with one edge each: the GAT output of node 0 is unchanged, so the oracle's node gradients on the copies are the
    per-edge reference for the three repeated edges."""
    g = _graph(3, [1, 1, 2, 1, 0], [0, 0, 0, 0, 1], (0,), F, lut, UNROLLED_SEED)
    x = torch.cat([g.x, g.x[1:2], g.x[1:2]], 0)
    ei = torch.tensor([[1, 3, 2, 4, 0], [0, 0, 0, 0, 1]], dtype=torch.long)
    return q.Data(x=x, edge_index=ei, y=g.y, num_nodes=5)


def mixed(F, lut):
    """``test_gpu_infer_lightpath._mixed`` (14 graphs) + the adjacent-LUT chain + the unrolled triple-edge graph."""
    return _mixed(F, lut) + [adjacent(F, lut), unrolled(F, lut)]


def lut_rows(batch, lut):
    return (batch.x[:, lut] == 1.0).nonzero().squeeze(1)


def oracle_xgrad(ref, batch, outputs=None, dtype=torch.float64):
    """``(out [L, O], grad [Q, N, F])`` of ``ref`` in ``dtype``: ``x.grad`` after ``out[:, o].sum().backward()``, plain
    autograd, one backward per requested output."""
    model = copy.deepcopy(ref).to(dtype).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    b = copy.copy(batch)
    b.x = batch.x.detach().to(dtype).clone().requires_grad_()
    out = model(b)[0]
    sel = list(range(out.shape[1])) if outputs is None else list(outputs)
    grads = []
    for o in sel:
        b.x.grad = None
        out[:, o].sum().backward(retain_graph=True)
        grads.append(b.x.grad.detach().clone())
    return out.detach(), torch.stack(grads)


def assemble(jac_self, jac_edge, edge_index, rows, N):
    """The identity that defines the result, in fp64 on the host: ``J[q] = zeros(N, F)``, ``J[q].index_add_(0, src,
    jac_edge[q])``, ``J[q][rows] += jac_self[q]`` -> ``[Q, N, F]``."""
    js, je = jac_self.detach().double().cpu(), jac_edge.detach().double().cpu()
    src, rows = edge_index[0].cpu(), rows.cpu()
    J = torch.zeros(js.shape[0], N, js.shape[2], dtype=torch.float64)
    for k in range(js.shape[0]):
        J[k].index_add_(0, src, je[k])
        J[k][rows] += js[k]
    return J


def message_mask(batch, rows):
    """``[E]`` bool: the edges that are a message into one of the nodes ``rows`` (target in ``rows``, source != target)."""
    src, dst = batch.edge_index
    is_row = torch.zeros(batch.x.shape[0], dtype=torch.bool)
    is_row[rows] = True
    return is_row[dst] & (src != dst)


def slices(ptr):
    p = [int(v) for v in ptr]
    return list(zip(p[:-1], p[1:]))


@functools.lru_cache(maxsize=None)
def parity_case(C, F, O, lut):
    """``(ref, batch, out64, grad64)`` of one parity case: computed once, shared, never modified."""
    ref = oracle_model(F, C, O, lut)
    batch = q.Batch.from_data_list(mixed(F, lut))
    out64, grad64 = oracle_xgrad(ref, batch)
    return ref, batch, out64, grad64


EDGE_SHAPES = ((1, 1, 1), (16, 256, 8))   # (F, C, O): only lanes 0 - 3 own an (h, f) pair; all 64 lanes do


@functools.lru_cache(maxsize=None)
def edge_case(F, C, O):
    """``(ref, batch, out64, grad64)`` at the ends of the envelope's widths (LUT column 0), three graphs with one LUT node
    each: in-degree 65 (messages at slice offsets 0, 63 and 64: across the chunk boundary of the scan), in-degree 129
    (three chunks) and in-degree 0 (only the appended self loop).  Model seed 0: the oracle's fp32 and fp64 ``x.grad``
    agree to ``TOL / 10`` on every graph's own slice, and no graph's gradient vanishes for any output."""
    ref = oracle_model(F, C, O, 0)
    batch = q.Batch.from_data_list([_star(65, F, 0, 60), _star(129, F, 0, 61), _graph(3, [0, 1], [1, 2], (0,), F, 0, 62)])
    out64, grad64 = oracle_xgrad(ref, batch)
    return ref, batch, out64, grad64


def independence_graphs(F=5, lut=1):
    """``(g, others)`` of the bitwise-independence test: a 150-star with back edges, and six other graphs (the sixth has
    two LUT nodes)."""
    g = _star(150, F, lut, 40, back=40)
    others = _chains(4, F, lut, first=7) + [_star(65, F, lut, 41), _graph(5, *_chain_edges(5), (1, 3), F, lut, 42)]
    return g, others


def relabelled(F=5, lut=1, seed=77, count=40):
    """Other features for the mixed batch, ``count`` random LUT nodes (several in some graphs, none in others): the data
    the captured call is replayed on."""
    batch = q.Batch.from_data_list(mixed(F, lut))
    gen = torch.Generator().manual_seed(seed)
    x2 = torch.rand(batch.x.shape, generator=gen)
    x2[:, lut] = 0.0
    x2[torch.randperm(x2.shape[0], generator=gen)[:count], lut] = 1.0
    batch.x = x2
    return batch


def first_lut_only(batch, lut=1):
    """``(only, first, has)``: ``batch`` with the LUT flag kept on the lowest-numbered LUT node of every graph only (the
    flag is a feature: the rows ``per_graph`` computes on ``only`` are all of its LUT rows, so the oracle can judge them);
    ``first`` those nodes, ``has`` their graphs."""
    rows = lut_rows(batch, lut)
    has = sorted(set(batch.batch[rows].tolist()))
    first = torch.tensor([int(rows[batch.batch[rows] == g][0]) for g in has])
    only = copy.copy(batch)
    only.x = batch.x.clone()
    only.x[:, lut] = 0.0
    only.x[first, lut] = 1.0
    return only, first, has


TRACK_STEP = 0.05


@functools.lru_cache(maxsize=None)
def tracking_case(C=20):
    """``(batch, (before, after), deltas)`` of the parameter-following test: the oracle model, the same model after every
    parameter has moved in place by ``deltas[name]`` (seeded, ``TRACK_STEP`` * normal), and those steps."""
    before = oracle_model(5, C, 3, 1)
    gen = torch.Generator().manual_seed(9)
    deltas = {name: TRACK_STEP * torch.randn(p.shape, generator=gen) for name, p in before.named_parameters()}
    after = copy.deepcopy(before)
    with torch.no_grad():
        for name, p in after.named_parameters():
            p.add_(deltas[name])
    batch = q.Batch.from_data_list(_chains(6, 5, 1) + [_star(65, 5, 1, 50), adjacent(5, 1)])
    return batch, (before, after), deltas
