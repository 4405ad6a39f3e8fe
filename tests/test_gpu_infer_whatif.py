"""GPU: K edits of a batch's graphs scored in one launch (``TopologicalPredictor.what_if`` /
``qot_topological_infer_whatif``).

The call is DEFINED as ``predict(materialise_what_if(...))`` and runs the eval kernel's own phases on an edge list whose
numbering rises as the materialised graph's does, so the comparison is ``torch.equal``: there is no tolerance to choose.
Beside it, the model's own eval forward at the suite's ``TOL``.  The candidates are ``infer_whatif_cases.edits()``: every
edit on the 7-node and on the 75-node graph of the base batch, alternating, in one call.  What is computed once per
``(H, D)`` -- models, predictor, the materialised batch and its rows -- is shared by the tests and only read."""
import functools

import pytest
import torch

import gnn_qot_estimation_amd as q
import infer_whatif_cases as WC
from gnn_qot_estimation_amd import _lib, infer
from helpers import TOL, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(16, 1), (16, 4), (32, 3), (64, 4)]


@functools.lru_cache(maxsize=None)
def _setup(H, D, device):
    _, hip = WC.models(device, H, D)
    pred = q.TopologicalPredictor(hip)
    w = WC.build(D)
    a, kw = WC.args(w, device)
    mat = infer.materialise_what_if(*a, **kw)
    return hip, pred, w, mat, pred(mat)


def _call(pred, w, device, **over):
    a, kw = WC.args(w, device)
    return pred.what_if(*a, **{**kw, **over})


@pytest.mark.parametrize("H,D", SHAPES)
def test_what_if_is_predict_of_the_materialised_batch_bit_for_bit(cuda_device, H, D):
    hip, pred, w, mat, want = _setup(H, D, cuda_device)
    out = _call(pred, w, cuda_device)
    pred.check_status()
    K = len(w.edits)
    assert tuple(out.shape) == (K, 3) and out.dtype == torch.float32 and out.grad_fn is None and out.device == want.device
    assert bool(torch.isfinite(out).all())
    for k, c in enumerate(w.edits):
        assert torch.equal(out[k], want[k]), (k, c.name, c.graph)
    assert torch.equal(out, _call(pred, w, cuda_device))                    # reproducible
    # the edits do change the answer: apart from the duplicates of "no edit" the rows of one graph differ
    rows = {tuple(out[k].tolist()) for k, c in enumerate(w.edits) if c.graph == 1}
    assert len(rows) >= 9, len(rows)
    # pointer arrays handed over as device tensors (one read each) give the same launch
    dev = lambda v: torch.tensor(v, device=cuda_device)
    a, kw = WC.args(w, cuda_device)
    assert torch.equal(pred.what_if(*a[:3], dev(w.add_ptr), drop=kw["drop"], drop_ptr=dev(w.drop_ptr), graph=kw["graph"]), out)


@pytest.mark.parametrize("H,D", SHAPES)
def test_what_if_matches_the_models_eval_forward_of_the_materialised_batch(cuda_device, H, D):
    hip, pred, w, mat, _ = _setup(H, D, cuda_device)
    out = _call(pred, w, cuda_device)
    with torch.no_grad():
        own = hip.eval()(mat)
    e = rel_err(out, own)
    print(f"H {H} D {D}: what_if vs model.eval()(materialised) {e:.3e}")
    assert e <= TOL, e


@pytest.mark.parametrize("H,D", SHAPES)
def test_no_edit_candidates_are_the_base_batchs_rows(cuda_device, H, D):
    """The three existing kernels are untouched: K = B candidates without an edit are ``predict(data)``, graph by graph."""
    hip, pred, w, _, _ = _setup(H, D, cuda_device)
    data = w.data.to(cuda_device)
    base = pred(data)
    none = (torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, D))
    out = pred.what_if(data, *none, [0, 0, 0], graph=torch.tensor([0, 1]))
    for g in range(2):
        assert torch.equal(out[g], base[g]), g
    out = pred.what_if(data, *none, [0, 0, 0, 0], drop=torch.zeros(0, dtype=torch.long), drop_ptr=[0, 0, 0, 0],
                       graph=torch.tensor([1, 0, 1]))
    assert torch.equal(out, base[[1, 0, 1]])
    assert tuple(pred.what_if(data, *none, [0], graph=torch.zeros(0, dtype=torch.long)).shape) == (0, 3)
    pred.check_status()


@pytest.mark.parametrize("H,D", [(16, 4), (64, 4)])
def test_a_candidates_row_does_not_depend_on_the_other_candidates(cuda_device, H, D):
    hip, pred, w, _, want = _setup(H, D, cuda_device)
    ks = [9, 2, 19, 4, 16, 7, 20, 13, 18]                                   # 9 of the 22, both graphs, adds and drops
    nine = _call(pred, WC.pick(w, ks), cuda_device)
    for where in (0, 8):                                                    # the first and the last of the nine, alone
        alone = _call(pred, WC.pick(w, [ks[where]]), cuda_device)
        assert tuple(alone.shape) == (1, 3) and torch.equal(alone[0], nine[where]), where
    assert torch.equal(nine, want[ks])
    pred.check_status()


def _big_graph(n, e, D, seed):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=gen)
    return q.Data(edge_index=ei, edge_attr=torch.rand(e, D, generator=gen), node_ids=torch.arange(n) % WC.V, num_nodes=n)


def test_a_candidate_exactly_at_the_edge_cap_and_one_above(cuda_device):
    H, D, n = 64, 4, 128
    hip, pred = _setup(H, D, cuda_device)[:2]
    cap = infer.what_if_edge_cap(n, H, D)
    assert cap == infer.edge_cap(n, H, D) and cap > 64
    data = q.Batch.from_data_list([_big_graph(n, cap - 2, D, 5)]).to(cuda_device)
    gen = torch.Generator().manual_seed(6)
    add = torch.randint(0, n, (2, 5), generator=gen).to(cuda_device)
    attr = torch.rand(5, D, generator=gen).to(cuda_device)
    # two additions reach the cap exactly (B == 1: no `graph`); a second candidate drops two edges and adds two
    a = (data, add[:, :4], attr[:4], [0, 2, 4])
    kw = dict(drop=torch.tensor([cap - 3, 0], device=cuda_device), drop_ptr=[0, 0, 2])
    out = pred.what_if(*a, **kw)
    pred.check_status()
    mat = infer.materialise_what_if(*a, **kw)
    assert mat.edge_ptr.tolist() == [0, cap, 2 * cap - 2]
    assert torch.equal(out, pred(mat)) and bool(torch.isfinite(out).all())
    # three additions are one too many, whatever is removed beside them (removals are not credited)
    with pytest.raises(ValueError, match=f"a candidate of {cap + 1} edges .* is above the what-if edge cap {cap}"):
        pred.what_if(data, add[:, :3], attr[:3], [0, 3], drop=torch.tensor([1, 2], device=cuda_device), drop_ptr=[0, 2])
    pred.check_status()
    # the largest graph plus the most additions is above the cap, no candidate's own sum is: the call goes through
    two = q.Batch.from_data_list([_big_graph(n, cap - 2, D, 5), _big_graph(9, 20, D, 8)]).to(cuda_device)
    add5 = torch.cat([add[:, :2], n + torch.randint(0, 9, (2, 5), generator=gen).to(cuda_device)], 1)
    attr5 = torch.cat([attr[:2], torch.rand(5, D, generator=gen).to(cuda_device)])
    a = (two, add5, attr5, [0, 2, 7])
    g = torch.tensor([0, 1], device=cuda_device)
    out = pred.what_if(*a, graph=g)
    pred.check_status()
    assert torch.equal(out, pred(infer.materialise_what_if(*a, graph=g)))


@pytest.mark.parametrize("kind", ["added endpoint in another graph", "added endpoint negative", "graph number too large",
                                  "graph number negative", "drop position in another graph", "drop position negative"])
def test_a_flagged_candidate_is_nan_alone(cuda_device, kind):
    H, D = 32, 3
    hip, pred, w, _, _ = _setup(H, D, cuda_device)
    ks = [1, 18, 4, 19]
    good = WC.pick(w, ks)
    want = _call(pred, good, cuda_device)
    pred.check_status()
    # the bad candidate goes in at position 2: one added edge and one removal, aimed at graph A (7 nodes, 12 edges)
    e0 = (torch.tensor([[2], [5]]), torch.rand(1, D), torch.tensor([3]), 0)
    src_dst, attr, drop, g = e0
    bit = 2
    if kind == "added endpoint in another graph":
        src_dst, bit = torch.tensor([[2], [WC.A_N]]), 1                     # node 7 is graph B's first
    elif kind == "added endpoint negative":
        src_dst, bit = torch.tensor([[-1], [2]]), 1
    elif kind == "graph number too large":
        g = 2
    elif kind == "graph number negative":
        g = -1
    elif kind == "drop position in another graph":
        drop = torch.tensor([len(WC.A_EDGES)])                              # position 12 is graph B's first
    elif kind == "drop position negative":
        drop = torch.tensor([-1])
    ap, dp = good.add_ptr, good.drop_ptr
    bad = WC.WhatIf(good.data,
                    torch.cat([good.add_edge_index[:, :ap[2]], src_dst, good.add_edge_index[:, ap[2]:]], 1),
                    torch.cat([good.add_edge_attr[:ap[2]], attr, good.add_edge_attr[ap[2]:]]),
                    ap[:3] + [v + 1 for v in ap[2:]],
                    torch.cat([good.drop[:dp[2]], drop, good.drop[dp[2]:]]),
                    dp[:3] + [v + 1 for v in dp[2:]],
                    torch.cat([good.graph[:2], torch.tensor([g]), good.graph[2:]]), None, None)
    out = _call(pred, bad, cuda_device)
    assert tuple(out.shape) == (5, 3) and bool(torch.isnan(out[2]).all())
    assert torch.equal(out[[0, 1, 3, 4]], want)
    with pytest.raises(_lib.QotError, match=r"flagged the batch \(status %d\)" % bit):
        pred.check_status()
    pred.check_status()                                                     # raised once, clean afterwards


def test_what_if_follows_an_in_place_parameter_update(cuda_device):
    H, D = 16, 4
    _, hip = WC.models(cuda_device, H, D, seed=1)                           # (a model of its own: it is changed here)
    pred = q.TopologicalPredictor(hip)
    w = WC.build(D)
    a, kw = WC.args(w, cuda_device)
    mat = infer.materialise_what_if(*a, **kw)
    before = pred.what_if(*a, **kw)
    assert torch.equal(before, pred(mat))
    with torch.no_grad():
        hip.conv1.lin_value.weight.mul_(1.5)
        hip.conv2.bias.add_(0.25)
        hip.mlp[3].weight.mul_(0.5)
    after = pred.what_if(*a, **kw)
    assert not torch.equal(after, before)
    assert torch.equal(after, pred(mat))
    with torch.no_grad():
        e = rel_err(after, hip(mat))
    print(f"after the update: what_if vs model.eval()(materialised) {e:.3e}")
    assert e <= TOL, e
    pred.check_status()
