"""GPU: ``LightpathPredictor.sensitivity`` (``qot_lightpath_infer_grad``) -- the eval-mode LUT rows, their
Jacobian wrt the node features of each row's one-hop in-neighbourhood and conv1's attention weights in one launch --
against ``oracle.sparse``'s LightpathGNN on the CPU by plain autograd in fp64 (``lightpath_grad_cases.py``; its soundness
is asserted in ``test_infer_lightpath_grad_cpu.py``) and against the engine's own ``x.grad``, both at ``TOL``; against
``predict(data)`` / ``predict.per_graph(data)`` bit for bit."""
import copy

import pytest
import torch

import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import _lib
import lightpath_grad_cases as C
from helpers import TOL, rel_err

pytestmark = pytest.mark.gpu


def _same(x, y):
    """``torch.equal`` with NaN equal to NaN."""
    if x.is_floating_point():
        x, y = x.nan_to_num(nan=7.0, posinf=8.0, neginf=9.0), y.nan_to_num(nan=7.0, posinf=8.0, neginf=9.0)
    return torch.equal(x, y)


def _plain(*tensors, device):
    for t in tensors:
        assert t.grad_fn is None and not t.requires_grad and t.device == device


def _engine_xgrad(hip, db, O):
    """``(out, lut_batch, grad [O, N, F])`` of the engine's eval forward with ``x.requires_grad_()``, one backward each."""
    leaf = copy.copy(db)
    leaf.x = db.x.detach().clone().requires_grad_()
    out, lb = hip(leaf)
    grads = []
    for o in range(O):
        leaf.x.grad = None
        out[:, o].sum().backward(retain_graph=True)
        grads.append(leaf.x.grad.detach().clone())
    return out.detach(), lb, torch.stack(grads)


def _parity(device, Cw, F, O, lut):
    ref, batch, out64, grad64 = C.parity_case(Cw, F, O, lut)
    hip = C.engine_model(ref, device)
    pred = q.LightpathPredictor(hip)
    db = batch.to(device)
    out, lb, js, je = pred.sensitivity(db)
    pred.check_status()
    _plain(out, lb, js, je, device=device)
    rows = C.lut_rows(batch, lut)
    N, E, L = batch.x.shape[0], batch.edge_index.shape[1], rows.numel()
    assert tuple(out.shape) == (L, O) and tuple(js.shape) == (O, L, F) and tuple(je.shape) == (O, E, F)
    want_out, want_lb = pred(db)
    assert torch.equal(out, want_out) and torch.equal(lb, want_lb) and torch.equal(lb.cpu(), batch.batch[rows])
    assert rel_err(out, out64) <= TOL
    assert torch.isfinite(out).all() and torch.isfinite(js).all() and torch.isfinite(je).all()
    J = C.assemble(js, je, batch.edge_index, rows, N)
    own_out, own_lb, own = _engine_xgrad(hip, batch.to(device), O)
    assert torch.equal(own_lb, lb)
    for k in range(O):
        e_or, e_en = rel_err(J[k], grad64[k]), rel_err(J[k], own[k])
        print(f"C {Cw} F {F} O {O} lut {lut} output {k}: vs oracle {e_or:.3e}, vs engine {e_en:.3e}")
        assert e_or <= TOL, (k, e_or)
        assert e_en <= TOL, (k, e_en)
    msg = C.message_mask(batch, rows)
    assert int(msg.sum()) > 0 and bool((je.cpu()[:, ~msg] == 0).all())
    return ref, batch, hip, pred, (out, lb, js, je), grad64


# ------------------------------------------------------------------ 1. parity over widths and shapes
@pytest.mark.parametrize("O", C.OUTPUTS)
@pytest.mark.parametrize("F", C.FEATURES)
@pytest.mark.parametrize("Cw", C.WIDTHS)
def test_parity_mixed_batch(cuda_device, Cw, F, O):
    for lut in C.lut_columns(F):
        _parity(cuda_device, Cw, F, O, lut)


# ------------------------------------------------------------------ 1b. the ends of the widths, the chunk boundary
@pytest.mark.parametrize("F,Cw,O", C.EDGE_SHAPES)
def test_chunk_boundaries_and_a_lone_self_loop_at_the_ends_of_the_widths(cuda_device, F, Cw, O):
    """In-degree 65, in-degree 129 and a LUT node with only its self loop, at ``(F, C, O) = (1, 1, 1)`` (lanes 0 - 3 own an
    ``(h, f)`` pair) and ``(16, 256, 8)`` (all 64 do): ``predict``, ``per_graph`` and ``sensitivity`` in both modes against
    the fp64 oracle, each graph on its own slice; the three calls' ``out`` bit for bit."""
    ref, batch, out64, grad64 = C.edge_case(F, Cw, O)
    pred = q.LightpathPredictor(C.engine_model(ref, cuda_device))
    db = batch.to(cuda_device)
    rows, N = C.lut_rows(batch, 0), batch.x.shape[0]
    out, lb = pred(db)
    per, count = pred.per_graph(db)
    assert lb.tolist() == [0, 1, 2] and count.tolist() == [1, 1, 1]
    assert torch.equal(per, out)
    for g in range(3):
        e = rel_err(out[g], out64[g])
        print(f"F {F} C {Cw} O {O} graph {g}: out vs oracle {e:.3e}")
        assert e <= TOL, (g, e)
    for per_graph in (False, True):
        s_out, second, js, je, (a_self, a_edge) = pred.sensitivity(db, per_graph=per_graph, return_attention_weights=True)
        assert torch.equal(s_out, out) and torch.equal(second, count if per_graph else lb)
        assert tuple(js.shape) == (O, 3, F) and tuple(je.shape) == (O, batch.edge_index.shape[1], F)
        J = C.assemble(js, je, batch.edge_index, rows, N)
        for g, (n0, n1) in enumerate(C.slices(batch.ptr)):
            for k in range(O):
                e = rel_err(J[k, n0:n1], grad64[k, n0:n1])
                print(f"F {F} C {Cw} O {O} per_graph {per_graph} graph {g} output {k}: vs oracle {e:.3e}")
                assert e <= TOL, (per_graph, g, k, e)
        total = a_self.double().cpu()
        total.index_add_(0, batch.batch[batch.edge_index[1]], a_edge.double().cpu())     # (non-messages hold 0)
        assert float((total - 1.0).abs().max()) <= 1e-5
    pred.check_status()


# ------------------------------------------------------------------ 2. edge level
def test_repeated_edges_get_their_own_share_and_an_input_self_loop_none(cuda_device):
    ref, batch, hip, pred, (out, lb, js, je), grad64 = _parity(cuda_device, 32, 5, 3, 1)
    nodes, edges = C.slices(batch.ptr), C.slices(batch.edge_ptr)
    e0 = edges[C.TRIPLE][0]
    got = je.cpu()[:, [e0 + k for k in C.TRIPLE_EDGES]]
    want = grad64[:, [nodes[15][0] + k for k in C.UNROLLED_NODES]]
    e = rel_err(got, want)
    print(f"triple edge vs the unrolled graph's node gradients {e:.3e}")
    assert e <= TOL and float(want.abs().max()) > 0
    assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])      # (the same features: the same share)
    loop = edges[C.SELF_LOOP][0] + 1
    assert batch.edge_index[0, loop] == batch.edge_index[1, loop]
    assert bool((je[:, loop] == 0).all())


# ------------------------------------------------------------------ 3. outputs selection
def test_outputs_selection(cuda_device):
    ref, batch, _, _ = C.parity_case(32, 5, 3, 1)
    pred = q.LightpathPredictor(C.engine_model(ref, cuda_device))
    db = batch.to(cuda_device)
    out, lb, js, je = pred.sensitivity(db)
    out2, lb2, js2, je2 = pred.sensitivity(db, outputs=[2, 0])
    assert tuple(js2.shape) == (2,) + tuple(js.shape[1:]) and tuple(je2.shape) == (2,) + tuple(je.shape[1:])
    assert torch.equal(out2, out) and torch.equal(lb2, lb)
    assert torch.equal(js2, js[[2, 0]]) and torch.equal(je2, je[[2, 0]])
    out1, _, js1, je1 = pred.sensitivity(db, outputs=(1,))
    assert torch.equal(out1, out) and torch.equal(js1, js[[1]]) and torch.equal(je1, je[[1]])
    with pytest.raises(ValueError, match="outputs must be"):
        pred.sensitivity(db, outputs=[3])
    pred.check_status()


# ------------------------------------------------------------------ 4. bitwise independence
def test_slices_do_not_depend_on_the_batch_the_mode_or_the_call(cuda_device):
    ref = C.oracle_model()
    pred = q.LightpathPredictor(C.engine_model(ref, cuda_device))
    g, others = C.independence_graphs()
    ne = g.edge_index.shape[1]
    res = {}
    for name, graphs in (("alone", [g]), ("first", [g] + others), ("last", others + [g])):
        res[name] = pred.sensitivity(q.Batch.from_data_list(graphs).to(cuda_device), return_attention_weights=True)
    a, f, l = res["alone"], res["first"], res["last"]
    assert a[0].shape[0] == 1 and f[0].shape[0] == l[0].shape[0] == 8
    assert torch.equal(a[0][0], f[0][0]) and torch.equal(a[0][0], l[0][7])
    assert torch.equal(a[2][:, 0], f[2][:, 0]) and torch.equal(a[2][:, 0], l[2][:, 7])
    assert torch.equal(a[3], f[3][:, :ne]) and torch.equal(a[3], l[3][:, -ne:])
    assert torch.equal(f[3][:, ne:], l[3][:, :-ne]) and torch.equal(f[2][:, 1:], l[2][:, :7])
    assert torch.equal(a[4][0][0], l[4][0][7]) and torch.equal(a[4][1], l[4][1][-ne:]) and torch.equal(a[4][1], f[4][1][:ne])
    # two calls
    last_b = q.Batch.from_data_list(others + [g]).to(cuda_device)
    again = pred.sensitivity(last_b, return_attention_weights=True)
    for x, y in zip(l[:4] + l[4], again[:4] + again[4]):
        assert torch.equal(x, y)
    # rows mode against per_graph: the second LUT node of the two-LUT graph (row 6) has no row there, its edges hold 0
    per = pred.sensitivity(last_b, per_graph=True, return_attention_weights=True)
    keep = [0, 1, 2, 3, 4, 5, 7]
    assert per[1].tolist() == [1, 1, 1, 1, 1, 2, 1] and l[1].tolist() == [0, 1, 2, 3, 4, 5, 5, 6]
    assert torch.equal(per[0], l[0][keep]) and torch.equal(per[2], l[2][:, keep]) and torch.equal(per[4][0], l[4][0][keep])
    cpu = q.Batch.from_data_list(others + [g])
    second = int(C.lut_rows(cpu, 1)[6])
    into_second = (cpu.edge_index[1] == second).to(cuda_device)
    assert int(into_second.sum()) == 2 and bool((l[3][:, into_second] != 0).any())
    assert torch.equal(per[3][:, ~into_second], l[3][:, ~into_second]) and bool((per[3][:, into_second] == 0).all())
    assert torch.equal(per[4][1][~into_second], l[4][1][~into_second]) and bool((per[4][1][into_second] == 0).all())
    pred.check_status()
    J = C.assemble(l[2], l[3], cpu.edge_index, C.lut_rows(cpu, 1), cpu.x.shape[0])
    assert rel_err(J, C.oracle_xgrad(ref, cpu)[1]) <= TOL


# ------------------------------------------------------------------ 5. attention weights
def test_attention_weights(cuda_device):
    ref, batch, _, _ = C.parity_case(32, 5, 3, 1)
    hip = C.engine_model(ref, cuda_device)
    pred = q.LightpathPredictor(hip)
    db = batch.to(cuda_device)
    out, lb, js, je, (a_self, a_edge) = pred.sensitivity(db, return_attention_weights=True)
    plain = pred.sensitivity(db)
    assert torch.equal(out, plain[0]) and torch.equal(js, plain[2]) and torch.equal(je, plain[3])
    _plain(a_self, a_edge, device=cuda_device)
    rows = C.lut_rows(batch, 1)
    E, L = batch.edge_index.shape[1], rows.numel()
    assert tuple(a_self.shape) == (L, 4) and tuple(a_edge.shape) == (E, 4)
    with torch.no_grad():
        _, _, attn = hip(db, return_attention_weights=True)
    (ei_loops, alpha), = attn
    own = {}
    for (s, d), row in zip(ei_loops.t().tolist(), alpha.double().cpu()):
        own.setdefault((s, d), row)                          # (repeated edges carry the same features: the same weights)
    a_self, a_edge = a_self.double().cpu(), a_edge.double().cpu()
    msg = C.message_mask(batch, rows)
    assert bool((a_edge[~msg] == 0).all())
    want_edge = torch.stack([own[(s, d)] for s, d in batch.edge_index[:, msg].t().tolist()])
    want_self = torch.stack([own[(i, i)] for i in rows.tolist()])
    e_edge, e_self = rel_err(a_edge[msg], want_edge), rel_err(a_self, want_self)
    print(f"alpha_edge vs engine {e_edge:.3e}, alpha_self vs engine {e_self:.3e}")
    assert e_edge <= TOL and e_self <= TOL
    total = a_self.clone()
    row_of = {i: r for r, i in enumerate(rows.tolist())}
    idx = torch.tensor([row_of[d] for d in batch.edge_index[1, msg].tolist()])
    total.index_add_(0, idx, a_edge[msg])
    assert float((total - 1.0).abs().max()) <= 1e-5
    pred.check_status()


# ------------------------------------------------------------------ 6. per_graph, and its capture
def test_per_graph_and_graph_capture(cuda_device):
    ref, batch, _, _ = C.parity_case(32, 5, 3, 1)
    pred = q.LightpathPredictor(C.engine_model(ref, cuda_device))
    db = batch.to(cuda_device)
    out, count, js, je = pred.sensitivity(db, per_graph=True)
    pred.check_status()
    want_out, want_count = pred.per_graph(db)
    B = batch.num_graphs
    assert count.dtype == torch.int32 and torch.equal(count, want_count) and tuple(js.shape) == (3, B, 5)
    assert _same(out, want_out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = pred.sensitivity(db, per_graph=True)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(cap, (out, count, js, je)):
        assert _same(x, y)
    # replayed on other data of the same shape: other LUT nodes, several in some graphs, none in others
    other = C.relabelled()
    db.x.copy_(other.x)
    graph.replay()
    torch.cuda.synchronize()
    fresh = pred.sensitivity(other.to(cuda_device), per_graph=True)
    pred.check_status()
    for x, y in zip(cap, fresh):
        assert _same(x, y)
    out, count, js, je = (t.cpu() for t in cap)
    none = (count == 0).nonzero().squeeze(1).tolist()
    assert none and int(count.max()) > 1
    edges = C.slices(other.edge_ptr)
    for g in range(B):
        e0, e1 = edges[g]
        if g in none:
            assert torch.isnan(out[g]).all() and torch.isnan(js[:, g]).all() and bool((je[:, e0:e1] == 0).all())
        else:
            assert torch.isfinite(out[g]).all() and torch.isfinite(js[:, g]).all() and torch.isfinite(je[:, e0:e1]).all()
    # ... and right: on the batch that keeps the flag of every graph's first LUT node only, against the oracle
    only, first, has = C.first_lut_only(other)
    single = pred.sensitivity(only.to(cuda_device), per_graph=True)
    pred.check_status()
    assert single[1].tolist() == [1 if g in has else 0 for g in range(B)]
    J = C.assemble(single[2][:, has], single[3], only.edge_index, first, only.x.shape[0])
    assert rel_err(J, C.oracle_xgrad(ref, only)[1]) <= TOL


# ------------------------------------------------------------------ 7. purity and parameter following
def test_parameters_are_followed_and_nothing_is_touched(cuda_device):
    batch, (before, after), deltas = C.tracking_case()
    hip = C.engine_model(before, cuda_device)                 # C = 20: a width the engine runs zero-padded
    hip.train()
    pred = q.LightpathPredictor(hip)
    db = batch.to(cuda_device)
    rows = C.lut_rows(batch, 1)
    state = {k: v.clone() for k, v in hip.state_dict().items()}
    old = pred.sensitivity(db, return_attention_weights=True)
    pred.sensitivity(db, per_graph=True)
    assert hip.training
    for k, v in hip.state_dict().items():
        assert torch.equal(v, state[k]), k
    J0 = C.assemble(old[2], old[3], batch.edge_index, rows, batch.x.shape[0])
    assert rel_err(J0, C.oracle_xgrad(before, batch)[1]) <= TOL
    with torch.no_grad():
        for name, p in hip.named_parameters():
            p.add_(deltas[name].to(cuda_device))               # in place: the next call reads the new values
    new = pred.sensitivity(db)
    out64, grad64 = C.oracle_xgrad(after, batch)
    J1 = C.assemble(new[2], new[3], batch.edge_index, rows, batch.x.shape[0])
    assert rel_err(new[0], out64) <= TOL and rel_err(J1, grad64) <= TOL
    assert rel_err(J1, J0) > TOL
    pred.check_status()


# ------------------------------------------------------------------ 8. status
def test_edge_outside_its_graph_is_flagged_and_its_slices_nan(cuda_device):
    from test_gpu_infer_lightpath import _chains
    pred = q.LightpathPredictor(C.engine_model(C.oracle_model(), cuda_device))
    graphs = _chains(3, 5, 1, first=3)
    clean = q.Batch.from_data_list(graphs)
    want = pred.sensitivity(clean.to(cuda_device), return_attention_weights=True)
    pred.check_status()
    bad = q.Batch.from_data_list(graphs)
    lo, hi = int(bad.edge_ptr[1]), int(bad.edge_ptr[2])
    into_lut = [e for e in range(lo, hi) if int(bad.edge_index[1, e]) == int(bad.ptr[1])]
    assert into_lut
    bad.edge_index[0, into_lut[0]] = int(bad.ptr[1]) - 1      # a node of graph 0: inside [0, N), outside graph 1
    inside = torch.zeros(bad.edge_index.shape[1], dtype=torch.bool)
    inside[lo:hi] = True
    for per_graph in (False, True):
        got = pred.sensitivity(bad.to(cuda_device), per_graph=per_graph, return_attention_weights=True)
        with pytest.raises(_lib.QotError, match="status 1"):
            pred.check_status()
        pred.check_status()                                   # (read and cleared)
        out, second, js, je = (t.cpu() for t in got[:4])
        a_self, a_edge = (t.cpu() for t in got[4])
        assert second.tolist() == ([1, 1, 1] if per_graph else [0, 1, 2])
        assert torch.isnan(out[1]).all() and torch.isnan(js[:, 1]).all() and torch.isnan(a_self[1]).all()
        assert torch.isnan(je[:, inside]).all() and torch.isnan(a_edge[inside]).all()
        for k in (0, 2):
            assert torch.equal(out[k], want[0][k].cpu()) and torch.equal(js[:, k], want[2][:, k].cpu())
            assert torch.equal(a_self[k], want[4][0][k].cpu())
        assert torch.equal(je[:, ~inside], want[3].cpu()[:, ~inside])
        assert torch.equal(a_edge[~inside], want[4][1].cpu()[~inside])


# ------------------------------------------------------------------ 9. a width the engine runs zero-padded
def test_zero_padded_width(cuda_device):
    ref, batch, hip, pred, _, _ = _parity(cuda_device, 20, 5, 3, 1)
    assert hip._qot_cp is not None and hip._qot_cp != 20      # the engine pads; the kernel reads the real parameters


# ------------------------------------------------------------------ LUT-less batches behave as __call__
def test_lut_less_batches(cuda_device):
    from gnn_qot_estimation_amd import synthetic as S
    hip = C.engine_model(C.oracle_model(), cuda_device)
    pred = q.LightpathPredictor(hip)
    db = S.lightpath_batch(4, lut=False).to(cuda_device)
    with pytest.raises(ValueError, match="No LUT node found in the batch.") as err:
        pred.sensitivity(db)
    assert not isinstance(err.value, q.infer.EnvelopeError)
    hip.allow_empty_lut = True
    out, lb, js, je, (a_self, a_edge) = pred.sensitivity(db, return_attention_weights=True)
    E = db.edge_index.shape[1]
    assert tuple(out.shape) == (0, 3) and tuple(lb.shape) == (0,) and tuple(js.shape) == (3, 0, 5)
    assert tuple(je.shape) == (3, E, 5) and bool((je == 0).all()) and tuple(a_self.shape) == (0, 4)
    assert tuple(a_edge.shape) == (E, 4) and bool((a_edge == 0).all())
    out, count, js, je = pred.sensitivity(db, per_graph=True)
    assert count.tolist() == [0] * 4 and torch.isnan(out).all() and torch.isnan(js).all() and bool((je == 0).all())
    pred.check_status()
