"""GPU: ``TopologicalPredictor.sensitivity`` (``qot_topological_infer_grad``) -- the eval-mode output, its
Jacobian wrt the edge features and conv1's attention weights in one launch -- against the fp64 oracle's plain autograd (one
backward per output), against the engine's own ``edge_attr.grad`` in eval mode with frozen parameters, and against a
central difference.  Inputs and references come from ``infer_grad_cases.py``; tests/test_infer_grad_cpu.py asserts that the
oracle's own fp32 and fp64 Jacobians agree to ``TOL / 10`` on every one of them."""
import pytest
import torch

import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import _lib, infer
import infer_grad_cases as C
from helpers import TOL, rel_err

pytestmark = pytest.mark.gpu


def _engine(hip, batch, device, outputs=None):
    """``(jac [Q, E, D], alpha [E, 1])`` of the engine: eval forward through autograd, one backward per output."""
    eb = batch.to(device)
    eb.edge_attr = eb.edge_attr.detach().clone().requires_grad_()
    out, (_, alpha) = hip(eb, return_attention_weights=True)
    sel = range(out.shape[1]) if outputs is None else outputs
    jac = []
    for o in sel:
        eb.edge_attr.grad = None
        out[:, o].sum().backward(retain_graph=True)
        g = eb.edge_attr.grad
        jac.append(torch.zeros_like(eb.edge_attr) if g is None else g.detach().clone())
    return torch.stack(jac), alpha.detach()


def _check(pred, hip, batch, device, out64, jac64, alpha64, engine=True, label=""):
    """Parity of one batch, per graph; returns ``(out, jac, alpha)``."""
    db = batch.to(device)
    out, jac, (ei, alpha) = pred.sensitivity(db, return_attention_weights=True)
    E, D = batch.edge_attr.shape
    assert tuple(jac.shape) == (jac64.shape[0], E, D) and tuple(alpha.shape) == (E, 1) and tuple(out.shape) == tuple(out64.shape)
    for t in (out, jac, alpha):
        assert t.grad_fn is None and not t.requires_grad and t.device == device and t.dtype == torch.float32
    assert torch.equal(ei.cpu(), batch.edge_index)
    assert torch.equal(out, pred(db)), "out is not the eval kernel's row bit for bit"
    assert rel_err(out, out64) <= TOL
    if engine:
        jac_en, alpha_en = _engine(hip, batch, device)
    worst = [0.0, 0.0, 0.0, 0.0]
    for g, (e0, e1) in enumerate(C.edge_slices(batch)):
        if e1 == e0:
            continue
        errs = [max(rel_err(jac[k, e0:e1], jac64[k, e0:e1]) for k in range(jac.shape[0])),
                rel_err(alpha[e0:e1], alpha64[e0:e1])]
        if engine:
            errs += [max(rel_err(jac[k, e0:e1], jac_en[k, e0:e1]) for k in range(jac.shape[0])),
                     rel_err(alpha[e0:e1], alpha_en[e0:e1])]
        print(f"{label} graph {g} ({e1 - e0} edges): jac vs oracle {errs[0]:.3e}, alpha vs oracle {errs[1]:.3e}"
              + (f", jac vs engine {errs[2]:.3e}, alpha vs engine {errs[3]:.3e}" if engine else ""))
        worst = [max(a, b) for a, b in zip(worst, errs + [0.0, 0.0])]
    assert max(worst) <= TOL, worst
    pred.check_status()
    return out, jac, alpha


# ------------------------------------------------------------------ 1. parity over widths and shapes
@pytest.mark.parametrize("H,D,O", C.PARITY)
def test_parity_mixed_batch(cuda_device, H, D, O):
    ref, batch, cap, out64, jac64, alpha64 = C.parity_case(H, D, O)
    assert batch.graph_sizes == (128, cap)
    hip = C.engine_model(ref, cuda_device)
    _check(q.TopologicalPredictor(hip), hip, batch, cuda_device, out64, jac64, alpha64, label=f"H {H} D {D} O {O}")


# ------------------------------------------------------------------ 2. degenerate graphs
@pytest.mark.parametrize("H", C.DEGENERATE_WIDTHS)
def test_degenerate_graphs(cuda_device, H):
    ref, graphs, batch, out64, jac64, alpha64 = C.degenerate_case(H)
    hip = C.engine_model(ref, cuda_device)
    pred = q.TopologicalPredictor(hip)
    out, jac, alpha = _check(pred, hip, batch, cuda_device, out64, jac64, alpha64, label=f"H {H}")
    assert torch.isfinite(out).all() and torch.isfinite(jac).all() and torch.isfinite(alpha).all()
    for g, (e0, e1) in zip(graphs, C.edge_slices(batch)):            # each of them alone (an edge-less BATCH among them)
        b = q.Batch.from_data_list([g])
        o1, j1, a1 = _check(pred, hip, b, cuda_device, *C.oracle_jacobian(ref, b), C.oracle_alpha(ref, b), engine=False)
        assert tuple(j1.shape) == (3, e1 - e0, 4) and torch.isfinite(j1).all() and torch.isfinite(o1).all()
        assert torch.equal(j1, jac[:, e0:e1]) and torch.equal(a1, alpha[e0:e1])
    empty = pred.sensitivity(q.Batch.from_data_list([graphs[0], graphs[4]]).to(cuda_device), outputs=[1, 0])[1]
    assert tuple(empty.shape) == (2, 0, 4)


# ------------------------------------------------------------------ 3. the outputs selection
def test_outputs_selection(cuda_device):
    ref = C.oracle_model(40, 32)
    pred = q.TopologicalPredictor(C.engine_model(ref, cuda_device))
    b = q.Batch.from_data_list([C.graph(40, 160, 4, 10), C.graph(7, 12, 4, 11), C.graph(33, 90, 4, 12)]).to(cuda_device)
    out, full = pred.sensitivity(b)
    out2, sel = pred.sensitivity(b, outputs=[2, 0])
    assert tuple(sel.shape) == (2,) + tuple(full.shape[1:])
    assert torch.equal(sel, full[[2, 0]]) and torch.equal(out, out2)
    assert torch.equal(pred.sensitivity(b, outputs=(1,))[1], full[[1]])
    for bad in ([], [3], [-1], [0, 0], [True], "0"):
        with pytest.raises(ValueError, match="outputs must be"):
            pred.sensitivity(b, outputs=bad)
    pred.check_status()


# ------------------------------------------------------------------ 4. batch independence and reproducibility
@pytest.mark.parametrize("H", [16, 64])
def test_slices_do_not_depend_on_the_batch(cuda_device, H):
    ref = C.oracle_model(40, H)
    pred = q.TopologicalPredictor(C.engine_model(ref, cuda_device))
    sizes = [(40, 160), (7, 12), (33, 90), (12, 30), (25, 80), (2, 2), (18, 50)]
    graphs = [C.graph(n, e, 4, 10 + k) for k, (n, e) in enumerate(sizes)]
    g, m = graphs[0], graphs[0].edge_index.shape[1]

    def run(gs):
        out, jac, (_, alpha) = pred.sensitivity(q.Batch.from_data_list(gs).to(cuda_device), return_attention_weights=True)
        return out, jac, alpha
    alone, first, last = run([g]), run([g] + graphs[1:]), run(graphs[1:] + [g])
    assert torch.equal(alone[1], first[1][:, :m]) and torch.equal(alone[1], last[1][:, -m:])
    assert torch.equal(alone[2], first[2][:m]) and torch.equal(alone[2], last[2][-m:])
    assert torch.equal(alone[0][0], first[0][0]) and torch.equal(alone[0][0], last[0][-1])
    assert torch.equal(first[1][:, m:], last[1][:, :-m]) and torch.equal(first[2][m:], last[2][:-m])
    again = run(graphs[1:] + [g])
    assert all(torch.equal(a, b) for a, b in zip(last, again))
    pred.check_status()


# ------------------------------------------------------------------ 5. parameter tracking
def test_parameters_are_tracked(cuda_device):
    batch, (first, stepped, loaded), grads = C.tracking_case()
    hip = C.engine_model(first, cuda_device)
    pred = q.TopologicalPredictor(hip)
    db = batch.to(cuda_device)

    def jac_now(ref):
        jac = pred.sensitivity(db)[1].clone()
        e_en, e_or = rel_err(jac, _engine(hip, batch, cuda_device)[0]), rel_err(jac, C.oracle_jacobian(ref, batch)[1])
        print(f"jac vs engine {e_en:.3e}, vs oracle {e_or:.3e}")
        assert e_en <= TOL and e_or <= TOL, (e_en, e_or)
        return jac
    old = jac_now(first)
    # one in-place SGD step along the oracle's gradients (the same fp32 arithmetic: the weights stay identical)
    with torch.no_grad():
        for name, p in hip.named_parameters():
            p.sub_((C.TRACK_LR * grads[name]).to(cuda_device))
    after_step = jac_now(stepped)
    assert rel_err(after_step, old) > TOL                 # the step moved the Jacobian by more than the comparison allows
    hip.load_state_dict(loaded.state_dict(), strict=True)
    after_load = jac_now(loaded)
    assert rel_err(after_load, after_step) > TOL
    pred.check_status()


# ------------------------------------------------------------------ 6. central difference (the definition, not the rounding)
def test_central_difference(cuda_device):
    """jac[q, e, d] against (f(x + h) - f(x - h)) / 2h of the fp64 oracle, h = 1e-2, at ``FD_POINTS``: every entry to 1e-3 of
    itself."""
    ref = C.oracle_model(12, 16)
    batch = q.Batch.from_data_list([C.fd_graph()])
    pred = q.TopologicalPredictor(C.engine_model(ref, cuda_device))
    jac = pred.sensitivity(batch.to(cuda_device))[1].double().cpu()
    for (e, d), slope in C.fd_slopes(ref, batch).items():
        for k in range(3):
            err = abs(float(slope[k]) - float(jac[k, e, d])) / abs(float(slope[k]))
            print(f"edge {e} feature {d} output {k}: slope {float(slope[k]):+.6e} jac {float(jac[k, e, d]):+.6e} rel {err:.2e}")
            assert err <= 1e-3, (e, d, k, err)
    pred.check_status()


# ------------------------------------------------------------------ 7. refusals, flags, purity
def test_refusals_name_the_condition(cuda_device):
    hip = C.engine_model(C.oracle_model(130, 16), cuda_device)
    pred = q.TopologicalPredictor(hip)
    cap = infer.grad_edge_cap(100, 16, 4)
    assert cap < infer.edge_cap(100, 16, 4)
    over = q.Batch.from_data_list([C.graph(100, cap + 2 + cap % 2, 4, 2, edges=cap + 1)]).to(cuda_device)
    with pytest.raises(ValueError, match=f"{cap + 1} edges is above the sensitivity edge cap {cap}"):
        pred.sensitivity(over)
    assert torch.isfinite(pred(over)).all()               # (the eval kernel takes it)
    at = q.Batch.from_data_list([C.graph(100, cap + 2 + cap % 2, 4, 2, edges=cap)]).to(cuda_device)
    assert all(torch.isfinite(t).all() for t in pred.sensitivity(at))
    with pytest.raises(ValueError, match="129 nodes"):
        pred.sensitivity(q.Batch.from_data_list([C.graph(10, 20), C.graph(129, 300, 4, 1)]).to(cuda_device))
    withx = q.Batch.from_data_list([C.graph(10, 20)]).to(cuda_device)
    withx.x = torch.rand(10, 16, device=cuda_device)
    with pytest.raises(ValueError, match="data.x is given"):
        pred.sensitivity(withx)
    bad = C.graph(12, 40, 4, 34)
    bad.node_ids = torch.arange(12) + 119                 # 130 >= num_nodes
    with pytest.raises(IndexError):
        pred.sensitivity(q.Batch.from_data_list([C.graph(10, 20), bad]).to(cuda_device))
    pred.check_status()
    # a model outside the envelope: the constructor's errors, and __call__'s when the model is altered afterwards
    with pytest.raises(ValueError, match="zero-padded"):
        q.TopologicalPredictor(q.TopologicalGNN(14, 20, 3, 4).to(cuda_device)).sensitivity(withx)
    ok = q.Batch.from_data_list([C.graph(10, 20)]).to(cuda_device)
    for other, what in ((q.TopologicalGNN(14, 16, 3, 4, num_layers=3), "num_layers"),
                        (q.TopologicalGNN(14, 16, 3, 5), "edge_dim 5"), (q.TopologicalGNN(14, 16, 9, 4), "out_channels 9")):
        altered = q.TopologicalPredictor(hip)
        altered.model = other.to(cuda_device)
        with pytest.raises(ValueError, match=what) as by_call:
            altered(ok)
        with pytest.raises(ValueError, match=what) as by_sens:
            altered.sensitivity(ok)
        assert str(by_call.value) == str(by_sens.value)
    hip.cpu()
    with pytest.raises(ValueError, match="CPU"):
        pred.sensitivity(withx)


def test_edge_outside_its_graph_is_flagged_and_its_slices_nan(cuda_device):
    pred = q.TopologicalPredictor(C.engine_model(C.oracle_model(16, 16), cuda_device))
    graphs = [C.graph(7, 12, 4, 1), C.graph(9, 20, 4, 2), C.graph(5, 8, 4, 3)]

    def run(b):
        out, jac, (_, alpha) = pred.sensitivity(b.to(cuda_device), return_attention_weights=True)
        return out, jac, alpha
    want = run(q.Batch.from_data_list(graphs))
    pred.check_status()
    bad = q.Batch.from_data_list(graphs)
    (a0, a1), (b0, b1), (c0, c1) = C.edge_slices(bad)
    bad.edge_index[0, b0] = int(bad.ptr[1]) - 1           # a node of graph 0: inside [0, N), outside graph 1
    out, jac, alpha = run(bad)
    with pytest.raises(_lib.QotError, match="status 1"):
        pred.check_status()
    pred.check_status()                                   # (read and cleared)
    assert torch.isnan(out[1]).all() and torch.isnan(jac[:, b0:b1]).all() and torch.isnan(alpha[b0:b1]).all()
    for s0, s1, g in ((a0, a1, 0), (c0, c1, 2)):
        assert torch.equal(out[g], want[0][g]) and torch.equal(jac[:, s0:s1], want[1][:, s0:s1])
        assert torch.equal(alpha[s0:s1], want[2][s0:s1])


def test_the_call_is_pure(cuda_device):
    hip = C.engine_model(C.oracle_model(30, 32), cuda_device)
    pred = q.TopologicalPredictor(hip)
    db = q.Batch.from_data_list([C.graph(30, 100, 4, 20), C.graph(12, 30, 4, 21)]).to(cuda_device)
    for mode in (False, True):
        hip.train(mode)
        before = pred(db).clone()
        versions = {k: p._version for k, p in hip.named_parameters()}
        state = {k: v.detach().clone() for k, v in hip.state_dict().items()}
        step = int(hip._qot_step)
        pred.sensitivity(db, return_attention_weights=True)
        pred.sensitivity(db, outputs=[1])
        assert hip.training is mode and int(hip._qot_step) == step
        assert {k: p._version for k, p in hip.named_parameters()} == versions
        for k, v in hip.state_dict().items():
            assert torch.equal(v, state[k]), k
        assert torch.equal(pred(db), before)
    pred.check_status()
