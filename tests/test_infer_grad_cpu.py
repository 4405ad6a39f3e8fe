"""CPU-side checks of the sensitivity path (``csrc/infer_grad.hip``, ``TopologicalPredictor.sensitivity``): the entry
points are declared, bound and exported; the envelope answers from the kernel's LDS layout; the entry point refuses before
any launch; the ``outputs`` argument check; and the soundness of the fixtures the GPU tests lean on -- the oracle's
Jacobian in fp32 and in fp64 must agree per graph to ``TOL / 10`` on every batch of ``infer_grad_cases.py`` (a gradient
jumps at a leaky_relu / relu kink: inputs on which the reference's own two precisions disagree cannot judge a kernel)."""
import ctypes
import os
import re

import pytest
import torch

import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import _lib, infer
import infer_grad_cases as C
from helpers import INFER_COMMON_REFUSALS, TOL, infer_common_args, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qot_topological_infer_grad", "qot_topological_infer_grad_supported", "qot_topological_infer_grad_max_edges")


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    declared = set(re.findall(r"\b(qot_[a-z0-9_]+)\s*\(", hdr))
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(_lib.SIGNATURES[name][1]) == decl.count(",") + 1, name
    # everything qot_topological_infer takes, then outputs, Q, jac, alpha; the stream comes last
    ev, gr = _lib.SIGNATURES["qot_topological_infer"][1], _lib.SIGNATURES["qot_topological_infer_grad"][1]
    assert gr[:len(ev) - 1] == ev[:-1] and gr[-1] is ctypes.c_void_p
    assert gr[len(ev) - 1:-1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(q.TopologicalPredictor, "sensitivity")
    assert _lib.SIGNATURES["qot_topological_infer_grad_supported"][1] == [ctypes.c_int] * 5
    assert _lib.SIGNATURES["qot_topological_infer_grad_max_edges"][1] == [ctypes.c_int] * 3


@pytest.mark.parametrize("n,H,D", [(75, 16, 4), (100, 64, 4), (128, 64, 4), (128, 32, 1), (2, 16, 2)])
def test_edge_cap_arithmetic(n, H, D):
    lib = _lib.load()
    cap, eval_cap = lib.qot_topological_infer_grad_max_edges(n, H, D), lib.qot_topological_infer_max_edges(n, H, D)
    assert cap == infer.grad_edge_cap(n, H, D) and 0 < cap <= eval_cap
    assert lib.qot_topological_infer_grad_supported(n, cap, H, D, 3) == 1
    assert lib.qot_topological_infer_grad_supported(n, cap + 1, H, D, 3) == 0
    assert lib.qot_topological_infer_grad_max_edges(129, H, D) == -1
    assert lib.qot_topological_infer_grad_max_edges(n, 48, D) == -1
    assert lib.qot_topological_infer_grad_supported(n, 10, H, 5, 3) == 0
    assert lib.qot_topological_infer_grad_supported(n, 10, H, D, 9) == 0


def test_edge_cap_floors():
    assert infer.grad_edge_cap(100, 64, 4) >= 400            # the headline shape
    assert infer.grad_edge_cap(75, 16, 4) >= 600             # the reference's own shape
    # -1 exactly where the eval kernel answers -1
    for n, H, D in [(129, 16, 4), (100, 48, 4), (100, 64, 5), (100, 64, 0), (-1, 16, 4)]:
        assert infer.edge_cap(n, H, D) == -1 and infer.grad_edge_cap(n, H, D) == -1, (n, H, D)


def test_entry_point_refuses_before_any_launch():
    fn = _lib.load().qot_topological_infer_grad
    one = ctypes.c_void_p(1)                                 # never dereferenced: every call below is refused first

    def call(Q=1, H=16, max_e=10, slope_conv=0.01, jac=one, outputs=one, O=3):
        return fn(one, one, one, one, one, 10, 10, 1, 10, max_e, one, 4 * H, one, 16, one, 16, one, one, one, one, one, one, one,
                  one, one, slope_conv, 0.01, one, H, 4, O, None, outputs, Q, jac, None, None)
    UNSUPPORTED, BADARG = -1, -2                             # include/qot_gnn.h: QOT_ERR_UNSUPPORTED, QOT_ERR_BADARG
    for kw in (dict(Q=0), dict(Q=4), dict(H=48), dict(max_e=1 << 21), dict(slope_conv=0.0), dict(slope_conv=-0.01),
               dict(Q=2, O=1)):
        assert call(**kw) == UNSUPPORTED, kw
    for kw in (dict(jac=None), dict(outputs=None)):
        assert call(**kw) == BADARG, kw


def _grad_call(Q=1, outputs=1, jac=1, alpha=None, **kw):
    p = ctypes.c_void_p
    return _lib.load().qot_topological_infer_grad(*infer_common_args(**kw), p(outputs), Q, p(jac), p(alpha), None)


@pytest.mark.parametrize("kw,code", INFER_COMMON_REFUSALS + [
    # the entry point's own checks, in its source order: the envelope, Q, slope_conv, outputs / jac
    (dict(Q=0), -1), (dict(Q=4), -1), (dict(Q=2, O=1), -1), (dict(slope_conv=0.0), -1), (dict(slope_conv=float("nan")), -1),
    (dict(outputs=None), -2), (dict(jac=None), -2), (dict(jac=None, E=0, B=0), 0),
    # two at once
    (dict(Q=0, outputs=None), -1), (dict(slope_conv=-1.0, jac=None), -1), (dict(H=48, outputs=None), -1),
    (dict(V=0, Q=0), -2), (dict(outputs=None, B=0), -2), (dict(Q=0, B=0), -1), (dict(slope_conv=0.0, B=0), -1),
    (dict(outputs=None, B=1 << 31), -2), (dict(Q=9, O=9), -1),
])
def test_entry_point_return_codes_before_any_launch(kw, code):
    assert _grad_call(**kw) == code


def test_outputs_argument_check_needs_no_device():
    assert infer.grad_outputs(None, 3) == [0, 1, 2]
    assert infer.grad_outputs([2, 0], 3) == [2, 0]
    assert infer.grad_outputs((1,), 3) == [1]
    for bad in ([], [3], [-1], [0, 0], [True], "0", 0, [0.0], ["0"], (), [0, 1, 2, 0]):
        with pytest.raises(ValueError, match="outputs must be"):
            infer.grad_outputs(bad, 3)


def test_sensitivity_checks_outputs_before_the_model_and_the_batch():
    pred = q.TopologicalPredictor.__new__(q.TopologicalPredictor)
    pred.model, pred._tables, pred._tag, pred._status = q.TopologicalGNN(14, 32, 3, 4), None, None, None
    with pytest.raises(ValueError, match="outputs must be"):
        pred.sensitivity(None, outputs=[3])
    with pytest.raises(ValueError, match="CPU"):
        pred.sensitivity(None)
    assert pred.model.training and int(pred.model._qot_step) == 0
    # a model altered after construction: the named ValueError of __call__, before the argument is looked at
    pred.model = q.TopologicalGNN(14, 16, 3, 4, num_layers=3)
    with pytest.raises(ValueError, match="num_layers"):
        pred.sensitivity(None, outputs=[3])
    pred.model = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="num_layers"):
        pred.sensitivity(None)


def _sound(jac32, jac64, batch):
    worst = 0.0
    for g, (e0, e1) in enumerate(C.edge_slices(batch)):
        if e1 == e0:
            continue
        for k in range(jac64.shape[0]):
            e = rel_err(jac32[k, e0:e1], jac64[k, e0:e1])
            worst = max(worst, e)
            assert e <= TOL / 10, (g, k, e)
    return worst


@pytest.mark.parametrize("H,D,O", C.PARITY)
def test_parity_fixtures_are_sound(H, D, O):
    ref, batch, cap, out64, jac64, alpha64 = C.parity_case(H, D, O)
    assert batch.graph_sizes == (128, cap) and C.edge_slices(batch)[4][1] - C.edge_slices(batch)[4][0] == cap
    assert tuple(jac64.shape) == (O, batch.edge_index.shape[1], D) and tuple(alpha64.shape) == (batch.edge_index.shape[1], 1)
    out32, jac32 = C.oracle_jacobian(ref, batch, dtype=torch.float32)
    assert rel_err(out32, out64) <= TOL / 10
    print(f"H {H} D {D} O {O}: oracle fp32 vs fp64 Jacobian {_sound(jac32, jac64, batch):.3e}")
    assert float(jac64.abs().max()) > 0


@pytest.mark.parametrize("H", C.DEGENERATE_WIDTHS)
def test_degenerate_and_central_difference_fixtures_are_sound(H):
    ref, graphs, batch, out64, jac64, _ = C.degenerate_case(H)
    _, jac32 = C.oracle_jacobian(ref, batch, dtype=torch.float32)
    _sound(jac32, jac64, batch)
    for g in graphs:                                         # each alone: the same slices
        b = q.Batch.from_data_list([g])
        _sound(C.oracle_jacobian(ref, b, dtype=torch.float32)[1], C.oracle_jacobian(ref, b)[1], b)
    ref, b = C.oracle_model(12, 16), q.Batch.from_data_list([C.fd_graph()])
    assert b.edge_index.shape[1] == 30 and b.num_nodes == 12
    jac64 = C.oracle_jacobian(ref, b)[1]
    _sound(C.oracle_jacobian(ref, b, dtype=torch.float32)[1], jac64, b)
    # no kink inside the step at the perturbed points: the oracle's autograd and its own difference quotient agree, entry
    # by entry, to a tenth of the GPU test's bound
    for (e, d), slope in C.fd_slopes(ref, b).items():
        for k in range(3):
            err = abs(float(slope[k]) - float(jac64[k, e, d])) / abs(float(slope[k]))
            assert err <= 1e-4, (e, d, k, err)


def test_tracking_fixtures_are_sound():
    """The batch of the parameter-tracking test at each of its three parameter sets; and the sets differ by more than TOL."""
    batch, refs, grads = C.tracking_case()
    jacs = []
    for ref in refs:
        jac64 = C.oracle_jacobian(ref, batch)[1]
        _sound(C.oracle_jacobian(ref, batch, dtype=torch.float32)[1], jac64, batch)
        jacs.append(jac64)
    assert rel_err(jacs[1], jacs[0]) > TOL and rel_err(jacs[2], jacs[1]) > TOL
    assert set(grads) == set(dict(refs[0].named_parameters()))
