"""CPU-side checks of the single-launch inference path (``csrc/infer.hip``, ``infer.TopologicalPredictor``): the new
entry points are declared, bound and exported; the envelope answer of ``qot_topological_infer_supported``; loud refusals
that need no GPU."""
import ctypes
import os
import re

import pytest
import torch

import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import _lib, harness, infer
from helpers import INFER_COMMON_REFUSALS, infer_common_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qot_topological_infer", "qot_topological_infer_supported", "qot_topological_infer_max_edges")


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    declared = set(re.findall(r"\b(qot_[a-z0-9_]+)\s*\(", hdr))
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the entry point's ctypes row has one type per declared parameter
    decl = re.search(r"int qot_topological_infer\(([^;]*)\);", hdr).group(1)
    assert len(_lib.SIGNATURES["qot_topological_infer"][1]) == decl.count(",") + 1


def test_supported_envelope():
    ok = _lib.load().qot_topological_infer_supported
    assert ok(129, 100, 16, 4, 3) == 0          # nodes
    assert ok(100, 100, 48, 4, 3) == 0          # width
    assert ok(100, 100, 16, 5, 3) == 0          # edge_dim
    assert ok(100, 100, 16, 4, 9) == 0          # outputs
    assert ok(75, 600, 16, 4, 3) == 1           # the reference's scale
    assert ok(100, 400, 64, 4, 3) == 1          # the headline shape
    assert ok(128, 0, 64, 4, 8) == 1 and ok(0, 0, 16, 1, 1) == 1
    assert ok(-1, 0, 16, 4, 3) == 0 and ok(10, -1, 16, 4, 3) == 0


@pytest.mark.parametrize("n,H,D", [(75, 16, 4), (100, 64, 4), (128, 64, 4), (128, 32, 1), (2, 16, 2)])
def test_supported_is_monotone_in_edges_up_to_its_cap(n, H, D):
    lib = _lib.load()
    cap = lib.qot_topological_infer_max_edges(n, H, D)
    assert cap == infer.edge_cap(n, H, D) and cap > 0
    seen_no = False
    edges = sorted(set(list(range(0, cap + 1, max(cap // 97, 1))) + [cap - 1, cap, cap + 1, cap + 2, 2 * cap, 1 << 20,
                                                                     (1 << 20) + 1]))
    answers = [(e, lib.qot_topological_infer_supported(n, e, H, D, 3)) for e in edges]
    for e, a in answers:
        assert a == (1 if e <= cap else 0), (e, a, cap)
        assert not (seen_no and a), e
        seen_no = seen_no or not a
    # more nodes or a wider model never raise the cap; outside the envelope there is none
    assert lib.qot_topological_infer_max_edges(128, H, D) <= cap
    assert lib.qot_topological_infer_max_edges(n, 64, D) <= cap
    assert lib.qot_topological_infer_max_edges(129, H, D) == -1 and lib.qot_topological_infer_max_edges(n, 48, D) == -1


# qot_topological_infer{,_mc,_grad}_max_edges at (n, H, D), as the library answered before the three envelopes were one
# function (1541 / 1114 / 677 at the headline shape also follow from infer_lds by hand)
PINNED_CAPS = {(100, 64, 4): (1541, 1114, 677), (75, 16, 4): (2240, 2160, 1385), (128, 32, 1): (5599, 4916, 3615)}


def test_edge_caps_are_pinned():
    lib = _lib.load()
    for shape, want in PINNED_CAPS.items():
        got = tuple(getattr(lib, f"qot_topological_infer{k}_max_edges")(*shape) for k in ("", "_mc", "_grad"))
        assert got == want, (shape, got, want)
        assert (infer.edge_cap(*shape), infer.mc_edge_cap(*shape), infer.grad_edge_cap(*shape)) == want


@pytest.mark.parametrize("kw,code", INFER_COMMON_REFUSALS)
def test_entry_point_return_codes_before_any_launch(kw, code):
    assert _lib.load().qot_topological_infer(*infer_common_args(**kw), None) == code


def test_predictor_refuses_a_cpu_model():
    m = q.TopologicalGNN(14, 32, 3, 4)
    with pytest.raises(ValueError, match="CPU"):
        q.TopologicalPredictor(m)


def test_predictor_refuses_models_outside_the_envelope_before_any_launch():
    with pytest.raises(ValueError, match="zero-padded"):
        q.TopologicalPredictor(q.TopologicalGNN(14, 20, 3, 4))
    with pytest.raises(ValueError, match="num_layers"):
        q.TopologicalPredictor(q.TopologicalGNN(14, 16, 3, 4, num_layers=3))
    with pytest.raises(ValueError, match="hidden width 128"):
        q.TopologicalPredictor(q.TopologicalGNN(14, 128, 3, 4))
    with pytest.raises(ValueError, match="edge_dim 6"):
        q.TopologicalPredictor(q.TopologicalGNN(14, 16, 3, 6))
    with pytest.raises(ValueError, match="out_channels 9"):
        q.TopologicalPredictor(q.TopologicalGNN(14, 16, 9, 4))


def test_evaluate_fused_is_for_the_topological_model_only():
    m = q.LightpathGNN(5, 8, 3, 1)
    with pytest.raises(ValueError, match="kind='topological' only"):
        harness.evaluate(m, [], kind="lightpath", fused=True, device="cpu")


def test_wcat_index_restates_nnconv_wcat():
    from gnn_qot_estimation_amd import functional as QF
    torch.manual_seed(0)
    h, k = 16, 6
    w2, b2, wroot = torch.randn(h * h, k), torch.randn(h * h), torch.randn(h, h)
    flat = torch.cat([w2.reshape(-1), b2, wroot.reshape(-1)])
    got = flat[infer.wcat_index(h, k, "cpu").long()].view((k + 2) * h, h)
    assert torch.equal(got, QF.nnconv_wcat(w2, b2, wroot, h, h, k))
