"""CPU-side checks of LightpathGNN's single-launch inference path (``csrc/infer_lightpath.hip``,
``infer.LightpathPredictor``): the entry point is declared, bound and exported; loud refusals that need no GPU."""
import ctypes
import os
import re

import pytest

import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import _lib, harness, infer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    declared = set(re.findall(r"\b(qot_[a-z0-9_]+)\s*\(", hdr))
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = "qot_lightpath_infer"
    assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    # the entry point's ctypes row has one type per declared parameter
    decl = re.search(r"int qot_lightpath_infer\(([^;]*)\);", hdr).group(1)
    assert len(_lib.SIGNATURES[name][1]) == decl.count(",") + 1
    assert q.LightpathPredictor is infer.LightpathPredictor and "LightpathPredictor" in q.__all__
    assert issubclass(infer.EnvelopeError, ValueError)


def test_predictor_refuses_a_cpu_model():
    with pytest.raises(infer.EnvelopeError, match="CPU"):
        q.LightpathPredictor(q.LightpathGNN(5, 32, 3, 1))


def test_predictor_refuses_models_outside_the_envelope_before_any_launch():
    with pytest.raises(infer.EnvelopeError, match="num_layers"):
        q.LightpathPredictor(q.LightpathGNN(5, 8, 3, 1, num_layers=2))
    with pytest.raises(infer.EnvelopeError, match="in_channels 17"):
        q.LightpathPredictor(q.LightpathGNN(17, 8, 3, 1))
    with pytest.raises(infer.EnvelopeError, match="output_dim 9"):
        q.LightpathPredictor(q.LightpathGNN(5, 8, 9, 1))


def test_evaluate_with_a_predictor_runs_on_one_process(monkeypatch):
    monkeypatch.setattr(harness, "_rank_world", lambda: (0, 2))
    m = q.LightpathGNN(5, 8, 3, 1)
    with pytest.raises(ValueError, match="one process"):
        harness.evaluate(m, [], kind="lightpath", predictor=lambda data: None, device="cpu")


def test_entry_refuses_shapes_outside_the_envelope_before_any_launch():
    fn = _lib.load().qot_lightpath_infer

    def rc(F=5, C=32, O=3, heads=4, lut_col=1, B=0):
        # no arrays: the envelope is answered first, and an empty batch (B = 0 in graphs mode) launches nothing
        return fn(None, None, None, None, None, None, 0, 0, 0, B, None, None, None, None, 0.2, None, None, None, None, 1e-5,
                  None, None, None, None, 0.01, None, None, F, C, O, heads, lut_col, None, None)

    assert rc() == 0
    assert rc(F=16, C=256, O=8, lut_col=15) == 0 and rc(F=1, C=1, O=1, lut_col=0) == 0
    for bad in (dict(F=0), dict(F=17), dict(C=0), dict(C=257), dict(O=0), dict(O=9), dict(heads=1), dict(heads=8),
                dict(lut_col=-1), dict(lut_col=5)):
        assert rc(**bad) == -1, bad                     # QOT_ERR_UNSUPPORTED
    assert rc(B=-1) == -2 and rc(B=3) == -2             # QOT_ERR_BADARG: negative size; rows to compute but no arrays
    assert rc(B=3, F=0) == -1                           # the envelope is answered before the arrays are looked at
