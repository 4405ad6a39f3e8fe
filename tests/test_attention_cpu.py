"""CPU: the attention-weights readout's C ABI and Python surface (no GPU needed)."""
import ctypes
import inspect
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qot_tconv_attention", "qot_gat_attention")


def test_entry_points_declared_bound_and_exported():
    from gnn_qot_estimation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    declared = set(re.findall(r"\b(qot_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 13 and "#define QOT_ABI_VERSION 13" in hdr
    assert _lib.load().qot_abi_version() == 13


def test_gat_attention_rejects_other_head_counts():
    from gnn_qot_estimation_amd import _lib
    # heads != 4 is refused before any pointer is looked at (no launch)
    code = _lib.load().qot_gat_attention(None, None, None, None, None, None, 0, None, 1, 2, 0.2, None)
    assert code == -1


def test_forward_signatures():
    import gnn_qot_estimation_amd as q
    for cls in (q.TransformerConv, q.GATConv, q.TopologicalGNN, q.LightpathGNN):
        p = inspect.signature(cls.forward).parameters
        assert "return_attention_weights" in p and not p["return_attention_weights"].default, cls.__name__


def test_auto_device_moves_nested_readouts():
    from gnn_qot_estimation_amd import auto_device
    out = auto_device._to((torch.ones(2), torch.zeros(3), [(torch.arange(4), torch.ones(1, 4))]), torch.device("cpu"))
    assert isinstance(out, tuple) and isinstance(out[2], list) and isinstance(out[2][0], tuple)
    assert torch.equal(out[2][0][0], torch.arange(4))
