"""The single-step cases of tests/test_gpu_dropout_oracle.py (one dropout-ON train step of ``TopologicalGNN`` against the
fp64 oracle running the same masks), shared with tests/test_dropout_oracle_cpu.py, which pins their conditioning without
a GPU (the masked oracle in fp32 against itself in fp64 must agree to ``TOL / 10``).

A case: ``batch()`` builds the host batch; ``model`` the constructor arguments; ``env`` the environment switches that
force a form; ``attrs`` attributes set on the HIP model; ``loss`` whether the step goes through ``forward_loss``;
``called`` / ``not_called`` the C entry points that must / must not have run; ``fold`` whether the read-out's backward
must have folded the last convolution's activation; ``head_hook``: the read-out is unfused and its dropout is torch's
``nn.Dropout`` (that one mask is read off a forward hook).
"""
import torch

SEED = (1 << 63) + 0x1234567       # bit 63 set: the site seeds wrap around 2^64


def _model(H, V, D=4, p=0.5, layers=2):
    return dict(num_nodes=V, hidden_channels=H, out_channels=3, edge_dim=D, dropout_p=p, num_layers=layers)


def _synthetic(cfg, B, **kw):
    def build():
        from gnn_qot_estimation_amd import synthetic as S
        return S.topological_batch(cfg, B, **kw)
    return build


def _mixed_nodes():
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    a = S.topological_batch(2, 1, n=10, e=24)
    b = S.topological_batch(2, 1, n=14, e=30, first_graph=5)
    g1 = q.Data(edge_index=a.edge_index, edge_attr=a.edge_attr, node_ids=a.node_ids, y=a.y, num_nodes=10)
    g2 = q.Data(edge_index=b.edge_index, edge_attr=b.edge_attr, node_ids=b.node_ids, y=b.y, num_nodes=14)
    batch = q.Batch.from_data_list([g1, g2, g1])
    assert batch.uniform_node_ids is None
    return batch


def _given_x():
    from gnn_qot_estimation_amd import synthetic as S
    batch = S.topological_batch(2, 4, n=20, e=60)
    batch.x = torch.randn(batch.num_nodes, 32, generator=torch.Generator().manual_seed(5))
    return batch


def _isolated_and_duplicates():
    """Zero in-degree rows (nodes 3 and 5), duplicate edges 1 -> 0 and a self loop 2 -> 2."""
    import gnn_qot_estimation_amd as q
    g = torch.Generator().manual_seed(1)
    ei = torch.tensor([[0, 1, 1, 2, 2, 4, 4], [1, 0, 0, 2, 1, 1, 0]])
    d = q.Data(edge_index=ei, edge_attr=torch.rand(7, 4, generator=g), node_ids=torch.arange(6), num_nodes=6)
    batch = q.Batch.from_data_list([d, d, d])
    batch.y = torch.rand(3, 3, generator=g)
    return batch


def _case(batch, model, env=None, attrs=None, loss=False, called=(), not_called=(), fold=None, head_hook=False):
    return dict(batch=batch, model=model, env=env or {}, attrs=attrs or {}, loss=loss, called=tuple(called),
                not_called=tuple(not_called), fold=fold, head_hook=head_hook)


_CFG2 = dict(n=100, e=400)             # 100-node graphs: table mode, every TransformerConv form is available
_SMALL = dict(n=40, e=140)
_FUSED_HEAD = ("qot_head_fwd", "qot_head_bwd")

CASES = {
    # ---- conv1 forms (H = 64: conv2 is the split-bf16 kernel unless said otherwise)
    "conv1_graph": _case(_synthetic(1, 16), _model(32, 14), called=("qot_tconv_fwd_graph", "qot_tconv_bwd_graph") + _FUSED_HEAD,
                         fold=True),
    "conv1_per_destination": _case(_synthetic(2, 8, **_CFG2), _model(64, 100),
                                   env=dict(QOT_NO_TCONV_GRAPH="1", QOT_NO_TCONV_TILE="1", QOT_NO_TCONV_SCORES="1"),
                                   called=("qot_tconv_fwd", "qot_tconv_bwd_dst", "qot_nnconv_fused_split"),
                                   not_called=("qot_tconv_fwd_graph", "qot_tconv_fwd_tile", "qot_tconv_fwd_rows")),
    "conv1_tile": _case(_synthetic(2, 8, **_CFG2), _model(64, 100), env=dict(QOT_NO_TCONV_GRAPH="1"),
                        called=("qot_tconv_fwd_tile", "qot_tconv_bwd_dst"), not_called=("qot_tconv_fwd_graph",)),
    # 200-node graphs: past the graph form (n <= 128) and the tile form (n <= 2 x 16 x 3), N = 4 V: scores / rows form
    "conv1_rows": _case(_synthetic(2, 4, n=200, e=600), _model(64, 200),
                        called=("qot_tconv_fwd_rows", "qot_tconv_bwd_dst_rows", "qot_nnconv_fused_split"),
                        not_called=("qot_tconv_fwd_graph", "qot_tconv_fwd_tile")),
    "conv1_node_mixed": _case(_mixed_nodes, _model(64, 14), called=("qot_tconv_fwd", "qot_step_advance"),
                              not_called=("qot_tconv_fwd_graph",)),
    "conv1_node_given_x": _case(_given_x, _model(32, 20), called=("qot_tconv_fwd", "qot_step_advance")),
    # ---- conv2 forms
    "conv2_h64_split_bf16": _case(_synthetic(2, 6, **_CFG2), _model(64, 100),
                                  called=("qot_nnconv_fused_split", "qot_nnconv_adjoint_dw"), not_called=("qot_nnconv_fused",)),
    "conv2_h64_f32_mfma": _case(_synthetic(2, 6, **_CFG2), _model(64, 100), env=dict(QOT_NNCONV_F32_MFMA="1"),
                                called=("qot_nnconv_fused", "qot_nnconv_adjoint_dw"), not_called=("qot_nnconv_fused_split",)),
    "conv2_h16": _case(_synthetic(2, 6, **_SMALL), _model(16, 40), called=("qot_nnconv_fused", "qot_nnconv_dw")),
    "conv2_h32": _case(_synthetic(2, 6, **_SMALL), _model(32, 40), called=("qot_nnconv_fused", "qot_nnconv_dw")),
    "conv2_h128": _case(_synthetic(2, 6, **_SMALL), _model(128, 40), called=("qot_nnconv_fused", "qot_nnconv_dw")),
    "conv2_h256": _case(_synthetic(2, 3, **_SMALL), _model(256, 40), called=("qot_nnconv_fused", "qot_nnconv_dw"),
                        not_called=_FUSED_HEAD, head_hook=True),
    "conv2_d6_materialised": _case(_synthetic(2, 5, edge_dim=6, **_SMALL), _model(64, 40, D=6),
                                   called=("qot_nnconv_agg", "qot_act_fwd"), not_called=("qot_nnconv_fused_split",)),
    "three_layers": _case(_synthetic(2, 6, **_SMALL), _model(32, 40, layers=3), called=_FUSED_HEAD, fold=True),
    # ---- read-out forms
    "head_fused_fold": _case(_synthetic(2, 6, **_CFG2), _model(64, 100), called=_FUSED_HEAD,
                             not_called=("qot_act_bwd_colsum",), fold=True),
    "head_no_fold": _case(_synthetic(2, 6, **_CFG2), _model(64, 100), attrs=dict(_qot_fold_head=False),
                          called=_FUSED_HEAD + ("qot_act_bwd_colsum",), fold=False),
    "head_train": _case(_synthetic(2, 6, **_CFG2), _model(64, 100), loss=True, called=("qot_head_train",),
                        not_called=_FUSED_HEAD, fold=True),
    "head_fwd_loss": _case(_synthetic(2, 6, **_CFG2), _model(64, 100), loss=True, env=dict(QOT_NO_HEAD_TRAIN="1"),
                           called=("qot_head_fwd_loss", "qot_head_bwd"), not_called=("qot_head_train",), fold=True),
    "head_unfused_h256": _case(_synthetic(2, 2, n=50, e=200), _model(256, 50), not_called=_FUSED_HEAD, head_hook=True),
    # ---- the rest
    "padded_h48": _case(_synthetic(1, 8), _model(48, 14), called=_FUSED_HEAD, fold=True),
    "launch_groups_off": _case(_synthetic(2, 8, **_CFG2), _model(64, 100), env=dict(QOT_NO_LAUNCH_GROUPS="1"),
                               called=_FUSED_HEAD, fold=True),
    "isolated_and_duplicates": _case(_isolated_and_duplicates, _model(16, 6), called=_FUSED_HEAD, fold=True),
    "p_0.1": _case(_synthetic(1, 16), _model(32, 14, p=0.1), called=("qot_tconv_fwd_graph",) + _FUSED_HEAD, fold=True),
    "p_0.9": _case(_synthetic(1, 16), _model(32, 14, p=0.9), called=("qot_tconv_fwd_graph",) + _FUSED_HEAD, fold=True),
}


def models(case, device=None):
    """``(oracle model, HIP model)`` with shared, seeded parameters (zero-initialised biases made non-zero); the HIP model
    only when a device is given."""
    from oracle import sparse as O
    torch.manual_seed(0)
    ref = O.TopologicalGNN(**case["model"])
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1 and p.abs().max() == 0:
                p.uniform_(-0.1, 0.1)
    if device is None:
        return ref, None
    import gnn_qot_estimation_amd as q
    hip = q.TopologicalGNN(**case["model"])
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref, hip.to(device)


def masks(case, batch, step, head=True):
    """The restated masks of the draw ``step`` for ``batch``."""
    from oracle import dropout as OD
    m = case["model"]
    return OD.topological_masks(SEED, step, m["dropout_p"], batch.num_nodes, batch.num_graphs, m["hidden_channels"],
                                num_layers=m["num_layers"], head=head)


def to_double(batch):
    """The host batch with its floating-point tensors in fp64 (for the fp64 oracle)."""
    import copy
    out = copy.copy(batch)
    for name in ("x", "edge_attr", "y"):
        t = getattr(batch, name, None)
        if isinstance(t, torch.Tensor) and t.is_floating_point():
            setattr(out, name, t.double())
    return out
