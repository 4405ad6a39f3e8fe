"""GPU: gradients wrt the edge features (``edge_attr.grad``) of TopologicalGNN and of its two operators, against the CPU
oracle's plain autograd, in every form the forward and backward can take (graph, per-destination plain / tiled, rows,
node path; NNConv at H = 64, the generic widths, the wide edge MLP), with the parameter gradients checked alongside.
Plus the invariants: asking for the edge gradient changes nothing else, and it is bitwise reproducible.  Dropout on is
checked against a central difference here (parameter gradients with dropout on are checked against the oracle running the
same masks in tests/test_gpu_dropout_oracle.py)."""
import pytest
import torch
import torch.nn.functional as F

from helpers import TOL, grad_compare as _grad_compare, rel_err

pytestmark = pytest.mark.gpu


def _models(kind, device, **kw):
    import gnn_qot_estimation_amd as q
    from oracle import sparse as O
    torch.manual_seed(0)
    if kind == "topo":
        ref = O.TopologicalGNN(**kw)
        hip = q.TopologicalGNN(**kw)
    else:
        ref = O.LightpathGNN(**kw)
        hip = q.LightpathGNN(**kw)
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1 and p.abs().max() == 0:      # zero-init biases: make them matter
                p.uniform_(-0.1, 0.1)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref, hip.to(device)


def _record(monkeypatch):
    """Names of the C entry points called from here on."""
    from gnn_qot_estimation_amd import _lib
    names = []
    real = _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return names


def _leaf_pair(batch, device):
    """(cpu batch, device batch), each with its edge features a leaf that requires grad."""
    batch.edge_attr = batch.edge_attr.detach().clone().requires_grad_()
    dbatch = batch.to(device)
    dbatch.edge_attr = dbatch.edge_attr.detach().requires_grad_()
    return batch, dbatch


def _check_topo(device, batch, H, V, D=4, layers=2, params=True):
    """Forward + smooth-L1 backward on both sides; edge_attr.grad and every parameter gradient against the oracle."""
    ref, hip = _models("topo", device, num_nodes=V, hidden_channels=H, out_channels=3, edge_dim=D, dropout_p=0.0,
                       num_layers=layers)
    ref.train(); hip.train()
    if not params:
        for p in list(ref.parameters()) + list(hip.parameters()):
            p.requires_grad_(False)
    batch, dbatch = _leaf_pair(batch, device)
    out_ref, out_hip = ref(batch), hip(dbatch)
    assert rel_err(out_hip, out_ref) <= TOL
    y = batch.y.view(-1, 3)
    F.smooth_l1_loss(out_ref, y).backward()
    F.smooth_l1_loss(out_hip, y.to(device)).backward()
    torch.cuda.synchronize()
    assert dbatch.edge_attr.grad is not None, "no gradient reached edge_attr"
    assert dbatch.edge_attr.grad.shape == dbatch.edge_attr.shape
    e = rel_err(dbatch.edge_attr.grad, batch.edge_attr.grad)
    assert e <= TOL, e
    if params:
        _grad_compare(ref, hip)
    return hip, dbatch


# ------------------------------------------------------------------ TransformerConv forms (table mode)
@pytest.mark.parametrize("H", [16, 32])
def test_graph_form_nsfnet(cuda_device, monkeypatch, H):
    from gnn_qot_estimation_amd import synthetic as S
    names = _record(monkeypatch)
    _check_topo(cuda_device, S.topological_batch(1, 16), H, 14)
    assert "qot_tconv_fwd_graph" in names and "qot_tconv_bwd_graph" in names
    assert "qot_tconv_edge_attr_grad" in names and "qot_nnconv_edge_attr_grad" in names


def test_graph_form_reference_scale(cuda_device, monkeypatch):
    """The reference's own shape: 75-node graphs, H = 16, D = 4."""
    from gnn_qot_estimation_amd import synthetic as S
    names = _record(monkeypatch)
    _check_topo(cuda_device, S.topological_batch(2, 32, n=75, e=160), 16, 75)
    assert "qot_tconv_fwd_graph" in names


@pytest.mark.parametrize("tile", [True, False])
def test_per_destination_form(cuda_device, monkeypatch, tile):
    from gnn_qot_estimation_amd import synthetic as S
    monkeypatch.setenv("QOT_NO_TCONV_GRAPH", "1")
    if not tile:
        monkeypatch.setenv("QOT_NO_TCONV_TILE", "1")
        monkeypatch.setenv("QOT_NO_TCONV_SCORES", "1")     # else the rows form takes this batch
    names = _record(monkeypatch)
    _check_topo(cuda_device, S.topological_batch(2, 8, n=100, e=400), 64, 100)
    assert "qot_tconv_bwd_dst" in names and "qot_tconv_bwd_graph" not in names
    assert ("qot_tconv_fwd_tile" if tile else "qot_tconv_fwd") in names


def test_rows_form(cuda_device, monkeypatch):
    from gnn_qot_estimation_amd import synthetic as S
    names = _record(monkeypatch)
    _check_topo(cuda_device, S.topological_batch(5, 4, n=300), 128, 300)
    assert "qot_tconv_fwd_rows" in names and "qot_tconv_bwd_dst_rows" in names


def test_node_path(cuda_device, monkeypatch):
    """``data.x`` given: TransformerConv on node rows; x.grad is not asked for here (x is data, not a leaf)."""
    from gnn_qot_estimation_amd import synthetic as S
    batch = S.topological_batch(2, 4, n=20, e=60)
    batch.x = torch.randn(batch.num_nodes, 32)
    names = _record(monkeypatch)
    _check_topo(cuda_device, batch, 32, 20)
    assert "qot_tconv_fwd" in names


# ------------------------------------------------------------------ NNConv widths and edge dims
@pytest.mark.parametrize("H,D", [(64, 4), (16, 4), (32, 4), (128, 4), (256, 4), (64, 6), (32, 8), (32, 1)])
def test_nnconv_widths(cuda_device, monkeypatch, H, D):
    from gnn_qot_estimation_amd import synthetic as S
    names = _record(monkeypatch)
    batch = S.topological_batch(2, 3 if H == 256 else 6, n=100 if H == 64 and D == 4 else 40,
                                e=400 if H == 64 and D == 4 else 140, edge_dim=D)
    _check_topo(cuda_device, batch, H, batch.num_nodes // batch.num_graphs, D=D)
    if D > 4:
        assert "qot_nnconv_agg" in names                  # the wide-edge path
    elif H == 64:
        assert "qot_nnconv_adjoint_dw" in names
    else:
        assert "qot_nnconv_dw" in names
    assert "qot_nnconv_edge_attr_grad" in names


def test_three_layers(cuda_device):
    from gnn_qot_estimation_amd import synthetic as S
    _check_topo(cuda_device, S.topological_batch(2, 6, n=40, e=140), 32, 40, layers=3)


def test_padded_width(cuda_device):
    """H = 20 runs zero-padded to 32 through the shadow model."""
    from gnn_qot_estimation_amd import synthetic as S
    hip, _ = _check_topo(cuda_device, S.topological_batch(1, 8), 20, 14)
    assert hip._qot_hp == 32


def test_isolated_nodes_and_duplicates(cuda_device):
    import gnn_qot_estimation_amd as q
    torch.manual_seed(1)
    ei = torch.tensor([[0, 1, 1, 2, 2, 4, 4], [1, 0, 0, 2, 1, 1, 0]])
    ea = torch.rand(7, 4)
    d = q.Data(edge_index=ei, edge_attr=ea, node_ids=torch.arange(6), num_nodes=6)
    batch = q.Batch.from_data_list([d, d])
    batch.y = torch.rand(2, 3)
    _check_topo(cuda_device, batch, 16, 6)


@pytest.mark.parametrize("groups", [True, False])
def test_launch_groups(cuda_device, monkeypatch, groups):
    from gnn_qot_estimation_amd import synthetic as S
    if not groups:
        monkeypatch.setenv("QOT_NO_LAUNCH_GROUPS", "1")
    _check_topo(cuda_device, S.topological_batch(2, 8, n=100, e=400), 64, 100)
    _check_topo(cuda_device, S.topological_batch(1, 16), 32, 14)


# ------------------------------------------------------------------ operators called directly
def test_operators_direct(cuda_device):
    import gnn_qot_estimation_amd as q
    from oracle import sparse as O
    torch.manual_seed(3)
    N, E, H, D = 50, 200, 32, 4
    ei = torch.randint(0, N, (2, E))
    x = torch.randn(N, H)
    ea = torch.randn(E, D)
    R = torch.randn(N, H)
    ref_t = O.TransformerConv(H, H, edge_dim=D)
    hip_t = q.TransformerConv(H, H, edge_dim=D)
    hip_t.load_state_dict(ref_t.state_dict(), strict=True)
    seq = lambda: torch.nn.Sequential(torch.nn.Linear(D, 2 * D), torch.nn.ReLU(), torch.nn.Linear(2 * D, H * H))
    ref_n = O.NNConv(H, H, seq())
    with torch.no_grad():
        ref_n.bias.uniform_(-0.1, 0.1)
    hip_n = q.NNConv(H, H, nn=seq(), aggr="mean")
    hip_n.load_state_dict(ref_n.state_dict(), strict=True)
    for ref_c, hip_c in ((ref_t, hip_t), (ref_n, hip_n)):
        hip_c.to(cuda_device)
        xr, ear = x.clone().requires_grad_(), ea.clone().requires_grad_()
        xd, ead = x.to(cuda_device).requires_grad_(), ea.to(cuda_device).requires_grad_()
        out_r = ref_c(xr, ei, ear)
        out_d = hip_c(xd, ei.to(cuda_device), ead)
        assert rel_err(out_d, out_r) <= TOL
        (out_r * R).sum().backward()
        (out_d * R.to(cuda_device)).sum().backward()
        assert ead.grad is not None and rel_err(ead.grad, ear.grad) <= TOL, type(hip_c).__name__
        assert rel_err(xd.grad, xr.grad) <= TOL
        _grad_compare(ref_c, hip_c)


# ------------------------------------------------------------------ invariants
def _run(hip, dbatch, y, want):
    for p in hip.parameters():
        p.grad = None
    ea = dbatch.edge_attr.detach().requires_grad_(want)
    dbatch.edge_attr = ea
    out = hip(dbatch)
    F.smooth_l1_loss(out, y).backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {n: p.grad.clone() for n, p in hip.named_parameters()}, ea.grad


@pytest.mark.parametrize("form", ["graph", "dst"])
def test_asking_changes_nothing_else(cuda_device, monkeypatch, form):
    from gnn_qot_estimation_amd import synthetic as S
    if form == "dst":
        monkeypatch.setenv("QOT_NO_TCONV_GRAPH", "1")
    _, hip = _models("topo", cuda_device, num_nodes=100, hidden_channels=64, out_channels=3, edge_dim=4, dropout_p=0.0)
    hip.train()
    batch = S.topological_batch(2, 8, n=100, e=400)
    dbatch = batch.to(cuda_device)
    y = batch.y.view(-1, 3).to(cuda_device)
    out0, g0, ea0 = _run(hip, dbatch, y, False)
    out1, g1, ea1 = _run(hip, dbatch, y, True)
    out2, g2, ea2 = _run(hip, dbatch, y, True)
    assert ea0 is None and ea1 is not None
    assert torch.equal(out0, out1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert torch.equal(ea1, ea2)                             # two identical backward passes: bitwise equal


def test_frozen_parameters(cuda_device):
    from gnn_qot_estimation_amd import synthetic as S
    _check_topo(cuda_device, S.topological_batch(1, 16), 32, 14, params=False)


# ------------------------------------------------------------------ dropout on: directional derivative
@pytest.mark.parametrize("form", ["graph", "dst"])
def test_dropout_directional_derivative(cuda_device, monkeypatch, form):
    from gnn_qot_estimation_amd import synthetic as S
    if form == "dst":
        monkeypatch.setenv("QOT_NO_TCONV_GRAPH", "1")
    _, hip = _models("topo", cuda_device, num_nodes=14, hidden_channels=32, out_channels=3, edge_dim=4, dropout_p=0.5)
    hip.train()
    batch = S.topological_batch(1, 16)
    dbatch = batch.to(cuda_device)
    y = batch.y.view(-1, 3).double()
    ea = dbatch.edge_attr.detach().clone()
    gen = torch.Generator().manual_seed(7)
    v = torch.randn(ea.shape, generator=gen).to(cuda_device)
    step0 = hip._qot_step.clone()

    def loss_at(t, grad=False):
        hip._qot_step.copy_(step0)                           # every forward draws the same dropout masks
        dbatch.edge_attr = t.detach().requires_grad_(grad)
        out = hip(dbatch)
        if grad:
            F.smooth_l1_loss(out, y.float().to(cuda_device), reduction="sum").backward()
            return float((dbatch.edge_attr.grad.double() * v.double()).sum())
        return float(F.smooth_l1_loss(out.detach().double().cpu(), y, reduction="sum"))

    dd = loss_at(ea, grad=True)
    eps = 1e-3
    fd = (loss_at(ea + eps * v) - loss_at(ea - eps * v)) / (2 * eps)
    assert abs(dd - fd) <= 2e-2 * max(abs(fd), abs(dd)), (dd, fd)
