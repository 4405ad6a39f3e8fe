"""The read-out head's kernels (csrc/head.hip: head_fwd / head_bwd / head_train / head_train_batched; csrc/misc.hip:
pool_fwd / pool_bwd; csrc/graph_prep.hip: batch_ptr) against the fp64 restatement of tests/head_cases.py, element by
element: ``|got - ref| <= k 2^-24 A`` with the count ``k`` and the magnitude ``A`` derived there, beside the existing head
test's global ``max|got - ref| <= 1e-5 max|ref|``.

Every case runs through three paths, each against the same reference:

  explicit  ``HeadFn`` without a loss, fed the reference's ``grad_out``:     qot_head_fwd      + qot_head_bwd
  unfused   ``HeadFn`` with a loss and QOT_NO_HEAD_TRAIN=1:                  qot_head_fwd_loss + qot_head_bwd
  train     ``HeadFn`` with a loss (the benchmark's timed step):            qot_head_train

with every buffer the Function allocates filled with NaN first (``torch.empty`` is wrapped for the duration), each path run
twice (bitwise equal: the kernels sum in a fixed order), and the entry points that ran asserted from the recorded
``_lib.call`` names.  The small cases are ragged batches of 41 graphs around every size threshold of the kernels; the trip
cases are the smallest batches at which workgroups take a second ... fifth trip through their grid-stride loops.

Every tensor's worst ``error / bound`` is printed before anything is asserted (``pytest -s``); it is a record, not a
threshold."""
import pytest
import torch

import head_cases as HC
from helpers import TOL, grad_compare, rel_err

pytestmark = pytest.mark.gpu

PATHS = {"explicit": ("qot_head_fwd", "qot_head_bwd"), "unfused": ("qot_head_fwd_loss", "qot_head_bwd"),
         "train": ("qot_head_train",)}
_HEAD_ENTRIES = ("qot_head_fwd", "qot_head_fwd_loss", "qot_head_bwd", "qot_head_train")


def _record(monkeypatch):
    from gnn_qot_estimation_amd import _lib
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def _nan_filled_empty(monkeypatch):
    """Every floating-point ``torch.empty`` comes back full of NaN: outputs, saved activations and the partials workspace
    of ``HeadFn`` / ``PoolFn`` are allocated that way, so an element no kernel writes stays NaN and fails the check."""
    real = torch.empty

    def empty(*a, **kw):
        t = real(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(torch, "empty", empty)


def _once(c, path, dev, go_ref):
    from gnn_qot_estimation_amd import functional as QF
    leaves = [t.to(dev).requires_grad_(True) for t in (c.x, c.w0, c.b0, c.w3, c.b3)]
    ptr = c.ptr.to(torch.int32).to(dev)

    def counter(v):
        return torch.tensor([v], dtype=torch.int64, device=dev)
    act = (c.slope, c.p, c.seed, counter(c.step) if c.p > 0 else None)
    in_act = side = None
    if c.fold:
        in_act, side = (c.in_slope, c.in_p, c.in_seed, counter(c.in_step) if c.in_p > 0 else None), {}
    res = {}
    if path == "explicit":
        out = QF.HeadFn.apply(leaves[0], ptr, *leaves[1:], c.B, act, in_act, side)
        saved = out.grad_fn.saved_tensors
        res.update(pool=saved[3].clone(), h=saved[4].clone())
        g = go_ref.to(dev)
    else:
        loss_out = torch.full((), float("nan"), dtype=torch.float32, device=dev)
        out, g = QF.HeadFn.apply(leaves[0], ptr, *leaves[1:], c.B, act, in_act, side,
                                 (c.y.to(dev), c.beta, loss_out, True))
        loss_rows = out.grad_fn.loss[0]
        if path == "unfused":
            saved = out.grad_fn.saved_tensors
            res.update(pool=saved[3].clone(), h=saved[4].clone())
    grads = torch.autograd.grad(out, leaves, g)
    torch.cuda.synchronize()
    res.update(out=out.detach(), gx=grads[0], gw0=grads[1], gb0=grads[2], gw3=grads[3], gb3=grads[4])
    if path != "explicit":
        res.update(grad_out=g, loss_rows=loss_rows, loss=loss_out)
    if c.fold:
        res["gbias"] = side["gbias"]
    return {k: v.detach().cpu() for k, v in res.items()}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(HC.CASES))
def test_head_against_fp64_element_by_element(cuda_device, monkeypatch, name, path):
    from gnn_qot_estimation_amd import _lib
    c = HC.head_case(name)
    ref = HC.head_reference(c)
    for k in _lib_switches():
        monkeypatch.delenv(k, raising=False)
    if path == "unfused":
        monkeypatch.setenv("QOT_NO_HEAD_TRAIN", "1")
    if c.cfg["kind"] == "trip":
        # the case is only worth its name while workgroups loop: fails loudly if the cap of 512 workgroups ever moves
        lib = _lib.load()
        blocks = lib.qot_head_train_blocks(c.B, c.H) if path == "train" else lib.qot_head_bwd_blocks(c.B)
        t = HC.trips(c.B, c.H, blocks, train=path == "train")
        print(f"{name} {path}: {blocks} workgroups, trips {sorted(set(t.values()))}")
        assert max(t.values()) >= 4 and len(set(t.values())) >= 2, (blocks, sorted(set(t.values())))
    calls = _record(monkeypatch)
    _nan_filled_empty(monkeypatch)
    go_ref = ref["grad_out"]["value"].float()
    first = _once(c, path, cuda_device, go_ref)
    ran = [k for k in calls if k in _HEAD_ENTRIES]
    again = _once(c, path, cuda_device, go_ref)
    # printed first, asserted afterwards
    figs = {k: HC.compare(first[k], ref[k]) for k in first}
    for k, f in figs.items():
        print(f"{name} {path} {k}: error/bound {f['ratio']:.3e}  global {f['glob']:.3e}  k <= {float(ref[k]['k'].max()):.0f}")
    assert tuple(ran) == PATHS[path], ran
    assert first["gx"].shape == (c.N, c.H)                     # rows of no graph do not exist
    assert ("gbias" in first) == c.fold
    expected = set(HC.CHECKED) - ({"pool", "h"} if path == "train" else {"grad_out", "loss_rows", "loss"} if
                                  path == "explicit" else set()) - (set() if c.fold else {"gbias"})
    assert set(first) == expected, (sorted(first), sorted(expected))
    for k in first:
        assert torch.equal(first[k], again[k]), (k, "two runs differ")
    HC.check_all(f"{name} {path}", first, ref)


def _lib_switches():
    return ("QOT_NO_HEAD_TRAIN", "QOT_NO_LAUNCH_GROUPS")


# ------------------------------------------------------------------ boundaries and the unfused pool
# (batch vector, B): a skipped id first, in the middle, several in a row, last (B beyond batch.max() + 1), N = 1, B = 1
def _batch_vectors():
    def rep(ids, counts):
        return torch.repeat_interleave(torch.tensor(ids), torch.tensor(counts))
    return {
        "skip_first": (rep([1, 2, 3], [3, 1, 70]), 4),
        "skip_middle": (rep([0, 1, 3, 4], [5, 1, 300, 2]), 5),
        "skip_several": (rep([0, 4, 5], [129, 2, 64]), 6),
        "skip_last": (rep([0, 1, 2], [2, 65, 3]), 5),
        "skip_everywhere": (rep([2, 3, 7, 9], [1, 128, 1, 127]), 12),
        "one_node": (torch.tensor([0]), 1),
        "one_node_of_three_ids": (torch.tensor([1]), 3),
        "one_graph": (torch.zeros(300, dtype=torch.long), 1),
        "many_graphs": (torch.arange(700).repeat_interleave(2), 700),       # more than one workgroup of 256 boundaries
    }


def _boundaries(batch, B, dev):
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd.graph import batch_index_for
    d = q.Data()
    d.batch = batch.to(dev)
    d.num_graphs = B
    return batch_index_for(d, batch.numel())


@pytest.mark.parametrize("name", list(_batch_vectors()))
def test_batch_ptr_equals_searchsorted(cuda_device, monkeypatch, name):
    batch, B = _batch_vectors()[name]
    calls = _record(monkeypatch)
    b32, ptr, B2 = _boundaries(batch, B, cuda_device)
    assert "qot_batch_ptr" in calls and B2 == B
    want = torch.searchsorted(batch, torch.arange(B + 1))
    assert ptr.dtype == torch.int32 and torch.equal(ptr.cpu().long(), want), (ptr.tolist(), want.tolist())
    assert torch.equal(b32.cpu().long(), batch)
    assert int(ptr[-1]) == batch.numel() and int(ptr[0]) == 0


@pytest.mark.parametrize("H", [16, 256])
@pytest.mark.parametrize("name", list(_batch_vectors()))
def test_pool_against_fp64_element_by_element(cuda_device, monkeypatch, name, H):
    """``PoolFn`` (qot_pool_fwd / qot_pool_bwd): the mean adds cnt rows (k = cnt + 16), its backward divides one number
    (k = 16)."""
    from gnn_qot_estimation_amd import functional as QF
    batch, B = _batch_vectors()[name]
    N = batch.numel()
    gen = torch.Generator().manual_seed(B * 1000 + H)
    x = torch.randn(N, H, generator=gen) * torch.tensor([0.25, 1.0, 4.0])[torch.randint(0, 3, (N, 1), generator=gen)]
    g = torch.randn(B, H, generator=gen)
    cnt = torch.bincount(batch, minlength=B)
    cm = cnt.clamp(min=1).double()[:, None]
    f64 = torch.float64
    ref = {"pool": dict(value=torch.zeros(B, H, dtype=f64).index_add_(0, batch, x.double()) / cm,
                        A=torch.zeros(B, H, dtype=f64).index_add_(0, batch, x.double().abs()) / cm,
                        k=cnt.double()[:, None] + HC.C0),
           "gx": dict(value=(g.double() / cm)[batch], A=(g.double().abs() / cm)[batch], k=torch.full((N, 1), float(HC.C0)))}
    for e in ref.values():
        e["bound"] = e["k"] * HC.U * e["A"]
    calls = _record(monkeypatch)
    b32, ptr, _ = _boundaries(batch, B, cuda_device)
    _nan_filled_empty(monkeypatch)
    xd = x.to(cuda_device).requires_grad_(True)
    runs = []
    for _ in range(2):
        out = QF.PoolFn.apply(xd, b32, ptr, B)
        gx, = torch.autograd.grad(out, xd, g.to(cuda_device))
        runs.append(dict(pool=out.detach().cpu(), gx=gx.cpu()))
    assert "qot_pool_fwd" in calls and "qot_pool_bwd" in calls
    assert runs[0]["gx"].shape == (N, H) and runs[0]["pool"].shape == (B, H)
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    assert bool((runs[0]["pool"][cnt == 0] == 0).all())          # a node-less id pools to exact zeros
    HC.check_all(f"pool {name} H={H}", runs[0], ref)


# ------------------------------------------------------------------ whole models with a node-less graph id
def _models(H, dev, V=12):
    import gnn_qot_estimation_amd as q
    from oracle import sparse as O
    torch.manual_seed(0)
    kw = dict(num_nodes=V, hidden_channels=H, out_channels=3, edge_dim=4, dropout_p=0.0)
    ref, hip = O.TopologicalGNN(**kw), q.TopologicalGNN(**kw)
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1 and p.abs().max() == 0:
                p.uniform_(-0.1, 0.1)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref, hip.to(dev)


def _gapped_batches(unique_ids=False):
    """Five graph ids, id 2 without a node: as a ``Batch`` whose ``ptr`` says so, and as a ``Data`` that carries ``batch``
    only (``B = batch.max() + 1``, as PyG's global_mean_pool takes it).  ``unique_ids``: node ``i`` of the batch reads table
    row ``i`` (34 rows)."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    graphs = []
    for g, n in enumerate((12, 9, 0, 1, 12)):
        if n < 2:                               # no node, or a single node without an edge
            graphs.append(q.Data(edge_index=torch.zeros(2, 0, dtype=torch.long), edge_attr=torch.zeros(0, 4),
                                 node_ids=torch.full((n,), 3, dtype=torch.long), y=torch.zeros(1, 3), num_nodes=n))
            continue
        b = S.topological_batch(2, 1, n=n, e=2 * n + 6, first_graph=g)
        graphs.append(q.Data(edge_index=b.edge_index, edge_attr=b.edge_attr, node_ids=b.node_ids, y=torch.zeros(1, 3),
                             num_nodes=n))
    batch = q.Batch.from_data_list(graphs)
    batch.y = torch.randn(5, 3, generator=torch.Generator().manual_seed(5)) * 1.5        # one row per id
    assert batch.ptr.tolist() == [0, 12, 21, 21, 22, 34] and batch.num_graphs == 5
    if unique_ids:
        batch.node_ids = torch.arange(34)
    data = q.Data(edge_index=batch.edge_index, edge_attr=batch.edge_attr, node_ids=batch.node_ids, y=batch.y)
    data.batch = batch.batch
    assert not hasattr(data, "num_graphs") and data.ptr is None and int(data.batch.max()) + 1 == 5
    return {"batch": batch, "data": data}


def _model_step(m, data, entry, beta=1.0):
    m.zero_grad(set_to_none=True)
    y = data.y.view(-1, 3)
    if entry == "forward_loss":
        out, loss, g = m.forward_loss(data, y, beta=beta)
        out.backward(g)
    else:
        out = m(data)
        loss = torch.nn.functional.smooth_l1_loss(out, y, beta=beta)
        loss.backward()
    return out.detach(), float(loss.detach())


@pytest.mark.parametrize("H", [16, 64, 128, 256])
def test_model_with_a_node_less_graph_id_in_the_middle(cuda_device, H):
    """``forward`` and ``forward_loss``, train mode at p = 0 and eval mode, against ``oracle.sparse.TopologicalGNN``: the
    node-less id pools to zero, its output row is ``mlp(0)`` and takes part in the loss (reference models.py:61)."""
    ref, hip = _models(H, cuda_device)
    for kind, host in _gapped_batches().items():
        dev_data = host.to(cuda_device)
        for mode in ("train", "eval"):
            ref.train(mode == "train"); hip.train(mode == "train")
            out_ref, loss_ref = _model_step(ref, host, "forward")
            assert out_ref.shape == (5, 3)
            for entry in ("forward", "forward_loss"):
                out, loss = _model_step(hip, dev_data, entry)
                torch.cuda.synchronize()
                e = rel_err(out, out_ref)
                print(f"H={H} {kind} {mode} {entry}: out {e:.3e} loss {abs(loss - loss_ref):.3e}")
                assert out.shape == (5, 3) and e <= TOL
                assert abs(loss - loss_ref) <= TOL * max(1.0, abs(loss_ref))
                print(f"H={H} {kind} {mode} {entry}: grads {grad_compare(ref, hip):.3e}")


@pytest.mark.parametrize("H", [16, 64, 128, 256])
def test_empty_x_equals_no_x_bit_for_bit(cuda_device, H):
    """``data.x = torch.empty(0)`` is the reference's way of saying "use the embedding" (models.py:51): same bits as
    ``x = None``: the same entry points in the same order, the same output, loss and gradients.  Every node reads a table
    row of its own here: the table's gradient is summed with fp32 atomics (grad_scale_cases.ATOMIC_EMBED), whose order
    varies from run to run, and a row with a single term has no order."""
    _, hip = _models(H, cuda_device, V=34)
    hip.train()
    res = []
    for x in (None, torch.empty(0)):
        data = _gapped_batches(unique_ids=True)["batch"]
        data.x = x
        with pytest.MonkeyPatch.context() as mp:
            calls = _record(mp)
            out, loss = _model_step(hip, data.to(cuda_device), "forward_loss")
            torch.cuda.synchronize()
        res.append((out, loss, {n: p.grad.clone() for n, p in hip.named_parameters()}, list(calls)))
    assert res[0][3] == res[1][3] and "qot_embed_bwd" in res[0][3]
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    differ = [n for n in res[0][2] if not torch.equal(res[0][2][n], res[1][2][n])]
    assert not differ, differ
