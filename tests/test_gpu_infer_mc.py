"""GPU: Monte-Carlo dropout in one launch (``TopologicalPredictor.sample`` / ``qot_topological_infer_mc``).

Draw ``t`` of ``sample(first_step=s)`` is defined as the train-mode forward of the engine at dropout step ``s + t``, whose
masks are a pure function of ``(site seed, step, flat element index)``.  So every draw is checked element-wise against the
fp64 oracle (``oracle.sparse``) running the restated masks of ``oracle.dropout.topological_masks`` -- the way
``tests/test_gpu_dropout_oracle.py`` checks a train step -- at the project's ``TOL`` in ``helpers.rel_err``; nothing here
is statistical.  Seed ``dropout_cases.SEED`` (bit 63 set: the site seeds wrap), ``first_step = 2^33 + 1`` (the 64-bit step
multiply).  The batch per width: graphs of 2, 7 and 75 nodes, one of R + 1 rows (R: the NNConv tile height, so a tile
boundary falls inside a graph), a one-node graph and one with an in-degree-0 node and a repeated edge, in an order that
starts the later graphs at non-zero row offsets.  Every test prints its figures before it asserts (``pytest -s``)."""
import json
import os

import pytest
import torch

import dropout_cases as DC
import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import _lib, harness, infer, synthetic as S
from helpers import TOL, rel_err

pytestmark = pytest.mark.gpu

SEED = DC.SEED
FIRST = 2 ** 33 + 1
V = 80


def _models(device, H, O=3, D=4, p=0.5, seed=0, num_nodes=V):
    from oracle import sparse as Osp
    torch.manual_seed(seed)
    ref = Osp.TopologicalGNN(num_nodes, H, O, D, dropout_p=p).eval()
    with torch.no_grad():
        for w in ref.parameters():
            if w.dim() == 1 and w.abs().max() == 0:      # zero-init biases: make them matter
                w.uniform_(-0.1, 0.1)
    hip = q.TopologicalGNN(num_nodes, H, O, D, dropout_p=p)
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip._qot_seed = SEED
    return ref.double(), hip.to(device).eval()


def _graph(n, e, D=4, g=0):
    b = S.topological_batch(2, 1, n=n, e=e, edge_dim=D, first_graph=g)
    return q.Data(edge_index=b.edge_index, edge_attr=b.edge_attr, node_ids=torch.arange(n), num_nodes=n)


def _custom(n, src, dst, D=4, seed=0):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)
    return q.Data(edge_index=ei, edge_attr=torch.rand(ei.shape[1], D, generator=gen), node_ids=torch.arange(n), num_nodes=n)


def _batch(H, D=4):
    R = 32 if H == 16 else 16                            # csrc/infer_dev.hpp: infer_tile_rows
    graphs = [_graph(7, 12, D, 1),
              _custom(1, [], [], D, 3),                                           # a single node
              _graph(R + 1, 4 * R, D, 2),                                         # a tile boundary inside the graph
              _graph(2, 2, D, 0),
              _custom(5, [0, 1, 1, 1, 2, 3], [1, 2, 2, 2, 3, 0], D, 2),           # node 4: in-degree 0; 1 -> 2 three times
              _graph(75, 300, D, 4)]
    return q.Batch.from_data_list(graphs)


def _oracle(ref, batch, step, p, H, sites=("conv1", "conv2", "head")):
    from oracle import dropout as OD
    keep = OD.topological_masks(SEED, step, p, batch.num_nodes, batch.num_graphs, H)
    with torch.no_grad():
        return ref(DC.to_double(batch), keep={k: v for k, v in keep.items() if k in sites})


# ------------------------------------------------------------------ 1. the oracle under restated masks
@pytest.mark.parametrize("O", [1, 3])
@pytest.mark.parametrize("D", [1, 4])
@pytest.mark.parametrize("H", [16, 32, 64])
def test_draws_match_the_masked_oracle(cuda_device, H, D, O):
    ref, hip = _models(cuda_device, H, O, D)
    batch = _batch(H, D)
    pred = q.TopologicalPredictor(hip)
    mean, std, draws = pred.sample(batch.to(cuda_device), 3, p=0.5, seed=SEED, first_step=FIRST, return_samples=True)
    pred.check_status()
    assert tuple(draws.shape) == (3, batch.num_graphs, O) and draws.dtype == torch.float32
    assert draws.grad_fn is None and mean.grad_fn is None and std.grad_fn is None
    for t in range(3):
        e = rel_err(draws[t], _oracle(ref, batch, FIRST + t, 0.5, H))
        print(f"H {H} D {D} O {O} draw {t}: vs masked oracle {e:.3e}")
        assert e <= TOL, (t, e)
    assert not torch.equal(draws[0], draws[1]) and not torch.equal(draws[1], draws[2])


# ------------------------------------------------------------------ 2. the engine's own train mode
@pytest.mark.parametrize("H", [16, 64])
def test_a_draw_is_the_engines_train_mode_forward_at_that_step(cuda_device, H):
    _, hip = _models(cuda_device, H)
    db = _batch(H).to(cuda_device)
    draws = q.TopologicalPredictor(hip).sample(db, 3, first_step=FIRST, return_samples=True)[2]      # p, seed: the model's
    t = 1
    hip.train()
    hip._qot_step.fill_(FIRST + t - 1)                   # the counter is incremented, then snapshotted
    with torch.no_grad():
        own = hip(db)
    assert int(hip._qot_step) == FIRST + t
    e = rel_err(draws[t], own)
    print(f"H {H}: draw {t} vs train-mode forward {e:.3e}")
    assert e <= TOL, e


# ------------------------------------------------------------------ 3. p = 0
@pytest.mark.parametrize("H", [16, 32, 64])
def test_p_zero_is_the_eval_kernel_bit_for_bit(cuda_device, H):
    _, hip = _models(cuda_device, H, p=0.5)
    db = _batch(H).to(cuda_device)
    pred = q.TopologicalPredictor(hip)
    want = pred(db)
    mean, std, draws = pred.sample(db, 3, p=0.0, first_step=FIRST, return_samples=True)
    for t in range(3):
        assert torch.equal(draws[t], want), t
    assert torch.equal(std, torch.zeros_like(std))
    hip.dropout.p = hip.mlp[2].p = 0.0                   # ... and through the model's own probabilities
    assert torch.equal(pred.sample(db, 2, return_samples=True)[2][1], want)


# ------------------------------------------------------------------ 4. chunks, steps, seeds
def test_draws_do_not_depend_on_chunk_or_count_and_are_reproducible(cuda_device):
    _, hip = _models(cuda_device, 32)
    db = _batch(32).to(cuda_device)
    pred = q.TopologicalPredictor(hip)
    kw = dict(p=0.5, seed=SEED, return_samples=True)
    by_chunk = [pred.sample(db, 5, first_step=FIRST, chunk=c, **kw)[2] for c in (1, 2, 5)]
    assert torch.equal(by_chunk[0], by_chunk[1]) and torch.equal(by_chunk[0], by_chunk[2])
    assert torch.equal(pred.sample(db, 5, first_step=FIRST, **kw)[2], by_chunk[0])                  # chunk=None
    four = pred.sample(db, 4, first_step=FIRST, **kw)[2]
    assert torch.equal(four, by_chunk[0][:4])
    assert torch.equal(four[2:], pred.sample(db, 2, first_step=FIRST + 2, **kw)[2])
    assert torch.equal(four, pred.sample(db, 4, first_step=FIRST, **kw)[2])
    other = pred.sample(db, 4, first_step=FIRST, p=0.5, seed=SEED + 1, return_samples=True)[2]
    assert not torch.equal(other, four)
    pred.check_status()


# ------------------------------------------------------------------ 5. statistics, separate probabilities
def test_mean_and_std_are_torchs_and_the_sites_have_their_own_probability(cuda_device):
    H = 16
    ref, hip = _models(cuda_device, H)
    batch = _batch(H)
    db = batch.to(cuda_device)
    pred = q.TopologicalPredictor(hip)
    mean, std, draws = pred.sample(db, 6, first_step=FIRST, return_samples=True)
    assert torch.equal(mean, draws.mean(0)) and torch.equal(std, draws.std(0, unbiased=True))
    assert tuple(mean.shape) == tuple(std.shape) == (batch.num_graphs, 3) and bool((std > 0).all())
    m2, s2 = pred.sample(db, 6, first_step=FIRST)
    assert torch.equal(m2, mean) and torch.equal(s2, std)
    # p_conv = 0, p_head = 0.5, from the model's modules: only the read-out's mask acts
    hip.dropout.p, ref.dropout.p = 0.0, 0.0
    assert hip.mlp[2].p == 0.5
    head_only = pred.sample(db, 3, first_step=FIRST, return_samples=True)[2]
    assert torch.equal(head_only, pred.sample(db, 3, p=(0.0, 0.5), first_step=FIRST, return_samples=True)[2])
    for t in range(3):
        e = rel_err(head_only[t], _oracle(ref, batch, FIRST + t, 0.5, H, sites=("head",)))
        print(f"head-only draw {t}: vs oracle {e:.3e}")
        assert e <= TOL, (t, e)
    assert not torch.equal(head_only[0], draws[0])


# ------------------------------------------------------------------ 6. purity
def test_sample_leaves_the_model_and_the_predictor_alone(cuda_device):
    H = 32
    _, hip = _models(cuda_device, H)
    batch = _batch(H)
    db = batch.to(cuda_device)
    y = torch.rand(batch.num_graphs, 3, generator=torch.Generator().manual_seed(9)).to(cuda_device)
    pred = q.TopologicalPredictor(hip)
    start = {k: v.detach().clone() for k, v in hip.state_dict().items()}

    def train_step():
        hip.train()
        opt = torch.optim.SGD(hip.parameters(), lr=0.1)
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.smooth_l1_loss(hip(db), y).backward()
        opt.step()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in hip.state_dict().items()}

    plain = train_step()
    hip.load_state_dict(start, strict=True)
    hip._qot_step.zero_()
    for mode in (False, True):
        hip.train(mode)
        before = pred(db).clone()
        pred.sample(db, 4)
        assert hip.training is mode and int(hip._qot_step) == 0
        for k, v in hip.state_dict().items():
            assert torch.equal(v, start[k]), k
        assert torch.equal(pred(db), before)
    after_sample = train_step()
    assert int(hip._qot_step) == 1
    for k in plain:
        assert torch.equal(after_sample[k], plain[k]), k
    assert any(not torch.equal(plain[k], start[k]) for k in plain)


# ------------------------------------------------------------------ 7. parameter following
def test_sample_follows_an_in_place_update(cuda_device):
    H = 32
    ref, hip = _models(cuda_device, H)
    batch = _batch(H)
    db = batch.to(cuda_device)
    pred = q.TopologicalPredictor(hip)
    old = pred.sample(db, 2, first_step=FIRST, return_samples=True)[2]
    with torch.no_grad():
        hip.conv2.lin.weight.mul_(1.5)
        ref.conv2.lin.weight.mul_(1.5)
    new = pred.sample(db, 2, first_step=FIRST, return_samples=True)[2]
    assert rel_err(new, old) > TOL
    for t in range(2):
        e = rel_err(new[t], _oracle(ref, batch, FIRST + t, 0.5, H))
        print(f"after the update, draw {t}: vs masked oracle {e:.3e}")
        assert e <= TOL, (t, e)


# ------------------------------------------------------------------ 8. refusals and status
def test_refusals_name_the_condition(cuda_device):
    _, hip = _models(cuda_device, 16, num_nodes=130)
    pred = q.TopologicalPredictor(hip)
    db = q.Batch.from_data_list([_graph(10, 20), _graph(12, 30, 4, 1)]).to(cuda_device)
    for bad in (1, 0, 4097, 2.0, True):
        with pytest.raises(ValueError, match="samples must be"):
            pred.sample(db, bad)
    for bad in (1.0, -0.1, 1.5, (0.5, 1.0), float("nan")):
        with pytest.raises(ValueError, match=r"p must lie in \[0, 1\)"):
            pred.sample(db, 4, p=bad)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="chunk must be"):
            pred.sample(db, 4, chunk=bad)
    for bad in (-1, 2 ** 63 - 3):
        with pytest.raises(ValueError, match="first_step must be"):
            pred.sample(db, 4, first_step=bad)
    assert torch.isfinite(pred.sample(db, 4, first_step=2 ** 63 - 4, p=0.5)[0]).all()
    # everything __call__ refuses
    with pytest.raises(ValueError, match="129 nodes"):
        pred.sample(q.Batch.from_data_list([_graph(10, 20), _graph(129, 300, 4, 1)]).to(cuda_device), 4)
    withx = q.Batch.from_data_list([_graph(10, 20)]).to(cuda_device)
    withx.x = torch.rand(10, 16, device=cuda_device)
    with pytest.raises(ValueError, match="data.x is given"):
        pred.sample(withx, 4)
    # the sampling kernel's own edge cap: lower than the eval kernel's, and named
    cap, eval_cap = infer.mc_edge_cap(100, 16, 4), infer.edge_cap(100, 16, 4)
    assert 0 < cap < eval_cap and cap == _lib.load().qot_topological_infer_mc_max_edges(100, 16, 4)

    def with_edges(e):
        g = _graph(100, e + 2 + e % 2, 4, 2)
        return q.Batch.from_data_list([q.Data(edge_index=g.edge_index[:, :e].contiguous(), edge_attr=g.edge_attr[:e].contiguous(),
                                              node_ids=torch.arange(100), num_nodes=100)]).to(cuda_device)
    over = with_edges(cap + 1)
    with pytest.raises(ValueError, match=f"{cap + 1} edges is above the sampling edge cap {cap}"):
        pred.sample(over, 4)
    assert torch.isfinite(pred(over)).all()              # ... which the eval kernel still takes
    assert torch.isfinite(pred.sample(with_edges(cap), 4, p=0.5)[0]).all()
    # node ids outside the table
    bad = _graph(12, 40, 4, 34)
    bad.node_ids = torch.arange(12) + 119                # 130 >= num_nodes
    with pytest.raises(IndexError):
        pred.sample(q.Batch.from_data_list([_graph(10, 20), bad]).to(cuda_device), 4)
    pred.check_status()
    hip.cpu()
    with pytest.raises(ValueError, match="CPU"):
        pred.sample(db, 4)


def test_edge_outside_its_graph_is_flagged_and_all_its_rows_nan(cuda_device):
    _, hip = _models(cuda_device, 16)
    pred = q.TopologicalPredictor(hip)
    graphs = [_graph(7, 12, 4, 1), _graph(9, 20, 4, 2), _graph(5, 8, 4, 3)]
    kw = dict(p=0.5, seed=SEED, first_step=FIRST, chunk=2, return_samples=True)
    want = pred.sample(q.Batch.from_data_list(graphs).to(cuda_device), 5, **kw)[2]
    pred.check_status()
    bad = q.Batch.from_data_list(graphs)
    bad.edge_index[0, int(bad.edge_ptr[1])] = int(bad.ptr[1]) - 1      # a node of graph 0: inside [0, N), outside graph 1
    got = pred.sample(bad.to(cuda_device), 5, **kw)[2]
    with pytest.raises(_lib.QotError, match="status 1"):
        pred.check_status()
    pred.check_status()                                  # (read and cleared)
    assert torch.isnan(got[:, 1]).all()
    assert torch.equal(got[:, 0], want[:, 0]) and torch.equal(got[:, 2], want[:, 2])


# ------------------------------------------------------------------ 9. harness and command line
def test_evaluate_returns_descaled_stds_beside_unchanged_predictions(cuda_device):
    data = []
    for g in range(40):
        b = S.topological_batch(2, 1, n=12, e=30, first_graph=g)
        y = b.edge_attr[:, :3].mean(0, keepdim=True)
        data.append(q.Data(edge_index=b.edge_index, edge_attr=b.edge_attr, node_ids=b.node_ids, y=y, num_nodes=12))
    shard = q.PackedGraphs.from_data_list(data)
    _, hip = _models(cuda_device, 16, num_nodes=12)
    kw = dict(kind="topological", batch_size=16, output_dim=3, device=cuda_device, fused=True)
    m0, t0, p0, s0 = harness.evaluate(hip, shard, return_predictions=True, **kw)
    m1, t1, p1, s1, std = harness.evaluate(hip, shard, return_predictions=True, mc_samples=4, mc_seed=SEED, **kw)
    assert m1 == m0 and torch.equal(t1, t0) and torch.equal(p1, p0) and s1 == s0
    assert tuple(std.shape) == (40, 3) and std.dtype == torch.float64 and bool((std > 0).all())
    m2, std2 = harness.evaluate(hip, shard, mc_samples=4, mc_seed=SEED, **kw)
    assert m2 == m0 and torch.equal(std2, std)
    # descaled by the range only: the first batch's stds times (max - min), no offset
    pred = q.TopologicalPredictor(hip)
    first = q.Batch.from_data_list(data[:16]).to(cuda_device)
    raw = pred.sample(first, 4, seed=SEED)[1].cpu().double()
    span = torch.tensor([33.49 - 12.47, 29.98 - 8.96, 1.98e-2 - 1.70e-12], dtype=torch.float64)
    assert rel_err(std[:16], raw * span) <= 1e-12
    assert bool((harness.evaluate(hip, shard, mc_samples=4, mc_p=0.0, **kw)[1] == 0).all())
    with pytest.raises(ValueError, match="needs fused=True"):
        harness.evaluate(hip, shard, kind="topological", device=cuda_device, mc_samples=4)


def test_cli_writes_the_std_file_only_when_asked(tmp_path, cuda_device):
    from gnn_qot_estimation_amd import test as test_cli, to_graph as TG
    from gnn_qot_estimation_amd.train import open_dataset
    ns = TG.synthetic_network_status(40, seed=8)
    data_dir = TG.store_graphs(ns, "topological", str(tmp_path / "networkx_graphs_topological"))
    root = str(tmp_path / "topological_training")
    dataset, meta = open_dataset("topological", data_dir, True, cuda_device)
    D = int(meta.get("edge_dim", dataset.edge_attr.shape[1]))
    torch.manual_seed(0)
    model = q.TopologicalGNN(75, 16, 3, D)
    os.makedirs(os.path.join(root, "models"))
    harness.save_checkpoint(os.path.join(root, "models", "model_0.pth"), model,
                            {"num_nodes": 75, "hidden_channels": 16, "output_dim": 3, "edge_dim": D, "FEATURES": None})
    args = ["--kind", "topological", "--data", data_dir, "--root", root, "--batch-size", "4", "--fused"]
    plain = test_cli.main(args)
    listing = sorted(os.listdir(plain))
    assert listing == ["results_metrics.json", "y_pred_descaled.json", "y_true_descaled.json"]
    kept = {n: open(os.path.join(plain, n)).read() for n in listing}
    folder = test_cli.main(args + ["--mc-samples", "4", "--mc-p", "0.5"])
    assert sorted(os.listdir(folder)) == ["results_metrics.json", "y_pred_descaled.json", "y_pred_std_descaled.json",
                                          "y_true_descaled.json"]
    for n in listing:                                    # the scored predictions stay the eval-mode ones: same bytes
        assert open(os.path.join(folder, n)).read() == kept[n], n
    std = torch.tensor(json.load(open(os.path.join(folder, "y_pred_std_descaled.json"))))
    y_pred = torch.tensor(json.load(open(os.path.join(folder, "y_pred_descaled.json"))))
    assert std.shape == y_pred.shape and std.shape[1] == 3 and bool((std > 0).all())
    with pytest.raises(SystemExit):
        test_cli.main(["--kind", "topological", "--data", data_dir, "--root", root, "--mc-samples", "4"])
