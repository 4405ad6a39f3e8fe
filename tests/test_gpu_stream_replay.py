"""Streamed replay (``harness.fit(..., stream=True)``): one captured step graph per batch shape, every batch staged on
the device into that shape's static buffers.

1. every topological case of ``helpers.TRAJECTORY_CASES`` against ``oracle.train_loop.train`` in fp64, with the bound
   (``TOL = 1e-4``), the metric and the printout of tests/test_gpu_training_trajectory.py (worst figures measured on an
   MI355X: DESIGN.md section 2, rows "streamed");
2. the run took the path: number of captured graphs, how the visits were issued, the staging kernel among the calls;
3. dropout on: the ``*_drop`` cases of 1. run against the oracle loop with the kernels' own masks restated
   (oracle/dropout.py; one draw per visit of a training batch, whichever way it is issued), which is the correctness
   check; bit-equality with the per-batch replay checks that the two modes agree;
4. the per-batch caches of ``graph.py`` do not survive a staging;
5. a node id outside the embedding table in a batch that is only ever replayed is reported at the end of its epoch.
"""
import pytest
import torch

import helpers as H
import stream_cases as SC
import test_gpu_training_trajectory as TT
from helpers import TOL

pytestmark = pytest.mark.gpu

TOPO_CASES = [n for n, c in H.TRAJECTORY_CASES.items() if c["kind"] == "topological"]


def _fit(name, device, tmp_path, monkeypatch, model_kw=None, graphs=None, **fit_kw):
    """``harness.fit`` of a case on a resident shard; returns ``(result dict as TT._fit_hip, History, call names)``."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import _lib, harness as Hn
    case = H.TRAJECTORY_CASES[name]
    ref_model = H.trajectory_oracle_model(case)
    hip = q.TopologicalGNN(**dict(case["model"], **(model_kw or {})))
    hip.load_state_dict(ref_model.state_dict(), strict=True)
    if case.get("dropout_seed") is not None:
        hip._qot_seed = case["dropout_seed"]
    data = q.PackedGraphs.from_data_list(H.trajectory_graphs(case) if graphs is None else graphs).to_device(device)
    made, calls = [], set()

    class _RecordingSGD(Hn.FusedSGD):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(Hn, "FusedSGD", _RecordingSGD)
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda nm, *a: (calls.add(nm), real(nm, *a))[1])
    best = str(tmp_path / "best_model.pth")
    hist = Hn.fit(hip, data, kind="topological", device=device, best_path=best, log=lambda s: None,
                  **dict(case["fit"], **fit_kw))
    torch.cuda.synchronize(device)
    assert len(made) == 1
    opt = made[0]
    assert opt.lr_dev is not None
    sizes = [p.numel() for p in opt.flat.params]
    got = {
        "loss": hist.loss, "val_loss": hist.val_loss, "r2": hist.r2, "val_r2": hist.val_r2,
        "best_val_r2": hist.best_val_r2, "epochs_run": hist.epochs_run, "stopped_early": hist.stopped_early,
        "skipped_graphs": hist.skipped_graphs,
        "state_dict": {k: v.detach().cpu() for k, v in hip.state_dict().items()},
        "best_state_dict": torch.load(best, map_location="cpu", weights_only=True),
        "momentum_buffers": [b.cpu() for b in opt.buf.split(sizes)],
        "param_names": [n for n, p in hip.named_parameters() if p.requires_grad],
        "dropout_draws": int(hip._qot_step),
    }
    return got, hist, calls


def _visits(case, epochs_run):
    """Batches a run of ``epochs_run`` epochs visits (training chunk + validation pass per epoch)."""
    from gnn_qot_estimation_amd import harness as Hn
    fit = case["fit"]
    tr, va, _ = Hn.split_ranges(case["data"]["count"])
    n = 0
    for epoch in range(epochs_run):
        chunk = Hn.epoch_chunk(epoch, len(tr), fit["chunk_fraction"])
        n += len(Hn.batch_ranges(range(chunk[0], chunk[-1] + 1), fit["batch_size"]))
        n += len(Hn.batch_ranges(va, fit["batch_size"]))
    return n


@pytest.mark.parametrize("name", TOPO_CASES)
def test_streamed_run_matches_the_fp64_loop(cuda_device, tmp_path, monkeypatch, name):
    got, hist, calls = _fit(name, cuda_device, tmp_path, monkeypatch, stream=True)
    TT._compare(name, "streamed", got)
    # the run took the path
    case = H.TRAJECTORY_CASES[name]
    rc = hist.replay_counts
    print(f"[streamed] {name}: {rc}")
    assert rc["graphs"] == SC.case_graph_count(case)
    assert rc["eager"] + rc["captured"] + rc["replayed"] == _visits(case, hist.epochs_run)
    assert rc["captured"] == rc["graphs"] and rc["eager"] <= rc["graphs"] + 1
    assert "qot_shard_stage" in calls


def test_graph_counts_of_both_replay_modes(cuda_device, tmp_path, monkeypatch):
    case = H.TRAJECTORY_CASES["topo_h16"]
    _, per_object, calls = _fit("topo_h16", cuda_device, tmp_path, monkeypatch, replay=True)
    assert per_object.replay_counts["graphs"] == 15                # 12 training batches + 3 validation batches
    rc = per_object.replay_counts
    assert rc["eager"] + rc["captured"] + rc["replayed"] == _visits(case, per_object.epochs_run)
    assert "qot_shard_stage" not in calls
    _, streamed, calls = _fit("topo_h16", cuda_device, tmp_path, monkeypatch, stream=True)
    assert streamed.replay_counts["graphs"] == 4 and "qot_shard_stage" in calls
    _, mixed, _ = _fit("topo_mixed_nodes", cuda_device, tmp_path, monkeypatch, stream=True)
    assert mixed.replay_counts["graphs"] == 7


def test_single_epoch_run_replays(cuda_device, tmp_path, monkeypatch):
    """What the per-batch replay cannot do: one epoch over fresh batches -- every batch visited once -- is replayed
    from the third batch of a shape on."""
    _, hist, _ = _fit("topo_h16", cuda_device, tmp_path, monkeypatch, stream=True, num_epochs=1, chunk_fraction=1.0)
    # 168 training graphs = 10 x 16 + 8: eager, capture, 8 replays; eager.  36 validation graphs = 2 x 16 + 4: eager, capture; eager
    rc = hist.replay_counts
    assert rc == {"eager": 4, "captured": 2, "replayed": 8, "graphs": 2}, rc


def test_dropout_run_is_bit_equal_to_the_per_batch_replay(cuda_device, tmp_path, monkeypatch):
    """Same seed, same kernels on the same values in the same order, counter-based masks: streamed and per-batch replay
    must agree bit for bit (parameters, momentum buffers, loss and R2 histories)."""
    runs = {}
    for mode, kw in (("streamed", dict(stream=True)), ("per_batch", dict(replay=True))):
        torch.manual_seed(1234)
        runs[mode] = _fit("topo_h64", cuda_device, tmp_path, monkeypatch, model_kw=dict(dropout_p=0.5), **kw)
    (a, ha, _), (b, hb, _) = runs["streamed"], runs["per_batch"]
    assert ha.replay_counts["graphs"] == 4 and hb.replay_counts["graphs"] == 15
    err = H.trajectory_errors(a, dict(b, param_names=a["param_names"]))
    worst = max(err.items(), key=lambda kv: kv[1])
    print(f"\n[streamed vs per-batch replay, dropout 0.5] worst {worst[0]} {worst[1]:.2e}")
    for key in ("loss", "val_loss", "r2", "val_r2"):
        assert a[key] == b[key], (key, a[key], b[key])
    assert a["best_val_r2"] == b["best_val_r2"] and a["epochs_run"] == b["epochs_run"]
    for which in ("state_dict", "best_state_dict"):
        for k, v in b[which].items():
            assert torch.equal(a[which][k], v), (which, k, H.rel_err(a[which][k], v))
    for n, x, y in zip(a["param_names"], a["momentum_buffers"], b["momentum_buffers"]):
        assert torch.equal(x, y), ("momentum", n, H.rel_err(x, y))
    # the masks were on: the same run without dropout ends elsewhere
    plain = TT._oracle("topo_h64")["loss"]
    assert max(abs(x - y) for x, y in zip(a["loss"], plain)) > 1e-3 * max(plain)


@pytest.mark.parametrize("name", ["topo_h16", "topo_mixed_nodes", "topo_h64"])
def test_slot_caches_do_not_survive_a_staging(cuda_device, name):
    """Different slices of one shape through one slot -- eager, capture (+ its replay), replay, replay: the outputs are
    the plain model's on ``device_batch`` of each slice.  With the slot's ``_qot_cache`` left alone the second slice would
    run on the first one's graph index / int32 copies."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    case = H.TRAJECTORY_CASES[name]
    ref_model = H.trajectory_oracle_model(case)
    hip = q.TopologicalGNN(**case["model"])
    hip.load_state_dict(ref_model.state_dict(), strict=True)
    hip.to(cuda_device).eval()
    shard = q.PackedGraphs.from_data_list(H.trajectory_graphs(case)).to_device(cuda_device)
    rep = Hn.StepReplayer(hip, "topological", 3, cuda_device, None, None, stream=True, shard=shard)
    sink = torch.zeros(16, 3, device=cuda_device)
    hook = hip.register_forward_hook(lambda m, args, out: sink.copy_(out))
    los = [0, 48, 96, 144, 0]                    # multiples of 3: one shape in the mixed case too
    ranges = [(lo, lo + 16) for lo in los]
    try:
        rep.begin_epoch(ranges, False)
        got = []
        for r in ranges:
            rep.run(r, False)
            got.append(sink.clone())
        rep.end_epoch()
    finally:
        hook.remove()
    assert rep.replay_counts() == {"eager": 1, "captured": 1, "replayed": 3, "graphs": 1}
    with torch.no_grad():
        for lo, out in zip(los, got):
            want = hip(shard.device_batch(lo, lo + 16))
            e = H.rel_err(out, want)
            print(f"[stale-cache guard] {name} lo {lo}: rel_err {e:.2e}, bitwise {torch.equal(out, want)}")
            assert e <= TOL, (name, lo, e)
    assert not torch.equal(got[0], got[1])       # the slices do differ


def test_bad_node_id_in_a_replayed_batch_is_reported(cuda_device, tmp_path, monkeypatch):
    """Graph 140 carries a node id == num_nodes.  It sits in the batch [132, 148) of the second chunk, which the streamed
    run reaches in epoch 1 when its shape's graph has long been captured: no host-side check ever sees it.  The staging
    kernel flags it (and stages the id as 0, so the step gathers nothing outside the table); ``fit(stream=True)`` raises
    ``IndexError`` at the END of that epoch, from the status word read with the epoch's statistics.  The eager loader
    raises the same error AT the step (``TopologicalGNN._check_node_ids`` reads the ids of every batch)."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    case = H.TRAJECTORY_CASES["topo_mixed_nodes"]
    graphs = H.trajectory_graphs(case)
    ids = graphs[140].node_ids.clone()
    ids[1] = case["model"]["num_nodes"]
    graphs[140].node_ids = ids
    sched = SC.case_schedules(case)["train"]
    shape = next(s for s, los in sched.items() if 132 in los)
    assert sched[shape].index(132) >= 2          # third or later batch of its shape: replayed
    logged = []
    hip = q.TopologicalGNN(**case["model"])
    shard = q.PackedGraphs.from_data_list(graphs).to_device(cuda_device)
    with pytest.raises(IndexError, match="index out of range"):
        Hn.fit(hip, shard, kind="topological", device=cuda_device, log=logged.append, stream=True, **case["fit"])
    torch.cuda.synchronize(cuda_device)
    assert sum(s.startswith("Epoch") for s in logged) == 1         # epoch 0 completed, epoch 1 raised at its end
    hip = q.TopologicalGNN(**case["model"])
    with pytest.raises(IndexError, match="index out of range"):
        Hn.fit(hip, q.PackedGraphs.from_data_list(graphs).pin(), kind="topological", device=cuda_device,
               log=lambda s: None, **case["fit"])
    torch.cuda.synchronize(cuda_device)
