"""Whole training runs: ``harness.fit`` on the HIP models against ``oracle.train_loop.train`` in fp64 on the CPU.

One forward and one backward of every kernel are pinned elsewhere; what carries over from step to step is pinned here:
the fused SGD update through the flat buffer, StepLR through the device-side learning rate, BatchNorm running statistics
(skipped batches included), per-step derived copies of the weights, ragged last batches, the loss average, early stopping
and the best-model file.  Every case (``helpers.TRAJECTORY_CASES``; conditioning pinned in
tests/test_oracle_train_loop_cpu.py) runs under the three ways of feeding ``fit``: the eager loader, a resident shard
without replay, a resident shard with captured and replayed steps.  Everything is compared with ``TOL = 1e-4`` in the
metric of ``helpers.trajectory_errors``.

The ``*_drop`` cases train with dropout ON (p = 0.5): the oracle loop runs the kernels' own counter-based masks, restated
by ``oracle/dropout.py`` from the base seed the HIP model is given (``_qot_seed``) and the number of the train-mode forward.
Every visit of a training batch -- eager, the one replay that follows its capture (a capture records, it does not
execute), every later replay -- is exactly one draw, and evaluation draws nothing, so the step sequence of all three
modes is 1, 2, 3, ... in batch order; the run's final ``_qot_step`` must equal the oracle loop's draw count.

Worst HIP-vs-fp64 figures measured on an MI355X are listed per case in DESIGN.md section 2.
"""
import functools

import pytest
import torch

import helpers as H
from helpers import TOL

pytestmark = pytest.mark.gpu

MODES = ("host", "resident_eager", "resident_replay")


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return H.oracle_trajectory(H.TRAJECTORY_CASES[name], torch.float64)


def _fit_hip(name, mode, device, tmp_path, monkeypatch):
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    case = H.TRAJECTORY_CASES[name]
    ref_model = H.trajectory_oracle_model(case)
    hip = (q.TopologicalGNN if case["kind"] == "topological" else q.LightpathGNN)(**case["model"])
    hip.load_state_dict(ref_model.state_dict(), strict=True)
    if case.get("dropout_seed") is not None:
        hip._qot_seed = case["dropout_seed"]
    graphs = H.trajectory_graphs(case)
    if mode == "host":
        # the eager loader's two sources: a pinned shard (DMA'd slices) and a plain host list (collated per batch)
        data = q.PackedGraphs.from_data_list(graphs).pin() if case["kind"] == "topological" else graphs
        replay = None
    else:
        data = q.PackedGraphs.from_data_list(graphs).to_device(device)
        replay = mode == "resident_replay"
    made = []

    class _RecordingSGD(Hn.FusedSGD):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(Hn, "FusedSGD", _RecordingSGD)
    best = str(tmp_path / "best_model.pth")
    hist = Hn.fit(hip, data, kind=case["kind"], device=device, best_path=best, log=lambda s: None, replay=replay,
                  **case["fit"])
    torch.cuda.synchronize(device)
    assert len(made) == 1
    opt = made[0]
    assert (opt.lr_dev is not None) == (mode == "resident_replay")          # the run took the path it was meant to take
    sizes = [p.numel() for p in opt.flat.params]
    return {
        "loss": hist.loss, "val_loss": hist.val_loss, "r2": hist.r2, "val_r2": hist.val_r2,
        "best_val_r2": hist.best_val_r2, "epochs_run": hist.epochs_run, "stopped_early": hist.stopped_early,
        "skipped_graphs": hist.skipped_graphs,
        "state_dict": {k: v.detach().cpu() for k, v in hip.state_dict().items()},
        "best_state_dict": torch.load(best, map_location="cpu", weights_only=True),
        "momentum_buffers": [b.cpu() for b in opt.buf.split(sizes)],
        "param_names": [n for n, p in hip.named_parameters() if p.requires_grad],
        "dropout_draws": int(getattr(hip, "_qot_step", 0)),
    }


def _compare(name, mode, got):
    case = H.TRAJECTORY_CASES[name]
    ref = _oracle(name)
    assert got["param_names"] == ref["param_names"]
    err = H.trajectory_errors(got, ref, H.trajectory_analytic_zero(case, ref["param_names"]))
    groups = {}
    for k, v in err.items():
        g = k.split("[")[0].split(":")[0]
        if g == "state_dict" and "running_" in k:
            g = "running_stats"
        if v >= groups.get(g, ("", -1.0))[1]:
            groups[g] = (k, v)
    print(f"\n[trajectory] {name} / {mode}: " + ", ".join(f"{g} {v:.2e}" for g, (k, v) in sorted(groups.items())))
    H.assert_trajectory_counters(got, ref)
    assert got["dropout_draws"] == ref["dropout_draws"], (got["dropout_draws"], ref["dropout_draws"])
    if case.get("dropout_seed") is not None:
        assert ref["dropout_draws"] > 0
    bad = {k: v for k, v in err.items() if not v <= TOL}
    assert not bad, (name, mode, sorted(bad.items(), key=lambda kv: -kv[1])[:8])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(H.TRAJECTORY_CASES))
def test_training_run_matches_the_fp64_loop(cuda_device, tmp_path, monkeypatch, name, mode):
    _compare(name, mode, _fit_hip(name, mode, cuda_device, tmp_path, monkeypatch))


@pytest.mark.parametrize("mode", ("resident_eager", "resident_replay"))
def test_training_run_per_destination_transformerconv(cuda_device, tmp_path, monkeypatch, mode):
    """The H = 64 run once more with the graph form switched off: the per-destination TransformerConv kernels (and the
    projected table they read) see updated parameters on every step too."""
    from gnn_qot_estimation_amd import _lib
    monkeypatch.setenv("QOT_NO_TCONV_GRAPH", "1")
    calls = set()
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.add(name), real(name, *a))[1])
    got = _fit_hip("topo_h64", mode, cuda_device, tmp_path, monkeypatch)
    assert any(c.startswith("qot_tconv_fwd") for c in calls), sorted(calls)
    assert "qot_tconv_fwd_graph" not in calls and "qot_tconv_bwd_graph" not in calls
    _compare("topo_h64", mode + " (per-destination)", got)
