"""``oracle.train_loop``: the plain restatement of the reference's training loops that whole HIP training runs are
compared with (tests/test_gpu_training_trajectory.py).  Pinned here without a GPU:

* by hand: learning-rate list, chunk indices, the loss denominator, the patience counter, R2;
* against ``harness.run_epoch`` on the CPU oracle model (torch's SGD behind a ``step()`` shim, ``harness.step_lr`` /
  ``epoch_chunk`` / ``split_ranges`` driving it): two independent statements of the loop, the same torch arithmetic;
* conditioning of every trajectory case: fp32 and fp64 runs of the oracle loop agree to ``TOL / 10`` in the metric the
  GPU test uses, and every ``val_r2 > best`` decision has a margin no implementation within ``TOL`` can cross.
"""
import functools
import math

import pytest
import torch

import helpers as H
from helpers import TOL
from oracle import train_loop as TL


@functools.lru_cache(maxsize=None)
def _run(name, dtype):
    return H.oracle_trajectory(H.TRAJECTORY_CASES[name], dtype)


# --------------------------------------------------------------------------- by hand
def test_split_and_chunk_indices():
    tr, va, te = TL.split(96)
    assert (tr[0], tr[-1], va[0], va[-1], te[0], te[-1]) == (0, 66, 67, 80, 81, 95)
    assert len(tr) == 67 and len(va) == 14 and len(te) == 15
    # 67 training graphs in two chunks of 33: graph 66 is never visited, epoch 2 is epoch 0 again
    assert TL.chunk_indices(0, 67, 0.5) == list(range(0, 33))
    assert TL.chunk_indices(1, 67, 0.5) == list(range(33, 66))
    assert TL.chunk_indices(2, 67, 0.5) == list(range(0, 33))
    # int(1 / 0.3) = 3 chunks of 22
    assert [TL.chunk_indices(e, 67, 0.3)[0] for e in range(4)] == [0, 22, 44, 0]
    assert TL.chunk_indices(2, 67, 0.3) == list(range(44, 66))
    # the reference's numbers: 10 chunks of 105 out of 1050
    assert TL.chunk_indices(13, 1050, 0.10) == list(range(315, 420))


def test_learning_rate_list_follows_steplr_stepped_after_each_epoch():
    for name in ("topo_h16", "lp_c8_skip_mid", "topo_early_stop"):
        fit = H.TRAJECTORY_CASES[name]["fit"]
        res = _run(name, torch.float32)
        assert len(res["lr"]) == res["epochs_run"]
        want = [fit["lr"] * fit["gamma"] ** (e // fit["step_size"]) for e in range(res["epochs_run"])]
        assert res["lr"] == pytest.approx(want, rel=1e-15)
        assert len(set(res["lr"])) > 1                       # a boundary is crossed


def test_early_stopping_counter_on_scripted_sequences():
    def play(seq, patience):
        st = TL.EarlyStopping(patience)
        for e, v in enumerate(seq):
            if st.update(e, v)[1]:
                return e, st.best_epoch, st.best
        return None, st.best_epoch, st.best
    assert play([0.1, 0.3, 0.2, 0.25, 0.9], 2) == (3, 1, 0.3)
    assert play([0.1, 0.3, 0.2, 0.25, 0.9], 3) == (None, 4, 0.9)
    assert play([0.5, 0.5, 0.5], 2) == (2, 0, 0.5)                       # a tie is not an improvement
    assert play([0.5, float("nan"), float("nan")], 2) == (2, 0, 0.5)     # neither is NaN
    assert play([0.2, 0.1, 0.3, 0.1, 0.1], 2) == (4, 2, 0.3)             # an improvement resets the counter
    assert play([-5.0], 1) == (None, 0, -5.0)


def test_early_stopping_case_stops_where_the_counter_says_and_keeps_the_best_epoch():
    case = H.TRAJECTORY_CASES["topo_early_stop"]
    seen = {}
    model = H.trajectory_oracle_model(case)
    res = TL.train(model, H.trajectory_graphs(case), case["kind"], dtype=torch.float64,
                   on_epoch=lambda e, m: seen.__setitem__(e, {k: v.clone() for k, v in m.state_dict().items()}),
                   **case["fit"])
    # replay the decisions from the recorded sequence
    st, stop_at = TL.EarlyStopping(case["fit"]["patience"]), None
    for e, v in enumerate(res["val_r2"]):
        if st.update(e, v)[1]:
            stop_at = e
            break
    assert res["stopped_early"] and stop_at == res["epochs_run"] - 1 == len(res["val_r2"]) - 1
    assert res["epochs_run"] < case["fit"]["num_epochs"]
    assert res["best_epoch"] == st.best_epoch < res["epochs_run"] - 1 and res["best_val_r2"] == st.best
    for k, v in res["best_state_dict"].items():
        assert torch.equal(v, seen[res["best_epoch"]][k]), k
    assert any(not torch.equal(v, res["state_dict"][k]) for k, v in res["best_state_dict"].items())


class _Stub(torch.nn.Module):
    """Three parameters: predicts ``w`` for every LUT node, raises like ``LightpathGNN`` when there is none."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.2, 0.5, 3.0]))

    def forward(self, data):
        mask = data.x[:, 1] == 1.0
        if not mask.any():
            raise ValueError("No LUT node found in the batch.")
        return data.x[mask][:, :1] * 0.0 + self.w, data.batch[mask]


def test_loss_denominator_counts_skipped_graphs():
    case = H.TRAJECTORY_CASES["lp_c8_skip_mid"]
    graphs = H.trajectory_graphs(case)
    res = TL.train(_Stub(), graphs, "lightpath", dtype=torch.float64, batch_size=4, num_epochs=2, patience=10, lr=0.0,
                   momentum=0.9, step_size=3, gamma=0.5, chunk_fraction=0.5, output_dim=3)
    w = torch.tensor([0.2, 0.5, 3.0]).double()          # the stub's fp32 parameter, cast as ``train`` casts it

    def graph_loss(g):                   # SmoothL1 (beta 1), mean over the three outputs of one graph
        d = (w - graphs[g].y.double().view(3)).abs()
        return float(torch.where(d < 1.0, 0.5 * d * d, d - 0.5).mean())
    # lr = 0: the model never moves; a batch's mean loss times its rows is the sum of its graphs' losses
    chunk0 = [g for g in range(0, 33) if not 8 <= g < 12]
    assert res["loss"][0] == pytest.approx(sum(graph_loss(g) for g in chunk0) / 33, rel=1e-12)       # 33, not 29
    assert res["loss"][1] == pytest.approx(sum(graph_loss(g) for g in range(33, 66)) / 33, rel=1e-12)
    assert res["val_loss"][0] == pytest.approx(sum(graph_loss(g) for g in range(67, 81)) / 14, rel=1e-12)
    assert res["skipped_graphs"] == 4 and res["epochs_run"] == 2


def test_r2_by_hand_and_against_sklearn():
    y = torch.tensor([[1.0, 2.0, 5.0], [2.0, 2.0, 5.0], [3.0, 2.0, 5.0], [6.0, 2.0, 5.0]])
    p = torch.tensor([[1.0, 2.0, 5.0], [2.0, 2.0, 5.5], [4.0, 2.0, 5.0], [5.0, 2.0, 5.0]])
    # column 0: mean 3, sst = 4 + 1 + 0 + 9 = 14, sse = 2;  column 1: constant and hit -> 1;  column 2: constant, missed -> 0
    assert TL.r2_uniform(y, p) == pytest.approx(((1 - 2 / 14) + 1.0 + 0.0) / 3, rel=1e-15)
    assert math.isnan(TL.r2_uniform(y[:0], p[:0]))
    try:
        from sklearn.metrics import r2_score
    except ImportError:
        return                      # only this comparison needs sklearn
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(50, 3, generator=g, dtype=torch.float64), torch.rand(50, 3, generator=g, dtype=torch.float64)
    assert TL.r2_uniform(a, b) == pytest.approx(r2_score(a.numpy(), b.numpy(), multioutput="uniform_average"), rel=1e-12)
    assert TL.r2_uniform(y, p) == pytest.approx(r2_score(y.double().numpy(), p.double().numpy(), multioutput="uniform_average"), rel=1e-12)


# --------------------------------------------------------------------------- harness.run_epoch on the CPU
class _TorchSGD:
    """``run_epoch`` only calls ``opt.step()``; on the CPU the fused HIP update is replaced by torch's."""

    def __init__(self, flat, lr, momentum):
        self.inner = torch.optim.SGD([flat.leaf], lr=lr, momentum=momentum)

    def step(self):
        self.inner.step()


@pytest.mark.parametrize("name", ["topo_h16", "topo_mixed_nodes", "lp_c8_skip_mid", "lp_c8_skip_last", "lp_c8_layers3"])
def test_harness_run_epoch_on_cpu_equals_the_oracle_loop(name):
    """Same torch arithmetic on identical batches through two independent statements of the loop: equal bit for bit
    (R2: streaming sums against two passes, both fp64 -- 1e-9)."""
    from gnn_qot_estimation_amd import harness as Hn
    from gnn_qot_estimation_amd.dp import FlatModel
    case = H.TRAJECTORY_CASES[name]
    fit = case["fit"]
    ref = _run(name, torch.float32)
    graphs = H.trajectory_graphs(case)
    model = H.trajectory_oracle_model(case)
    flat = FlatModel(model)
    opt = _TorchSGD(flat, fit["lr"], fit["momentum"])
    crit = torch.nn.SmoothL1Loss()
    tr, va, _ = Hn.split_ranges(len(graphs))
    kw = dict(kind=case["kind"], batch_size=fit["batch_size"], out_dim=fit["output_dim"], device="cpu", criterion=crit)
    skipped = 0
    for epoch in range(ref["epochs_run"]):
        chunk = Hn.epoch_chunk(epoch, len(tr), fit["chunk_fraction"])
        opt.inner.param_groups[0]["lr"] = Hn.step_lr(fit["lr"], epoch, fit["step_size"], fit["gamma"])
        t = Hn.run_epoch(model, graphs, range(tr[0] + chunk[0], tr[0] + chunk[-1] + 1), flat=flat, opt=opt, **kw)
        v = Hn.run_epoch(model, graphs, va, **kw)
        skipped += t["skipped"]
        assert t["avg_loss"] == ref["loss"][epoch] and v["avg_loss"] == ref["val_loss"][epoch], epoch
        assert t["r2"] == pytest.approx(ref["r2"][epoch], rel=1e-9, abs=1e-9)
        assert v["r2"] == pytest.approx(ref["val_r2"][epoch], rel=1e-9, abs=1e-9)
    assert skipped == ref["skipped_graphs"]
    sd = model.state_dict()
    assert list(sd.keys()) == list(ref["state_dict"].keys())
    for k, v in ref["state_dict"].items():
        assert torch.equal(sd[k], v), k


# --------------------------------------------------------------------------- conditioning of the trajectory cases
@pytest.mark.parametrize("name", list(H.TRAJECTORY_CASES))
def test_trajectory_case_is_well_conditioned(name):
    """fp32 rounding alone moves no compared quantity by more than TOL / 10 (measured: at most 4e-6)."""
    case = H.TRAJECTORY_CASES[name]
    r32, r64 = _run(name, torch.float32), _run(name, torch.float64)
    H.assert_trajectory_counters(r32, r64)
    assert r32["best_epoch"] == r64["best_epoch"]
    err = H.trajectory_errors(r32, r64, H.trajectory_analytic_zero(case, r64["param_names"]))
    worst = max(err, key=err.get)
    print(f"{name}: worst fp32-vs-fp64 {worst} {err[worst]:.2e}")
    assert err[worst] <= TOL / 10, (worst, err[worst])
    # every early-stopping decision: both sides are within TOL * max(1, |r2|) of these numbers, so a margin above
    # twice that cannot flip; 10x is asked of every case, 100x of the early-stopping case
    best = float("-inf")
    for v in r64["val_r2"]:
        if best > float("-inf"):
            need = (100 if name == "topo_early_stop" else 10) * TOL * max(1.0, abs(v), abs(best))
            assert abs(v - best) >= need, (name, v, best)
        best = max(best, v)
    if name == "topo_early_stop":
        assert r64["stopped_early"] and r64["epochs_run"] < case["fit"]["num_epochs"]
    else:
        assert not r64["stopped_early"] and r64["epochs_run"] == case["fit"]["num_epochs"]
    if case["kind"] == "lightpath":
        assert r64["skipped_graphs"] > 0
