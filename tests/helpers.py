"""Shared helpers for parity tests: relative error, weight sharing oracle <-> HIP modules."""
import torch


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a-b| / max(|b|_inf, tiny): the <=1e-4 'rel fp32' bar of BASELINE.json's north_star."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if a.numel() == 0 and b.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


TOL = 1e-4  # BASELINE.json north_star: outputs match the reference forward to <=1e-4 rel fp32


def grad_compare(ref, hip, analytic_zero=()):
    """Every parameter gradient of ``hip`` against ``ref``'s; returns the worst error.

    A gradient that is analytically zero (e.g. lin_key.bias: softmax is shift invariant) is pure rounding noise in both
    implementations, so each parameter's error is taken relative to max(its own magnitude, 1e-3 x the largest gradient
    in the model); a name in ``analytic_zero`` relative to the largest gradient."""
    worst = 0.0
    rp = dict(ref.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in rp.values() if p.grad is not None)
    for name, p in hip.named_parameters():
        if rp[name].grad is None:                        # unused on both sides (the embedding when data.x is given)
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        a, b = p.grad.detach().double().cpu(), rp[name].grad.detach().double()
        floor = gmax if name in analytic_zero else 1e-3 * gmax
        e = float((a - b).abs().max() / max(float(b.abs().max()), floor))
        worst = max(worst, e)
        assert e <= TOL, (name, e)
    return worst


# --------------------------------------------------------------------------- whole training runs
# The cases of tests/test_gpu_training_trajectory.py (HIP ``harness.fit`` against ``oracle.train_loop.train`` in fp64)
# and of tests/test_oracle_train_loop_cpu.py (conditioning: the oracle loop in fp32 against itself in fp64 must stay
# within TOL / 10 in the same metric, else the case is chaotic and gets replaced -- never a looser bound).
#
# Two chunks per run (``chunk_fraction`` 0.5) and 8 epochs: every training batch is visited four times (eager, capture,
# two replays in the replayed runs); ``step_size`` 2 (3 for lightpath) puts StepLR boundaries inside the replayed epochs.
# The topological runs of 240 graphs are the 7-epoch run of the existing replay test plus one epoch, so that the second
# chunk gets its fourth visit too.
def _topo_fit(**kw):
    return dict(dict(batch_size=16, num_epochs=8, patience=10, lr=0.05, momentum=0.9, step_size=2, gamma=0.5,
                     chunk_fraction=0.5, output_dim=3), **kw)


def _lp_fit(**kw):
    return dict(dict(batch_size=4, num_epochs=8, patience=10, lr=0.1, momentum=0.9, step_size=3, gamma=0.5,
                     chunk_fraction=0.5, output_dim=3), **kw)


def _topo_model(H, V=12, D=4, p=0.0):
    return dict(num_nodes=V, hidden_channels=H, out_channels=3, edge_dim=D, dropout_p=p)


def _lp_model(C, layers=1):
    return dict(in_channels=5, hidden_channels=C, output_dim=3, is_lut_index=1, dropout_p=0.0, num_layers=layers)


# base seed of the dropout-on cases: bit 62 set, so that the site seeds (base + golden ratio * site, mod 2^64) use all
# 64 bits; the HIP model gets it as ``_qot_seed``
DROPOUT_SEED = (1 << 62) + 20240517

TRAJECTORY_CASES = {
    # reference scale; ragged last batch (84 = 5 * 16 + 4)
    "topo_h16": dict(kind="topological", model=_topo_model(16), data=dict(count=240), fit=_topo_fit()),
    # graph-form TransformerConv + split-bf16 NNConv forward / grad-h + the H = 64 weight-gradient kernel
    "topo_h64": dict(kind="topological", model=_topo_model(64), data=dict(count=240), fit=_topo_fit()),
    # generic-width NNConv kernels and their per-step permuted weights
    "topo_h128": dict(kind="topological", model=_topo_model(128), data=dict(count=120), fit=_topo_fit()),
    # zero-padded width: the padded shadow parameters must follow the update
    "topo_h48": dict(kind="topological", model=_topo_model(48), data=dict(count=240), fit=_topo_fit()),
    # materialised-operand NNConv path
    "topo_d6_h32": dict(kind="topological", model=_topo_model(32, D=6), data=dict(count=240, D=6), fit=_topo_fit()),
    # graphs of 8 / 10 / 12 nodes: node path (no table mode), general CSR build per batch
    "topo_mixed_nodes": dict(kind="topological", model=_topo_model(16), data=dict(count=240, mixed=True),
                             fit=_topo_fit()),
    # early stopping (the margins of every ``val_r2 > best`` decision are pinned in test_oracle_train_loop_cpu.py)
    "topo_early_stop": dict(kind="topological", model=_topo_model(16), data=dict(count=240),
                            fit=_topo_fit(num_epochs=12, patience=2, lr=0.1, step_size=4)),
    # a LUT-less batch in the middle of chunk 0; running statistics
    "lp_c8_skip_mid": dict(kind="lightpath", model=_lp_model(8), data=dict(count=96, no_lut=range(8, 12)),
                           fit=_lp_fit()),
    # the LUT-less batches are the LAST ones of chunk 0 (graphs 28..32 of 0..32): skipped right before validation
    "lp_c8_skip_last": dict(kind="lightpath", model=_lp_model(8), data=dict(count=96, no_lut=range(28, 33)),
                            fit=_lp_fit()),
    # thin first layer on / off, logits epilogue
    "lp_c32": dict(kind="lightpath", model=_lp_model(32), data=dict(count=96, no_lut=range(8, 12)), fit=_lp_fit()),
    "lp_c128": dict(kind="lightpath", model=_lp_model(128), data=dict(count=48, no_lut=range(4, 8)), fit=_lp_fit()),
    # BatchNorm folded into the next projection, three sets of running statistics
    "lp_c8_layers3": dict(kind="lightpath", model=_lp_model(8, layers=3), data=dict(count=96, no_lut=range(8, 12)),
                          fit=_lp_fit()),
    # zero-padded width with buffers
    "lp_c24": dict(kind="lightpath", model=_lp_model(24), data=dict(count=96, no_lut=range(8, 12)), fit=_lp_fit()),
    # dropout ON (p = 0.5, the models' default): the oracle loop runs the kernels' own masks, restated by
    # oracle/dropout.py from ``dropout_seed`` and the number of the train-mode forward.  Copies of topo_h16 / topo_h64 /
    # topo_h48 / topo_d6_h32: graph-form and split-bf16 epilogues, masks numbered at the padded width 64, and the
    # separate activation kernel of the materialised path.
    "topo_h16_drop": dict(kind="topological", model=_topo_model(16, p=0.5), data=dict(count=240), fit=_topo_fit(),
                          dropout_seed=DROPOUT_SEED),
    "topo_h64_drop": dict(kind="topological", model=_topo_model(64, p=0.5), data=dict(count=240), fit=_topo_fit(),
                          dropout_seed=DROPOUT_SEED),
    "topo_h48_drop": dict(kind="topological", model=_topo_model(48, p=0.5), data=dict(count=240), fit=_topo_fit(),
                          dropout_seed=DROPOUT_SEED),
    "topo_d6_h32_drop": dict(kind="topological", model=_topo_model(32, D=6, p=0.5), data=dict(count=240, D=6),
                             fit=_topo_fit(), dropout_seed=DROPOUT_SEED),
}


def trajectory_graphs(case):
    """The case's dataset as a host list of ``Data`` (seeded; same graphs on every call)."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    d = case["data"]
    out = []
    if case["kind"] == "topological":
        D = d.get("D", 4)
        for g in range(d["count"]):
            n = (8, 10, 12)[g % 3] if d.get("mixed") else 12
            b = S.topological_batch(2, 1, n=n, e=2 * n + 6, edge_dim=D, first_graph=g)
            y = b.edge_attr[:, :3].mean(0, keepdim=True)        # a target the model can learn
            out.append(q.Data(edge_index=b.edge_index, edge_attr=b.edge_attr, node_ids=b.node_ids, y=y, num_nodes=n))
        return out
    lp = S.lightpath_batch(d["count"])
    for g in range(d["count"]):
        s = q.shard_graphs(lp, g, d["count"])
        x = s.x.clone()
        if g in d["no_lut"]:
            x[:, 1] = 0.0
        out.append(q.Data(x=x, edge_index=s.edge_index, y=s.y, num_nodes=s.num_nodes))
    return out


def trajectory_oracle_model(case):
    """The seeded ``oracle.sparse`` model of a case, zero-initialised biases made non-zero (as test_gpu_parity._models)."""
    from oracle import sparse as O
    torch.manual_seed(0)
    ref = (O.TopologicalGNN if case["kind"] == "topological" else O.LightpathGNN)(**case["model"])
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1 and p.abs().max() == 0:
                p.uniform_(-0.1, 0.1)
    return ref


def trajectory_analytic_zero(case, names):
    """Parameters whose gradient is analytically zero, so that their trajectory is accumulated rounding noise: the
    bias of a ``GATConv`` in front of a train-mode BatchNorm.  Compared against the model's largest magnitude."""
    if case["kind"] != "lightpath":
        return set()
    return {n for n in names if n.startswith("conv") and n.endswith(".bias") and n.count(".") == 1}


def _tensor_err(a, b, floor):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def trajectory_errors(got, ref, analytic_zero=()):
    """``{quantity: error}`` of a run ``got`` against the reference run ``ref``, every entry normalised so that the
    assertion is ``error <= TOL``.  Both are dicts with ``loss / val_loss / r2 / val_r2`` (lists), ``best_val_r2``,
    ``state_dict``, ``best_state_dict``, ``momentum_buffers`` (a list in parameter order) and ``param_names``.

    * losses per epoch: ``|a - b| / max(|b|, first epoch's value)``;  R2: ``|a - b| / max(1, |b|)``;
    * every parameter and BatchNorm running statistic, of the final state and of the best-epoch snapshot:
      max-abs error over ``max(|ref|_inf, 1e-3 * largest parameter magnitude)``, analytic-zero biases over the largest
      magnitude; momentum buffers the same way with the largest buffer magnitude.
    Counters (``epochs_run``, ``stopped_early``, ``skipped_graphs``, ``num_batches_tracked``) are compared for equality
    by the caller (``assert_trajectory_counters``)."""
    err = {}
    for key in ("loss", "val_loss"):
        a, b = got[key], ref[key]
        assert len(a) == len(b), (key, len(a), len(b))
        floor = abs(b[0])
        for e, (x, y) in enumerate(zip(a, b)):
            err[f"{key}[{e}]"] = abs(x - y) / max(abs(y), floor)
    for key in ("r2", "val_r2"):
        a, b = got[key], ref[key]
        assert len(a) == len(b), (key, len(a), len(b))
        for e, (x, y) in enumerate(zip(a, b)):
            err[f"{key}[{e}]"] = abs(x - y) / max(1.0, abs(y))
    err["best_val_r2"] = abs(got["best_val_r2"] - ref["best_val_r2"]) / max(1.0, abs(ref["best_val_r2"]))
    names = list(ref["param_names"])
    for which in ("state_dict", "best_state_dict"):
        a, b = got[which], ref[which]
        assert list(a.keys()) == list(b.keys()), which
        pmax = max(float(b[n].double().abs().max()) for n in names)
        for k in b:
            if k.endswith("num_batches_tracked"):
                continue
            err[f"{which}:{k}"] = _tensor_err(a[k], b[k], pmax if k in analytic_zero else 1e-3 * pmax)
    a, b = got["momentum_buffers"], ref["momentum_buffers"]
    assert len(a) == len(b) == len(names)
    bmax = max(float(t.double().abs().max()) for t in b)
    for n, x, y in zip(names, a, b):
        err[f"momentum:{n}"] = _tensor_err(x.reshape(y.shape), y, bmax if n in analytic_zero else 1e-3 * bmax)
    return err


def assert_trajectory_counters(got, ref):
    for key in ("epochs_run", "stopped_early", "skipped_graphs"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    for which in ("state_dict", "best_state_dict"):
        for k, v in ref[which].items():
            if k.endswith("num_batches_tracked"):
                assert int(got[which][k]) == int(v), (which, k, int(got[which][k]), int(v))


def oracle_trajectory(case, dtype, **kw):
    """``oracle.train_loop.train`` on a case, with the parameter names added.  A case with a ``dropout_seed`` runs the
    restated masks from step counter 0 (a fresh model's): train-mode forward ``k`` draws step ``k``."""
    from oracle import train_loop
    model = trajectory_oracle_model(case)
    if case.get("dropout_seed") is not None:
        kw = dict(dict(dropout=(case["dropout_seed"], 0)), **kw)
    res = train_loop.train(model, trajectory_graphs(case), case["kind"], dtype=dtype, **case["fit"], **kw)
    res["param_names"] = [n for n, p in model.named_parameters() if p.requires_grad]
    return res


def infer_common_args(H=16, D=4, O=3, **kw):
    """The arguments ``qot_topological_infer``, ``_mc`` and ``_grad`` share, up to the status word, for calls that are
    refused (or, with ``B = 0``, answered) before any pointer is read: every pointer is 1 unless ``kw`` names it."""
    import ctypes
    a = dict(node_ids=1, edge_index=1, edge_attr=1, node_ptr=1, edge_ptr=1, N=10, E=10, B=1, n_max=10, max_e=10, t4=1,
             ld4=4 * H, M=1, ldm=16, P=1, V=16, w_edge=1, w1=1, b1=1, wcat=1, bias2=1, w0=1, b0=1, w3=1, b3=1,
             slope_conv=0.01, slope_head=0.01, out=1, H=H, D=D, O=O, status=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    pointers = ("node_ids", "edge_index", "edge_attr", "node_ptr", "edge_ptr", "t4", "M", "P", "w_edge", "w1", "b1", "wcat",
                "bias2", "w0", "b0", "w3", "b3", "out", "status")
    return [ctypes.c_void_p(v) if k in pointers else v for k, v in a.items()]


# the returns every entry point of the single-launch family makes before its own checks are over, by the argument that
# provokes them: (kwargs of infer_common_args, QOT_OK 0 / QOT_ERR_UNSUPPORTED -1 / QOT_ERR_BADARG -2)
INFER_COMMON_REFUSALS = [
    (dict(N=-1), -2), (dict(E=-1), -2), (dict(B=-1), -2), (dict(n_max=-1), -2), (dict(max_e=-1), -2), (dict(V=0), -2),
    (dict(H=48), -1), (dict(D=5), -1), (dict(O=9), -1), (dict(n_max=129), -1), (dict(max_e=1 << 21), -1),
    (dict(B=0), 0), (dict(B=1 << 31), -1),
    (dict(ld4=60), -2), (dict(ld4=66), -2), (dict(ldm=15), -2),
    (dict(node_ptr=None), -2), (dict(t4=None), -2), (dict(b3=None), -2), (dict(out=None), -2),
    (dict(node_ids=None), -2), (dict(edge_attr=None), -2),
    # two at once: the earlier check of the source order wins
    (dict(V=0, H=48), -2),                      # sizes before the envelope
    (dict(H=48, B=0), -1),                      # the envelope before the empty batch
    (dict(B=0, out=None, ld4=0), 0),            # an empty batch before the leading dimensions and the pointers
    (dict(B=1 << 31, out=None), -1),            # the batch bound before the pointers
    (dict(N=0, E=0, node_ids=None, edge_index=None, edge_attr=None, B=1 << 31), -1),   # (legal nulls, then the bound)
]
