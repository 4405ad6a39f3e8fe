"""Padded streamed replay on the GPU (``fit(..., stream=True, pad_edges=True)``): batches of
unequal edge totals through one slot and one captured graph per graph count.

3. ``qot_shard_stage_padded`` alone: the real slice bit-equal to ``device_batch``, the pad part equal to the Python
   restatement ``stream_pad_cases.pad_layout`` (integers and zeros: no tolerance), refused slices stage nothing;
4. the model on a padded slot against the model on the unpadded batch: forward bit-equal, gradients within TOL;
5. whole runs against ``oracle/train_loop.py`` in fp64, TOL = 1e-4, compared as tests/test_gpu_training_trajectory.py
   compares (conditioning of the cases: tests/test_stream_pad_cpu.py);
6. graph counts: 4 captured graphs where exact-shape slots would take 10;
7. dropout on: a whole run against the fp64 loop running the same masks (``pad_h64_drop``, oracle/dropout.py), and one
   epoch against the per-batch replay within TOL.

The error-path cases run on bounded accesses only: a refused slice stages nothing.
"""
import functools

import pytest
import torch

import helpers as H
import stream_pad_cases as PC
import test_gpu_stream_replay as SR
from helpers import TOL

pytestmark = pytest.mark.gpu

REAL_FIELDS = ("edge_attr", "node_ids", "x", "y", "ptr", "edge_ptr", "batch")
MAX_M = 36


def _shard(device):
    import gnn_qot_estimation_amd as q
    return q.PackedGraphs.from_data_list(PC.pad_graphs()).to_device(device)


def _plan(shard, fit=None):
    from gnn_qot_estimation_amd import harness as Hn
    fit = fit or H._topo_fit()
    return Hn.stream_pad_plan(shard.node_ptr, shard.edge_ptr,
                              Hn.fit_batch_ranges(len(shard), fit["batch_size"], fit["chunk_fraction"]), shard.graph_sizes)


def _assert_padded(slot, shard, lo, B, n, max_m, what=""):
    """The slot after ``stage(lo)``: real part against ``device_batch``, pad part against ``pad_layout``."""
    ref = shard.device_batch(lo, lo + B)
    got = slot.batch
    P, E_cap = slot.pad_graphs, slot.E
    E_real = ref.edge_index.shape[1]
    N = B * n
    assert got.num_graphs == B + P and got.real_graphs == B and got.num_nodes == (B + P) * n, what
    assert got.edge_index.shape == (2, E_cap) and got.batch.shape == ((B + P) * n,), what
    assert got.ptr.shape == (B + P + 1,) and got.edge_ptr.shape == (B + P + 1,), what
    assert int(slot.ctl[2]) == lo and int(slot.ctl[3]) == E_real, (what, slot.ctl[:4].tolist())
    # real part, field by field, bit for bit
    assert torch.equal(got.edge_index[:, :E_real], ref.edge_index), (what, "edge_index", lo)
    rows = {"edge_attr": E_real, "node_ids": N, "x": N, "y": None, "ptr": B + 1, "edge_ptr": B + 1, "batch": N}
    for f in REAL_FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        assert (a is None) == (b is None), (what, f)
        if b is None:
            continue
        a = a if rows[f] is None else a[:rows[f]]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, tuple(a.shape), tuple(b.shape))
        assert torch.equal(a, b), (what, f, lo)
    # pad part: integers and zeros, exactly
    lay = PC.pad_layout(B, n, max_m, P, E_real, E_cap)
    t = lambda v: torch.tensor(v, dtype=torch.long)
    assert torch.equal(got.edge_index[:, E_real:].cpu(), t(lay["edge_index"]).view(2, -1)), (what, "pad edges", lo)
    if got.edge_attr is not None:
        assert got.edge_attr[E_real:].shape[0] == E_cap - E_real
        assert not bool(got.edge_attr[E_real:].view(torch.int32).any()), (what, "pad edge_attr", lo)
    if got.x is not None:
        assert got.x[N:].shape[0] == P * n and not bool(got.x[N:].view(torch.int32).any()), (what, "pad x", lo)
    if got.node_ids is not None:
        assert torch.equal(got.node_ids[N:].cpu(), t(lay["node_ids"])), (what, "pad node_ids", lo)
    assert torch.equal(got.batch[N:].cpu(), t(lay["batch"])), (what, "pad batch", lo)
    assert torch.equal(got.ptr[B + 1:].cpu(), t(lay["ptr"])), (what, "pad ptr", lo)
    assert torch.equal(got.edge_ptr[B + 1:].cpu(), t(lay["edge_ptr"])), (what, "pad edge_ptr", lo)
    return E_real


def _snapshot(slot):
    return {f: getattr(slot.batch, f).clone() for f in ("edge_index",) + REAL_FIELDS if getattr(slot.batch, f) is not None}


# --------------------------------------------------------------------------- 3. staging alone
def test_padded_staging_of_the_unequal_shard(cuda_device):
    shard = _shard(cuda_device)
    assert shard.graph_sizes == (PC.N_NODES, MAX_M)
    plan = _plan(shard)
    seen = set()
    for B, los in ((16, (0, 16, 32, 48, 100, 132, 184, 0)), (4, (80, 164, 200))):
        slot = shard.padded_stage_slot(B, plan[B]["E_cap"], plan[B]["P"], num_embeddings=12)
        assert (slot.B, slot.N, slot.E) == plan[B]["shape"] and slot.batch.y.shape[0] == B
        for lo in los:
            slot.stage(lo)                           # every stage() overwrites the previous batch's pad region too
            seen.add((B, _assert_padded(slot, shard, lo, B, PC.N_NODES, MAX_M, f"B {B}")))
        assert int(slot.status.item()) == 0
    # the smallest and the largest batch of both graph counts went through
    assert {(16, 484), (16, 492), (4, 114), (4, 124)} <= seen


def _odd_shard(device, count=40, D=3, F=5):
    """Graphs of 7 nodes with 12 .. 18 edges, odd and even, in runs of ten small / ten large graphs: real slices END at odd
    offsets, so the pad regions of the int64 fields start 8 bytes off a 16-byte line and those of the fp32 rows 4 * D
    (4 * F) bytes off; windows of 5 / 12 graphs spread over more than one graph's 18 edges (2 / 3 pad graphs)."""
    import gnn_qot_estimation_amd as q
    gen = torch.Generator().manual_seed(11)
    graphs = []
    for g in range(count):
        n, e = 7, 12 + 5 * ((g // 10) % 2) + (g * g) % 3
        src = torch.randint(0, n, (e,), generator=gen)
        dst = (src + 1 + torch.randint(0, n - 1, (e,), generator=gen)) % n
        graphs.append(q.Data(edge_index=torch.stack([src, dst]), edge_attr=torch.rand(e, D, generator=gen),
                             y=torch.rand(1, 3, generator=gen), x=torch.rand(n, F, generator=gen),
                             node_ids=torch.randperm(n, generator=gen), num_nodes=n))
    return q.PackedGraphs.from_data_list(graphs).to_device(device)


@pytest.mark.parametrize("B", [5, 1, 12])
def test_padded_staging_at_odd_offsets_and_two_pad_graphs(cuda_device, B):
    from gnn_qot_estimation_amd import harness as Hn
    shard = _odd_shard(cuda_device)
    n, max_m = shard.graph_sizes
    assert (n, max_m) == (7, 18)
    windows = [(lo, lo + B) for lo in range(0, len(shard) - B + 1)]
    plan = Hn.stream_pad_plan(shard.node_ptr, shard.edge_ptr, windows, shard.graph_sizes)[B]
    assert plan["P"] == {5: 2, 1: 1, 12: 3}[B]       # (89 - 63) / 18, (18 - 12) / 18, (202 - 162) / 18, rounded up
    slot = shard.padded_stage_slot(B, plan["E_cap"], plan["P"])
    parities = set()
    for lo, _ in windows:
        slot.stage(lo)
        E_real = _assert_padded(slot, shard, lo, B, n, max_m, f"odd B {B}")
        parities.add((E_real % 2, (B * n) % 2))
    assert int(slot.status.item()) == 0
    assert len({p[0] for p in parities}) == 2        # pad regions started on and off a 16-byte line


def test_padded_schedule_and_captured_launch(cuda_device):
    shard = _shard(cuda_device)
    plan = _plan(shard)
    slot = shard.padded_stage_slot(16, plan[16]["E_cap"], plan[16]["P"], num_embeddings=12)
    slot.stage(0)                                    # eager first (loads the code object outside the capture)
    torch.cuda.synchronize(cuda_device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        slot.stage()
    los = [32, 0, 148, 16]
    slot.set_schedule(los)
    for k, lo in enumerate(los):
        g.replay()
        _assert_padded(slot, shard, lo, 16, PC.N_NODES, MAX_M, f"replay {k}")
    assert int(slot.status.item()) == 0 and int(slot.ctl[0]) == 4


def test_padded_slot_refuses_what_does_not_fit(cuda_device):
    from gnn_qot_estimation_amd import _lib, loader as L
    shard = _shard(cuda_device)
    plan = _plan(shard)
    E_cap = plan[16]["E_cap"]
    # (a) spare above P * max_m: a slot whose capacity lies more than one pad graph above every batch
    slot = shard.padded_stage_slot(16, E_cap + 2 * MAX_M, 1, num_embeddings=12)
    before = _snapshot(slot)
    slot.stage(0)                                    # 484 edges: 80 spare > 36
    assert int(slot.status.item()) == L.STAGE_BAD_SHAPE and int(slot.ctl[2]) == -1
    for f, t in before.items():
        assert torch.equal(getattr(slot.batch, f), t), f
    with pytest.raises(_lib.QotError, match="inconsistent batch slices"):
        L.check_stage_status(slot.status)
    assert int(slot.status.item()) == 0
    # (b) more edges than the slot holds
    small = shard.padded_stage_slot(16, plan[16]["E_min"], 0, num_embeddings=12)
    small.stage(0)                                   # 484 = E_min: fits exactly, no pad graph
    _assert_padded(small, shard, 0, 16, PC.N_NODES, MAX_M, "exact fit")
    before = _snapshot(small)
    small.stage(32)                                  # 492 edges
    assert int(small.status.item()) == L.STAGE_BAD_SHAPE
    for f, t in before.items():
        assert torch.equal(getattr(small.batch, f), t), f
    small.status.zero_()
    # (c) range errors as in the exact-shape slot
    for lo in (230, -1, 10 ** 12):
        small.stage(lo)
        assert int(small.status.item()) == L.STAGE_BAD_RANGE, lo
        small.status.zero_()
    # (d) a node id outside the table in the real part is staged as 0 and flagged; pad ids are 0 .. n-1 and never flagged
    low = shard.padded_stage_slot(16, E_cap, 1, num_embeddings=11)
    low.stage(16)
    assert int(low.status.item()) == L.STAGE_BAD_NODE_ID
    ref = shard.device_batch(16, 32)
    assert torch.equal(low.batch.node_ids[:192], torch.where(ref.node_ids >= 11, torch.zeros_like(ref.node_ids), ref.node_ids))
    assert low.batch.node_ids[192:].tolist() == list(range(12))
    # (e) the host refuses a plan that does not cover a batch before anything is launched
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    model = q.TopologicalGNN(**PC.PAD_CASES["pad_h16"]["model"]).to(cuda_device)
    rep = Hn.StepReplayer(model, "topological", 3, cuda_device, None, None, stream=True, shard=shard, pad_edges=True)
    rep.plan_padding([(0, 16), (100, 116)])          # both 484 edges: P = 0
    with pytest.raises(ValueError, match="not covered by the padding plan"):
        rep.begin_epoch([(0, 16), (32, 48)], False)
    with pytest.raises(ValueError, match="not covered by the padding plan"):
        rep.begin_epoch([(80, 84)], False)


# --------------------------------------------------------------------------- 4. the model on a padded slot
def _models(name, device, train):
    import gnn_qot_estimation_amd as q
    case = PC.PAD_CASES[name]
    hip = q.TopologicalGNN(**case["model"])
    hip.load_state_dict(H.trajectory_oracle_model(case).state_dict(), strict=True)
    return hip.to(device).train(train)


def _forward_backward(model, batch, B):
    model.zero_grad(set_to_none=True)
    batch._qot_cache = {}                            # the cache rule of section 4.11: the slot was rewritten behind torch's back
    out = model(batch)
    loss = torch.nn.functional.smooth_l1_loss(out[:B], batch.y.view(-1, 3))
    loss.backward()
    return out.detach()[:B].clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, float(loss.detach())


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train_p0"])
@pytest.mark.parametrize("name", list(PC.PAD_CASES))
def test_model_on_a_padded_slot(cuda_device, name, train):
    """``model(slot.batch)[:B]`` against ``model(device_batch)``: the same rows at the same positions, so bit-equal; every
    parameter gradient of ``loss(out[:B], y)`` within TOL of the unpadded batch's (per-workgroup partial sums are cut
    differently when N grows).  Gradient metric of tests/test_gpu_parity.py: each parameter's max-abs error over
    max(its own magnitude, 1e-3 x the model's largest gradient); ``conv1.lin_key.bias`` (analytically zero: softmax is
    shift invariant) over the largest gradient."""
    shard = _shard(cuda_device)
    plan = _plan(shard)
    model = _models(name, cuda_device, train)
    worst_g = 0.0
    for B, lo in ((16, 0), (16, 32), (16, 132), (4, 164), (4, 80)):     # smallest / largest / middle; ragged likewise
        slot = shard.padded_stage_slot(B, plan[B]["E_cap"], plan[B]["P"], num_embeddings=12)
        slot.stage(lo)
        assert int(slot.status.item()) == 0
        out_p, g_p, loss_p = _forward_backward(model, slot.batch, B)
        assert model(slot.batch).shape[0] == B + plan[B]["P"]
        out_r, g_r, loss_r = _forward_backward(model, shard.device_batch(lo, lo + B), B)
        e = H.rel_err(out_p, out_r)
        bitwise = torch.equal(out_p, out_r)
        gmax = max(float(g.abs().max()) for g in g_r.values())
        errs = {}
        for n, g in g_r.items():
            floor = gmax if n == "conv1.lin_key.bias" else 1e-3 * gmax
            errs[n] = float((g_p[n].double() - g.double()).abs().max() / max(float(g.abs().max()), floor))
        wn = max(errs, key=errs.get)
        worst_g = max(worst_g, errs[wn])
        print(f"\n[padded slot] {name} {'train' if train else 'eval'} B {B} lo {lo}: forward rel_err {e:.2e}, bitwise {bitwise}, "
              f"loss {loss_p:.9g} / {loss_r:.9g}, worst gradient {wn} {errs[wn]:.2e}")
        assert e <= TOL, (name, B, lo, e)
        assert bitwise, (name, B, lo, e)
        bad = {n: v for n, v in errs.items() if not v <= TOL}
        assert not bad, (name, B, lo, bad)
    assert worst_g <= TOL


# --------------------------------------------------------------------------- 5. / 6. whole runs
@functools.lru_cache(maxsize=None)
def _oracle(name):
    return PC.oracle_run(PC.ALL_CASES[name], torch.float64)


def _fit(name, device, tmp_path, monkeypatch, **kw):
    """``harness.fit`` on the unequal shard (``PAD_CASES[name]`` has the model and fit settings of the trajectory case)."""
    base = {"pad_h16": "topo_h16", "pad_h64": "topo_h64", "pad_h64_drop": "topo_h64_drop"}[name]
    assert H.TRAJECTORY_CASES[base]["model"] == PC.ALL_CASES[name]["model"]
    assert H.TRAJECTORY_CASES[base]["fit"] == PC.ALL_CASES[name]["fit"]
    assert H.TRAJECTORY_CASES[base].get("dropout_seed") == PC.ALL_CASES[name].get("dropout_seed")
    return SR._fit(base, device, tmp_path, monkeypatch, graphs=PC.pad_graphs(), **kw)


@pytest.mark.parametrize("name", list(PC.ALL_CASES))
def test_padded_run_matches_the_fp64_loop(cuda_device, tmp_path, monkeypatch, name):
    """``pad_h64_drop``: dropout ON against the oracle loop running the same masks; the run's final step counter equals the
    loop's draw count (one draw per visit of a training batch, pad graphs or not)."""
    from gnn_qot_estimation_amd import harness as Hn
    got, hist, calls = _fit(name, cuda_device, tmp_path, monkeypatch, stream=True, pad_edges=True)
    ref = _oracle(name)
    assert got["param_names"] == ref["param_names"]
    err = H.trajectory_errors(got, ref)
    groups = {}
    for k, v in err.items():
        g = k.split("[")[0].split(":")[0]
        if v >= groups.get(g, ("", -1.0))[1]:
            groups[g] = (k, v)
    print(f"\n[trajectory] {name} / streamed, padded: " + ", ".join(f"{g} {v:.2e}" for g, (k, v) in sorted(groups.items())))
    # the run took the path: 4 graphs where exact-shape slots take one per (shape, direction)
    rc = hist.replay_counts
    print(f"[padded] {name}: {rc}")
    shard_n, shard_e = PC.offsets()
    train, val = PC.run_ranges(PC.ALL_CASES[name]["fit"])
    exact = len(Hn.stream_schedule(shard_n, shard_e, train)) + len(Hn.stream_schedule(shard_n, shard_e, val))
    assert len(Hn.stream_schedule(shard_n, shard_e, train + val)) > 4 and exact > 4      # the data exercises the feature
    assert rc["graphs"] == 4
    visits = hist.epochs_run * (len(train) // 2 + len(val))
    assert (rc["eager"], rc["captured"], rc["replayed"]) == (4, 4, visits - 8), (rc, visits)
    assert "qot_shard_stage_padded" in calls and "qot_shard_stage" not in calls
    H.assert_trajectory_counters(got, ref)
    assert got["dropout_draws"] == ref["dropout_draws"], (got["dropout_draws"], ref["dropout_draws"])
    assert (ref["dropout_draws"] > 0) == (name in PC.PAD_DROP_CASES)
    bad = {k: v for k, v in err.items() if not v <= TOL}
    assert not bad, (name, sorted(bad.items(), key=lambda kv: -kv[1])[:8])


def test_exact_shape_slots_on_the_unequal_shard_take_ten_graphs(cuda_device, tmp_path, monkeypatch):
    """What the padding is for: plain ``stream=True`` on the same shard keeps serving it, with one slot and one graph per
    exact (shape, direction)."""
    _, hist, calls = _fit("pad_h16", cuda_device, tmp_path, monkeypatch, stream=True)
    assert hist.replay_counts["graphs"] == 10 and "qot_shard_stage_padded" not in calls


# --------------------------------------------------------------------------- 7. dropout on
def test_padded_dropout_run_against_the_per_batch_replay(cuda_device, tmp_path, monkeypatch):
    """Dropout 0.5, H = 64, one epoch, same seed: real elements keep their element indices in the padded batch, so the masks
    are the same and only the summation order of the gradient partials differs; one epoch keeps that from being
    amplified.  Parameters and momentum buffers (and the epoch's loss / R2) within TOL in ``helpers.trajectory_errors``."""
    runs = {}
    for mode, kw in (("padded", dict(stream=True, pad_edges=True)), ("per_batch", dict(replay=True))):
        torch.manual_seed(1234)
        runs[mode] = _fit("pad_h64", cuda_device, tmp_path, monkeypatch, model_kw=dict(dropout_p=0.5), num_epochs=1, **kw)
    (a, ha, _), (b, hb, _) = runs["padded"], runs["per_batch"]
    assert ha.epochs_run == hb.epochs_run == 1
    assert ha.replay_counts["graphs"] == 2 and ha.replay_counts["replayed"] > 0      # (16, train) and (16, eval)
    err = H.trajectory_errors(a, dict(b, param_names=a["param_names"]))
    worst = max(err.items(), key=lambda kv: kv[1])
    print(f"\n[padded vs per-batch replay, dropout 0.5, one epoch] worst {worst[0]} {worst[1]:.2e}")
    # the masks were on: the same epoch without dropout ends elsewhere
    plain = _oracle("pad_h64")["loss"][0]
    assert abs(a["loss"][0] - plain) > 1e-3 * plain
    bad = {k: v for k, v in err.items() if not v <= TOL}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
