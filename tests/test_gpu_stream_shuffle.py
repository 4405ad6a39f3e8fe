"""Shuffled streamed replay on the GPU (``fit(..., stream=True, pad_edges=True, shuffle=True)``):
batches of arbitrary graphs gathered on the device into one slot and one captured graph per graph count.

1. ``qot_shard_stage_gather`` alone: the real part bit-equal to the host collation of the listed graphs, the pad part
   equal to ``stream_pad_cases.pad_layout``, the identity order equal to the padded slot's consecutive staging;
2. one captured launch walks the schedule; a used-up schedule stages nothing;
3. refused batches (id out of range, too few / too many edges) stage nothing;
4. the model on a gather slot against the model on the host-collated batch: forward bit-equal, gradients within TOL;
5. whole shuffled runs against the shuffled fp64 loop (``stream_shuffle_cases.shuffled_oracle_run``), TOL = 1e-4;
6. dropout 0.5, one epoch: the streamed shuffled run against the eager shuffled loop on the host dataset.

The error-path cases run on bounded accesses only: a refused batch stages nothing.
"""
import functools

import pytest
import torch

import helpers as H
import stream_pad_cases as PC
import stream_shuffle_cases as SC
from helpers import TOL

pytestmark = pytest.mark.gpu

FIELDS = ("edge_index", "edge_attr", "node_ids", "x", "y", "ptr", "edge_ptr", "batch")


@functools.lru_cache(maxsize=None)
def _host(which):
    return PC.pad_graphs() if which == "pad" else SC.edge5_graphs()


def _shard(device, which="pad"):
    import gnn_qot_estimation_amd as q
    return q.PackedGraphs.from_data_list(_host(which)).to_device(device)


def _worst_case(B, counts, max_m):
    """A slot that takes ANY list of B graphs: the B largest graphs' total, and pad graphs for the spread to the B smallest."""
    s = sorted(counts)
    e_cap, e_min = sum(s[-B:]), sum(s[:B])
    return e_cap, -(-(e_cap - e_min) // max_m)


def _assert_gathered(slot, host, ids, n, max_m, what=""):
    """The slot after staging ``ids``: real part against the host collation, pad part against ``pad_layout``."""
    import gnn_qot_estimation_amd as q
    ref = q.Batch.from_data_list([host[g] for g in ids])
    got = slot.batch
    B, P, E_cap = len(ids), slot.pad_graphs, slot.E
    E_real, N = ref.edge_index.shape[1], B * n
    assert got.num_graphs == B + P and got.real_graphs == B and got.num_nodes == (B + P) * n, what
    assert int(slot.ctl[2]) >= 0 and int(slot.ctl[3]) == E_real, (what, slot.ctl[:4].tolist())
    rows = {"edge_attr": E_real, "node_ids": N, "x": N, "y": None, "ptr": B + 1, "edge_ptr": B + 1, "batch": N}
    assert torch.equal(got.edge_index[:, :E_real].cpu(), ref.edge_index), (what, "edge_index", ids)
    for f in FIELDS[1:]:
        a, b = getattr(got, f), getattr(ref, f)
        assert (a is None) == (b is None), (what, f)
        if b is None:
            continue
        a = (a if rows[f] is None else a[:rows[f]]).cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, tuple(a.shape), tuple(b.shape))
        assert torch.equal(a, b), (what, f, ids)
    lay = PC.pad_layout(B, n, max_m, P, E_real, E_cap)
    t = lambda v: torch.tensor(v, dtype=torch.long)
    assert torch.equal(got.edge_index[:, E_real:].cpu(), t(lay["edge_index"]).view(2, -1)), (what, "pad edges", ids)
    if got.edge_attr is not None:
        assert not bool(got.edge_attr[E_real:].view(torch.int32).any()), (what, "pad edge_attr")
    if got.x is not None:
        assert got.x[N:].shape[0] == P * n and not bool(got.x[N:].view(torch.int32).any()), (what, "pad x")
    if got.node_ids is not None:
        assert torch.equal(got.node_ids[N:].cpu(), t(lay["node_ids"])), (what, "pad node_ids")
    assert torch.equal(got.batch[N:].cpu(), t(lay["batch"])), (what, "pad batch")
    assert torch.equal(got.ptr[B + 1:].cpu(), t(lay["ptr"])), (what, "pad ptr")
    assert torch.equal(got.edge_ptr[B + 1:].cpu(), t(lay["edge_ptr"])), (what, "pad edge_ptr")
    return E_real


def _snapshot(slot):
    return {f: getattr(slot.batch, f).clone() for f in FIELDS if getattr(slot.batch, f) is not None}


def _orders(B, G, lo):
    gen = torch.Generator().manual_seed(100 + B)
    perm = torch.randperm(G, generator=gen)[:B].tolist()
    identity = list(range(lo, lo + B))
    repeated = list(perm)
    repeated[-1] = repeated[0]
    return {"random": perm, "reversed": identity[::-1], "repeated": repeated, "identity": identity}


# --------------------------------------------------------------------------- 1. staging alone
@pytest.mark.parametrize("which", ["pad", "edge5"])
@pytest.mark.parametrize("B", [16, 4, 5, 7])
def test_gather_staging_bit_for_bit(cuda_device, which, B):
    shard, host = _shard(cuda_device, which), _host(which)
    n, max_m = shard.graph_sizes
    G = len(shard)
    counts = [g.num_edges for g in host]
    E_cap, P = _worst_case(B, counts, max_m)
    slot = shard.gather_stage_slot(B, E_cap, P, num_embeddings=n)
    assert (slot.B, slot.N, slot.E) == (B + P, (B + P) * n, E_cap) and slot.batch.y.shape[0] == B
    lo = 3
    starts = set()
    for name, ids in _orders(B, G, lo).items():
        slot.stage(ids)
        _assert_gathered(slot, host, ids, n, max_m, f"{which} B {B} {name}")
        starts |= {int(v) % 2 for v in slot.batch.edge_ptr[:B].tolist()}
    assert int(slot.status.item()) == 0
    if which == "edge5":
        assert starts == {0, 1}                      # segments started on and off a 16-byte line
    # the identity order is the padded slot's consecutive slice, over the WHOLE slot
    padded = shard.padded_stage_slot(B, E_cap, P, num_embeddings=n)
    padded.stage(lo)
    for f in FIELDS:
        a, b = getattr(slot.batch, f), getattr(padded.batch, f)
        assert (a is None) == (b is None), f
        assert a is None or torch.equal(a, b), (which, B, f)
    assert int(padded.status.item()) == 0


# --------------------------------------------------------------------------- 2. schedule and capture
def test_gather_schedule_and_captured_launch(cuda_device):
    from gnn_qot_estimation_amd import loader as L
    shard, host = _shard(cuda_device), _host("pad")
    E_cap, P = _worst_case(16, [g.num_edges for g in host], 36)
    slot = shard.gather_stage_slot(16, E_cap, P, num_embeddings=12, capacity=4)
    slot.stage(list(range(16)))                      # eager first (loads the code object outside the capture)
    torch.cuda.synchronize(cuda_device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        slot.stage()
    order = torch.randperm(len(shard), generator=torch.Generator().manual_seed(7))[:64].tolist()
    slot.set_schedule(order)
    for k in range(4):
        g.replay()
        _assert_gathered(slot, host, order[16 * k:16 * k + 16], 12, 36, f"replay {k}")
        assert int(slot.ctl[2]) == k
    assert int(slot.status.item()) == 0 and int(slot.ctl[0]) == 4
    # the schedule is used up: RANGE, nothing staged, the position stays
    before = _snapshot(slot)
    g.replay()
    assert int(slot.status.item()) == L.STAGE_BAD_RANGE and int(slot.ctl[2]) == -1 and int(slot.ctl[0]) == 4
    for f, t in before.items():
        assert torch.equal(getattr(slot.batch, f), t), f
    slot.status.zero_()
    with pytest.raises(ValueError, match="capacity"):
        slot.set_schedule(list(range(80)))
    with pytest.raises(ValueError, match="per batch"):
        slot.set_schedule(list(range(17)))


# --------------------------------------------------------------------------- 3. refusals
def test_gather_slot_refuses_what_does_not_fit(cuda_device):
    from gnn_qot_estimation_amd import _lib, loader as L
    shard, host = _shard(cuda_device), _host("pad")
    counts = [g.num_edges for g in host]
    small = sorted(range(len(host)), key=lambda g: counts[g])[:16]       # 16 x 26 edges
    large = sorted(range(len(host)), key=lambda g: -counts[g])[:16]      # 16 x 36 edges
    assert sum(counts[g] for g in small) == 416 and sum(counts[g] for g in large) == 576
    slot = shard.gather_stage_slot(16, 500, 1, num_embeddings=12)        # takes totals 464 .. 500
    good = list(range(16))                                               # 484 edges
    slot.stage(good)
    _assert_gathered(slot, host, good, 12, 36, "good")
    before = _snapshot(slot)
    offs = slot.offs.clone()

    def refused(ids, bit, what):
        slot.stage(ids)
        assert int(slot.status.item()) == bit and int(slot.ctl[2]) == -1, (what, int(slot.status.item()))
        for f, t in before.items():
            assert torch.equal(getattr(slot.batch, f), t), (what, f)
        with pytest.raises(_lib.QotError, match="inconsistent batch slices"):
            L.check_stage_status(slot.status)
        assert int(slot.status.item()) == 0

    for bad in (len(shard), -1, 10 ** 12):
        refused(good[:5] + [bad] + good[6:], L.STAGE_BAD_RANGE, f"id {bad}")
    refused(small, L.STAGE_BAD_SHAPE, "spare above P * max_m")           # 500 - 416 = 84 > 36
    refused(large, L.STAGE_BAD_SHAPE, "total above E_cap")               # 576 > 500
    assert not torch.equal(slot.offs, offs)          # the refused batches' offsets went to the scratch, not to edge_ptr
    slot.stage(good[::-1])                           # and the slot still works
    _assert_gathered(slot, host, good[::-1], 12, 36, "after refusals")
    assert int(slot.status.item()) == 0
    # a node id outside the table is staged as 0 and flagged, as in the other slots
    low = shard.gather_stage_slot(16, 500, 1, num_embeddings=11)
    low.stage(good)
    assert int(low.status.item()) == L.STAGE_BAD_NODE_ID
    import gnn_qot_estimation_amd as q
    ids = q.Batch.from_data_list([host[g] for g in good]).node_ids
    assert torch.equal(low.batch.node_ids[:192].cpu(), torch.where(ids >= 11, torch.zeros_like(ids), ids))
    assert low.batch.node_ids[192:].tolist() == list(range(12))
    # the host refuses an order the plan does not cover before anything is launched
    from gnn_qot_estimation_amd import harness as Hn
    model = q.TopologicalGNN(**SC.CASES["pad_h16"]["model"]).to(cuda_device)
    rep = Hn.StepReplayer(model, "topological", 3, cuda_device, None, None, stream=True, shard=shard, pad_edges=True,
                          shuffle=True, seed=0)
    rep.shuffle_plan = {16: {"E_cap": 500, "E_min": 464, "P": 1, "shape": (17, 204, 500)}}
    with pytest.raises(ValueError, match="not covered by the padding plan"):
        rep.begin_epoch([(0, 16)], True, order=small)
    with pytest.raises(ValueError, match="not covered by the padding plan"):
        rep.begin_epoch([(0, 4)], True, order=[0, 1, 2, 3])
    with pytest.raises(ValueError, match="needs its order"):
        rep.begin_epoch([(0, 16)], True)


# --------------------------------------------------------------------------- 4. the model on a gather slot
def _forward_backward(model, batch, B):
    model.zero_grad(set_to_none=True)
    batch._qot_cache = {}                            # the cache rule of section 4.11: the slot was rewritten behind torch's back
    out = model(batch)
    loss = torch.nn.functional.smooth_l1_loss(out[:B], batch.y.view(-1, 3))
    loss.backward()
    return out.detach()[:B].clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, float(loss.detach())


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train_p0"])
@pytest.mark.parametrize("name", list(SC.CASES))
def test_model_on_a_gather_slot(cuda_device, name, train):
    """``model(slot.batch)[:B]`` against the model on ``Batch.from_data_list`` of the same graphs moved to the device (with
    the shard's ``graph_sizes`` hint, which every batch of a shard carries): the same rows at the same positions, so
    bit-equal; parameter gradients in the metric and within the bound of ``test_gpu_stream_pad.test_model_on_a_padded_slot``."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    shard, host = _shard(cuda_device), _host("pad")
    case = SC.CASES[name]
    plan = Hn.stream_shuffle_plan(shard.node_ptr, shard.edge_ptr, Hn.fit_train_chunks(len(shard), 0.5, 8), 16, SC.SEED,
                                  shard.graph_sizes)
    hip = q.TopologicalGNN(**case["model"])
    hip.load_state_dict(H.trajectory_oracle_model(case).state_dict(), strict=True)
    model = hip.to(cuda_device).train(train)
    order0 = Hn.epoch_order(range(0, 84), SC.SEED, 0)
    order1 = Hn.epoch_order(range(84, 168), SC.SEED, 1)
    worst_g = 0.0
    for B, ids in ((16, order0[:16]), (16, order1[16:32]), (16, order1[64:80]), (4, order0[80:]), (4, order1[80:])):
        slot = shard.gather_stage_slot(B, plan[B]["E_cap"], plan[B]["P"], num_embeddings=12)
        slot.stage(ids)
        assert int(slot.status.item()) == 0
        out_p, g_p, loss_p = _forward_backward(model, slot.batch, B)
        ref = q.Batch.from_data_list([host[g] for g in ids]).to(cuda_device)
        ref.graph_sizes = shard.graph_sizes
        out_r, g_r, loss_r = _forward_backward(model, ref, B)
        e = H.rel_err(out_p, out_r)
        bitwise = torch.equal(out_p, out_r)
        gmax = max(float(g.abs().max()) for g in g_r.values())
        errs = {}
        for n, g in g_r.items():
            floor = gmax if n == "conv1.lin_key.bias" else 1e-3 * gmax
            errs[n] = float((g_p[n].double() - g.double()).abs().max() / max(float(g.abs().max()), floor))
        wn = max(errs, key=errs.get)
        worst_g = max(worst_g, errs[wn])
        print(f"\n[gather slot] {name} {'train' if train else 'eval'} B {B}: forward rel_err {e:.2e}, bitwise {bitwise}, "
              f"loss {loss_p:.9g} / {loss_r:.9g}, worst gradient {wn} {errs[wn]:.2e}")
        assert e <= TOL, (name, B, e)
        assert bitwise, (name, B, e)
        bad = {n: v for n, v in errs.items() if not v <= TOL}
        assert not bad, (name, B, bad)
    assert worst_g <= TOL


# --------------------------------------------------------------------------- 5. whole runs
@functools.lru_cache(maxsize=None)
def _oracle(name):
    return SC.shuffled_oracle_run(SC.CASES[name], torch.float64)


def _fit(name, device, tmp_path, monkeypatch, resident=True, model_kw=None, **fit_kw):
    """``harness.fit`` of a case of ``SC.CASES`` on the unequal shard (resident, or pinned on the host); returns
    ``(result dict as test_gpu_stream_replay._fit, History, call names)``."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import _lib, harness as Hn
    case = SC.CASES[name]
    hip = q.TopologicalGNN(**dict(case["model"], **(model_kw or {})))
    hip.load_state_dict(H.trajectory_oracle_model(case).state_dict(), strict=True)
    data = q.PackedGraphs.from_data_list(PC.pad_graphs())
    data = data.to_device(device) if resident else data.pin()
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
    sizes = [p.numel() for p in opt.flat.params]
    got = {
        "loss": hist.loss, "val_loss": hist.val_loss, "r2": hist.r2, "val_r2": hist.val_r2,
        "best_val_r2": hist.best_val_r2, "epochs_run": hist.epochs_run, "stopped_early": hist.stopped_early,
        "skipped_graphs": hist.skipped_graphs,
        "state_dict": {k: v.detach().cpu() for k, v in hip.state_dict().items()},
        "best_state_dict": torch.load(best, map_location="cpu", weights_only=True),
        "momentum_buffers": [b.cpu() for b in opt.buf.split(sizes)],
        "param_names": [n for n, p in hip.named_parameters() if p.requires_grad],
    }
    return got, hist, calls


@pytest.mark.parametrize("name", list(SC.CASES))
def test_shuffled_run_matches_the_shuffled_fp64_loop(cuda_device, tmp_path, monkeypatch, name):
    got, hist, calls = _fit(name, cuda_device, tmp_path, monkeypatch, stream=True, pad_edges=True, shuffle=True, seed=SC.SEED)
    ref = _oracle(name)
    assert got["param_names"] == ref["param_names"]
    err = H.trajectory_errors(got, ref)
    groups = {}
    for k, v in err.items():
        g = k.split("[")[0].split(":")[0]
        if v >= groups.get(g, ("", -1.0))[1]:
            groups[g] = (k, v)
    print(f"\n[trajectory] {name} / streamed, shuffled: " + ", ".join(f"{g} {v:.2e}" for g, (k, v) in sorted(groups.items())))
    rc = hist.replay_counts
    print(f"[shuffled] {name}: {rc}")
    assert rc["graphs"] == 4                         # (16, train), (4, train), (16, eval), (4, eval)
    train, val = PC.run_ranges(SC.CASES[name]["fit"])
    visits = hist.epochs_run * (len(train) // 2 + len(val))
    assert (rc["eager"], rc["captured"], rc["replayed"]) == (4, 4, visits - 8), (rc, visits)
    assert {"qot_shard_stage_gather", "qot_shard_stage_padded"} <= calls and "qot_shard_stage" not in calls
    H.assert_trajectory_counters(got, ref)
    bad = {k: v for k, v in err.items() if not v <= TOL}
    assert not bad, (name, sorted(bad.items(), key=lambda kv: -kv[1])[:8])


def test_shuffled_run_differs_from_the_unshuffled_padded_run(cuda_device, tmp_path, monkeypatch):
    """The order was in fact applied: same case, same settings, the final parameters end elsewhere."""
    a, _, _ = _fit("pad_h16", cuda_device, tmp_path, monkeypatch, stream=True, pad_edges=True, shuffle=True, seed=SC.SEED)
    b, _, calls = _fit("pad_h16", cuda_device, tmp_path, monkeypatch, stream=True, pad_edges=True)
    assert "qot_shard_stage_gather" not in calls
    far = H.trajectory_errors(a, dict(b, param_names=a["param_names"]))
    assert max(v for k, v in far.items() if k.startswith("state_dict:")) > 10 * TOL


# --------------------------------------------------------------------------- 6. dropout on
def test_shuffled_dropout_run_against_the_eager_shuffled_loop(cuda_device, tmp_path, monkeypatch):
    """Dropout 0.5, H = 64, one epoch, same seeds: the gathered batch holds the host-collated batch's elements at the same
    flat indices, so the masks are the same and only the summation order of the gradient partials differs (pad rows,
    N grows); one epoch keeps that from being amplified.  The bound of
    ``test_gpu_stream_pad.test_padded_dropout_run_against_the_per_batch_replay``: TOL in ``helpers.trajectory_errors``."""
    runs = {}
    for mode, kw in (("streamed", dict(stream=True, pad_edges=True)), ("eager", dict(resident=False))):
        torch.manual_seed(1234)
        runs[mode] = _fit("pad_h64", cuda_device, tmp_path, monkeypatch, model_kw=dict(dropout_p=0.5), num_epochs=1,
                          shuffle=True, seed=SC.SEED, **kw)
    (a, ha, ca), (b, hb, cb) = runs["streamed"], runs["eager"]
    assert ha.epochs_run == hb.epochs_run == 1
    assert ha.replay_counts["graphs"] == 2 and ha.replay_counts["replayed"] > 0
    assert hb.replay_counts == {} and "qot_shard_stage_gather" in ca and "qot_shard_stage_gather" not in cb
    err = H.trajectory_errors(a, dict(b, param_names=a["param_names"]))
    worst = max(err.items(), key=lambda kv: kv[1])
    print(f"\n[shuffled streamed vs eager shuffled loop, dropout 0.5, one epoch] worst {worst[0]} {worst[1]:.2e}")
    plain = _oracle("pad_h64")["loss"][0]             # the masks were on: the same epoch without dropout ends elsewhere
    assert abs(a["loss"][0] - plain) > 1e-3 * plain
    bad = {k: v for k, v in err.items() if not v <= TOL}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
