"""Shuffled streamed replay (``fit(..., stream=True, pad_edges=True, shuffle=True)``), host part: the epoch orders, the
padding plan over every batch of every epoch against a brute-force restatement, the ABI of the gather staging, the
refusals, and the conditioning of the whole-run cases of tests/test_gpu_stream_shuffle.py (the
shuffled oracle loop in fp32 against fp64 within TOL / 10, every ``val_r2 > best`` decision with a margin of at least
10 x TOL).
"""
import ctypes
import functools
import inspect
import itertools
import os

import pytest
import torch

import helpers as H
import stream_pad_cases as PC
import stream_shuffle_cases as SC
from helpers import TOL


# --------------------------------------------------------------------------- 1. the orders
def test_epoch_order_is_a_seeded_permutation():
    from gnn_qot_estimation_amd import harness as Hn
    idx = range(84, 168)
    a = Hn.epoch_order(idx, 3, 5)
    assert sorted(a) == list(idx) and a != list(idx)
    assert a == Hn.epoch_order(idx, 3, 5)                      # a pure function of (seed, epoch)
    torch.manual_seed(99)                                      # ... that neither reads nor moves the global generator
    state = torch.get_rng_state()
    assert a == Hn.epoch_order(idx, 3, 5) and torch.equal(state, torch.get_rng_state())
    assert a != Hn.epoch_order(idx, 3, 6) and a != Hn.epoch_order(idx, 4, 5)
    orders = {tuple(Hn.epoch_order(idx, 0, e)) for e in range(8)}
    assert len(orders) == 8                                    # a fresh order every epoch
    assert Hn.epoch_order(range(0), 0, 0) == [] and Hn.epoch_order(range(7, 8), 0, 0) == [7]


# --------------------------------------------------------------------------- 2. the plan
@pytest.mark.parametrize("seed", [SC.SEED, 1, 12345])
def test_plan_against_brute_force(seed):
    from gnn_qot_estimation_amd import harness as Hn
    fit = H._topo_fit()
    node_ptr, edge_ptr = PC.offsets()
    counts = [PC.edge_count(g) for g in range(PC.COUNT)]
    chunks = Hn.fit_train_chunks(PC.COUNT, fit["chunk_fraction"], fit["num_epochs"])
    assert chunks == [range(0, 84), range(84, 168)] * 4
    plan = Hn.stream_shuffle_plan(node_ptr, edge_ptr, chunks, fit["batch_size"], seed, (PC.N_NODES, 36))
    want, seen = SC.brute_force_plan(counts, chunks, fit["batch_size"], seed, PC.N_NODES, 36)
    assert plan == want and set(plan) == {16, 4}
    assert len(seen[16]) == 8 * 5 and len(seen[4]) == 8
    for B, es in seen.items():
        for e in es:
            assert 0 <= plan[B]["E_cap"] - e <= plan[B]["P"] * 36, (B, e, plan[B])
        assert plan[B]["shape"] == (B + plan[B]["P"], (B + plan[B]["P"]) * PC.N_NODES, plan[B]["E_cap"])
    # the totals of random subsets concentrate: far fewer pad graphs than the worst case (16 x 36 - 16 x 26 = 160 edges: 5)
    assert plan[16]["P"] <= 3 and plan[4]["P"] <= 2
    print(f"seed {seed}: {plan}")


def test_plan_refuses_mixed_node_counts():
    from gnn_qot_estimation_amd import harness as Hn
    import stream_cases as SCS
    node_ptr, edge_ptr = SCS.case_offsets(H.TRAJECTORY_CASES["topo_mixed_nodes"])
    with pytest.raises(ValueError, match="same node count"):
        Hn.stream_shuffle_plan(node_ptr, edge_ptr, [range(0, 32)], 16, 0, (12, 30))


# --------------------------------------------------------------------------- 3. ABI
def test_gather_staging_is_declared_bound_and_exported():
    from gnn_qot_estimation_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "qot_gnn.h")).read()
    assert "int qot_shard_stage_gather(" in hdr and "#define QOT_ABI_VERSION 13" in hdr and _lib.ABI_VERSION == 13
    res, args = _lib.SIGNATURES["qot_shard_stage_gather"]
    decl = hdr[hdr.index("int qot_shard_stage_gather("):]
    decl = decl[:decl.index(";")]
    assert len(args) == decl.count(",") + 1 and res is ctypes.c_int
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "qot_shard_stage_gather")
    assert _lib.load().qot_abi_version() == 13


# --------------------------------------------------------------------------- 4. refusals and defaults
def test_shuffle_refusals():
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    case = SC.CASES["pad_h16"]
    model = q.TopologicalGNN(**case["model"])
    quiet = dict(device="cpu", log=lambda s: None)
    host = q.PackedGraphs.from_data_list(PC.pad_graphs())
    resident = host.to_device("cpu")                 # the shard only has to claim residency for these checks
    fit = lambda data, **kw: Hn.fit(model, data, **dict(dict(kind="topological", shuffle=True), **kw), **quiet, **case["fit"])
    with pytest.raises(ValueError, match="stream=True, pad_edges=True"):
        fit(resident)
    with pytest.raises(ValueError, match="stream=True, pad_edges=True"):
        fit(resident, stream=True)
    with pytest.raises(ValueError, match="topological"):
        fit(resident, kind="lightpath", stream=True, pad_edges=True)
    mixed = q.PackedGraphs.from_data_list(H.trajectory_graphs(H.TRAJECTORY_CASES["topo_mixed_nodes"])).to_device("cpu")
    with pytest.raises(ValueError, match="same node count"):
        fit(mixed, stream=True, pad_edges=True)
    with pytest.raises(ValueError, match="HBM-resident"):
        fit(host, stream=True, pad_edges=True)
    for world in (2, 8):
        with pytest.raises(ValueError, match="single process"):
            Hn.check_shuffle(resident, "topological", world, True, True)
        with pytest.raises(ValueError, match="single process"):
            Hn.check_shuffle(host, "topological", world, None, None)
    Hn.check_shuffle(resident, "topological", 1, True, True)
    Hn.check_shuffle(host, "lightpath", 1, None, None)          # a host dataset takes the eager loop, whatever the model
    run = lambda data, **kw: Hn.run_epoch(model, data, range(0, 16), kind="topological", batch_size=16, out_dim=3, device="cpu",
                                          criterion=None, shuffle=True, **kw)
    with pytest.raises(ValueError, match="stream=True, pad_edges=True"):
        run(resident)
    with pytest.raises(ValueError, match="same node count"):
        run(mixed, stream=True, pad_edges=True)
    with pytest.raises(ValueError, match="stream=True, pad_edges=True"):
        Hn.StepReplayer(model, "topological", 3, "cpu", None, None, stream=True, shard=resident, shuffle=True)
    with pytest.raises(ValueError, match="HBM-resident"):
        q.GatherStageSlot(host, 16, 500, 1)
    with pytest.raises(ValueError, match="same node count"):
        q.GatherStageSlot(mixed, 16, 500, 1)


# every refusal of the option checks, by a short name: (exception type, full message)
_OPTION_REFUSALS = {
    "replayer_host": (ValueError, 'a StepReplayer shuffles on an HBM-resident shard (a host dataset takes the eager loop)'),
    "pad_stream": (ValueError, 'pad_edges=True needs stream=True: the padding belongs to the static slots of streamed replay'),
    "shuffle_host": (ValueError, 'stream=True needs an HBM-resident shard (PackedGraphs.to_device); shuffle=True on a host '
                                  'dataset runs the eager loop'),
    "stream_host": (ValueError, 'stream=True needs an HBM-resident shard (PackedGraphs.to_device): batches are staged on the '
                                 "device from the shard's flat tensors"),
    "shuffle_world": (ValueError, 'shuffle=True needs a single process: every rank would have to gather its share of every batch'),
    "stream_kind": (ValueError, "stream=True needs kind='topological': LightpathGNN's LUT row count is data-dependent and its "
                                 'skip rule is decided on the host per batch (it keeps the per-batch replay)'),
    "shuffle_needs": (ValueError, 'shuffle=True on a resident shard needs stream=True, pad_edges=True: shuffled batches are '
                                   'gathered on the device into padded slots (or keep the shard on the host: PackedGraphs.pin)'),
    "run_replayer": (ValueError, 'stream=True needs a StepReplayer(stream=True, shard=dataset)'),
    "stream_world": (ValueError, "stream=True needs a single process: a data-parallel rank's share and loss scale are per batch "
                                  '(it keeps the per-batch replay)'),
    "shuffle_kind": (ValueError, "shuffle=True on a resident shard needs kind='topological' (streamed replay does)"),
    "pad_mixed": (ValueError, 'pad_edges=True needs a shard whose graphs all have the same node count (mixed node counts keep '
                               'stream=True with exact-shape slots)'),
    "shuffle_mixed": (ValueError, 'shuffle=True on a resident shard needs graphs that all have the same node count'),
}
# (dataset, kind, world) -> the outcomes "fit/run_epoch/StepReplayer" (one name: of all three) for (stream, pad_edges,
# shuffle) = FFF, FFT, FTF, FTT, TFF, TFT, TTF, TTT: a name of _OPTION_REFUSALS, or "ok" when every option check let the
# call through.  Recorded by running _option_outcomes at the commit before the checks were gathered into one function.
_OPTION_TABLE = {
    ("host", "topological", 1):
        "ok ok/ok/replayer_host pad_stream shuffle_host stream_host shuffle_host stream_host shuffle_host",
    ("host", "topological", 2):
        "ok shuffle_world pad_stream shuffle_world stream_host shuffle_world stream_host shuffle_world",
    ("host", "lightpath", 1):
        "ok ok/ok/replayer_host pad_stream shuffle_host stream_kind shuffle_host stream_kind shuffle_host",
    ("host", "lightpath", 2):
        "ok shuffle_world pad_stream shuffle_world stream_kind shuffle_world stream_kind shuffle_world",
    ("uniform", "topological", 1):
        "ok shuffle_needs pad_stream shuffle_needs ok/run_replayer/ok shuffle_needs ok/run_replayer/ok "
        "ok/run_replayer/ok",
    ("uniform", "topological", 2):
        "ok shuffle_world pad_stream shuffle_world stream_world shuffle_world stream_world shuffle_world",
    ("uniform", "lightpath", 1):
        "ok shuffle_kind pad_stream shuffle_kind stream_kind shuffle_kind stream_kind shuffle_kind",
    ("uniform", "lightpath", 2):
        "ok shuffle_world pad_stream shuffle_world stream_kind shuffle_world stream_kind shuffle_world",
    ("mixed", "topological", 1):
        "ok shuffle_needs pad_stream shuffle_needs ok/run_replayer/ok shuffle_needs pad_mixed shuffle_mixed",
    ("mixed", "topological", 2):
        "ok shuffle_world pad_stream shuffle_world stream_world shuffle_world stream_world shuffle_world",
    ("mixed", "lightpath", 1):
        "ok shuffle_kind pad_stream shuffle_kind stream_kind shuffle_kind stream_kind shuffle_kind",
    ("mixed", "lightpath", 2):
        "ok shuffle_world pad_stream shuffle_world stream_kind shuffle_world stream_kind shuffle_world",
}


class _Reached(Exception):
    """Raised by the first statement behind the option checks: the call was accepted."""


def _option_outcomes(monkeypatch):
    """``{(dataset, kind, world): [outcome of fit / run_epoch / StepReplayer per option triple]}`` as ``(type, message)`` or
    "ok": the loop whose results at the parent commit are the literal table above."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn

    class Model:                                     # fit moves the model to the device right behind its checks
        def to(self, device):
            raise _Reached

    def loader(*a, **kw):                            # ... and run_epoch without stream=True builds its loader
        raise _Reached

    monkeypatch.setattr(Hn, "GraphLoader", loader)
    monkeypatch.setattr(torch.cuda, "graph_pool_handle", lambda: None)
    host = q.PackedGraphs.from_data_list(PC.pad_graphs())
    datasets = {"host": host, "uniform": host.to_device("cpu"),      # the shard only has to claim residency
                "mixed": q.PackedGraphs.from_data_list(H.trajectory_graphs(H.TRAJECTORY_CASES["topo_mixed_nodes"])).to_device("cpu")}

    def outcome(call):
        try:
            call()
        except _Reached:
            return "ok"
        except Exception as err:                     # noqa: BLE001  (the table pins the type)
            return (type(err), str(err))
        return "ok"

    out = {}
    for (name, data), kind, world in itertools.product(datasets.items(), ("topological", "lightpath"), (1, 2)):
        monkeypatch.setattr(Hn, "_rank_world", lambda world=world: (0, world))
        cells = []
        for stream, pad_edges, shuffle in itertools.product((False, True), repeat=3):
            opts = dict(stream=stream, pad_edges=pad_edges, shuffle=shuffle)
            cells.append((
                outcome(lambda: Hn.fit(Model(), data, kind=kind, device="cpu", log=lambda s: None, **opts)),
                outcome(lambda: Hn.run_epoch(Model(), data, range(0, 16), kind=kind, batch_size=16, out_dim=3, device="cpu",
                                             criterion=None, **opts)),
                outcome(lambda: Hn.StepReplayer(Model(), kind, 3, "cpu", None, None, collective=world == 2, shard=data, **opts))))
        out[(name, kind, world)] = cells
    return out


def test_option_checks_table(monkeypatch):
    """fit, run_epoch and the StepReplayer constructor over every combination of dataset, kind, world and the three options:
    the exception type and full message of the first check that refuses, or acceptance -- which also pins the order of
    the checks.  (run_epoch with ``stream=True`` and no replayer is refused behind its option checks: "run_replayer".)"""
    got = _option_outcomes(monkeypatch)
    assert set(got) == set(_OPTION_TABLE)
    for row, cells in got.items():
        want = [[c if c == "ok" else _OPTION_REFUSALS[c] for c in (cell.split("/") * 3)[-3:]] for cell in _OPTION_TABLE[row].split()]
        assert len(want) == 8 and [list(c) for c in cells] == want, (row, cells)


# the three staging entry points refuse a bad argument set before any launch (no GPU needed): QOT_ERR_BADARG = -2.  Every row
# changes one thing in an argument set that would be accepted: (entry points, changed arguments)
_STAGE_BADARGS = [
    ("epg", dict(ctl=None)), ("epg", dict(status=None)), ("epg", dict(node_ptr=None)), ("epg", dict(edge_ptr=None)),
    ("epg", dict(dst_ptr=None)), ("epg", dict(dst_edge_ptr=None)), ("ep", dict(graph_of_node=None)), ("g", dict(offs=None)),
    ("epg", dict(sched_cap=0)), ("epg", dict(G=0)), ("epg", dict(N_total=-1)), ("epg", dict(E_total=-1)), ("epg", dict(B=0)),
    ("epg", dict(E=-1)), ("epg", dict(max_edges=-1)), ("epg", dict(V=-1)), ("e", dict(N=-1)), ("e", dict(max_nodes=-1)),
    ("epg", dict(D=-1)), ("epg", dict(F=-1)), ("epg", dict(Y=-1)),
    ("pg", dict(n=0)), ("pg", dict(P=-1)), ("pg", dict(P=1, n=1)), ("pg", dict(P=1, max_edges=0)),
    ("pg", dict(n=(1 << 20) + 1)), ("pg", dict(max_edges=(1 << 20) + 1)), ("pg", dict(B=(1 << 39))), ("pg", dict(P=(1 << 39))),
    ("g", dict(sched_cap=(1 << 57))),                # sched_cap * B ids with B = 4: past INT64_MAX >> 4
    ("epg", dict(edge_index=None)), ("epg", dict(dst_edge_index=None)), ("epg", dict(dst_batch=None)),
    ("epg", dict(dst_edge_attr=None)), ("epg", dict(dst_node_ids=None)), ("epg", dict(dst_x=None)), ("epg", dict(dst_y=None)),
    # two at once
    ("epg", dict(ctl=None, sched_cap=0)), ("pg", dict(P=1, n=1, dst_x=None)), ("g", dict(offs=None, dst_batch=None)),
]


def _stage_call(entry, **kw):
    from gnn_qot_estimation_amd import _lib
    one = 1                                           # a non-null pointer, never dereferenced: every call is refused first
    a = dict(ctl=one, sched_cap=4, status=one, offs=one, node_ptr=one, edge_ptr=one, graph_of_node=one, G=8, N_total=96,
             E_total=200, edge_index=one, edge_attr=one, D=4, node_ids=one, x=one, F=2, y=one, Y=3, B=4, N=48, n=12, E=100,
             P=1, max_nodes=12, max_edges=30, V=12, dst_edge_index=one, dst_edge_attr=one, dst_node_ids=one, dst_x=one,
             dst_y=one, dst_ptr=one, dst_edge_ptr=one, dst_batch=one)
    a.update(kw)
    shard = ("G", "N_total", "E_total", "edge_index", "edge_attr", "D", "node_ids", "x", "F", "y", "Y")
    dst = ("V", "dst_edge_index", "dst_edge_attr", "dst_node_ids", "dst_x", "dst_y", "dst_ptr", "dst_edge_ptr", "dst_batch")
    order = {"qot_shard_stage": ("ctl", "sched_cap", "status", "node_ptr", "edge_ptr", "graph_of_node") + shard
                                + ("B", "N", "E", "max_nodes", "max_edges") + dst,
             "qot_shard_stage_padded": ("ctl", "sched_cap", "status", "node_ptr", "edge_ptr", "graph_of_node") + shard
                                       + ("B", "n", "E", "P", "max_edges") + dst,
             "qot_shard_stage_gather": ("ctl", "sched_cap", "status", "offs", "node_ptr", "edge_ptr") + shard
                                       + ("B", "n", "E", "P", "max_edges") + dst}[entry]
    return getattr(_lib.load(), entry)(*[a[k] for k in order], None)


def test_stage_entry_points_refuse_bad_arguments():
    names = {"e": "qot_shard_stage", "p": "qot_shard_stage_padded", "g": "qot_shard_stage_gather"}
    for entries, kw in _STAGE_BADARGS:
        for e in entries:
            assert _stage_call(names[e], **kw) == -2, (names[e], kw)


def test_shuffle_is_off_by_default():
    from gnn_qot_estimation_amd import harness as Hn, train
    for fn in (Hn.fit, Hn.run_epoch, Hn.StepReplayer.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["shuffle"].default is None and sig["seed"].default == 0
    src = inspect.getsource(train)
    assert "--shuffle" in src and "--seed" in src


# --------------------------------------------------------------------------- 5. conditioning of the whole-run cases
@functools.lru_cache(maxsize=None)
def _run(name, dtype):
    return SC.shuffled_oracle_run(SC.CASES[name], dtype)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_shuffled_case_is_well_conditioned(name):
    r32, r64 = _run(name, torch.float32), _run(name, torch.float64)
    H.assert_trajectory_counters(r32, r64)
    assert r32["best_epoch"] == r64["best_epoch"] and r32["orders"] == r64["orders"]
    err = H.trajectory_errors(r32, r64)
    worst = max(err, key=err.get)
    print(f"{name}: worst fp32-vs-fp64 {worst} {err[worst]:.2e}")
    assert err[worst] <= TOL / 10, (worst, err[worst])
    best, margin = float("-inf"), float("inf")
    for v in r64["val_r2"]:
        if best > float("-inf"):
            need = 10 * TOL * max(1.0, abs(v), abs(best))
            margin = min(margin, abs(v - best) / need)
            assert abs(v - best) >= need, (name, v, best)
        best = max(best, v)
    print(f"{name}: smallest val_r2 margin {margin:.1f} x the required 10 x TOL")
    assert not r64["stopped_early"] and r64["epochs_run"] == SC.CASES[name]["fit"]["num_epochs"]
    # the loop did shuffle: every epoch's order is a permutation of its chunk and no two epochs share one
    assert len({tuple(o) for o in r64["orders"]}) == 8
    assert all(sorted(o) == list(range(84 * (e % 2), 84 * (e % 2) + 84)) for e, o in enumerate(r64["orders"]))


def test_shuffled_loop_differs_from_the_unshuffled_one():
    plain = PC.oracle_run(PC.PAD_CASES["pad_h16"], torch.float64)
    far = H.trajectory_errors(_run("pad_h16", torch.float64), plain)
    assert max(far.values()) > 100 * TOL


def test_validation_pass_of_a_shuffled_run_is_consecutive(monkeypatch):
    """``fit`` hands ``shuffle`` to its training passes only: a validation pass through the same replayer is accepted and
    writes consecutive schedules; a TRAINING pass that disagrees with the replayer is refused.  (Stubs in place of the
    device work: this checks the host plumbing of ``run_epoch``.)"""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    monkeypatch.setattr(torch.cuda, "graph_pool_handle", lambda: None)
    shard = q.PackedGraphs.from_data_list(PC.pad_graphs()).to_device("cpu")
    model = q.TopologicalGNN(**SC.CASES["pad_h16"]["model"])
    cpu = torch.device("cpu")
    rep = Hn.StepReplayer(model, "topological", 3, cpu, None, None, stream=True, shard=shard, pad_edges=True, shuffle=True,
                          seed=SC.SEED)
    rep.plan_padding(Hn.fit_batch_ranges(PC.COUNT, 16, 0.5))
    rep.plan_shuffle(Hn.fit_train_chunks(PC.COUNT, 0.5, 8), 16)
    ran = []
    monkeypatch.setattr(rep, "run", lambda r, training: ran.append((r, training)) or True)
    monkeypatch.setattr(rep, "end_epoch", lambda: None)
    kw = dict(kind="topological", batch_size=16, out_dim=3, device=cpu, criterion=None, replayer=rep, stream=True, pad_edges=True)
    Hn.run_epoch(model, shard, range(168, 204), **kw)                                   # validation, as fit calls it
    assert ran == [((168, 184), False), ((184, 200), False), ((200, 204), False)]
    assert type(rep.slots[(16, False)]) is q.PaddedStageSlot and rep.slots[(16, False)].ctl[:6].tolist() == [0, 2, -1, 0, 168, 184]
    ran.clear()
    Hn.run_epoch(model, shard, range(0, 84), opt=object(), shuffle=True, seed=SC.SEED, epoch=0, **kw)
    assert [t for _, t in ran] == [True] * 6
    order = Hn.epoch_order(range(0, 84), SC.SEED, 0)
    assert type(rep.slots[(16, True)]) is q.GatherStageSlot and rep.slots[(16, True)].ctl[4:84].tolist() == order[:80]
    assert rep.slots[(4, True)].ctl[:8].tolist() == [0, 1, -1, 0] + order[80:]
    for bad in (dict(), dict(shuffle=True, seed=SC.SEED + 1)):
        with pytest.raises(ValueError, match="what the StepReplayer was built with"):
            Hn.run_epoch(model, shard, range(0, 84), opt=object(), **bad, **kw)
