"""Streamed replay, host part: how an epoch's batches are grouped into shapes (one static slot and one captured graph per
shape and direction), and the refusals of ``stream=True``.

The expected shapes are derived by hand from ``harness.split_ranges`` / ``epoch_chunk`` with batch 16 and
``chunk_fraction`` 0.5 on 240 graphs: 168 training graphs in two chunks of 84 = 5 x 16 + 4, 36 validation graphs =
2 x 16 + 4.  A ``topo_h16`` graph has 12 nodes and 2 * 12 + 6 = 30 edges; a ``topo_mixed_nodes`` graph ``g`` has
(8, 10, 12)[g % 3] nodes and (22, 26, 30)[g % 3] edges, so 16 consecutive graphs starting at ``g0`` hold 158 / 160 / 162
nodes for ``g0 % 3`` = 0 / 1 / 2 (five full cycles of 30 nodes plus the first graph of the next); the ragged batches
start at 80, 164 and 200, all with ``g0 % 3`` = 2: 12 + 8 + 10 + 12 = 42 nodes.  Edges: 2 N + 6 B.
"""
import pytest
import torch

import helpers as H
import stream_cases as SC


def _counts(groups):
    return {shape: len(los) for shape, los in groups.items()}


def _mixed(g0, B):
    n = sum((8, 10, 12)[g % 3] for g in range(g0, g0 + B))
    return (B, n, 2 * n + 6 * B)


def test_schedule_of_the_uniform_case():
    s = SC.case_schedules(H.TRAJECTORY_CASES["topo_h16"])
    assert _counts(s["train"]) == {(16, 192, 480): 10, (4, 48, 120): 2}
    assert _counts(s["eval"]) == {(16, 192, 480): 2, (4, 48, 120): 1}
    # visiting order inside a shape: chunk 0 (graphs 0 .. 83), then chunk 1 (84 .. 167); validation 168 .. 203
    assert s["train"][(16, 192, 480)] == [0, 16, 32, 48, 64, 84, 100, 116, 132, 148]
    assert s["train"][(4, 48, 120)] == [80, 164]
    assert s["eval"][(16, 192, 480)] == [168, 184] and s["eval"][(4, 48, 120)] == [200]
    assert SC.case_graph_count(H.TRAJECTORY_CASES["topo_h16"]) == 4


def test_schedule_of_the_mixed_case():
    s = SC.case_schedules(H.TRAJECTORY_CASES["topo_mixed_nodes"])
    assert _counts(s["train"]) == {(16, 158, 412): 4, (16, 160, 416): 4, (16, 162, 420): 2, (4, 42, 108): 2}
    assert _counts(s["eval"]) == {(16, 158, 412): 1, (16, 160, 416): 1, (4, 42, 108): 1}
    # the same from the per-graph rule: full batches start at 0, 16, ... and 84, 100, ...; ragged ones at 80, 164, 200
    for lo in (0, 16, 32, 48, 64, 84, 100, 116, 132, 148):
        assert lo in s["train"][_mixed(lo, 16)]
    for lo in (80, 164):
        assert lo in s["train"][_mixed(lo, 4)]
    assert s["eval"][_mixed(168, 16)] == [168] and s["eval"][_mixed(184, 16)] == [184] and s["eval"][_mixed(200, 4)] == [200]
    assert SC.case_graph_count(H.TRAJECTORY_CASES["topo_mixed_nodes"]) == 7


def test_batch_ranges_and_shape():
    from gnn_qot_estimation_amd import harness as Hn
    assert Hn.batch_ranges(range(5, 40), 16) == [(5, 21), (21, 37), (37, 40)]
    assert Hn.batch_ranges(range(0), 16) == []
    with pytest.raises(ValueError):
        Hn.batch_ranges(range(0, 10, 2), 4)
    with pytest.raises(ValueError):
        Hn.batch_ranges([0, 1, 2], 4)
    node_ptr = torch.tensor([0, 3, 5, 9, 10])
    edge_ptr = torch.tensor([0, 4, 4, 10, 12])
    assert Hn.batch_shape(node_ptr, edge_ptr, 1, 3) == (2, 6, 6)
    assert Hn.stream_schedule(node_ptr, edge_ptr, [(0, 2), (2, 4), (1, 3)]) == {(2, 5, 4): [0], (2, 5, 8): [2], (2, 6, 6): [1]}


def _topo(case="topo_h16"):
    import gnn_qot_estimation_amd as q
    c = H.TRAJECTORY_CASES[case]
    return q.TopologicalGNN(**c["model"]), H.trajectory_graphs(c), c


def test_stream_refuses_a_host_list_and_a_pinned_shard():
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    model, graphs, c = _topo()
    with pytest.raises(ValueError, match="HBM-resident"):
        Hn.fit(model, graphs, kind="topological", device="cpu", log=lambda s: None, stream=True, **c["fit"])
    shard = q.PackedGraphs.from_data_list(graphs)          # host shard (what pin() returns, page-locked or not)
    assert shard.device is None
    with pytest.raises(ValueError, match="HBM-resident"):
        Hn.fit(model, shard, kind="topological", device="cpu", log=lambda s: None, stream=True, **c["fit"])
    shard.pinned = True                                     # as after pin(): still not resident
    with pytest.raises(ValueError, match="HBM-resident"):
        Hn.fit(model, shard, kind="topological", device="cpu", log=lambda s: None, stream=True, **c["fit"])
    with pytest.raises(ValueError, match="HBM-resident"):
        Hn.run_epoch(model, shard, range(0, 16), kind="topological", batch_size=16, out_dim=3, device="cpu",
                     criterion=None, stream=True)
    with pytest.raises(ValueError, match="HBM-resident"):
        Hn.StepReplayer(model, "topological", 3, "cpu", None, None, stream=True, shard=shard)


def test_stream_refuses_lightpath():
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    c = H.TRAJECTORY_CASES["lp_c8_skip_mid"]
    model = q.LightpathGNN(**c["model"])
    with pytest.raises(ValueError, match="topological"):
        Hn.fit(model, H.trajectory_graphs(c), kind="lightpath", device="cpu", log=lambda s: None, stream=True, **c["fit"])


def test_stream_is_off_by_default():
    import inspect
    from gnn_qot_estimation_amd import harness as Hn
    for fn in (Hn.fit, Hn.run_epoch, Hn.StepReplayer.__init__):
        assert inspect.signature(fn).parameters["stream"].default is None
    assert Hn.History().replay_counts == {}
