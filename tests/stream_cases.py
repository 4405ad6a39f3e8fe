"""What a streamed run of a ``helpers.TRAJECTORY_CASES`` case visits, from the split alone (shared by the streamed-replay
tests): the batches of one pass over all training chunks and of one validation pass, grouped by shape."""
import torch

import helpers as H


def case_offsets(case):
    """(node_ptr, edge_ptr) of the case's graphs, as ``PackedGraphs`` keeps them (host int64)."""
    graphs = H.trajectory_graphs(case)
    n = torch.tensor([0] + [g.num_nodes for g in graphs], dtype=torch.long).cumsum(0)
    e = torch.tensor([0] + [g.num_edges for g in graphs], dtype=torch.long).cumsum(0)
    return n, e


def case_schedules(case):
    """``{"train": {(B, N, E): [lo, ...]}, "eval": {...}}``: one pass over every training chunk, one validation pass."""
    from gnn_qot_estimation_amd import harness as Hn
    node_ptr, edge_ptr = case_offsets(case)
    fit = case["fit"]
    tr, va, _ = Hn.split_ranges(node_ptr.numel() - 1)
    train = []
    for epoch in range(int(1 / fit["chunk_fraction"])):
        chunk = Hn.epoch_chunk(epoch, len(tr), fit["chunk_fraction"])
        train += Hn.batch_ranges(range(tr[0] + chunk[0], tr[0] + chunk[-1] + 1), fit["batch_size"])
    return {"train": Hn.stream_schedule(node_ptr, edge_ptr, train),
            "eval": Hn.stream_schedule(node_ptr, edge_ptr, Hn.batch_ranges(va, fit["batch_size"]))}


def case_graph_count(case):
    """Captured graphs a streamed run ends with: distinct (shape, direction) pairs."""
    s = case_schedules(case)
    return len(s["train"]) + len(s["eval"])
