"""Data and plain restatements shared by the padded streamed-replay tests (tests/test_stream_pad_cpu.py,
tests/test_gpu_stream_pad.py).

The shard: 240 topological graphs of 12 nodes whose EDGE COUNTS DIFFER, ``e_g = 26 + 2 ((g g + g // 5) mod 6)`` (26 .. 36),
as the reference's ``to_graph.create_topological_graph`` gives one edge per distinct connection of a sample; targets as
``helpers.trajectory_graphs`` builds them; the fit settings of ``helpers._topo_fit()`` (batch 16, two chunks of 84 = 5 x 16
+ 4 graphs, 36 = 2 x 16 + 4 validation graphs).

``pad_layout`` restates, with per-edge Python loops, what the staging launch writes behind the real slice.  It shares no
code with ``csrc/stage.hip`` or ``loader.py``.
"""
import torch

import helpers as H

COUNT, N_NODES, EDGE_DIM = 240, 12, 4
# Graph g is drawn from the generator's seed g + SEED_OFFSET.  With offset 0 the H = 64 run fails the conditioning rule of
# DESIGN.md section 2 (oracle loop fp32 against fp64: 4.0e-4 in the momentum buffers, whose last value is a near-cancelling
# sum; bound TOL / 10 = 1e-5), so that data set is replaced, not the bound: 1000 is the first offset of 0, 1000, 2000, ...
# that meets the rule at both widths (H = 16: 1.4e-6, H = 64: 7.5e-6; smallest val_r2 margin 11 x the required one).  Edge
# counts, node count and targets are unaffected.  tests/test_stream_pad_cpu.py checks the rule on every run.
SEED_OFFSET = 1000

PAD_CASES = {
    "pad_h16": dict(kind="topological", model=H._topo_model(16), fit=H._topo_fit()),
    # graph-form TransformerConv and the split-bf16 NNConv kernels
    "pad_h64": dict(kind="topological", model=H._topo_model(64), fit=H._topo_fit()),
}

# dropout ON (p = 0.5): the oracle loop runs the kernels' masks (oracle/dropout.py).  Pad graphs are appended AFTER the real
# ones, so real elements keep their flat indices and the oracle's masks are the [N_real, H] / [B_real, H] prefixes of the
# slot's -- which is what the loop draws for the unpadded batch.
PAD_DROP_CASES = {
    "pad_h64_drop": dict(kind="topological", model=H._topo_model(64, p=0.5), fit=H._topo_fit(), dropout_seed=H.DROPOUT_SEED),
}
ALL_CASES = dict(PAD_CASES, **PAD_DROP_CASES)


def edge_count(g):
    return 26 + 2 * ((g * g + g // 5) % 6)


def pad_graphs():
    """The shard as a host list of ``Data`` (seeded; same graphs on every call)."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    out = []
    for g in range(COUNT):
        b = S.topological_batch(2, 1, n=N_NODES, e=edge_count(g), edge_dim=EDGE_DIM, first_graph=g + SEED_OFFSET)
        assert b.edge_index.shape[1] == edge_count(g)
        y = b.edge_attr[:, :3].mean(0, keepdim=True)
        out.append(q.Data(edge_index=b.edge_index, edge_attr=b.edge_attr, node_ids=b.node_ids, y=y, num_nodes=N_NODES))
    return out


def offsets():
    """(node_ptr, edge_ptr) of the shard from the edge-count rule alone (host int64)."""
    n = torch.arange(COUNT + 1, dtype=torch.long) * N_NODES
    e = torch.tensor([0] + [edge_count(g) for g in range(COUNT)], dtype=torch.long).cumsum(0)
    return n, e


def run_ranges(fit):
    """``(training ranges of one pass over every chunk, validation ranges)`` of a ``fit`` with these settings."""
    from gnn_qot_estimation_amd import harness as Hn
    tr, va, _ = Hn.split_ranges(COUNT)
    train = []
    for epoch in range(int(1 / fit["chunk_fraction"])):
        chunk = Hn.epoch_chunk(epoch, len(tr), fit["chunk_fraction"])
        train += Hn.batch_ranges(range(tr[0] + chunk[0], tr[0] + chunk[-1] + 1), fit["batch_size"])
    return train, Hn.batch_ranges(va, fit["batch_size"])


def oracle_run(case, dtype):
    """``oracle.train_loop.train`` on a case of ``ALL_CASES``, with the parameter names added (a case with a
    ``dropout_seed``: restated masks from step counter 0, as ``helpers.oracle_trajectory``)."""
    from oracle import train_loop
    model = H.trajectory_oracle_model(case)
    kw = dict(dropout=(case["dropout_seed"], 0)) if case.get("dropout_seed") is not None else {}
    res = train_loop.train(model, pad_graphs(), case["kind"], dtype=dtype, **case["fit"], **kw)
    res["param_names"] = [n for n, p in model.named_parameters() if p.requires_grad]
    return res


def pad_layout(B, n, max_m, P, E_real, E_cap):
    """What lies behind the real slice of a padded slot, as Python lists: pad graph ``p`` owns nodes
    ``[(B + p) n, (B + p + 1) n)`` and takes ``min(max_m, spare left)`` edges, edge ``k`` of it running
    ``k mod n -> (k + 1) mod n`` inside that range."""
    spare = E_cap - E_real
    assert 0 <= spare <= P * max_m
    src, dst, sizes = [], [], []
    for p in range(P):
        m = min(max_m, spare)
        spare -= m
        first = (B + p) * n
        for k in range(m):
            src.append(first + k % n)
            dst.append(first + (k + 1) % n)
        sizes.append(m)
    assert spare == 0
    edge_ptr, total = [], E_real
    for m in sizes:
        total += m
        edge_ptr.append(total)
    return {
        "edge_index": [src, dst],                                           # columns E_real .. E_cap of the slot
        "sizes": sizes,                                                     # edges per pad graph
        "node_ids": [v for _ in range(P) for v in range(n)],                # nodes B n .. (B + P) n
        "batch": [B + p for p in range(P) for _ in range(n)],
        "ptr": [(B + p + 1) * n for p in range(P)],                         # entries B + 1 .. B + P
        "edge_ptr": edge_ptr,
    }
