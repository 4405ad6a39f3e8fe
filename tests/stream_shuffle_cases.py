"""Data and plain restatements shared by the shuffled streamed-replay tests (tests/test_stream_shuffle_cpu.py,
tests/test_gpu_stream_shuffle.py): ``fit(..., stream=True, pad_edges=True, shuffle=True, seed=s)``, DESIGN.md section 4.11.

The shard is the unequal shard of tests/stream_pad_cases.py (240 graphs of 12 nodes, 26 .. 36 edges, batch 16, ragged
batch of 4), the cases are its ``PAD_CASES`` (H = 16 and H = 64, dropout off), and ``edge5_graphs`` is a tiny second shard
whose ``edge_attr`` rows hold FIVE floats and whose graphs have 9 nodes: fp32 segments then start at any multiple of 4
bytes, int64 segments at odd and even multiples of 8.

``shuffled_oracle_run`` is the fp64 loop the whole runs are compared with: ``oracle.train_loop``'s pieces (split, chunk,
one pass, early stopping) with each epoch's chunk handed to its pass in ``harness.epoch_order(chunk, seed, epoch)`` -- the
one function the plan, the streamed run and the eager loop all call.

SEED.  Conditioning rule of DESIGN.md section 2 (the loop in fp32 against itself in fp64 within TOL / 10 = 1e-5 in
``helpers.trajectory_errors``; tests/test_stream_shuffle_cpu.py checks it on every run): a seed that fails it is
replaced, never the bound.  Seeds were tried in the order 0, 1, 2, ...: see ``SEED_FIGURES``.  Seed 0, the first one tried,
meets the rule (smallest ``val_r2`` margin 17 x the required 10 x TOL at H = 16, 62 x at H = 64); seed 1 would not
(H = 64: 1.8e-5 in ``momentum:conv2.nn.0.bias``).
"""
import torch

import helpers as H
import stream_pad_cases as PC

CASES = PC.PAD_CASES
# worst fp32-vs-fp64 figure of the shuffled oracle loop per seed, (H = 16, H = 64); the first seed with both <= 1e-5 is SEED
SEED_FIGURES = {0: (1.1e-6, 2.3e-6), 1: (9.2e-7, 1.8e-5), 2: (9.0e-7, 1.4e-6)}
SEED = 0


def shuffled_oracle_run(case, dtype, seed=None):
    """The reference training loop with shuffled epochs on the unequal shard; the result dict of
    ``oracle.train_loop.train`` plus ``param_names``."""
    from oracle import train_loop as TL
    from gnn_qot_estimation_amd import harness as Hn
    seed = SEED if seed is None else seed
    fit = case["fit"]
    model = H.trajectory_oracle_model(case)
    model.to(dtype)
    graphs = [TL._cast(g, dtype) for g in PC.pad_graphs()]
    train_idx, val_idx, _ = TL.split(len(graphs))
    val_graphs = [graphs[i] for i in val_idx]
    params = [p for p in model.parameters() if p.requires_grad]
    optimizer = torch.optim.SGD(params, lr=fit["lr"], momentum=fit["momentum"])
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=fit["step_size"], gamma=fit["gamma"])
    criterion = torch.nn.SmoothL1Loss()
    stopper = TL.EarlyStopping(fit["patience"])
    res = {"loss": [], "r2": [], "val_loss": [], "val_r2": [], "skipped_graphs": 0, "stopped_early": False, "epochs_run": 0,
           "best_state_dict": None, "orders": []}
    for epoch in range(fit["num_epochs"]):
        pos = TL.chunk_indices(epoch, len(train_idx), fit["chunk_fraction"])
        order = Hn.epoch_order(range(train_idx[pos[0]], train_idx[pos[-1]] + 1), seed, epoch)
        res["orders"].append(order)
        t = TL._one_pass(model, [graphs[g] for g in order], case["kind"], fit["batch_size"], fit["output_dim"], criterion,
                         optimizer)
        v = TL._one_pass(model, val_graphs, case["kind"], fit["batch_size"], fit["output_dim"], criterion)
        res["loss"].append(t["loss"]); res["r2"].append(t["r2"])
        res["val_loss"].append(v["loss"]); res["val_r2"].append(v["r2"])
        res["epochs_run"] = epoch + 1
        improved, stop = stopper.update(epoch, v["r2"])
        if improved:
            res["best_state_dict"] = TL._snapshot(model)
        if stop:
            res["stopped_early"] = True
            break
        scheduler.step()
    res["dropout_draws"] = 0
    res["best_val_r2"], res["best_epoch"] = stopper.best, stopper.best_epoch
    res["state_dict"] = TL._snapshot(model)
    res["momentum_buffers"] = [optimizer.state[p]["momentum_buffer"].detach().clone() for p in params]
    res["param_names"] = [n for n, p in model.named_parameters() if p.requires_grad]
    return res


def brute_force_plan(edge_counts, chunks, batch_size, seed, n, max_m):
    """``harness.stream_shuffle_plan`` restated with plain loops over per-graph edge counts; also returns every batch's edge
    total as ``{B: [e, ...]}``."""
    from gnn_qot_estimation_amd import harness as Hn
    seen = {}
    for epoch, chunk in enumerate(chunks):
        order = Hn.epoch_order(chunk, seed, epoch)
        k = 0
        while k < len(order):
            ids = order[k:k + batch_size]
            e = 0
            for g in ids:
                e += edge_counts[g]
            seen.setdefault(len(ids), []).append(e)
            k += batch_size
    plan = {}
    for B, es in seen.items():
        lo, hi = min(es), max(es)
        P = 0
        while P * max_m < hi - lo:
            P += 1
        plan[B] = {"E_cap": hi, "E_min": lo, "P": P, "shape": (B + P, (B + P) * n, hi)}
    return plan, seen


EDGE5 = dict(count=24, n=9, D=5, max_m=15)


def edge5_graphs():
    """24 graphs of 9 nodes with 9 .. 15 edges (odd and even counts), ``edge_attr`` of 5 floats per edge, permuted node
    ids, ``x`` rows of 3 floats."""
    import gnn_qot_estimation_amd as q
    gen = torch.Generator().manual_seed(5)
    n, D = EDGE5["n"], EDGE5["D"]
    out = []
    for g in range(EDGE5["count"]):
        e = 9 + (g * 5) % 7
        src = torch.randint(0, n, (e,), generator=gen)
        dst = (src + 1 + torch.randint(0, n - 1, (e,), generator=gen)) % n
        out.append(q.Data(edge_index=torch.stack([src, dst]), edge_attr=torch.rand(e, D, generator=gen),
                          y=torch.rand(1, 3, generator=gen), x=torch.rand(n, 3, generator=gen),
                          node_ids=torch.randperm(n, generator=gen), num_nodes=n))
    return out
