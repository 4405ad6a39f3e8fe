"""Streamed replay against the per-batch replay of another tree (the parent commit), on a synthetic HBM-resident shard of
DISTINCT graphs (``synthetic.topological_batch`` seeds), dropout 0.5.

    python tools/bench_stream_fit.py --scale reference|headline --parent-tree DIR [--out FILE.json]

``DIR`` holds the other tree's ``gnn_qot_estimation_amd`` package with its built ``libqot_gnn.so`` (a checkout of the
parent commit, built with ``make -C gnn_qot_estimation_amd/csrc``).  Every measurement runs in a fresh child process
of this script (one tree per process), the two trees alternating:

 (a) steady-state device time per step: events around ``--replays`` (>= 200) replays after warm-up, several rounds,
     median.  Streamed: ``StepReplayer(stream=True)`` walking the shard batch by batch (stage + in-graph index build +
     step).  Per-batch: the other tree's ``StepReplayer`` replaying one cached batch object (index cached).
 (b) wall time of the reference's schedule (35 epochs over 10 chunks, ``harness.fit`` end to end, host clock around a
     final synchronise): ``fit(stream=True)`` here, ``fit(replay=True)`` there; the process's first run (which also
     loads every code object) and a second one with a fresh model, replayer and captures.
 (c) captured graphs and ``torch.cuda.memory_reserved()`` after (b), both modes (of the process: two runs).

    scale       nodes / graph   edges / graph   hidden   batch
    reference   75              300             16       512
    headline    100             400             64       1024

``--unequal``: the shard's graphs keep their node count but differ in EDGES (``unequal_edge_count``: spread evenly over
148 .. 452 around the scale's 300, 148 = 2 (n - 1) being the generator's floor of a spanning tree), as the reference's
topological data does.  Compared on that shard: the other tree's two modes -- ``fit(replay=True)`` and ``fit(stream=True)``
with exact-shape slots -- against ``fit(stream=True, pad_edges=True)`` here (wall time of both runs of a process, captured
graphs, reserved memory); and (a) the padded streamed step on it against the exact-shape streamed step on the equal-sized
shard of the same mean size (both in this tree), with the plan's ``P``, ``E_cap``, ``E_min``.

``--unequal --shuffle``: (a) alone, on the unequal shard -- the shuffled streamed step of this tree
(``StepReplayer(stream=True, pad_edges=True, shuffle=True)``: gather staging of ``epoch_order`` batches, epoch after epoch
over the whole shard) against the other tree's consecutive padded streamed step, alternating fresh processes; with both
plans.  ``--shard-cache DIR`` keeps the generated shards between calls.

Prints one JSON object (and writes it to ``--out``).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

SCALES = {"reference": dict(n=75, e=300, hidden=16, batch=512), "headline": dict(n=100, e=400, hidden=64, batch=1024)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unequal_edge_count(g, e):
    """Directed edges of graph ``g`` of the unequal shard: ``e - 152 .. e + 152`` in steps of 2, mean ``e``."""
    return e + 2 * ((g * 7919) % 153 - 76)


def unequal_shard(graphs, n, e):
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    out = []
    for g in range(graphs):
        b = S.topological_batch(2, 1, n=n, e=unequal_edge_count(g, e), first_graph=g)
        out.append(q.Data(edge_index=b.edge_index, edge_attr=b.edge_attr, node_ids=b.node_ids, y=b.y, num_nodes=n))
    return q.PackedGraphs.from_data_list(out)


def _child(args):
    sys.path.insert(0, args.tree)
    import torch
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import harness as Hn
    from gnn_qot_estimation_amd.dataset import load_shard
    assert os.path.realpath(os.path.dirname(os.path.dirname(q.__file__))) == os.path.realpath(args.tree), q.__file__
    sc = SCALES[args.scale]
    dev = torch.device("cuda:0")
    shard = load_shard(args.shard)[0].to_device(dev)
    torch.manual_seed(0)
    model = q.TopologicalGNN(sc["n"], sc["hidden"], 3, 4, dropout_p=0.5).to(dev)
    B = sc["batch"]
    out = {"mode": args.child}
    if args.child in ("step_streamed", "step_per_batch", "step_padded", "step_shuffled"):
        flat = Hn.FlatModel(model)
        opt = Hn.FusedSGD(flat, lr=0.01, momentum=0.9, device_lr=True)
        opt.lr = 0.01
        nb = len(shard) // B
        if args.child == "step_shuffled":
            rep = Hn.StepReplayer(model, "topological", 3, dev, flat, opt, stream=True, shard=shard, pad_edges=True,
                                  shuffle=True, seed=0)
            steps = 3 + 20 + args.replays
            epochs = -(-steps // nb)
            chunks = [range(0, nb * B)] * epochs      # every epoch walks the whole shard in a fresh order
            order = [g for e in range(epochs) for g in Hn.epoch_order(chunks[e], 0, e)][:steps * B]
            ranges = [(0, B)] * steps                 # a gather slot is keyed by the graph count alone
            rep.schedule_capacity = steps
            out["pad_plan"] = {str(k): v for k, v in rep.plan_shuffle(chunks, B).items()}
            feed = lambda k: ranges[k]
            begin = lambda: rep.begin_epoch(ranges, True, order=order)
        elif args.child in ("step_streamed", "step_padded"):
            pad = args.child == "step_padded"
            rep = Hn.StepReplayer(model, "topological", 3, dev, flat, opt, stream=True, shard=shard,
                                  **(dict(pad_edges=True) if pad else {}))
            ranges = [((k % nb) * B, (k % nb) * B + B) for k in range(3 + 20 + args.replays)]
            rep.schedule_capacity = len(ranges)       # the walk wraps round the shard inside one schedule
            if pad:
                out["pad_plan"] = {str(k): v for k, v in rep.plan_padding(ranges).items()}
            feed = lambda k: ranges[k]
            begin = lambda: rep.begin_epoch(ranges, True)
        else:
            rep = Hn.StepReplayer(model, "topological", 3, dev, flat, opt)
            data = shard.device_batch(0, B, cache=True)
            feed = lambda k: data
            begin = lambda: None
        rounds = []
        for _ in range(args.rounds):
            begin()
            for k in range(3 + 20):                   # eager, capture, replay; then warm-up replays
                rep.run(feed(k), True)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for k in range(23, 23 + args.replays):
                rep.run(feed(k), True)
            t1.record()
            torch.cuda.synchronize(dev)
            rounds.append(t0.elapsed_time(t1) * 1e3 / args.replays)
            if args.child != "step_per_batch":
                rep.end_epoch()
        out.update(step_us_rounds=rounds, step_us_median=statistics.median(rounds), graphs=len(rep.graphs),
                   batches_walked=nb if args.child != "step_per_batch" else 1)
    else:
        made = []

        class _Rec(Hn.StepReplayer):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                made.append(self)

        Hn.StepReplayer = _Rec
        kw = {"fit_streamed": dict(stream=True), "fit_padded": dict(stream=True, pad_edges=True),
              "fit_per_batch": dict(replay=True)}[args.child]
        walls = []
        for _ in range(2):        # the first run also loads every code object; the second (a fresh model, replayer and
            made.clear()          # captures) is the run alone
            torch.manual_seed(0)
            model = q.TopologicalGNN(sc["n"], sc["hidden"], 3, 4, dropout_p=0.5).to(dev)
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            hist = Hn.fit(model, shard, kind="topological", batch_size=B, num_epochs=35, patience=10 ** 6, device=dev,
                          log=lambda s: None, **kw)
            torch.cuda.synchronize(dev)
            walls.append(time.perf_counter() - t)
        out.update(fit_wall_s=walls[0], fit_wall_warm_s=walls[1], epochs_run=hist.epochs_run, graphs=len(made[0].graphs),
                   memory_reserved_mb=torch.cuda.memory_reserved(dev) / 2 ** 20,
                   memory_allocated_mb=torch.cuda.memory_allocated(dev) / 2 ** 20,
                   replay_counts=getattr(hist, "replay_counts", None), final_loss=hist.loss[-1],
                   pad_plan={str(k): v for k, v in getattr(made[0], "pad_plan", {}).items()})
    print("CHILD_JSON " + json.dumps(out), flush=True)


def _run_child(mode, tree, args, shard):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree, "--scale", args.scale, "--shard", shard,
           "--replays", str(args.replays), "--rounds", str(args.rounds)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    if res.returncode != 0:
        raise RuntimeError(f"{mode} in {tree} failed with status {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    line = [l for l in res.stdout.splitlines() if l.startswith("CHILD_JSON ")][-1]
    return json.loads(line[len("CHILD_JSON "):])


def _commit(tree):
    try:
        return subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", choices=list(SCALES), default="headline")
    ap.add_argument("--parent-tree", default=None, help="tree of the commit to compare with (built)")
    ap.add_argument("--graphs", type=int, default=30000, help="graphs in the shard (70 %% train, 10 chunks)")
    ap.add_argument("--unequal", action="store_true", help="graphs of unequal edge counts: the padded mode against both "
                                                            "modes of the other tree (module docstring)")
    ap.add_argument("--shuffle", action="store_true", help="with --unequal: the shuffled streamed step here against the "
                                                            "other tree's consecutive padded streamed step")
    ap.add_argument("--shard-cache", default=None, help="directory that keeps the generated shards between calls")
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2, help="alternations of the two trees per measurement")
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--this-commit", default=None)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--shard", default=None)
    args = ap.parse_args()
    if args.child:
        return _child(args)
    if args.replays < 200:
        ap.error("--replays must be at least 200")
    sys.path.insert(0, ROOT)
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    from gnn_qot_estimation_amd.dataset import save_shard
    sc = SCALES[args.scale]
    res = {"scale": args.scale, **sc, "graphs_in_shard": args.graphs, "dropout": 0.5, "replays": args.replays,
           "this_commit": args.this_commit or _commit(ROOT),
           "parent_commit": args.parent_commit or (_commit(args.parent_tree) if args.parent_tree else None)}
    if args.unequal:
        return _main_unequal(args, res, sc)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "shard.pt")
        save_shard(path, q.PackedGraphs.from_batch(S.topological_batch(2, args.graphs, n=sc["n"], e=sc["e"])))
        trees = [("streamed", ROOT)] + ([("per_batch", args.parent_tree)] if args.parent_tree else [])
        for what in ("step", "fit"):
            for rep in range(args.repeats):
                for mode, tree in trees:
                    r = _run_child(f"{what}_{mode}", tree, args, path)
                    res.setdefault(f"{what}_{mode}", []).append(r)
                    print(f"# {what}_{mode} [{rep}]: " + json.dumps({k: v for k, v in r.items() if k != "mode"}),
                          flush=True)
    med = lambda key, field: statistics.median(r[field] for r in res[key]) if key in res else None
    res["summary"] = {
        "streamed_step_us": med("step_streamed", "step_us_median"), "per_batch_step_us": med("step_per_batch", "step_us_median"),
        "streamed_fit_s": med("fit_streamed", "fit_wall_s"), "per_batch_fit_s": med("fit_per_batch", "fit_wall_s"),
        "streamed_fit_warm_s": med("fit_streamed", "fit_wall_warm_s"), "per_batch_fit_warm_s": med("fit_per_batch", "fit_wall_warm_s"),
        "streamed_graphs": med("fit_streamed", "graphs"), "per_batch_graphs": med("fit_per_batch", "graphs"),
        "streamed_reserved_mb": med("fit_streamed", "memory_reserved_mb"),
        "per_batch_reserved_mb": med("fit_per_batch", "memory_reserved_mb"),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def _main_unequal(args, res, sc):
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    from gnn_qot_estimation_amd.dataset import save_shard
    other = args.parent_tree or ROOT
    res.update(unequal=True, edge_counts=[sc["e"] - 152, sc["e"] + 152],
               other_tree_is_parent=bool(args.parent_tree))
    with tempfile.TemporaryDirectory() as tmp:
        if args.shard_cache:
            os.makedirs(args.shard_cache, exist_ok=True)
            tmp = args.shard_cache
        uneq = os.path.join(tmp, f"unequal_{args.scale}_{args.graphs}.pt")
        equal = os.path.join(tmp, f"equal_{args.scale}_{args.graphs}.pt")
        if not os.path.exists(uneq):
            save_shard(uneq, unequal_shard(args.graphs, sc["n"], sc["e"]))
        if args.shuffle:
            return _main_shuffle(args, res, other, uneq)
        if not os.path.exists(equal):
            save_shard(equal, q.PackedGraphs.from_batch(S.topological_batch(2, args.graphs, n=sc["n"], e=sc["e"])))
        runs = [("fit_padded", ROOT, uneq, "fit_padded"), ("fit_streamed", other, uneq, "fit_streamed_exact"),
                ("fit_per_batch", other, uneq, "fit_per_batch"), ("step_padded", ROOT, uneq, "step_padded"),
                ("step_streamed", ROOT, equal, "step_streamed_equal")]
        for rep in range(args.repeats):
            for mode, tree, shard, key in runs:
                r = _run_child(mode, tree, args, shard)
                res.setdefault(key, []).append(r)
                print(f"# {key} [{rep}]: " + json.dumps({k: v for k, v in r.items() if k != "mode"}), flush=True)
    res["summary"] = {key: {"fit_wall_s": [r["fit_wall_s"] for r in res[key]],
                            "fit_wall_warm_s": [r["fit_wall_warm_s"] for r in res[key]],
                            "graphs": res[key][0]["graphs"], "memory_reserved_mb": res[key][0]["memory_reserved_mb"]}
                      for key in ("fit_padded", "fit_streamed_exact", "fit_per_batch")}
    res["summary"]["step_padded_us"] = [r["step_us_median"] for r in res["step_padded"]]
    res["summary"]["step_streamed_equal_us"] = [r["step_us_median"] for r in res["step_streamed_equal"]]
    res["summary"]["pad_plan"] = res["fit_padded"][0]["pad_plan"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def _main_shuffle(args, res, other, uneq):
    res["shuffle"] = True
    for rep in range(args.repeats):
        for mode, tree, key in (("step_shuffled", ROOT, "step_shuffled"), ("step_padded", other, "step_padded_other")):
            r = _run_child(mode, tree, args, uneq)
            res.setdefault(key, []).append(r)
            print(f"# {key} [{rep}]: " + json.dumps({k: v for k, v in r.items() if k != "mode"}), flush=True)
    res["summary"] = {"step_shuffled_us": [r["step_us_median"] for r in res["step_shuffled"]],
                      "step_padded_other_us": [r["step_us_median"] for r in res["step_padded_other"]],
                      "shuffle_plan": res["step_shuffled"][0]["pad_plan"], "pad_plan": res["step_padded_other"][0]["pad_plan"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
