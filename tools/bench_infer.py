"""Milliseconds per call of ``TopologicalPredictor(model)(data)`` (the single-launch inference kernel, csrc/infer.hip)
against the two ways the default path offers for the same eval-mode forward:

  (a) ``model.eval()(data)`` under ``torch.no_grad()``, eager;
  (b) the same forward replayed from a captured graph of that one batch (a lower bound for (a): a planning tool that
      scores fresh candidates has no captured batch to replay).

Shapes: the reference's scale (V = 75, H = 16, D = 4, O = 3; 75-node graphs of 600 directed edges) at B = 1, 8 and 512,
and the headline shape (n = 100, e = 400, H = 64) at B = 1 and 1024.  Per shape: the outputs of the three ways are compared
first; then WARMUP calls of each, then ROUNDS rounds that alternate the three ways, each call timed by the host clock between
two device synchronisations; the figure is the median over the rounds (min and max are printed with it).  One JSON line
per shape, and a markdown table at the end; ``--out FILE`` also writes the JSON lines there.

    python tools/bench_infer.py [--rounds 50] [--warmup 10] [--out prof_out/bench_infer.jsonl]

``--kind lightpath``: ``LightpathPredictor`` (csrc/infer_lightpath.hip) instead -- milliseconds per call of ``predict(data)``,
``predict.per_graph(data)`` and the eager eval ``model(data)`` under ``torch.no_grad()``, alternating in one process, on
``synthetic.lightpath_batch`` graphs at C = 32, F = 5 and B = 1, 8, 512 and 65 536 (64 distinct graphs, tiled).  Every call
sees the same batch object, so the LUT rows of ``predict`` and of the model are the cached ones (no host read inside the
timed calls).  Per way the median and the interquartile range; a difference of two medians that does not exceed the larger
of the two interquartile ranges is reported as no difference.

    python tools/bench_infer.py --kind lightpath [--out profiles/bench_infer_lightpath.jsonl]

``--mc T``: Monte-Carlo dropout (csrc/infer_mc.hip) -- milliseconds per call of ``predict.sample(data, T)``
(one launch for the T draws, two small torch launches for mean and std) against the only other way to T stochastic
forwards: ``model.train()`` and T calls of ``model(data)`` under ``torch.no_grad()`` (the stack of their outputs is not
reduced: the eager side is charged less than it would cost).  p = 0.5 at all three sites; the reference shape at B = 1, 8
and 512 and the headline shape at B = 1.  The draws of both ways are compared first (draw t of ``sample(first_step=1)`` is
the train-mode forward at dropout step 1 + t); then both alternate in one process, median and interquartile range as for
``--kind lightpath``.

    python tools/bench_infer.py --mc 32 [--out profiles/bench_infer_mc.jsonl]

``--grad``: per-link sensitivity (csrc/infer_grad.hip) -- milliseconds per call of
``predict.sensitivity(data)`` (output and the whole Jacobian wrt the edge features, one launch) against the other route to
the same numbers: ``model.eval()`` forward with ``edge_attr.requires_grad_()``, parameters frozen, one
``backward(retain_graph=True)`` per output.  The reference shape at B = 1 and 512 and the headline shape at B = 1; the two
Jacobians are compared first; then both alternate in one process, each call between two ``torch.cuda.Event``s, median and
interquartile range as above.

    python tools/bench_infer.py --grad [--out profiles/bench_infer_grad.jsonl]

``--kind lightpath --grad``: per-neighbour sensitivity of the LUT rows (csrc/infer_lightpath_grad.hip) --
milliseconds per call of ``predict.sensitivity(data)`` (the rows and their Jacobian wrt the node features of every row's
in-neighbourhood: two fills and one launch) against the other route to the same numbers: ``x.requires_grad_()``, the eval
``model(data)``, parameters frozen, one ``backward(retain_graph=True)`` per output.  ``synthetic.lightpath_batch`` chains at
C = 32, F = 5, O = 3 and B = 1, 8 and 512; ``jac_self`` / ``jac_edge`` are put together by the index-add identity and
compared with autograd's ``x.grad`` first; then both alternate in one process, each call between two
``torch.cuda.Event``s, median and interquartile range as above.

    python tools/bench_infer.py --kind lightpath --grad [--out profiles/bench_infer_lightpath_grad.jsonl]

``--what-if K [K ...]``: K edits of one network state scored in one launch (csrc/infer_whatif.hip) --
milliseconds per call of ``predict.what_if(data, ...)`` against (a) ``infer.materialise_what_if(...)`` followed by
``predict(batch)`` per call, what a caller without ``what_if`` does for every fresh set of candidates, and (b) ``predict``
alone on a batch materialised beforehand (the same arithmetic: a lower bound for (a), no candidate is ever fresh there).
One base graph at the reference shape and at the headline shape; each candidate is one lightpath: the two directed edges
between a seeded pair of nodes.  The edges and their features live on the device, ``add_ptr`` is a host tensor.  The rows of the three ways
are compared first (equal bits); then they alternate in one process, each call between two ``torch.cuda.Event``s, median
and interquartile range as above.

    python tools/bench_infer.py --what-if 1 64 1024 [--out profiles/bench_infer_whatif.jsonl]

``--kind lightpath --what-if K [K ...]``: K candidate lightpaths scored in one launch (csrc/infer_lightpath_whatif.hip,
DESIGN.md 4.19) -- milliseconds per call of ``predict.what_if(data, ...)`` against (a)
``infer.materialise_lightpath_what_if(...)`` followed by ``predict(batch)`` per call and (b) ``predict`` alone on a batch
materialised beforehand, as above.  One ``synthetic.lightpath_batch`` graph (a chain of 20 lightpaths, node 0 the LUT) at
C = 32, F = 5; every candidate is about the LUT node and has a fresh feature row, 2 removals (seeded positions of the
graph's 38 edges) and 2 additions (seeded sources).  The rows of the three ways are compared first (equal bits; the
graph has one LUT node, so the LUT rows of the materialised batch are the candidates in order and (a) and (b) pick
nothing); output and the interquartile rule as for the topological table.

    python tools/bench_infer.py --kind lightpath --what-if 1 8 64 1024 [--out profiles/bench_infer_lightpath_whatif.jsonl]

``--kind lightpath --from-status``: the LUT rows straight from network-status samples (csrc/infer_lightpath_status.hip,
DESIGN.md 4.20) -- milliseconds per call of ``predict.from_status(status)`` against
``predict.per_graph(to_graph.device_batch(status, "lightpath"))`` (two builder launches, one host read, the row kernel;
that path is what it was before ``from_status`` existed).  ``synthetic_network_status`` samples on the 60 x 72 grid (64
distinct ones, tiled) at S = 1, 8, 512, C = 32, F = 5, threshold 0.05.  The rows of the two ways are compared first (equal
bits); then they alternate in one process, each call between two ``torch.cuda.Event``s, median and interquartile range and
the "no difference" rule as above.

    python tools/bench_infer.py --kind lightpath --from-status [--out profiles/bench_infer_lightpath_status.jsonl]

``--kind topological --from-status``: the same for ``TopologicalPredictor`` (csrc/infer_topological_status.hip, DESIGN.md
4.21) -- ``predict.from_status(status)`` against ``predict(to_graph.device_batch(status, "topological"))``, at S = 1, 8, 512
and hidden widths 64 and 16 (V = 75, edge_dim 4, 3 outputs); same samples, same protocol.

    python tools/bench_infer.py --kind topological --from-status [--out profiles/bench_infer_topological_status.jsonl]

``--kind lightpath --place K [K ...]``: K candidate (route, slot) assignments of a new lightpath scored against one status
sample in one launch (csrc/infer_lightpath_place.hip) -- milliseconds per call of ``predict.place(status,
...)`` against (a) ``infer.materialise_placement(...)`` (K edited copies of the sample) followed by
``predict.from_status(edited)`` per call and (b) ``to_graph.device_batch(status)`` (two builder launches, one host read)
followed by ``predict.what_if`` per call, with each candidate's interferers worked out beforehand on the host
(``to_graph.placement_neighbourhood``) and its feature row scaled beforehand -- what a caller had to do before ``place``
existed.  One ``synthetic_network_status`` sample on the 60 x 72 grid without a lightpath under test of its own; every
candidate takes one free slot on 1 - 6 free links (seeded; ``--cells N``: on N links, ``--links L``: a grid of L links
instead of 60 -- the pair tells the cost of the sample scan, O(L Q), from that of the walk, O(cells Q)); C = 32, F = 5,
threshold 0.05.  For (b) the sample also
holds a placeholder lightpath under test on channel (0, 0), out of reach of every candidate, whose node the candidates
take over.  The rows of the three ways are compared first (equal bits); output and the interquartile rule as above.

    python tools/bench_infer.py --kind lightpath --place 1 8 64 1024 [--out profiles/bench_infer_lightpath_place.jsonl]

``--kind topological --place K [K ...]``: the same question for ``TopologicalPredictor`` (csrc/infer_topological_place.hip,
DESIGN.md 4.23) -- ``predict.place(status, ...)`` against ``infer.materialise_placement(...)`` followed by
``predict.from_status(edited)`` per call, at hidden widths 64 and 16 (V = 75, edge_dim 4, 3 outputs).  The same sample and
cells as above (``--links``, ``--cells`` as there); a third of the candidates join a random node pair, a third the pair of
a lightpath of the sample (in the reverse orientation) with a conn above every conn of the sample, a third such a pair
with a conn below.  Rows and link counts of the two ways are compared first (equal bits); two medians count as different
when they are further apart than the sum of their interquartile ranges.

    python tools/bench_infer.py --kind topological --place 1 8 64 1024 [--out profiles/bench_infer_topological_place.jsonl]

``--place K [K ...] --release R`` (either kind): a reroute -- every candidate releases R lightpaths of the sample in the same
launch (csrc/infer_*_place_release.hip).  ``predict.place(..., release=, release_ptr=)`` against (a)
``infer.materialise_placement(..., release, release_ptr)`` followed by ``predict.from_status(edited)`` -- the only way
before -- and (b) plain ``predict.place`` of the same candidates with nothing released: the cost of the edit itself, timed
in an alternation of its own (``release_pair_ms`` beside ``place_ms``), away from (a)'s K copies of the sample.  Each
candidate sits one slot beside a channel of a lightpath of the sample, on that link and on 0 - 5 more free links; that
lightpath is released (an interferer of the unreleased placement; in the topological model the winner of its node pair),
and R - 1 more; one channel of the last released lightpath is one of the candidate's cells -- in (b) a free cell of the
candidate's slot takes its place, so both walk as many cells.  ``--kind lightpath`` runs at threshold 0.12: at 0.05 the
neighbour slot, 0.05 away, does not interfere.  The rows of ``place(release=)`` and (a) are compared first (equal bits).

    python tools/bench_infer.py --kind lightpath --place 1 8 64 1024 --release 2 [--out profiles/bench_infer_lightpath_place_release.jsonl]
    python tools/bench_infer.py --kind topological --place 1 8 64 1024 --release 2 [--out profiles/bench_infer_topological_place_release.jsonl]

``--kind lightpath --place-impact K [K ...]``: the admission decision's second half -- ``predict.place_impact(status, ...)``
(csrc/infer_lightpath_place_impact.hip, DESIGN.md 4.25: the K candidates' rows and, in the same launch, the rows of the
established lightpaths each one disturbs, before and after) against (a) the only way before: two
``infer.materialise_retest`` calls (one sample per (candidate, interferer) pair, without and with the candidate), each
followed by ``to_graph.device_batch`` and ``predict`` -- with the pairs worked out on the host beforehand
(``to_graph.placement_neighbourhood``) and their arguments uploaded, which favours (a) -- and (b) plain ``predict.place`` of
the same candidates: what the retest costs beyond admission, timed in an alternation of its own.  One
``synthetic_network_status`` sample on the 60 x 72 grid without a lightpath under test of its own; every candidate takes one
slot on 1 - 4 links and has two interferers or more (asserted on the inputs); C = 32, F = 5, threshold 0.12,
``max_affected`` 8.  The rows of ``place_impact`` and (a), and of ``place_impact`` and (b), are compared first (equal bits);
two medians count as different when they are further apart than the sum of their interquartile ranges.

    python tools/bench_infer.py --kind lightpath --place-impact 1 8 64 1024 [--out profiles/bench_infer_lightpath_place_impact.jsonl]

``--kind lightpath --retest S [S ...]``: the standing question about a network state -- ``predict.retest(status)``
(csrc/infer_lightpath_retest.hip, DESIGN.md 4.26: every established lightpath of S status samples retested as the lightpath
under test, one launch) against (a) the only way before: ``infer.materialise_retest`` over all (sample, lightpath) pairs --
one edited copy of a sample per pair -- then ``to_graph.device_batch`` and ``predict``, with the pairs worked out on the
host beforehand and uploaded, which favours (a); and (b) ``predict.from_status`` of the same samples, one row per sample:
what a retested row costs beside it, timed in an alternation of its own.  S ``synthetic_network_status`` samples on the 60 x
72 grid, each with its own lightpath under test; C = 32, F = 5, threshold 0.12, ``max_lightpaths`` 256, ``chunk`` as
``infer.retest_chunk`` picks it (reported).  The rows of ``retest`` and (a) are compared first (equal bits); two medians
count as different when they are further apart than the sum of their interquartile ranges.

    python tools/bench_infer.py --kind lightpath --retest 1 8 64 512 [--out profiles/bench_infer_lightpath_retest.jsonl]

``--kind lightpath --reroute-impact K [K ...] [--release R]``: whom a reroute helps and whom it hurts --
``predict.reroute_impact(status, ..., release=, release_ptr=)`` (csrc/infer_lightpath_reroute_impact.hip)
against (a) the only way before: two ``infer.materialise_retest`` calls over the (candidate, affected lightpath) pairs, the
second with the candidate and ``release=``, each followed by ``to_graph.device_batch`` and ``predict`` -- the pairs worked
out on the host beforehand (``to_graph.reroute_impact``) and uploaded, which favours (a); (b) ``predict.place_impact`` of the
same candidates with nothing released; (c) ``predict.place(release=)``.  Each is timed in an alternation of its own with
``reroute_impact``.  ``--place-impact``'s sample and candidates; every candidate releases R lightpaths (default 2), the first
of them one that some survivor loses as a source (asserted on the inputs).  The rows of ``reroute_impact`` and (a), and its
``out`` / ``count`` and (c)'s, are compared first (equal bits).

    python tools/bench_infer.py --kind lightpath --reroute-impact 1 8 64 1024 --release 2 [--out profiles/bench_infer_lightpath_reroute_impact.jsonl]

``--kind lightpath --place-slots R [R ...] [--width W] [--chunk C]``: given a route, which slot? --
``predict.place_slots(status, ...)`` (csrc/infer_lightpath_place_slots.hip, DESIGN.md 4.28: R routes of 3 links, each swept
over all 72 start slots of one 60 x 72 ``synthetic_network_status`` sample, one launch, nothing read back) against (a) the
only way before: ``infer.materialise_slot_sweep`` -- the occupancy pass, the host read of the free slots, the building of
``place``'s lists -- followed by ``predict.place``; (b) ``predict.place`` on those lists built outside the timed region,
timed in an alternation of its own: what the shared scan is worth without the saved host work (``place`` spreads one
workgroup per free slot over the device, ``place_slots`` runs the rows of a chunk one after the other on one wave).  C =
32, F = 5, threshold 0.12, the chunk ``infer.place_slots_chunk`` picks unless ``--chunk`` names one (reported).  ``free`` and
the rows of the three ways are compared first (equal bits).

    python tools/bench_infer.py --kind lightpath --place-slots 1 8 64 [--width W] [--out profiles/bench_infer_lightpath_place_slots.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gnn_qot_estimation_amd as q  # noqa: E402
from gnn_qot_estimation_amd import synthetic as S  # noqa: E402

SHAPES = [
    dict(name="reference B=1", V=75, n=75, e=600, H=16, B=1),
    dict(name="reference B=8", V=75, n=75, e=600, H=16, B=8),
    dict(name="reference B=512", V=75, n=75, e=600, H=16, B=512),
    dict(name="headline B=1", V=100, n=100, e=400, H=64, B=1),
    dict(name="headline B=1024", V=100, n=100, e=400, H=64, B=1024),
]


def batch_for(shape, device):
    distinct = min(shape["B"], 64)                         # distinct graphs are generated once, then tiled
    base = S.topological_batch(2, distinct, n=shape["n"], e=shape["e"], edge_dim=4)
    return S.tile_batch(base, shape["B"] // distinct).to(device)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(shape, device, rounds, warmup):
    torch.manual_seed(0)
    model = q.TopologicalGNN(shape["V"], shape["H"], 3, 4, dropout_p=0.0).to(device).eval()
    data = batch_for(shape, device)
    predictor = q.TopologicalPredictor(model)

    def eager():
        with torch.no_grad():
            return model(data)

    for _ in range(3):
        want = eager()
    got = predictor(data)
    torch.cuda.synchronize()
    err = float((got.double() - want.double()).abs().max() / want.double().abs().max())
    assert err <= 1e-4, (shape["name"], err)

    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        replay_out = eager()
    graph.replay()
    torch.cuda.synchronize()
    err_replay = float((replay_out.double() - want.double()).abs().max() / want.double().abs().max())
    assert err_replay <= 1e-6, (shape["name"], err_replay)

    ways = {"fused": lambda: predictor(data), "eager": eager, "replay": graph.replay}
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed(fn))
    res = dict(shape=shape["name"], **{k: shape[k] for k in ("V", "n", "e", "H", "B")}, rounds=rounds, rel_err=err)
    for k, ts in times.items():
        res[f"{k}_ms"] = statistics.median(ts)
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


MC_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[3]]


def measure_mc(shape, T, device, rounds, warmup):
    torch.manual_seed(0)
    model = q.TopologicalGNN(shape["V"], shape["H"], 3, 4, dropout_p=0.5).to(device).train()
    data = batch_for(shape, device)
    predict = q.TopologicalPredictor(model)

    def eager():
        with torch.no_grad():
            return [model(data) for _ in range(T)]

    eager()
    model._qot_step.zero_()
    want = torch.stack(eager())                            # dropout steps 1 ... T
    got = predict.sample(data, T, first_step=1, return_samples=True)[2]
    torch.cuda.synchronize()
    predict.check_status()
    err = float((got.double() - want.double()).abs().max() / want.double().abs().max())
    assert err <= 1e-4, (shape["name"], err)
    assert not torch.equal(got[0], got[1])

    ways = {"sample": lambda: predict.sample(data, T), "eager": eager}
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed(fn))
    from gnn_qot_estimation_amd import infer
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    res = dict(shape=shape["name"], kind="mc", T=T, p=0.5, chunk=infer.mc_chunk(shape["B"], T, cus), compute_units=cus,
               **{k: shape[k] for k in ("V", "n", "e", "H", "B")}, rounds=rounds, rel_err=err)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_mc(args, device, commit):
    rows = []
    for shape in MC_SHAPES:
        res = measure_mc(shape, args.mc, device, args.rounds, args.warmup)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(f"\n| shape | chunk | sample(T={args.mc}) ms (IQR) | {args.mc} train-mode forwards ms (IQR) | eager / sample |")
    print("|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['shape']} (n={r['n']}, e={r['e']}, H={r['H']}) | {r['chunk']} | {cell('sample')} | {cell('eager')} | "
              f"{verdict(r, 'sample')} |")


GRAD_SHAPES = [SHAPES[0], SHAPES[2], SHAPES[3]]


def timed_event(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def measure_grad(shape, device, rounds, warmup):
    torch.manual_seed(0)
    model = q.TopologicalGNN(shape["V"], shape["H"], 3, 4, dropout_p=0.0).to(device).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    data = batch_for(shape, device)
    predict = q.TopologicalPredictor(model)
    leaf = batch_for(shape, device)
    leaf.edge_attr = leaf.edge_attr.detach().clone().requires_grad_()

    def autograd():
        out = model(leaf)
        jac = []
        for o in range(out.shape[1]):
            leaf.edge_attr.grad = None
            out[:, o].sum().backward(retain_graph=True)
            jac.append(leaf.edge_attr.grad)
        return out, jac

    for _ in range(3):
        want_out, want = autograd()
    want = torch.stack(want)
    out, got = predict.sensitivity(data)
    torch.cuda.synchronize()
    predict.check_status()
    err = float((got.double() - want.double()).abs().max() / want.double().abs().max())
    err_out = float((out.double() - want_out.double()).abs().max() / want_out.double().abs().max())
    assert err <= 1e-4 and err_out <= 1e-4, (shape["name"], err, err_out)

    ways = {"sensitivity": lambda: predict.sensitivity(data), "eager": autograd}
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed_event(fn))
    res = dict(shape=shape["name"], kind="grad", outputs=3, **{k: shape[k] for k in ("V", "n", "e", "H", "B")}, rounds=rounds,
               rel_err=err)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_grad(args, device, commit):
    rows = []
    for shape in GRAD_SHAPES:
        res = measure_grad(shape, device, args.rounds, args.warmup)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| shape | sensitivity ms (IQR) | forward + 3 backward ms (IQR) | autograd / sensitivity |")
    print("|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['shape']} (n={r['n']}, e={r['e']}, H={r['H']}) | {cell('sensitivity')} | {cell('eager')} | "
              f"{verdict(r, 'sensitivity')} |")


WHAT_IF_SHAPES = [SHAPES[0], SHAPES[3]]


def measure_what_if(shape, K, device, rounds, warmup):
    from gnn_qot_estimation_amd import infer
    torch.manual_seed(0)
    model = q.TopologicalGNN(shape["V"], shape["H"], 3, 4, dropout_p=0.0).to(device).eval()
    data = batch_for(shape, device)                        # B = 1: the network state
    predict = q.TopologicalPredictor(model)
    gen = torch.Generator().manual_seed(K)
    u = torch.randint(0, shape["n"], (K,), generator=gen)
    v = (u + 1 + torch.randint(0, shape["n"] - 1, (K,), generator=gen)) % shape["n"]        # v != u
    add = torch.stack([torch.stack([u, v], 1).reshape(-1), torch.stack([v, u], 1).reshape(-1)]).to(device)   # u->v, v->u
    attr = torch.rand(2 * K, 4, generator=gen).to(device)
    add_ptr = torch.arange(0, 2 * K + 1, 2)                # a host tensor: checked on the host, uploaded per call
    mat = infer.materialise_what_if(data, add, attr, add_ptr)

    ways = {"what_if": lambda: predict.what_if(data, add, attr, add_ptr),
            "materialise": lambda: predict(infer.materialise_what_if(data, add, attr, add_ptr)),
            "prebuilt": lambda: predict(mat)}
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    assert torch.equal(got["what_if"], got["prebuilt"]) and torch.equal(got["materialise"], got["prebuilt"]), shape["name"]
    assert tuple(got["what_if"].shape) == (K, 3) and bool(torch.isfinite(got["what_if"]).all())
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed_event(fn))
    res = dict(shape=shape["name"], kind="what_if", K=K, added_per_candidate=2,
               **{k: shape[k] for k in ("V", "n", "e", "H", "B")}, rounds=rounds, equal_bits=True)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def versus(r, other):
    """``other`` against ``what_if``: the ratio of the medians, or "no difference" (module docstring)."""
    a, b = r["what_if_ms"], r[f"{other}_ms"]
    if abs(a - b) <= max(r["what_if_iqr_ms"], r[f"{other}_iqr_ms"]):
        return "no difference"
    return f"{b / a:.2f}x"


def main_what_if(args, device, commit):
    rows = []
    for shape in WHAT_IF_SHAPES:
        for K in args.what_if:
            res = measure_what_if(shape, K, device, args.rounds, args.warmup)
            res["commit"] = commit or None
            res["device"] = torch.cuda.get_device_name(0)
            rows.append(res)
            print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| shape | K | what_if ms (IQR) | (a) materialise + predict ms (IQR) | (b) predict, prebuilt ms (IQR) | (a) / what_if "
          "| (b) / what_if |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['shape']} (n={r['n']}, e={r['e']}, H={r['H']}) | {r['K']} | {cell('what_if')} | {cell('materialise')} | "
              f"{cell('prebuilt')} | {versus(r, 'materialise')} | {versus(r, 'prebuilt')} |")


def measure_lightpath_what_if(K, device, rounds, warmup):
    from gnn_qot_estimation_amd import infer
    torch.manual_seed(0)
    model = q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval()
    data = S.lightpath_batch(1, min_nodes=20, max_nodes=20).to(device)     # one graph: the lightpath under test and 19 others
    n, e = int(data.x.shape[0]), int(data.edge_index.shape[1])
    predict = q.LightpathPredictor(model)
    gen = torch.Generator().manual_seed(K)
    x_lut = torch.rand(K, 5, generator=gen)
    x_lut[:, 1] = 1.0
    x_lut = x_lut.to(device)
    node = torch.zeros(K, dtype=torch.long, device=device)                  # every candidate is about the LUT node
    add = (1 + torch.randint(0, n - 1, (2 * K,), generator=gen)).to(device)
    first = torch.randint(0, e, (K,), generator=gen)
    drop = torch.stack([first, (first + 1 + torch.randint(0, e - 1, (K,), generator=gen)) % e], 1).reshape(-1).to(device)
    ptr = torch.arange(0, 2 * K + 1, 2)                    # a host tensor: checked on the host, uploaded per call
    kw = dict(x_lut=x_lut, add_src=add, add_ptr=ptr, drop=drop, drop_ptr=ptr, node=node)
    mat, node_new = infer.materialise_lightpath_what_if(data, 1, **kw)
    # the graph has one LUT node, so the LUT rows of the materialised batch are the candidates, in order: nothing to pick
    assert torch.equal(model._lut_rows(mat), node_new)

    ways = {"what_if": lambda: predict.what_if(data, **kw)[0],
            "materialise": lambda: predict(infer.materialise_lightpath_what_if(data, 1, **kw)[0])[0],
            "prebuilt": lambda: predict(mat)[0]}
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    assert torch.equal(got["what_if"], got["prebuilt"]) and torch.equal(got["materialise"], got["prebuilt"]), K
    assert tuple(got["what_if"].shape) == (K, 3) and bool(torch.isfinite(got["what_if"]).all())
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed_event(fn))
    res = dict(shape="lightpath B=1", kind="lightpath_what_if", K=K, added_per_candidate=2, dropped_per_candidate=2, B=1,
               C=32, F=5, N=n, E=e, rounds=rounds, equal_bits=True)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_lightpath_what_if(args, device, commit):
    rows = []
    for K in args.what_if:
        res = measure_lightpath_what_if(K, device, args.rounds, args.warmup)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| shape | K | what_if ms (IQR) | (a) materialise + predict ms (IQR) | (b) predict, prebuilt ms (IQR) | (a) / what_if "
          "| (b) / what_if |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['shape']} (N={r['N']}, E={r['E']}, C={r['C']}, F={r['F']}) | {r['K']} | {cell('what_if')} | "
              f"{cell('materialise')} | {cell('prebuilt')} | {versus(r, 'materialise')} | {versus(r, 'prebuilt')} |")


STATUS_SIZES = (1, 8, 512)


STATUS_WIDTHS = (64, 16)                                    # --kind topological: the headline's width, the reference's


def measure_from_status(Sn, device, rounds, warmup, H=None):
    """``H``: ``None`` measures ``LightpathPredictor``, a hidden width ``TopologicalPredictor`` at that width."""
    from gnn_qot_estimation_amd import to_graph as TG
    torch.manual_seed(0)
    distinct = min(Sn, 64)                                  # distinct samples are generated once, then tiled
    ns = TG.synthetic_network_status(distinct, seed=0)      # the 60 x 72 grid
    st = ns.to_device(device, [g % distinct for g in range(Sn)])
    if H is None:
        model = q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval()
        predict = q.LightpathPredictor(model)
        ways = {"from_status": lambda: predict.from_status(st)[0],
                "graphs": lambda: predict.per_graph(TG.device_batch(st, "lightpath"))[0]}
        what = dict(kind="lightpath_from_status", C=32, F=5)
    else:
        model = q.TopologicalGNN(75, H, 3, 4, dropout_p=0.0).to(device).eval()
        predict = q.TopologicalPredictor(model)
        ways = {"from_status": lambda: predict.from_status(st)[0],
                "graphs": lambda: predict(TG.device_batch(st, "topological"))}
        what = dict(kind="topological_from_status", H=H, D=4, V=75)
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    assert torch.equal(got["from_status"], got["graphs"]) and bool(torch.isfinite(got["graphs"]).all()), Sn
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed_event(fn))
    res = dict(shape="status 60 x 72", S=Sn, P=int(st.data.shape[1]), L=60, Q=72, rounds=rounds, equal_bits=True, **what)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_from_status(args, device, commit):
    rows = []
    topological = args.kind == "topological"
    for H in (STATUS_WIDTHS if topological else (None,)):
        for Sn in STATUS_SIZES:
            res = measure_from_status(Sn, device, args.rounds, args.warmup, H)
            res["commit"] = commit or None
            res["device"] = torch.cuda.get_device_name(0)
            rows.append(res)
            print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    other = "device_batch + predict" if topological else "device_batch + per_graph"
    print(f"\n| {'H | ' if topological else ''}S | from_status ms (IQR) | {other} ms (IQR) | graphs / from_status |")
    print("|---|---|---|---|" + ("---|" if topological else ""))
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        a, b = r["from_status_ms"], r["graphs_ms"]
        same = abs(a - b) <= max(r["from_status_iqr_ms"], r["graphs_iqr_ms"])
        head = f"| {r['H']} " if topological else ""
        print(f"{head}| {r['S']} | {cell('from_status')} | {cell('graphs')} | {'no difference' if same else f'{b / a:.2f}x'} |")


def measure_place(K, device, rounds, warmup, thr=0.05, num_links=60, per_candidate=None):
    import numpy as np
    from gnn_qot_estimation_amd import infer, to_graph as TG
    torch.manual_seed(0)
    model = q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval()
    predict = q.LightpathPredictor(model)
    ns = TG.synthetic_network_status(1, num_links=num_links, seed=0)      # the 60 x 72 grid by default
    fi, feats = ns.feature_indexes, list(TG.DEFAULT_FEATURES)
    data = ns.data.copy()
    under_test = (data[0, fi["osnr"]] == -1) & (data[0, fi["snr"]] == -1) & (data[0, fi["ber"]] == -1)
    data[0][:, under_test] = 0.0                            # the sample's own lightpath under test goes
    data[0, :, 0, :4] = 0.0                                 # room for (b)'s placeholder: nobody within 3 slots of (0, 0)
    L, Q = data.shape[2], data.shape[3]
    free = ~np.any(data[0] != 0, axis=0)
    rng = np.random.default_rng(K)
    values, cells, ptr = np.zeros((K, len(ns.lp_feat))), [], [0]
    for k in range(K):
        want = per_candidate or int(rng.integers(1, 7))
        while True:                                         # one slot (>= 4: clear of the placeholder) on 1 - 6 free links
            slot = int(rng.integers(4, Q))
            open_links = np.flatnonzero(free[:, slot])
            if len(open_links) >= want:
                links = rng.choice(open_links, size=want, replace=False)
                break
        cells.append(np.stack([links, np.full_like(links, slot)]))
        ptr.append(ptr[-1] + len(links))
        v = values[k]
        v[fi["conn_id"]], v[fi["src_id"]], v[fi["dst_id"]] = 10000 + k, 1, 2
        v[fi["mod_order"]], v[fi["path_len"]] = float(rng.choice([4, 8, 16, 32, 64])), float(rng.integers(24214, 7834746))
        v[fi["num_spans"]], v[fi["freq"]] = float(rng.integers(1, 107)), ns.freq[slot]
        v[fi["osnr"]] = v[fi["snr"]] = v[fi["ber"]] = -1.0
    cells = np.concatenate(cells, axis=1).astype(np.int64)
    status_of = lambda d: TG.NetworkStatus(d, ns.target, ns.lp_feat, ns.metric, ns.link, ns.freq).to_device(device)  # noqa: E731
    st = status_of(data)
    samples = torch.zeros(K, dtype=torch.int64, device=device)
    values_d, cells_d = torch.from_numpy(values).to(device), torch.from_numpy(cells).to(device)
    ptr_d = torch.tensor(ptr, dtype=torch.int64, device=device)
    # (b): the placeholder under test on (0, 0) is the first lightpath seen, node 0; the candidates take its node over
    held = data.copy()
    held[0, :, 0, 0] = values[0]
    held[0, fi["conn_id"], 0, 0] = 9999.0
    st_b = status_of(held)
    _, _, vec = TG._occupied(held[0])
    seen = vec[fi["conn_id"]].astype(np.int64)
    node_of = {int(seen[i]): n for n, i in enumerate(np.sort(np.unique(seen, return_index=True)[1]))}
    assert node_of[9999] == 0
    add, add_ptr = [], [0]
    for k in range(K):
        near = TG.placement_neighbourhood(data[0], ns.freq, fi, cells[:, ptr[k]:ptr[k + 1]], thr)
        add += [node_of[c] for c in near]
        add_ptr.append(len(add))
    cols = TG._column_tables(st, "lightpath", feats)[0]    # (lp_feat row, min, max - min, has_range) per sorted column
    row = cols[:, 0].long()
    raw = values_d[:, row.clamp(min=0)]
    x_lut = torch.where(cols[:, 3] != 0, (raw - cols[:, 1]) / cols[:, 2], raw)
    x_lut = torch.where(row < 0, torch.ones_like(x_lut), x_lut).float()      # the is_lut column
    what_if = dict(x_lut=x_lut, add_src=torch.tensor(add, dtype=torch.int64, device=device),
                   add_ptr=torch.tensor(add_ptr, dtype=torch.int64), node=torch.zeros(K, dtype=torch.int64, device=device))

    ways = {"place": lambda: predict.place(st, samples, values_d, cells_d, ptr_d, feats, thr)[0],
            "materialise": lambda: predict.from_status(infer.materialise_placement(st, samples, values_d, cells_d, ptr_d),
                                                       None, feats, thr)[0],
            "what_if": lambda: predict.what_if(TG.device_batch(st_b, "lightpath", feats, None, thr), **what_if)[0]}
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    assert torch.equal(got["place"], got["materialise"]) and torch.equal(got["place"], got["what_if"]), K
    assert tuple(got["place"].shape) == (K, 3) and bool(torch.isfinite(got["place"]).all())
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed_event(fn))
    res = dict(shape=f"status {L} x {Q}", kind="lightpath_place", K=K, cells=int(cells.shape[1]), interferers=len(add),
               lightpaths=len(node_of) - 1, S=1, P=int(st.data.shape[1]), L=L, Q=Q, C=32, F=5, freq_threshold=thr, rounds=rounds,
               equal_bits=True)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_place(args, device, commit):
    rows = []
    for K in args.place:
        res = measure_place(K, device, args.rounds, args.warmup, num_links=args.links, per_candidate=args.cells)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| grid | K | cells | interferers | place ms (IQR) | (a) materialise_placement + from_status ms (IQR) | (b) device_batch + "
          "what_if ms (IQR) | (a) / place | (b) / place |")
    print("|---|---|---|---|---|---|---|---|---|")

    def against(r, other):
        a, b = r["place_ms"], r[other + "_ms"]
        same = abs(a - b) <= max(r["place_iqr_ms"], r[other + "_iqr_ms"])
        return "no difference" if same else f"{b / a:.2f}x"
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['L']} x {r['Q']} | {r['K']} | {r['cells']} | {r['interferers']} | {cell('place')} | {cell('materialise')} | {cell('what_if')} | "
              f"{against(r, 'materialise')} | {against(r, 'what_if')} |")


def measure_topological_place(K, H, device, rounds, warmup, num_links=60, per_candidate=None):
    import numpy as np
    from gnn_qot_estimation_amd import infer, to_graph as TG
    torch.manual_seed(0)
    model = q.TopologicalGNN(75, H, 3, 4, dropout_p=0.0).to(device).eval()
    predict = q.TopologicalPredictor(model)
    ns = TG.synthetic_network_status(1, num_links=num_links, seed=0)      # the 60 x 72 grid by default
    fi, feats = ns.feature_indexes, list(TG.DEFAULT_FEATURES)
    data = ns.data
    L, Q = data.shape[2], data.shape[3]
    free = ~np.any(data[0] != 0, axis=0)
    held = data[0][:, ~free]                                # the sample's lightpaths, a column per occupied channel
    rng = np.random.default_rng(K)
    values, cells, ptr = np.zeros((K, len(ns.lp_feat))), [], [0]
    outcomes = {"new or random pair": 0, "takes the pair": 0, "loses the pair": 0}
    for k in range(K):
        want = per_candidate or int(rng.integers(1, 7))
        while True:                                         # one slot on 1 - 6 free links
            slot = int(rng.integers(0, Q))
            open_links = np.flatnonzero(free[:, slot])
            if len(open_links) >= want:
                links = rng.choice(open_links, size=want, replace=False)
                break
        cells.append(np.stack([links, np.full_like(links, slot)]))
        ptr.append(ptr[-1] + len(links))
        v = values[k]
        # a third each: a random node pair; the pair of a lightpath of the sample with a conn above all; with one below all
        if k % 3 == 0:
            v[fi["conn_id"]], (v[fi["src_id"]], v[fi["dst_id"]]) = 10000 + k, rng.integers(1, 76, size=2)
            outcomes["new or random pair"] += 1
        else:
            other = held[:, int(rng.integers(0, held.shape[1]))]
            v[fi["src_id"]], v[fi["dst_id"]] = other[fi["dst_id"]], other[fi["src_id"]]
            v[fi["conn_id"]] = 10000 + k if k % 3 == 1 else -1 - k
            outcomes["takes the pair" if k % 3 == 1 else "loses the pair"] += 1
        v[fi["mod_order"]], v[fi["path_len"]] = float(rng.choice([4, 8, 16, 32, 64])), float(rng.integers(24214, 7834746))
        v[fi["num_spans"]], v[fi["freq"]] = float(rng.integers(1, 107)), ns.freq[slot]
        v[fi["osnr"]] = v[fi["snr"]] = v[fi["ber"]] = -1.0
    cells = np.concatenate(cells, axis=1).astype(np.int64)
    st = ns.to_device(device)
    samples = torch.zeros(K, dtype=torch.int64, device=device)
    values_d, cells_d = torch.from_numpy(values).to(device), torch.from_numpy(cells).to(device)
    ptr_d = torch.tensor(ptr, dtype=torch.int64, device=device)

    ways = {"place": lambda: predict.place(st, samples, values_d, cells_d, ptr_d, feats),
            "materialise": lambda: predict.from_status(infer.materialise_placement(st, samples, values_d, cells_d, ptr_d),
                                                       None, feats)}
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    assert torch.equal(got["place"][0], got["materialise"][0]) and torch.equal(got["place"][1], got["materialise"][1]), K
    assert tuple(got["place"][0].shape) == (K, 3) and bool(torch.isfinite(got["place"][0]).all())
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed_event(fn))
    res = dict(shape=f"status {L} x {Q}", kind="topological_place", K=K, H=H, D=4, V=75, cells=int(cells.shape[1]),
               candidates=outcomes, S=1, P=int(st.data.shape[1]), L=L, Q=Q, rounds=rounds, equal_bits=True)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_topological_place(args, device, commit):
    rows = []
    for H in STATUS_WIDTHS:
        for K in args.place:
            res = measure_topological_place(K, H, device, args.rounds, args.warmup, num_links=args.links, per_candidate=args.cells)
            res["commit"] = commit or None
            res["device"] = torch.cuda.get_device_name(0)
            rows.append(res)
            print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| H | grid | K | cells | place ms (IQR) | materialise_placement + from_status ms (IQR) | materialise / place |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        a, b = r["place_ms"], r["materialise_ms"]
        same = abs(a - b) <= r["place_iqr_ms"] + r["materialise_iqr_ms"]    # differ: by more than the sum of the IQRs
        print(f"| {r['H']} | {r['L']} x {r['Q']} | {r['K']} | {r['cells']} | {cell('place')} | {cell('materialise')} | "
              f"{'no difference' if same else f'{b / a:.2f}x'} |")


def measure_place_release(kind, K, R, H, device, rounds, warmup, thr=0.12, num_links=60, per_candidate=None):
    """``place(..., release=)`` of K candidates, R released lightpaths each, against (a) ``materialise_placement(release=)`` +
    ``from_status`` and (b) plain ``place`` of the same candidates with nothing released (the reused cell swapped for a free
    one on the same slot, so that both walk as many cells)."""
    import numpy as np
    from gnn_qot_estimation_amd import infer, to_graph as TG
    torch.manual_seed(0)
    if kind == "lightpath":
        predict = q.LightpathPredictor(q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval())
    else:
        predict = q.TopologicalPredictor(q.TopologicalGNN(75, H, 3, 4, dropout_p=0.0).to(device).eval())
    ns = TG.synthetic_network_status(1, num_links=num_links, seed=0)      # the 60 x 72 grid by default
    fi, feats = ns.feature_indexes, list(TG.DEFAULT_FEATURES)
    data = ns.data.copy()
    if kind == "lightpath":                                 # the sample's own lightpath under test goes, as in --place
        under_test = (data[0, fi["osnr"]] == -1) & (data[0, fi["snr"]] == -1) & (data[0, fi["ber"]] == -1)
        data[0][:, under_test] = 0.0
    L, Q = data.shape[2], data.shape[3]
    free = ~np.any(data[0] != 0, axis=0)
    occ = np.argwhere(~free)
    conn_of = data[0, fi["conn_id"]].astype(np.int64)
    conns = sorted({int(conn_of[l, f]) for l, f in occ})
    if R > min(len(conns), infer.PLACE_MAX_RELEASE):
        raise SystemExit(f"--release {R}: the sample holds {len(conns)} lightpaths, the cap is {infer.PLACE_MAX_RELEASE}")
    # channels with a free neighbour slot on their link: where a candidate meets an interferer at 0.05 < thr
    beside = [(int(l), int(f), int(g)) for l, f in occ for g in (f - 1, f + 1) if 0 <= g < Q and free[l, g]]
    rng = np.random.default_rng(K)
    values, cells, plain_cells, ptr, release = np.zeros((K, len(ns.lp_feat))), [], [], [0], []
    met, winners = 0, 0
    for k in range(K):
        want = per_candidate or int(rng.integers(1, 7))
        while True:                                         # next to a lightpath's channel, on 1 - 6 free links of that slot
            l0, f0, slot = beside[int(rng.integers(len(beside)))]
            open_links = np.setdiff1d(np.flatnonzero(free[:, slot]), [l0])
            if len(open_links) >= want:                     # (want - 1 more for the candidate, one for plain place's swap)
                links = np.concatenate([[l0], rng.choice(open_links, size=want, replace=False)])
                break
        first = int(conn_of[l0, f0])                        # released: an interferer of the unreleased placement
        others = [c for c in conns if c != first]
        rel = [first] + [int(c) for c in rng.choice(others, size=R - 1, replace=False)]
        reuse = occ[[int(conn_of[l, f]) == rel[-1] for l, f in occ]][0]         # a channel of a released lightpath
        mine = np.stack([links[:want], np.full(want, slot)])
        cells.append(np.concatenate([mine, reuse.reshape(2, 1)], axis=1))
        plain_cells.append(np.concatenate([mine, np.array([[links[want]], [slot]])], axis=1))
        ptr.append(ptr[-1] + want + 1)
        release += rel
        met += first in TG.placement_neighbourhood(data[0], ns.freq, fi, mine, thr)
        v = values[k]
        if kind == "lightpath" or k % 3 == 0:
            v[fi["conn_id"]], (v[fi["src_id"]], v[fi["dst_id"]]) = 10000 + k, rng.integers(1, 76, size=2)
        else:                                               # the pair of the released neighbour, above or below every conn
            v[fi["src_id"]], v[fi["dst_id"]] = data[0, fi["dst_id"], l0, f0], data[0, fi["src_id"], l0, f0]
            v[fi["conn_id"]] = 10000 + k if k % 3 == 1 else -1 - k
        v[fi["mod_order"]], v[fi["path_len"]] = float(rng.choice([4, 8, 16, 32, 64])), float(rng.integers(24214, 7834746))
        v[fi["num_spans"]], v[fi["freq"]] = float(rng.integers(1, 107)), ns.freq[slot]
        v[fi["osnr"]] = v[fi["snr"]] = v[fi["ber"]] = -1.0
    if kind == "topological":                               # how many candidates release the winner of some node pair
        won = set(TG.topological_links(data[0], fi)[1].tolist())
        winners = sum(bool(won & set(release[k * R:(k + 1) * R])) for k in range(K))
        assert winners == K
    else:
        assert met == K
    st = TG.NetworkStatus(data, ns.target, ns.lp_feat, ns.metric, ns.link, ns.freq).to_device(device)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)       # noqa: E731
    samples, values_d = torch.zeros(K, dtype=torch.int64, device=device), torch.from_numpy(values).to(device)
    cells_d, plain_d, ptr_d = dev(np.concatenate(cells, axis=1)), dev(np.concatenate(plain_cells, axis=1)), dev(ptr)
    rel_d, rptr_d = dev(release), dev(np.arange(K + 1) * R)
    tail = (feats, thr) if kind == "lightpath" else (feats,)
    ways = {"release": lambda: predict.place(st, samples, values_d, cells_d, ptr_d, *tail, release=rel_d, release_ptr=rptr_d),
            "materialise": lambda: predict.from_status(infer.materialise_placement(st, samples, values_d, cells_d, ptr_d,
                                                                                   rel_d, rptr_d), None, *tail),
            "place": lambda: predict.place(st, samples, values_d, plain_d, ptr_d, *tail)}
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    assert torch.equal(got["release"][0], got["materialise"][0]) and torch.equal(got["release"][1], got["materialise"][1]), K
    assert tuple(got["release"][0].shape) == (K, 3) and all(bool(torch.isfinite(g[0]).all()) for g in got.values())
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    # two alternations, so that plain place is not timed right behind materialise_placement's K copies of the sample: the
    # call that follows them is up to a third slower at K >= 64 (measured: DESIGN.md 4.24), whichever of the two it is
    times = {k: [] for k in ("release", "materialise", "release_pair", "place")}
    for _ in range(rounds):
        times["release"].append(timed_event(ways["release"]))
        times["materialise"].append(timed_event(ways["materialise"]))
    for _ in range(warmup):
        ways["release"](), ways["place"]()
    for _ in range(rounds):
        times["release_pair"].append(timed_event(ways["release"]))
        times["place"].append(timed_event(ways["place"]))
    res = dict(shape=f"status {L} x {Q}", kind=f"{kind}_place_release", K=K, R=R, cells=int(ptr[-1]), lightpaths=len(conns), S=1,
               P=int(st.data.shape[1]), L=L, Q=Q, rounds=rounds, equal_bits=True, released_interferers=met,
               released_winners=winners)
    res.update(dict(C=32, F=5, freq_threshold=thr) if kind == "lightpath" else dict(H=H, D=4, V=75))
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_place_release(args, device, commit):
    rows = []
    for H in ((None,) if args.kind == "lightpath" else STATUS_WIDTHS):
        for K in args.place:
            res = measure_place_release(args.kind, K, args.release, H, device, args.rounds, args.warmup, num_links=args.links,
                                        per_candidate=args.cells)
            res["commit"] = commit or None
            res["device"] = torch.cuda.get_device_name(0)
            rows.append(res)
            print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| H | grid | K | R | cells | place(release=) ms (IQR) | (a) materialise_placement(release=) + from_status ms (IQR) | "
          "(a) / release | place(release=) beside (b) ms (IQR) | (b) plain place ms (IQR) | release / (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")

    def ratio(r, num, den):                                 # differ: by more than the sum of the IQRs
        same = abs(r[num + "_ms"] - r[den + "_ms"]) <= r[num + "_iqr_ms"] + r[den + "_iqr_ms"]
        return "no difference" if same else f"{r[num + '_ms'] / r[den + '_ms']:.2f}x"
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r.get('H', '-')} | {r['L']} x {r['Q']} | {r['K']} | {r['R']} | {r['cells']} | {cell('release')} | "
              f"{cell('materialise')} | {ratio(r, 'materialise', 'release')} | {cell('release_pair')} | {cell('place')} | "
              f"{ratio(r, 'release_pair', 'place')} |")


def measure_place_impact(K, device, rounds, warmup, thr=0.12, max_affected=8):
    """``place_impact`` of K candidates against (a) two ``materialise_retest`` calls + ``device_batch`` + ``predict`` over
    the (candidate, interferer) pairs, worked out on the host beforehand, and (b) plain ``place`` of the same candidates."""
    import numpy as np
    from gnn_qot_estimation_amd import infer, to_graph as TG
    torch.manual_seed(0)
    predict = q.LightpathPredictor(q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval())
    ns = TG.synthetic_network_status(1, seed=0)             # the 60 x 72 grid
    fi, feats = ns.feature_indexes, list(TG.DEFAULT_FEATURES)
    data = ns.data.copy()
    under_test = (data[0, fi["osnr"]] == -1) & (data[0, fi["snr"]] == -1) & (data[0, fi["ber"]] == -1)
    data[0][:, under_test] = 0.0                            # the sample's own lightpath under test goes, as in --place:
    L, Q = data.shape[2], data.shape[3]                     # every retest sample of (a) then holds one LUT node, its pair's
    free = ~np.any(data[0] != 0, axis=0)
    conn_of = data[0, fi["conn_id"]].astype(np.int64)
    # per free cell, the lightpaths within two slots on its link (0.10 < thr); a candidate takes one slot on the links where
    # that set is not empty, as many of them as it needs to meet two lightpaths or more
    near = {(l, g): {int(conn_of[l, f]) for f in range(max(0, g - 2), min(Q, g + 3)) if not free[l, f]}
            for l in range(L) for g in range(Q) if free[l, g]}
    by_slot = {}
    for (l, g), who in near.items():
        if who:
            by_slot.setdefault(g, []).append(l)
    slots = sorted(g for g, ls in by_slot.items() if len(set().union(*(near[l, g] for l in ls))) >= 2)
    assert slots, "no slot of the sample lets a candidate meet two lightpaths"
    rng = np.random.default_rng(K)
    values, cells, ptr, pairs = np.zeros((K, len(ns.lp_feat))), [], [0], []
    for k in range(K):
        slot = slots[int(rng.integers(len(slots)))]
        links, met = [], set()
        for l in rng.permutation(by_slot[slot]):
            links.append(int(l))
            met |= near[int(l), slot]
            if len(met) >= 2 and len(links) >= int(rng.integers(1, 5)):
                break
        mine = np.stack([np.asarray(links), np.full(len(links), slot)])
        cells.append(mine)
        ptr.append(ptr[-1] + len(links))
        v = values[k]
        v[fi["conn_id"]], v[fi["src_id"]], v[fi["dst_id"]] = 10000 + k, 1, 2
        v[fi["mod_order"]], v[fi["path_len"]] = float(rng.choice([4, 8, 16, 32, 64])), float(rng.integers(24214, 7834746))
        v[fi["num_spans"]], v[fi["freq"]] = float(rng.integers(1, 107)), ns.freq[slot]
        v[fi["osnr"]] = v[fi["snr"]] = v[fi["ber"]] = -1.0
        affected = TG.placement_neighbourhood(data[0], ns.freq, fi, mine, thr)
        assert len(affected) >= 2, (k, affected)            # a condition on the inputs: two interferers or more each
        pairs += [(k, i, c) for i, c in enumerate(affected[:max_affected])]
    st = TG.NetworkStatus(data, ns.target, ns.lp_feat, ns.metric, ns.link, ns.freq).to_device(device)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)       # noqa: E731
    samples, values_d = torch.zeros(K, dtype=torch.int64, device=device), torch.from_numpy(values).to(device)
    cells_d, ptr_d = dev(np.concatenate(cells, axis=1)), dev(ptr)
    # (a)'s arguments, one row per pair, prepared beforehand: which favours (a)
    T = len(pairs)
    pk, pi = dev([k for k, _, _ in pairs]), dev([i for _, i, _ in pairs])
    psamples, pconns, pvalues = torch.zeros(T, dtype=torch.int64, device=device), dev([c for _, _, c in pairs]), values_d[pk]
    pcells = dev(np.concatenate([cells[k] for k, _, _ in pairs], axis=1))
    pptr = dev(np.cumsum([0] + [cells[k].shape[1] for k, _, _ in pairs]))

    def retest():
        before = predict(TG.device_batch(infer.materialise_retest(st, psamples, pconns), "lightpath", feats, None, thr))[0]
        after = predict(TG.device_batch(infer.materialise_retest(st, psamples, pconns, pvalues, pcells, pptr), "lightpath",
                                        feats, None, thr))[0]
        return before, after
    ways = {"impact": lambda: predict.place_impact(st, samples, values_d, cells_d, ptr_d, feats, thr, max_affected),
            "retest": retest,
            "place": lambda: predict.place(st, samples, values_d, cells_d, ptr_d, feats, thr)}
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    r = got["impact"]
    assert torch.equal(r.before[pk, pi], got["retest"][0]) and torch.equal(r.after[pk, pi], got["retest"][1]), K
    assert torch.equal(r.out, got["place"][0]) and torch.equal(r.count, got["place"][1]) and int(r.n_affected.min()) >= 2
    assert torch.equal(r.affected[pk, pi], pconns) and bool(torch.isfinite(got["retest"][1]).all())
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    # two alternations, as --release: plain place is not timed right behind (a)'s copies of the sample
    times = {k: [] for k in ("impact", "retest", "impact_pair", "place")}
    for _ in range(rounds):
        times["impact"].append(timed_event(ways["impact"]))
        times["retest"].append(timed_event(ways["retest"]))
    for _ in range(warmup):
        ways["impact"](), ways["place"]()
    for _ in range(rounds):
        times["impact_pair"].append(timed_event(ways["impact"]))
        times["place"].append(timed_event(ways["place"]))
    res = dict(shape=f"status {L} x {Q}", kind="lightpath_place_impact", K=K, max_affected=max_affected, cells=int(ptr[-1]),
               pairs=T, affected_min=int(r.n_affected.min()), affected_max=int(r.n_affected.max()),
               lightpaths=len(set(conn_of[~free].tolist())), S=1, P=int(st.data.shape[1]), L=L, Q=Q, C=32, F=5,
               freq_threshold=thr, rounds=rounds, equal_bits=True)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_place_impact(args, device, commit):
    rows = []
    for K in args.place_impact:
        res = measure_place_impact(K, device, args.rounds, args.warmup)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| grid | K | pairs | place_impact ms (IQR) | (a) 2 x (materialise_retest + device_batch + predict) ms (IQR) | "
          "(a) / impact | place_impact beside (b) ms (IQR) | (b) plain place ms (IQR) | impact / (b) |")
    print("|---|---|---|---|---|---|---|---|---|")

    def ratio(r, num, den):                                 # differ: by more than the sum of the IQRs
        same = abs(r[num + "_ms"] - r[den + "_ms"]) <= r[num + "_iqr_ms"] + r[den + "_iqr_ms"]
        return "no difference" if same else f"{r[num + '_ms'] / r[den + '_ms']:.2f}x"
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['L']} x {r['Q']} | {r['K']} | {r['pairs']} | {cell('impact')} | {cell('retest')} | "
              f"{ratio(r, 'retest', 'impact')} | {cell('impact_pair')} | {cell('place')} | {ratio(r, 'impact_pair', 'place')} |")


def measure_reroute_impact(K, R, device, rounds, warmup, thr=0.12, max_affected=8):
    """``reroute_impact`` of K candidates, R released lightpaths each, against (a) two ``materialise_retest`` calls (the
    second with ``release=``) + ``device_batch`` + ``predict`` over the (candidate, affected lightpath) pairs, worked out on
    the host beforehand, (b) ``place_impact`` of the same candidates with nothing released and (c) ``place(release=)``."""
    import numpy as np
    from gnn_qot_estimation_amd import infer, to_graph as TG
    torch.manual_seed(0)
    predict = q.LightpathPredictor(q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval())
    ns = TG.synthetic_network_status(1, seed=0)             # the 60 x 72 grid
    fi, feats = ns.feature_indexes, list(TG.DEFAULT_FEATURES)
    data = ns.data.copy()
    under_test = (data[0, fi["osnr"]] == -1) & (data[0, fi["snr"]] == -1) & (data[0, fi["ber"]] == -1)
    data[0][:, under_test] = 0.0                            # as --place-impact: every retest sample of (a) holds one LUT node
    L, Q = data.shape[2], data.shape[3]
    free = ~np.any(data[0] != 0, axis=0)
    conn_of = data[0, fi["conn_id"]].astype(np.int64)
    conns = sorted(set(conn_of[~free].tolist()))
    if R > min(len(conns) - 2, infer.PLACE_MAX_RELEASE):
        raise SystemExit(f"--release {R}: the sample holds {len(conns)} lightpaths, the cap is {infer.PLACE_MAX_RELEASE}")
    # the candidates are --place-impact's: one slot on the links where a lightpath sits within two slots (0.10 < thr)
    near = {(l, g): {int(conn_of[l, f]) for f in range(max(0, g - 2), min(Q, g + 3)) if not free[l, f]}
            for l in range(L) for g in range(Q) if free[l, g]}
    by_slot = {}
    for (l, g), who in near.items():
        if who:
            by_slot.setdefault(g, []).append(l)
    slots = sorted(g for g, ls in by_slot.items() if len(set().union(*(near[l, g] for l in ls))) >= 2)
    assert slots, "no slot of the sample lets a candidate meet two lightpaths"
    # who loses whom: the released lightpaths are drawn among those with a neighbour of their own
    sources = {c: set(TG._sources_of(data[0], ns.freq, fi, c, thr)[1]) for c in conns}
    sociable = [c for c in conns if sources[c]]
    rng = np.random.default_rng(K)
    values, cells, ptr, release, pairs = np.zeros((K, len(ns.lp_feat))), [], [0], [], []
    kinds = [0, 0, 0]                                       # affected lightpaths that gain only, lose only, do both
    for k in range(K):
        slot = slots[int(rng.integers(len(slots)))]
        links, met = [], set()
        for l in rng.permutation(by_slot[slot]):
            links.append(int(l))
            met |= near[int(l), slot]
            if len(met) >= 2 and len(links) >= int(rng.integers(1, 5)):
                break
        mine = np.stack([np.asarray(links), np.full(len(links), slot)])
        cells.append(mine)
        ptr.append(ptr[-1] + len(links))
        v = values[k]
        v[fi["conn_id"]], v[fi["src_id"]], v[fi["dst_id"]] = 10000 + k, 1, 2
        v[fi["mod_order"]], v[fi["path_len"]] = float(rng.choice([4, 8, 16, 32, 64])), float(rng.integers(24214, 7834746))
        v[fi["num_spans"]], v[fi["freq"]] = float(rng.integers(1, 107)), ns.freq[slot]
        v[fi["osnr"]] = v[fi["snr"]] = v[fi["ber"]] = -1.0
        while True:                                         # released: a lightpath with a source of its own, then R - 1 others
            first = sociable[int(rng.integers(len(sociable)))]
            rel = [first] + [int(c) for c in rng.choice([c for c in conns if c != first], size=R - 1, replace=False)]
            if sources[first] - set(rel):                   # ... that leave it a surviving neighbour
                break
        release += rel
        impact = TG.reroute_impact(data[0], ns.freq, fi, v, mine, thr, rel)
        assert any(t[6] for t in impact), (k, impact)       # a condition on the inputs: somebody loses a source
        for t in impact:
            kinds[0 if not t[6] else 1 if not t[5] else 2] += 1
        pairs += [(k, i, t[0]) for i, t in enumerate(impact[:max_affected])]
    st = TG.NetworkStatus(data, ns.target, ns.lp_feat, ns.metric, ns.link, ns.freq).to_device(device)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)       # noqa: E731
    samples, values_d = torch.zeros(K, dtype=torch.int64, device=device), torch.from_numpy(values).to(device)
    cells_d, ptr_d = dev(np.concatenate(cells, axis=1)), dev(ptr)
    rel_d, rptr_d = dev(release), dev(np.arange(K + 1) * R)
    # (a)'s arguments, one row per pair, prepared beforehand: which favours (a)
    T = len(pairs)
    pk, pi = dev([k for k, _, _ in pairs]), dev([i for _, i, _ in pairs])
    psamples, pconns, pvalues = torch.zeros(T, dtype=torch.int64, device=device), dev([c for _, _, c in pairs]), values_d[pk]
    pcells = dev(np.concatenate([cells[k] for k, _, _ in pairs], axis=1))
    pptr = dev(np.cumsum([0] + [cells[k].shape[1] for k, _, _ in pairs]))
    prel, prptr = dev(np.concatenate([release[k * R:(k + 1) * R] for k, _, _ in pairs])), dev(np.arange(T + 1) * R)

    def retest():
        before = predict(TG.device_batch(infer.materialise_retest(st, psamples, pconns), "lightpath", feats, None, thr))[0]
        after = predict(TG.device_batch(infer.materialise_retest(st, psamples, pconns, pvalues, pcells, pptr, release=prel,
                                                                 release_ptr=prptr), "lightpath", feats, None, thr))[0]
        return before, after
    ways = {"reroute": lambda: predict.reroute_impact(st, samples, values_d, cells_d, ptr_d, feats, thr, max_affected,
                                                      release=rel_d, release_ptr=rptr_d),
            "retest": retest,
            "impact": lambda: predict.place_impact(st, samples, values_d, cells_d, ptr_d, feats, thr, max_affected),
            "release": lambda: predict.place(st, samples, values_d, cells_d, ptr_d, feats, thr, release=rel_d, release_ptr=rptr_d)}
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    r = got["reroute"]
    assert torch.equal(r.before[pk, pi], got["retest"][0]) and torch.equal(r.after[pk, pi], got["retest"][1]), K
    assert torch.equal(r.out, got["release"][0]) and torch.equal(r.count, got["release"][1])
    assert torch.equal(r.affected[pk, pi], pconns) and bool(torch.isfinite(got["retest"][1]).all())
    assert int(r.lost.max()) >= 1 and int(r.n_affected.min()) >= 1
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    # three alternations, as --place-impact: neither launch is timed right behind (a)'s copies of the sample
    times = {}
    for mine, other in (("reroute", "retest"), ("reroute_b", "impact"), ("reroute_c", "release")):
        times[mine], times[other] = [], []
        for _ in range(warmup):
            ways["reroute"](), ways[other]()
        for _ in range(rounds):
            times[mine].append(timed_event(ways["reroute"]))
            times[other].append(timed_event(ways[other]))
    res = dict(shape=f"status {L} x {Q}", kind="lightpath_reroute_impact", K=K, R=R, max_affected=max_affected,
               cells=int(ptr[-1]), pairs=T, affected_min=int(r.n_affected.min()), affected_max=int(r.n_affected.max()),
               gain_only=kinds[0], lose_only=kinds[1], both=kinds[2], lightpaths=len(conns), S=1, P=int(st.data.shape[1]),
               L=L, Q=Q, C=32, F=5, freq_threshold=thr, rounds=rounds, equal_bits=True)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_reroute_impact(args, device, commit):
    rows = []
    for K in args.reroute_impact:
        res = measure_reroute_impact(K, args.release or 2, device, args.rounds, args.warmup)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| grid | K | R | pairs | reroute_impact ms (IQR) | (a) 2 x (materialise_retest + device_batch + predict) ms (IQR) | "
          "(a) / reroute | beside (b) ms (IQR) | (b) place_impact ms (IQR) | reroute / (b) | beside (c) ms (IQR) | "
          "(c) place(release=) ms (IQR) | reroute / (c) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")

    def ratio(r, num, den):                                 # differ: by more than the sum of the IQRs
        same = abs(r[num + "_ms"] - r[den + "_ms"]) <= r[num + "_iqr_ms"] + r[den + "_iqr_ms"]
        return "no difference" if same else f"{r[num + '_ms'] / r[den + '_ms']:.2f}x"
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['L']} x {r['Q']} | {r['K']} | {r['R']} | {r['pairs']} | {cell('reroute')} | {cell('retest')} | "
              f"{ratio(r, 'retest', 'reroute')} | {cell('reroute_b')} | {cell('impact')} | {ratio(r, 'reroute_b', 'impact')} | "
              f"{cell('reroute_c')} | {cell('release')} | {ratio(r, 'reroute_c', 'release')} |")


def measure_retest(S, device, rounds, warmup, thr=0.12, max_lightpaths=256):
    """``retest`` of every lightpath of S status samples against (a) ``materialise_retest`` over all (sample, lightpath)
    pairs + ``device_batch`` + ``predict`` -- the pairs worked out on the host beforehand -- and (b) ``from_status`` of the
    same samples: one row per sample."""
    import numpy as np
    from gnn_qot_estimation_amd import infer, to_graph as TG
    torch.manual_seed(0)
    predict = q.LightpathPredictor(q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval())
    ns = TG.synthetic_network_status(S, seed=0)             # the 60 x 72 grid
    fi, feats = ns.feature_indexes, list(TG.DEFAULT_FEATURES)
    L, Q = ns.data.shape[2], ns.data.shape[3]
    orders = []                                             # per sample: its conns in first-seen (scan) order
    for s in range(S):
        occupied = np.any(ns.data[s] != 0, axis=0).ravel()
        conn = ns.data[s, fi["conn_id"]].ravel()[occupied].astype(np.int64)
        _, first = np.unique(conn, return_index=True)
        orders.append(conn[np.sort(first)].tolist())
    pairs = [(s, i, c) for s in range(S) for i, c in enumerate(orders[s][:max_lightpaths])]
    T = len(pairs)
    st = ns.to_device(device)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)       # noqa: E731
    ps, pi, pconns = dev([s for s, _, _ in pairs]), dev([i for _, i, _ in pairs]), dev([c for _, _, c in pairs])
    chunk = infer.retest_chunk(S, max_lightpaths, torch.cuda.get_device_properties(device).multi_processor_count)

    def materialise():
        batch = TG.device_batch(infer.materialise_retest(st, ps, pconns), "lightpath", feats, None, thr)
        return predict(batch)[0], batch
    ways = {"retest": lambda: predict.retest(st, None, None, feats, thr, max_lightpaths),
            "materialise": materialise,
            "from_status": lambda: predict.from_status(st, None, feats, thr)}
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    r, (rows, batch) = got["retest"], got["materialise"]
    luts = predict.model._lut_rows(batch)
    at = torch.searchsorted(luts, batch.ptr.to(device)[:-1] + pi)
    assert torch.equal(luts[at], batch.ptr.to(device)[:-1] + pi)
    assert torch.equal(r.out[ps, pi], rows[at]) and bool(torch.isfinite(rows[at]).all()), S       # equal bits
    assert torch.equal(r.conn[ps, pi], pconns) and r.n.tolist() == [len(o) for o in orders]
    assert torch.equal(r.count, got["from_status"][1])
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    # two alternations, as --place-impact: from_status is not timed right behind (a)'s copies of the samples
    times = {k: [] for k in ("retest", "materialise", "retest_pair", "from_status")}
    for _ in range(rounds):
        times["retest"].append(timed_event(ways["retest"]))
        times["materialise"].append(timed_event(ways["materialise"]))
    for _ in range(warmup):
        ways["retest"](), ways["from_status"]()
    for _ in range(rounds):
        times["retest_pair"].append(timed_event(ways["retest"]))
        times["from_status"].append(timed_event(ways["from_status"]))
    res = dict(shape=f"status {L} x {Q}", kind="lightpath_retest", S=S, max_lightpaths=max_lightpaths, chunk=chunk, pairs=T,
               lightpaths_min=int(r.n.min()), lightpaths_max=int(r.n.max()), P=int(st.data.shape[1]), L=L, Q=Q, C=32, F=5,
               freq_threshold=thr, rounds=rounds, equal_bits=True)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_retest(args, device, commit):
    rows = []
    for S in args.retest:
        res = measure_retest(S, device, args.rounds, args.warmup, max_lightpaths=args.max_lightpaths)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| grid | S | pairs | chunk | retest ms (IQR) | (a) materialise_retest + device_batch + predict ms (IQR) | "
          "(a) / retest | retest beside (b) ms (IQR) | (b) from_status ms (IQR) | retest / (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|")

    def ratio(r, num, den):                                 # differ: by more than the sum of the IQRs
        same = abs(r[num + "_ms"] - r[den + "_ms"]) <= r[num + "_iqr_ms"] + r[den + "_iqr_ms"]
        return "no difference" if same else f"{r[num + '_ms'] / r[den + '_ms']:.2f}x"
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['L']} x {r['Q']} | {r['S']} | {r['pairs']} | {r['chunk']} | {cell('retest')} | {cell('materialise')} | "
              f"{ratio(r, 'materialise', 'retest')} | {cell('retest_pair')} | {cell('from_status')} | "
              f"{ratio(r, 'retest_pair', 'from_status')} |")


def measure_place_slots(R, device, rounds, warmup, thr=0.12, width=1, chunk=None):
    """``place_slots`` of R routes of 3 links over every start slot of one status sample against (a) the only way
    before -- ``materialise_slot_sweep`` (occupancy, the host read of the free slots, list building) + ``place`` -- and (b)
    ``place`` on those lists built outside the timed region: what the shared scan is worth without the saved host work."""
    import numpy as np
    from gnn_qot_estimation_amd import infer, to_graph as TG
    torch.manual_seed(0)
    predict = q.LightpathPredictor(q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval())
    ns = TG.synthetic_network_status(1, seed=0)             # the 60 x 72 grid
    fi, feats = ns.feature_indexes, list(TG.DEFAULT_FEATURES)
    data = ns.data.copy()
    under_test = (data[0, fi["osnr"]] == -1) & (data[0, fi["snr"]] == -1) & (data[0, fi["ber"]] == -1)
    data[0][:, under_test] = 0.0                            # as --place: the sample's own lightpath under test goes
    L, Q = data.shape[2], data.shape[3]
    rng = np.random.default_rng(R)
    values, links = np.zeros((R, len(ns.lp_feat))), []
    for r in range(R):
        links += [int(l) for l in rng.choice(L, size=3, replace=False)]
        v = values[r]
        v[fi["conn_id"]], v[fi["src_id"]], v[fi["dst_id"]] = 10000 + r, 1, 2
        v[fi["mod_order"]], v[fi["path_len"]] = float(rng.choice([4, 8, 16, 32, 64])), float(rng.integers(24214, 7834746))
        v[fi["num_spans"]] = float(rng.integers(1, 107))
        v[fi["osnr"]] = v[fi["snr"]] = v[fi["ber"]] = -1.0
    st = TG.NetworkStatus(data, ns.target, ns.lp_feat, ns.metric, ns.link, ns.freq).to_device(device)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device)       # noqa: E731
    samples, values_d, links_d, ptr_d = torch.zeros(R, dtype=torch.int64, device=device), torch.from_numpy(values).to(device), \
        dev(links), dev(3 * np.arange(R + 1))
    used = chunk or infer.place_slots_chunk(R, Q, torch.cuda.get_device_properties(device).multi_processor_count)
    sw = infer.materialise_slot_sweep(st, samples, values_d, links_d, ptr_d, width=width)      # (b)'s lists, built beforehand
    K = int(sw.route.shape[0])
    assert 0 < K < R * Q, (K, R, Q)                         # a condition on the inputs: free and occupied slots both

    def materialise():
        m = infer.materialise_slot_sweep(st, samples, values_d, links_d, ptr_d, width=width)
        return predict.place(st, m.samples, m.values, m.cells, m.cell_ptr, feats, thr)[0], m
    ways = {"slots": lambda: predict.place_slots(st, samples, values_d, links_d, ptr_d, feats, thr, width=width, chunk=chunk),
            "materialise": materialise,
            "place": lambda: predict.place(st, sw.samples, sw.values, sw.cells, sw.cell_ptr, feats, thr)[0]}
    got = {k: fn() for k, fn in ways.items()}
    torch.cuda.synchronize()
    predict.check_status()
    r, (rows, m) = got["slots"], got["materialise"]
    assert torch.equal(r.free, sw.free) and torch.equal(m.free, sw.free)
    assert torch.equal(r.out[sw.route, sw.slot], rows) and torch.equal(rows, got["place"]), R   # equal bits
    assert bool(torch.isfinite(rows).all()) and bool(torch.isnan(r.out[~r.free]).all())
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    # two alternations, as --retest: plain place is not timed right behind (a)'s list building
    times = {k: [] for k in ("slots", "materialise", "slots_pair", "place")}
    for _ in range(rounds):
        times["slots"].append(timed_event(ways["slots"]))
        times["materialise"].append(timed_event(ways["materialise"]))
    for _ in range(warmup):
        ways["slots"](), ways["place"]()
    for _ in range(rounds):
        times["slots_pair"].append(timed_event(ways["slots"]))
        times["place"].append(timed_event(ways["place"]))
    res = dict(shape=f"status {L} x {Q}", kind="lightpath_place_slots", R=R, route_links=3, width=width, chunk=used, free=K,
               cells=int(sw.cells.shape[1]), P=int(st.data.shape[1]), L=L, Q=Q, C=32, F=5, freq_threshold=thr, rounds=rounds,
               equal_bits=True)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_place_slots(args, device, commit):
    rows = []
    for R in args.place_slots:
        res = measure_place_slots(R, device, args.rounds, args.warmup, width=args.width, chunk=args.chunk)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| grid | R | width | chunk | free | place_slots ms (IQR) | (a) materialise_slot_sweep + place ms (IQR) | "
          "(a) / place_slots | place_slots beside (b) ms (IQR) | (b) place on prebuilt lists ms (IQR) | place_slots / (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")

    def ratio(r, num, den):                                 # differ: by more than the sum of the IQRs
        same = abs(r[num + "_ms"] - r[den + "_ms"]) <= r[num + "_iqr_ms"] + r[den + "_iqr_ms"]
        return "no difference" if same else f"{r[num + '_ms'] / r[den + '_ms']:.2f}x"
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['L']} x {r['Q']} | {r['R']} | {r['width']} | {r['chunk']} | {r['free']} | {cell('slots')} | "
              f"{cell('materialise')} | {ratio(r, 'materialise', 'slots')} | {cell('slots_pair')} | {cell('place')} | "
              f"{ratio(r, 'slots_pair', 'place')} |")


LIGHTPATH_SIZES = (1, 8, 512, 65536)


def measure_lightpath(B, device, rounds, warmup):
    torch.manual_seed(0)
    model = q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval()
    distinct = min(B, 64)
    data = S.tile_batch(S.lightpath_batch(distinct), B // distinct).to(device)
    predict = q.LightpathPredictor(model)

    def eager():
        with torch.no_grad():
            return model(data)

    for _ in range(3):
        want, want_b = eager()
    got, got_b = predict(data)
    per, count = predict.per_graph(data)
    torch.cuda.synchronize()
    predict.check_status()
    scale = want.double().abs().max()
    err = float((got.double() - want.double()).abs().max() / scale)
    err_per = float((per.double() - want.double()).abs().max() / scale)       # (one LUT node per graph, graph order)
    assert torch.equal(got_b, want_b) and bool((count == 1).all()) and err <= 1e-4 and err_per <= 1e-4, (B, err, err_per)

    ways = {"predict": lambda: predict(data), "per_graph": lambda: predict.per_graph(data), "eager": eager}
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed(fn))
    res = dict(shape=f"lightpath B={B}", kind="lightpath", B=B, C=32, F=5, N=int(data.x.shape[0]),
               E=int(data.edge_index.shape[1]), rounds=rounds, rel_err=err, rel_err_per_graph=err_per)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


LIGHTPATH_GRAD_SIZES = (1, 8, 512)


def measure_lightpath_grad(B, device, rounds, warmup):
    torch.manual_seed(0)
    model = q.LightpathGNN(5, 32, 3, 1, dropout_p=0.0).to(device).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    distinct = min(B, 64)
    data = S.tile_batch(S.lightpath_batch(distinct), B // distinct).to(device)
    leaf = S.tile_batch(S.lightpath_batch(distinct), B // distinct).to(device)
    leaf.x = leaf.x.detach().clone().requires_grad_()
    predict = q.LightpathPredictor(model)

    def autograd():
        out, lb = model(leaf)
        jac = []
        for o in range(out.shape[1]):
            leaf.x.grad = None
            out[:, o].sum().backward(retain_graph=True)
            jac.append(leaf.x.grad)
        return out, jac

    for _ in range(3):
        want_out, want = autograd()
    want = torch.stack(want).double()
    out, lb, jac_self, jac_edge = predict.sensitivity(data)
    torch.cuda.synchronize()
    predict.check_status()
    rows = model._lut_rows(data)
    got = torch.zeros_like(want)                           # the identity: J.index_add_(0, src, jac_edge); J[lut] += jac_self
    for k in range(got.shape[0]):
        got[k].index_add_(0, data.edge_index[0], jac_edge[k].double())
        got[k][rows] += jac_self[k].double()
    err = float((got - want).abs().max() / want.abs().max())
    want_out = want_out.detach().double()
    err_out = float((out.double() - want_out).abs().max() / want_out.abs().max())
    assert err <= 1e-4 and err_out <= 1e-4, (B, err, err_out)

    ways = {"sensitivity": lambda: predict.sensitivity(data), "eager": autograd}
    for _ in range(warmup):
        for fn in ways.values():
            fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed_event(fn))
    res = dict(shape=f"lightpath B={B}", kind="lightpath_grad", outputs=3, B=B, C=32, F=5, N=int(data.x.shape[0]),
               E=int(data.edge_index.shape[1]), rows=int(rows.numel()), rounds=rounds, rel_err=err, rel_err_out=err_out)
    for k, ts in times.items():
        q1, _, q3 = statistics.quantiles(ts, n=4)
        res[f"{k}_ms"], res[f"{k}_iqr_ms"] = statistics.median(ts), q3 - q1
        res[f"{k}_min_ms"], res[f"{k}_max_ms"] = min(ts), max(ts)
    return res


def main_lightpath_grad(args, device, commit):
    rows = []
    for B in LIGHTPATH_GRAD_SIZES:
        res = measure_lightpath_grad(B, device, args.rounds, args.warmup)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| B (nodes, edges) | sensitivity ms (IQR) | forward + 3 backward ms (IQR) | autograd / sensitivity |")
    print("|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['B']} ({r['N']}, {r['E']}) | {cell('sensitivity')} | {cell('eager')} | {verdict(r, 'sensitivity')} |")


def verdict(r, way):
    """``way`` against the eager forward: the ratio of the medians, or "no difference" (module docstring)."""
    a, b = r[f"{way}_ms"], r["eager_ms"]
    if abs(a - b) <= max(r[f"{way}_iqr_ms"], r["eager_iqr_ms"]):
        return "no difference"
    return f"{b / a:.2f}x"


def main_lightpath(args, device, commit):
    rows = []
    for B in LIGHTPATH_SIZES:
        res = measure_lightpath(B, device, args.rounds, args.warmup)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| B (nodes, edges) | predict ms (IQR) | per_graph ms (IQR) | eager ms (IQR) | eager / predict | eager / per_graph |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: f"{r[k + '_ms']:.3f} ({r[k + '_iqr_ms']:.3f})"                     # noqa: E731
        print(f"| {r['B']} ({r['N']}, {r['E']}) | {cell('predict')} | {cell('per_graph')} | {cell('eager')} | "
              f"{verdict(r, 'predict')} | {verdict(r, 'per_graph')} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kind", choices=["topological", "lightpath"], default="topological")
    ap.add_argument("--mc", type=int, default=None, metavar="T",
                    help="Monte-Carlo dropout: predict.sample(data, T) against T train-mode forwards")
    ap.add_argument("--grad", action="store_true",
                    help="sensitivity: predict.sensitivity(data) against eval forward + one backward per output "
                         "(with --kind lightpath: LightpathPredictor's)")
    ap.add_argument("--what-if", type=int, nargs="+", default=None, metavar="K", dest="what_if",
                    help="what-if: predict.what_if on K one-lightpath candidates against materialise_what_if + predict and "
                         "predict on a prebuilt batch (with --kind lightpath: LightpathPredictor's, K candidates of the "
                         "LUT node)")
    ap.add_argument("--from-status", action="store_true", dest="from_status",
                    help="predict.from_status(status) against device_batch + per_graph (--kind lightpath) or device_batch + "
                         "predict (--kind topological)")
    ap.add_argument("--place", type=int, nargs="+", default=None, metavar="K",
                    help="predict.place on K candidates of one status sample against materialise_placement + from_status "
                         "(--kind lightpath: and against device_batch + what_if with the interferers precomputed)")
    ap.add_argument("--links", type=int, default=60, metavar="L",
                    help="with --place: the links of the sample's grid (the scan of a sample is O(L Q): 6 against 60 tells "
                         "what the scan costs)")
    ap.add_argument("--cells", type=int, default=None, metavar="N",
                    help="with --place: N links per candidate instead of 1 - 6 (the walk is O(cells Q))")
    ap.add_argument("--release", type=int, default=None, metavar="R",
                    help="with --place: every candidate releases R lightpaths of the sample in the same launch (place(..., "
                         "release=)), against materialise_placement(release=) + from_status and against plain place")
    ap.add_argument("--place-impact", type=int, nargs="+", default=None, metavar="K", dest="place_impact",
                    help="--kind lightpath: predict.place_impact on K candidates of one status sample against "
                         "materialise_retest + device_batch + predict over the (candidate, interferer) pairs and against "
                         "plain place")
    ap.add_argument("--reroute-impact", type=int, nargs="+", default=None, metavar="K", dest="reroute_impact",
                    help="--kind lightpath: predict.reroute_impact on K candidates of one status sample, each releasing R "
                         "lightpaths (--release R, default 2), against materialise_retest(release=) + device_batch + predict "
                         "over the (candidate, affected lightpath) pairs, against place_impact and against place(release=)")
    ap.add_argument("--retest", type=int, nargs="+", default=None, metavar="S",
                    help="--kind lightpath: predict.retest on every lightpath of S status samples against materialise_retest "
                         "+ device_batch + predict over the (sample, lightpath) pairs and against from_status")
    ap.add_argument("--max-lightpaths", type=int, default=256, metavar="M", dest="max_lightpaths",
                    help="with --retest: the slots per sample (the grid is S * ceil(M / chunk) workgroups, each of which "
                         "discovers its sample: 32 against 256 tells what the workgroups without a lightpath cost)")
    ap.add_argument("--place-slots", type=int, nargs="+", default=None, metavar="R", dest="place_slots",
                    help="--kind lightpath: predict.place_slots on R routes of 3 links over every start slot of one status "
                         "sample against materialise_slot_sweep + place and against place on prebuilt lists")
    ap.add_argument("--width", type=int, default=1, metavar="W",
                    help="with --place-slots: the slots a candidate occupies on every link of its route (1 ... 8)")
    ap.add_argument("--chunk", type=int, default=None, metavar="C",
                    help="with --place-slots: the start slots per workgroup (1 ... 32) instead of infer.place_slots_chunk's")
    args = ap.parse_args()
    if args.place_slots is None and (args.width != 1 or args.chunk is not None):
        raise SystemExit("--width and --chunk go with --place-slots")
    if args.place_slots is not None and (args.kind != "lightpath" or args.place is not None or args.from_status
                                         or args.mc is not None or args.grad or args.what_if is not None
                                         or args.place_impact is not None or args.reroute_impact is not None
                                         or args.retest is not None or any(r < 1 for r in args.place_slots)
                                         or not 1 <= args.width <= 8 or (args.chunk is not None and not 1 <= args.chunk <= 32)):
        raise SystemExit("--kind lightpath --place-slots R [R ...] (R >= 1) [--width 1 ... 8] [--chunk 1 ... 32] is a run of its own")
    if args.retest is None and args.max_lightpaths != 256:
        raise SystemExit("--max-lightpaths goes with --retest")
    if args.retest is not None and (args.kind != "lightpath" or args.place is not None or args.from_status
                                    or args.mc is not None or args.grad or args.what_if is not None
                                    or args.place_impact is not None or any(s < 1 for s in args.retest)):
        raise SystemExit("--kind lightpath --retest S [S ...] (S >= 1) is a run of its own")
    if args.place_impact is not None and (args.kind != "lightpath" or args.place is not None or args.from_status
                                          or args.mc is not None or args.grad or args.what_if is not None
                                          or any(k < 1 for k in args.place_impact)):
        raise SystemExit("--kind lightpath --place-impact K [K ...] (K >= 1) is a run of its own")
    if args.reroute_impact is not None and (args.kind != "lightpath" or args.place is not None or args.from_status
                                            or args.mc is not None or args.grad or args.what_if is not None
                                            or args.place_impact is not None or args.retest is not None
                                            or any(k < 1 for k in args.reroute_impact)):
        raise SystemExit("--kind lightpath --reroute-impact K [K ...] (K >= 1) is a run of its own")
    if args.place is None and (args.links != 60 or args.cells is not None
                               or (args.release is not None and args.reroute_impact is None)):
        raise SystemExit("--links and --cells go with --place, --release with --place or --reroute-impact")
    if args.release is not None and args.release < 1:
        raise SystemExit("--release R (R >= 1)")
    if args.links < 6 or (args.cells is not None and not 1 <= args.cells <= args.links):
        raise SystemExit("--links L (>= 6, what synthetic_network_status routes over) and --cells N (1 ... L)")
    if args.place is not None and (args.from_status or args.mc is not None or args.grad or args.what_if is not None
                                   or any(k < 1 for k in args.place)):
        raise SystemExit("--place K [K ...] (K >= 1) is a run of its own")
    if args.from_status and (args.mc is not None or args.grad or args.what_if is not None):
        raise SystemExit("--from-status is a run of its own")
    if args.what_if is not None and (args.mc is not None or args.grad or any(k < 1 for k in args.what_if)):
        raise SystemExit("--what-if K [K ...] (K >= 1) is a run of its own")
    if args.mc is not None and args.kind != "topological":
        raise SystemExit("--mc is for the topological model")
    if args.mc is not None and args.grad:
        raise SystemExit("--mc and --grad are separate runs")
    if args.rounds < 20:
        raise SystemExit("--rounds: at least 20 timed calls per way")
    if not torch.cuda.is_available():
        raise SystemExit("bench_infer.py needs an MI355X: no GPU is visible (nothing is measured on the CPU)")
    device = torch.device("cuda:0")
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    if args.place_slots is not None:
        return main_place_slots(args, device, commit)
    if args.reroute_impact is not None:
        return main_reroute_impact(args, device, commit)
    if args.place_impact is not None:
        return main_place_impact(args, device, commit)
    if args.retest is not None:
        return main_retest(args, device, commit)
    if args.place is not None and args.release is not None:
        return main_place_release(args, device, commit)
    if args.place is not None:
        return (main_place if args.kind == "lightpath" else main_topological_place)(args, device, commit)
    if args.from_status:
        return main_from_status(args, device, commit)
    if args.kind == "lightpath" and args.what_if is not None:
        return main_lightpath_what_if(args, device, commit)
    if args.kind == "lightpath":
        return (main_lightpath_grad if args.grad else main_lightpath)(args, device, commit)
    if args.what_if is not None:
        return main_what_if(args, device, commit)
    if args.mc is not None:
        return main_mc(args, device, commit)
    if args.grad:
        return main_grad(args, device, commit)
    rows = []
    for shape in SHAPES:
        res = measure(shape, device, args.rounds, args.warmup)
        res["commit"] = commit or None
        res["device"] = torch.cuda.get_device_name(0)
        rows.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print("\n| shape | fused ms | (a) eager ms | (b) replay ms | eager / fused | replay / fused |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['shape']} (n={r['n']}, e={r['e']}, H={r['H']}) | {r['fused_ms']:.3f} | {r['eager_ms']:.3f} | "
              f"{r['replay_ms']:.3f} | {r['eager_ms'] / r['fused_ms']:.2f} | {r['replay_ms'] / r['fused_ms']:.2f} |")


if __name__ == "__main__":
    main()
