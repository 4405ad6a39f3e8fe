"""Samples per second of graph construction from network-status samples: the device builder (``csrc/status_graph.hip``,
``to_graph.build_shard(DeviceStatus, ...)``) against the host path ``to_graph.build_shard(ns, ...).to_device()`` on the same
``synthetic_network_status`` (default 60 x 72 grid), both representations, S = 64, 1024 and 16 384 samples per call.

Protocol of ``tools/bench_infer.py``: both ways alternate in one process; per way WARMUP calls, then ROUNDS timed calls,
each timed by the host clock between two device synchronisations; the figure is the median with the interquartile range; a
difference of two medians that does not exceed the larger of the two interquartile ranges is reported as no difference.
Before anything is timed the device shard is compared with the host shard in canonical link order (``torch.equal``).

The host path costs milliseconds per sample, so its rounds shrink with S (``--host-seconds`` bounds the time spent on it
per shape: at least 3 rounds when one call fits, else the row says NOT MEASURED).  Samples above 1024 are tiles of 1024
distinct ones (the generator itself is a Python loop).  The one-off upload of the status chunk (``NetworkStatus.to_device``)
is timed separately and reported on a line of its own.

    python tools/bench_to_graph.py [--sizes 64 1024 16384] [--rounds 20] [--warmup 3] [--out profiles/bench_to_graph.jsonl]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gnn_qot_estimation_amd import to_graph as TG  # noqa: E402

DISTINCT = 1024
FIELDS = ("node_ptr", "edge_ptr", "edge_index", "x", "edge_attr", "node_ids", "y")


def status_of(S):
    base = TG.synthetic_network_status(min(S, DISTINCT), seed=0)
    if S <= DISTINCT:
        return base
    reps = S // DISTINCT
    return TG.NetworkStatus(np.tile(base.data, (reps, 1, 1, 1)), np.tile(base.target, (reps, 1)), base.lp_feat, base.metric,
                            base.link, base.freq)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(ts):
    if len(ts) < 2:
        return ts[0], float("nan")
    q1, _, q3 = statistics.quantiles(ts, n=4)
    return statistics.median(ts), q3 - q1


def measure(ns, st, rep, device, rounds, warmup, host_seconds, check):
    S = len(ns)
    dev_fn = lambda: TG.build_shard(st, rep)                                   # noqa: E731
    host_fn = lambda: TG.build_shard(ns, rep).to_device(device)                # noqa: E731
    res = dict(representation=rep, S=S, links=int(ns.data.shape[2]), freqs=int(ns.data.shape[3]), rounds=rounds)
    got = dev_fn()
    if check:
        want = TG.canonical_shard(TG.build_shard(ns, rep, samples=range(min(S, 256))))
        part = TG.build_shard(st, rep, samples=range(min(S, 256)))
        for name in FIELDS:
            a, b = getattr(part, name), getattr(want, name)
            assert (a is None and b is None) or torch.equal(a.cpu(), b), (rep, S, name)
    res["nodes"], res["links_directed"] = int(got.node_ptr[-1]), int(got.edge_ptr[-1])
    one_host = timed(host_fn)                                                   # also the host way's first warm-up call
    host_rounds = min(rounds, int(host_seconds / max(one_host, 1e-9)))
    for _ in range(warmup):
        dev_fn()
    dev_t, host_t = [], []
    for r in range(rounds):
        dev_t.append(timed(dev_fn))
        if r < host_rounds:
            host_t.append(timed(host_fn))
    med, iqr = spread(dev_t)
    res.update(device_s=med, device_iqr_s=iqr, device_samples_per_s=S / med)
    if host_rounds >= 3:
        hmed, hiqr = spread(host_t)
        res.update(host_s=hmed, host_iqr_s=hiqr, host_samples_per_s=S / hmed, host_rounds=host_rounds)
        res["verdict"] = "no difference" if abs(hmed - med) <= max(iqr, hiqr) else f"{hmed / med:.1f}x"
    else:
        res.update(host_s=None, host_rounds=0, host_first_call_s=one_host,
                   verdict=f"NOT MEASURED (one host call takes {one_host:.1f} s: fewer than 3 rounds in {host_seconds:.0f} s)")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024, 16384])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-seconds", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_to_graph.py needs an MI355X: no GPU is visible (nothing is measured on the CPU)")
    device = torch.device("cuda:0")
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    rows = []
    for S in args.sizes:
        ns = status_of(S)
        st = ns.to_device(device)                                               # warm-up of the allocator
        del st
        ups = []
        for _ in range(3):
            holder = []
            ups.append(timed(lambda: holder.append(ns.to_device(device))))
            st = holder[0]
        up = dict(kind="upload", S=S, bytes=int(ns.data.nbytes + ns.target.nbytes), upload_s=statistics.median(ups),
                  commit=commit or None, device=torch.cuda.get_device_name(0))
        rows.append(up)
        print(json.dumps(up), flush=True)
        for rep in ("lightpath", "topological"):
            res = measure(ns, st, rep, device, args.rounds, args.warmup, args.host_seconds, check=True)
            res.update(kind="build", commit=commit or None, device=torch.cuda.get_device_name(0))
            rows.append(res)
            print(json.dumps(res), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    for r in rows:
                        f.write(json.dumps(r) + "\n")
        del st
    print("\n| representation | S | device samples/s (median s, IQR s) | host samples/s (median s, IQR s, rounds) | host / device |")
    print("|---|---|---|---|---|")
    for r in rows:
        if r["kind"] == "upload":
            print(f"| upload of the chunk | {r['S']} | {r['bytes'] / 2**20:.0f} MiB in {r['upload_s']:.3f} s | - | - |")
            continue
        host = "NOT MEASURED" if r["host_s"] is None else \
            f"{r['host_samples_per_s']:.0f} ({r['host_s']:.3f}, {r['host_iqr_s']:.3f}, {r['host_rounds']})"
        print(f"| {r['representation']} | {r['S']} | {r['device_samples_per_s']:.0f} ({r['device_s']:.5f}, {r['device_iqr_s']:.5f}) | "
              f"{host} | {r['verdict']} |")


if __name__ == "__main__":
    main()
