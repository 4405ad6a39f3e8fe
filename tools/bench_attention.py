"""Cost of the attention-weights readout (``return_attention_weights=True``): eager eval forward of the model with and
without it, interleaved rounds in one process, torch.cuda.Event timing (median of the per-round medians), at three
shapes: the reference scale (TopologicalGNN, 75-node / 200-edge graphs, H = 16, B = 512), cfg2 (TopologicalGNN, 100-node /
400-edge graphs, H = 64, B = 1024) and a LightpathGNN shape (3 GATConv layers, C = 128, 4096 chain graphs of 2..20
nodes).  Then the attention launches of one forward, recorded with their arguments and replayed alone (20 back to back
per timed window).  One JSON line per shape.  Usage: python tools/bench_attention.py [--iters N] [--rounds R]"""
import argparse, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import _lib, synthetic as S

SHAPES = {"reference": dict(kind="topo", B=512, n=75, e=200, H=16), "cfg2": dict(kind="topo", B=1024, n=100, e=400, H=64),
          "lightpath_3x128": dict(kind="lightpath", B=4096, C=128, layers=3)}


def event_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        fn()
        en.record()
        torch.cuda.synchronize()
        times.append(st.elapsed_time(en))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, s in SHAPES.items():
        torch.manual_seed(0)
        if s["kind"] == "topo":
            batch = S.topological_batch(2, s["B"], n=s["n"], e=s["e"]).to(dev)
            model = q.TopologicalGNN(s["n"], s["H"], 3, 4).to(dev).eval()
        else:
            batch = S.lightpath_batch(s["B"]).to(dev)
            model = q.LightpathGNN(5, s["C"], 3, 1, num_layers=s["layers"]).to(dev).eval()

        def fwd(want):
            with torch.no_grad():
                model(batch, return_attention_weights=True) if want else model(batch)

        plain, attn = [], []
        for _ in range(args.rounds):           # interleaved A/B rounds
            plain.append(event_ms(lambda: fwd(False), args.iters))
            attn.append(event_ms(lambda: fwd(True), args.iters))
        rec = []
        real = _lib.call

        def call(fname, *a):
            if fname in ("qot_tconv_attention", "qot_gat_attention"):
                rec.append((fname, a))
            return real(fname, *a)
        _lib.call = call
        try:
            fwd(True)
        finally:
            _lib.call = real
        torch.cuda.synchronize()
        p, a = statistics.median(plain), statistics.median(attn)
        row = {"shape": name, **s, "nodes": batch.num_nodes, "edges": batch.num_edges, "fwd_ms": round(p, 4),
               "fwd_attention_ms": round(a, 4), "added_ms": round(a - p, 4),
               "fwd_ms_rounds": [round(t, 4) for t in plain], "fwd_attention_ms_rounds": [round(t, 4) for t in attn]}
        for k, (fname, a_) in enumerate(rec):      # 20 back-to-back launches per timed window: the kernel, not the event
            row[f"{fname}_{k}_us"] = round(1e3 * event_ms(lambda: [real(fname, *a_) for _ in range(20)], args.iters) / 20, 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
