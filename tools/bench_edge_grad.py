"""Cost of edge_attr.grad: eager forward + backward of TopologicalGNN (train mode, dropout 0.5) with and without
``edge_attr.requires_grad``, at the reference's scale (75-node graphs, H = 16, D = 4, batch 512) and at cfg2's shape
(1024 graphs of 100 nodes / 400 edges, H = 64), under torch.cuda.Event timing; then the pieces the edge gradient adds,
replayed alone: the TransformerConv kernel, the NNConv kernel and the g Wk^T product NNConv feeds it.  One JSON line
per shape.  Usage: python tools/bench_edge_grad.py [--iters N]"""
import argparse, json, os, statistics, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gnn_qot_estimation_amd as q
from gnn_qot_estimation_amd import _lib, synthetic as S

SHAPES = {"reference": dict(B=512, n=75, e=200, H=16), "cfg2": dict(B=1024, n=100, e=400, H=64)}


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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, s in SHAPES.items():
        torch.manual_seed(0)
        batch = S.topological_batch(2, s["B"], n=s["n"], e=s["e"]).to(dev)
        y = batch.y.view(-1, 3)
        model = q.TopologicalGNN(s["n"], s["H"], 3, 4, dropout_p=0.5).to(dev).train()
        ea0 = batch.edge_attr.detach()

        def step(want):
            for p in model.parameters():
                p.grad = None
            batch.edge_attr = ea0.detach().requires_grad_(want)
            F.smooth_l1_loss(model(batch), y).backward()

        plain = event_ms(lambda: step(False), args.iters)
        with_grad = event_ms(lambda: step(True), args.iters)
        # the edge-gradient launches of one backward, recorded with their arguments and replayed alone
        rec = {}
        real = _lib.call

        def call(fname, *a):
            if fname.endswith("_edge_attr_grad"):
                rec[fname] = a
            return real(fname, *a)
        _lib.call = call
        try:
            step(True)
        finally:
            _lib.call = real
        torch.cuda.synchronize()
        row = {"shape": name, **s, "D": 4, "nodes": batch.num_nodes, "edges": batch.num_edges,
               "fwd_bwd_ms": round(plain, 4), "fwd_bwd_edge_grad_ms": round(with_grad, 4),
               "added_ms": round(with_grad - plain, 4)}
        for fname, a in rec.items():
            row[fname + "_us"] = round(1e3 * event_ms(lambda: real(fname, *a), args.iters), 2)
        H, K = s["H"], 8
        g, wk = torch.randn(batch.num_nodes, H, device=dev), torch.randn(K * H, H, device=dev)
        row["ga_product_us"] = round(1e3 * event_ms(lambda: g @ wk.t(), args.iters), 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
