"""How much of the stage-1 sums' time the grad-h kernel's ragged last round absorbs (cfg2 shape, interleaved rounds in ONE
process).  Four timed forms, each `it` back-to-back calls between two events:
  gradh          qot_nnconv_gradh_split alone (partials left in the workspace, as the training step calls it)
  gradh_hosted   the same call carrying the step's stage-1 sums as tail workgroups (qot_nnconv_gradh_host_roles)
  sums           one qot_run_roles launch of the same sums alone
  gradh_then_sums  the two launches back to back (the schedule without hosting)
The sums are the step's: the NNConv weight-gradient slabs, the TransformerConv graph-form partial rows, the read-out's
partials and the loss rows, at the sizes the library states for 1024 graphs of 100 nodes.  absorbed = gradh + sums -
gradh_hosted; saved_vs_two_launches = gradh_then_sums - gradh_hosted."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_qot_estimation_amd import _lib, functional as QF, synthetic as S
from gnn_qot_estimation_amd.graph import build_graph_index
dev = torch.device("cuda:0")
B, n_g = 1024, 100
b = S.topological_batch(2, B, n=n_g, e=400).to(dev)
N, H, D, K, O = b.num_nodes, 64, 4, 8, 3
g = build_graph_index(b.edge_index, N)
f = lambda *s: torch.randn(*s, device=dev)
x, gout, w1, b1 = f(N, H), f(N, H), f(K, D), f(K)
assert QF.nnconv_split_bf16(), "the split planes are packed only without QOT_NNCONV_F32_MFMA=1"
wp, _, _, split = QF.nnconv_pack(f(H * H, K) / 16, f(H * H) / 16, f(H, H) / 8, H, K)
bsplit, stride = split[wp.numel():], split.numel() // 3
lib = _lib.load()
wsh = torch.empty(lib.qot_nnconv_gradh_workspace_floats(D), device=dev)
slabs = f(lib.qot_nnconv_adjoint_dw_workspace_floats(D))
gpar = torch.empty((K + 2) * H * H, device=dev)
t_rows, t_len = int(lib.qot_tconv_bwd_graph_blocks(B)), int(lib.qot_tconv_graph_row_floats(n_g, H, D))
h_rows, h_len = int(lib.qot_head_train_blocks(B, H)), H * H + H + O * H + O + H
parts = [f(t_rows, t_len), f(h_rows, h_len), f(B, 1)]
outs = [torch.empty(p.shape[1], device=dev) for p in parts]
roles = [_lib.make_role(_lib.ROLE_NNCONV_SLAB_SUM64, (slabs, None, gpar), (N, D))] + \
        [_lib.make_role(_lib.ROLE_SUM_ROWS, (p, o), (p.shape[0], p.shape[1], 0)) for p, o in zip(parts, outs)]
mb = (slabs.numel() * min(256, torch.cuda.get_device_properties(dev).multi_processor_count) // 256 +
      sum(p.numel() for p in parts)) * 4 / 1e6
P = _lib.ptr
def gradh():
    _lib.call("qot_nnconv_gradh_split", P(gout), H, P(x), H, P(b.edge_attr), P(w1), P(b1), P(g.rowptr), P(g.col), P(g.eid),
              P(g.invdeg), P(bsplit), stride, None, None, P(wsh), N, H, D)
def gradh_hosted():
    _lib.host_roles(roles)
    gradh()
def sums():
    _lib.run_roles(roles)
def gradh_then_sums():
    gradh()
    sums()
forms = {"gradh": gradh, "gradh_hosted": gradh_hosted, "sums": sums, "gradh_then_sums": gradh_then_sums}
def t(fn, it=300):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    st.record()
    for _ in range(it): fn()
    en.record(); torch.cuda.synchronize()
    return st.elapsed_time(en) / it * 1e3
for _ in range(10):                    # both kernels for a while before anything is timed: the clocks settle
    for fn in forms.values():
        for _ in range(100): fn()
torch.cuda.synchronize()
# the hosted sums leave the bits of the launch of their own
sums(); torch.cuda.synchronize(); ref = [o.clone() for o in outs + [gpar]]
for o in outs + [gpar]: o.fill_(float("nan"))
gradh_hosted(); torch.cuda.synchronize()
same = all(torch.equal(a.view(torch.int32), o.view(torch.int32)) for a, o in zip(ref, outs + [gpar]))
res = {k: [] for k in forms}
for rnd in range(6):
    for k, fn in forms.items():
        res[k].append(round(t(fn), 1))
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
out = {"sums_MB": round(mb, 1), "us": res, "median": med, "hosted_bits_equal": same,
       "absorbed_us": round(med["gradh"] + med["sums"] - med["gradh_hosted"], 1),
       "saved_vs_two_launches_us": round(med["gradh_then_sums"] - med["gradh_hosted"], 1)}
print(json.dumps(out))
