"""A/B of nnconv_mfma64 (the H = 64 forward) in its split-bf16 form (interleaved rounds in ONE process, cfg2 shape, fused
activation + dropout as the training step calls it).  A = the fp32 operand tile in LDS, split after every read
(QOT_NNCONV_FWD_SPLIT_AFTER_READ=1), B = the tile split once by the gather, bf16 planes in LDS, two K phases (default);
qot_nnconv_fused_split reads the variable on every call.  With QOT_LIB_A / QOT_LIB_B set: two builds of the library instead,
the variable left alone."""
import ctypes as C, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_qot_estimation_amd import _lib, functional as QF, synthetic as S
from gnn_qot_estimation_amd.graph import build_graph_index
ENV = "QOT_NNCONV_FWD_SPLIT_AFTER_READ"
dev = torch.device("cuda:0")
b = S.topological_batch(2, 1024, n=100, e=400).to(dev)
N, H, D, K = b.num_nodes, 64, 4, 8
g = build_graph_index(b.edge_index, N)
f = lambda *s: torch.randn(*s, device=dev)
x, w1, b1, bias = f(N, H), f(K, D), f(K), f(H)
assert QF.nnconv_split_bf16(), "the split planes are packed only without QOT_NNCONV_F32_MFMA=1"
wp, _, _, split = QF.nnconv_pack(f(H * H, K) / 16, f(H * H) / 16, f(H, H) / 8, H, K)
stride = split.numel() // 3
step = torch.zeros(1, dtype=torch.int64, device=dev)
if os.environ.get("QOT_LIB_A") or os.environ.get("QOT_LIB_B"):
    variants = {tag: (os.environ["QOT_LIB_" + tag], None) for tag in ("A", "B")}
else:
    variants = {"A": (_lib.LIB_PATH, "1"), "B": (_lib.LIB_PATH, "0")}
libs = {}
for tag, (path, after_read) in variants.items():
    lib = C.CDLL(path)
    fn = lib.qot_nnconv_fused_split
    fn.restype = C.c_int
    fn.argtypes = _lib.SIGNATURES["qot_nnconv_fused_split"][1]
    libs[tag] = (fn, torch.empty(N, H, device=dev), path, after_read)
def run(tag):
    fn, out, _, after_read = libs[tag]
    if after_read is not None: os.environ[ENV] = after_read
    rc = fn(x.data_ptr(), H, b.edge_attr.data_ptr(), w1.data_ptr(), b1.data_ptr(), g.rowptr.data_ptr(), g.col.data_ptr(),
            g.eid.data_ptr(), g.invdeg.data_ptr(), split.data_ptr(), stride, bias.data_ptr(), out.data_ptr(), N, H, D,
            1, 0.01, 0.5, 1234, step.data_ptr(), _lib.stream())
    assert rc == 0, rc
def t(tag, it=400):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    run(tag)
    st.record()
    for _ in range(it): run(tag)
    en.record(); torch.cuda.synchronize()
    return st.elapsed_time(en) / it * 1e3
for _ in range(20):                    # ~0.5 s of both forms before anything is timed: the clocks settle over the first tens of ms
    for tag in libs:
        for _ in range(200): run(tag)
torch.cuda.synchronize()
run("A"); torch.cuda.synchronize(); oa = libs["A"][1].clone()
run("B"); torch.cuda.synchronize(); ob = libs["B"][1]
# another per-wave summation order: last bits differ, the dropout masks (a hash of the element's index) do not
rel = float((oa - ob).abs().max() / oa.abs().max())
same_zeros = bool(torch.equal(oa == 0, ob == 0))
res = {"A": [], "B": []}
for rnd in range(8):
    for tag in ("A", "B"):
        res[tag].append(round(t(tag), 1))
out = {k: {"lib": libs[k][2], ENV: libs[k][3], "us": v, "min": min(v), "median": sorted(v)[len(v) // 2]} for k, v in res.items()}
out["max_rel_difference"] = rel
out["same_dropped_elements"] = same_zeros
print(json.dumps(out))
