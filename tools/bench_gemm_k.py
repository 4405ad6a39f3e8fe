"""qot_gemm_nt against the library over the inner dimension K at a fixed flop count (N = 512): separates the per-tile costs
(prologue, epilogue: once per 128 x 128 output tile whatever K) from the per-stage costs of the main loop."""
import os, sys, json
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_qot_estimation_amd import _lib


def timeit(fn, it=10, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it): fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / it


dev = torch.device("cuda")
N = 512
for K in (128, 256, 512, 1024, 2048, 4096):
    M = 707008 * 512 // K // 128 * 128
    x, w = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev)
    z = torch.empty(M, N, device=dev)
    s, t = torch.rand(K, device=dev) + 0.5, torch.randn(K, device=dev)
    fl = 2.0 * M * N * K
    lib = timeit(lambda: torch.mm(x, w.t(), out=z))
    ours = timeit(lambda: _lib.call("qot_gemm_nt", x, K, w, K, z, N, M, N, K, None, None, None))
    aff = timeit(lambda: _lib.call("qot_gemm_nt", x, K, w, K, z, N, M, N, K, s, t, None))
    print(json.dumps({"K": K, "M": M, "lib_tf": round(fl / lib / 1e9, 1), "nt_tf": round(fl / ours / 1e9, 1),
                      "nt_affine_tf": round(fl / aff / 1e9, 1)}))
    del x, z
