"""The weight-gradient product of the H = 64 NNConv adjoint kernel (nnconv_adjoint_dw64, csrc/nnconv_mfma.hip) as
split-bf16 MFMAs: gWcat^T += U^T x from the U tile and the tile's own x rows, both split after their LDS reads.

Checked at the smallest shapes at which that loop can go wrong: the gradients of w2 / b2 / wroot stay within 2x (max) and
1.5x (RMS) of the fp32-MFMA loop's error against an fp64 restatement (QOT_NNCONV_F32_MFMA=1, same test); x.grad, whose
product stays on the fp32 MFMA, is bitwise what it is under QOT_NNCONV_F32_MFMA=1; the split path is bitwise
reproducible; and the C entry point returns x^T U as bench.py calls it.  Every test prints its figures before it
asserts (``pytest -s``)."""
import os

import pytest
import torch

from gnn_qot_estimation_amd import _lib
from gnn_qot_estimation_amd import functional as QF
from gnn_qot_estimation_amd.graph import build_graph_index

from test_gpu_nnconv_split_bf16 import _errs, _params, _run

pytestmark = pytest.mark.gpu

H = 64
WEIGHTS = ("w2", "b2", "wroot")


def _graph(case, gen):
    if case == "two_tiles":             # the second tile holds one row
        return 33, torch.randint(0, 33, (2, 40), generator=gen)
    if case == "self_loop":
        return 1, torch.zeros(2, 1, dtype=torch.int64)
    if case == "no_edges":
        return 5, torch.zeros(2, 0, dtype=torch.int64)
    if case == "hub":
        # node 3 has 40 out-edges (three 16-edge batches of the transposed walk); nodes 2, 5, 8, ... have none (their U
        # rows are zero in the K + 1 gathered blocks, inside both full tiles and the 6-row third one)
        N = 70
        srcs = torch.tensor([j for j in range(N) if j % 3 != 2])
        src = torch.cat([torch.full((40,), 3, dtype=torch.int64), srcs[torch.randint(0, len(srcs), (150,), generator=gen)]])
        return N, torch.stack([src, torch.randint(0, N, (190,), generator=gen)])
    N = 8229                            # "carry": 258 tiles, more than one per workgroup on a 256-CU part
    return N, torch.randint(0, N, (2, 3 * N), generator=gen)


def _ref64(p, ei, N, dev):
    """NNConv(aggr='mean') in fp64 with autograd (as tests/test_gpu_nnconv_split_bf16.py states it), on ``dev``."""
    t = {k: v.to(dev).double().clone().requires_grad_(k not in ("g", "ea")) for k, v in p.items()}
    src, dst = ei[0].to(dev), ei[1].to(dev)
    h = torch.relu(t["ea"] @ t["w1"].t() + t["b1"])
    We = (h @ t["w2"].t() + t["b2"]).view(-1, H, H)
    msg = torch.einsum("ea,eao->eo", t["x"][src], We)
    deg = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, dst, torch.ones(len(dst), dtype=torch.float64, device=dev))
    agg = torch.zeros(N, H, dtype=torch.float64, device=dev).index_add_(0, dst, msg) / deg.clamp(min=1)[:, None]
    out = agg + t["x"] @ t["wroot"].t() + t["bias"]
    (out * t["g"]).sum().backward()
    return {k: t[k].grad.cpu() for k in WEIGHTS}


_CASES = {}


def _case(name, D, dev, scaled=False):
    """Inputs, the fp64 gradients and both kernels' gradients of one case: computed once, shared, left unchanged."""
    key = (name, D, scaled)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(11)
        N, ei = _graph(name, gen)
        p = _params(N, ei.shape[1], D, gen)
        if scaled:
            p["x"], p["g"] = p["x"] * 2.0 ** 20, p["g"] * 2.0 ** -20
        _CASES[key] = dict(N=N, ei=ei, p=p, ref=_ref64(p, ei, N, dev), split=_run(p, ei, N, dev, True)[1],
                           f32=_run(p, ei, N, dev, False)[1])
    return _CASES[key]


def _check_rule(tag, a_split, a_f32, ref):
    es, en = _errs(a_split, ref), _errs(a_f32, ref)
    print(tag, "split", es, "fp32 MFMA", en)
    assert es["max"] <= 2.0 * en["max"] + 1e-7, (tag, es, en)
    assert es["rms"] <= 1.5 * en["rms"] + 1e-8, (tag, es, en)


SHAPES = [("two_tiles", 4), ("self_loop", 4), ("no_edges", 4), ("hub", 1), ("hub", 2), ("hub", 3), ("hub", 4), ("carry", 4)]


@pytest.mark.parametrize("name,D", SHAPES)
def test_weight_gradients_against_fp64(cuda_device, name, D):
    c = _case(name, D, cuda_device)
    for k in WEIGHTS:
        _check_rule((name, D, k), c["split"][k], c["f32"][k], c["ref"][k])


def test_weight_gradients_scaled_operands(cuda_device):
    """x scaled by 2^20 and g by 2^-20: the splits see other exponents, the products the same magnitudes."""
    c = _case("hub", 4, cuda_device, scaled=True)
    for k in WEIGHTS:
        _check_rule(("hub scaled", k), c["split"][k], c["f32"][k], c["ref"][k])


@pytest.mark.parametrize("name,D", SHAPES)
def test_grad_x_is_untouched(cuda_device, name, D):
    """The grad_x product has the same inputs and the same fp32 loop in both forms."""
    c = _case(name, D, cuda_device)
    assert torch.equal(c["split"]["x"], c["f32"]["x"])


@pytest.mark.parametrize("name,D", [("hub", 4), ("carry", 4)])
def test_split_path_is_bitwise_reproducible(cuda_device, name, D):
    c = _case(name, D, cuda_device)
    again = _run(c["p"], c["ei"], c["N"], cuda_device, True)[1]
    for k in again:
        assert torch.equal(again[k], c["split"][k]), k


def test_c_abi_returns_x_t_u(cuda_device):
    """qot_nnconv_adjoint_dw called directly: param_layout 2 (main kernel only, as bench.py's kernel table calls it), then 0,
    which returns gwcat_t[(k, o)][a] = sum_j U_j[(k, o)] x_j[a]; U restated in fp64 from the same inputs."""
    dev = cuda_device
    D, K = 4, 8
    gen = torch.Generator().manual_seed(11)
    N, ei = _graph("hub", gen)
    p = _params(N, ei.shape[1], D, gen)
    graph = build_graph_index(ei.to(dev), N)
    KT = (K + 2) * H
    x, g, ea, w1, b1 = (p[k].to(dev).contiguous() for k in ("x", "g", "ea", "w1", "b1"))
    wp = torch.randn(KT * H, generator=gen).to(dev)[QF.nnconv_perm_index(KT, dev)].contiguous()
    ws = torch.empty(_lib.load().qot_nnconv_adjoint_dw_workspace_floats(D), dtype=torch.float32, device=dev)
    gx = torch.empty(N, H, device=dev)
    P = _lib.ptr

    def call(layout, f32):
        gwt = torch.full((KT, H), float("nan"), device=dev)
        old = os.environ.get("QOT_NNCONV_F32_MFMA")
        os.environ["QOT_NNCONV_F32_MFMA"] = "1" if f32 else "0"
        try:
            _lib.call("qot_nnconv_adjoint_dw", P(g), H, P(x), H, P(ea), P(w1), P(b1), P(graph.rowptr_t), P(graph.col_t),
                      P(graph.eid_t), P(graph.invdeg), P(wp), P(gx), P(gwt), layout, P(ws), N, H, D)
            torch.cuda.synchronize()
        finally:
            if old is None:
                del os.environ["QOT_NNCONV_F32_MFMA"]
            else:
                os.environ["QOT_NNCONV_F32_MFMA"] = old
        return gwt.cpu()

    got = {}
    for f32 in (False, True):
        assert bool(call(2, f32).isnan().all())        # slabs only: gwcat_t is not written
        got[f32] = call(0, f32)
    # U_j = [ sum_{e: j->i} h_e[k] invdeg_i g_i (k < K) | sum_e invdeg_i g_i | g_j ]
    src, dst = ei[0], ei[1]
    g64, x64, invdeg = p["g"].double(), p["x"].double(), graph.invdeg.cpu().double()
    h = torch.relu(p["ea"].double() @ p["w1"].double().t() + p["b1"].double())          # [E, K]
    gi = invdeg[dst][:, None] * g64[dst]                                                # [E, 64]
    U = torch.zeros(N, K + 2, H, dtype=torch.float64)
    U[:, :K].index_add_(0, src, h[:, :, None] * gi[:, None, :])
    U[:, K].index_add_(0, src, gi)
    U[:, K + 1] = g64
    ref = U.view(N, KT).t() @ x64
    _check_rule("gwcat_t", got[False], got[True], ref)
    # and not merely as wrong as each other: an entry is a sum of at most 70 products of sums of at most 40, in fp32
    # (110 x 2^-24 = 6.6e-6 of sum |terms|, itself a few times the largest entry); a wrong row map is an error of order 1
    assert _errs(got[False], ref)["max"] <= 1e-4 and _errs(got[True], ref)["max"] <= 1e-4
