"""Numerics of the split-bf16 form of the H = 64 NNConv kernels (csrc/split_bf16.hpp): every fp32 product as six bf16
cross products of three-way splits.  The split planes must reconstruct the weights exactly; the forward output and the
gradients of x, the edge MLP (through grad-h) and the output-layer weights must stay as close to an fp64 restatement as
the fp32-MFMA kernels (QOT_NNCONV_F32_MFMA=1) are; the split path must be bitwise reproducible."""
import os

import pytest
import torch

from gnn_qot_estimation_amd import _lib
from gnn_qot_estimation_amd import functional as QF
from gnn_qot_estimation_amd.graph import build_graph_index

pytestmark = pytest.mark.gpu

H = 64


def _graph(case, gen):
    if case == "cfg2":                  # 64 graphs of 100 nodes / 400 edges, block-diagonal
        n, e, B = 100, 400, 64
        src = torch.randint(0, n, (B, e), generator=gen) + (torch.arange(B) * n)[:, None]
        dst = torch.randint(0, n, (B, e), generator=gen) + (torch.arange(B) * n)[:, None]
        return n * B, torch.stack([src.reshape(-1), dst.reshape(-1)])
    if case == "powerlaw":              # in-degrees ~ rank^-1.2 (a few hubs with hundreds of in-edges)
        N, E = 3000, 12000
        p = (torch.arange(N, dtype=torch.float64) + 1) ** -1.2
        dst = torch.multinomial(p, E, replacement=True, generator=gen)
        return N, torch.stack([torch.randint(0, N, (E,), generator=gen), dst])
    if case == "isolated":              # the upper half of the nodes has no edges at all
        N = 1000
        return N, torch.randint(0, N // 2, (2, 2500), generator=gen)
    N = 1000 + 13                       # "ragged": a node count that is not a multiple of 32
    return N, torch.randint(0, N, (2, 4 * N), generator=gen)


def _params(N, E, D, gen):
    K = 2 * D
    return dict(x=torch.randn(N, H, generator=gen), ea=torch.rand(E, D, generator=gen),
                w1=torch.randn(K, D, generator=gen) * 0.5, b1=torch.randn(K, generator=gen) * 0.5,
                w2=torch.randn(H * H, K, generator=gen) / 16, b2=torch.randn(H * H, generator=gen) / 16,
                wroot=torch.randn(H, H, generator=gen) / 8, bias=torch.randn(H, generator=gen),
                g=torch.randn(N, H, generator=gen))


def _ref64(p, ei, N):
    """NNConv(aggr='mean') in fp64 with autograd: out_i = mean_{j->i} x_j W(e) + W_root x_i + bias."""
    t = {k: v.double().clone().requires_grad_(k not in ("g", "ea")) for k, v in p.items()}
    src, dst = ei[0], ei[1]
    h = torch.relu(t["ea"] @ t["w1"].t() + t["b1"])                          # [E, K]
    We = (h @ t["w2"].t() + t["b2"]).view(-1, H, H)                            # [E, a, o]
    msg = torch.einsum("ea,eao->eo", t["x"][src], We)
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, dst, torch.ones(len(dst), dtype=torch.float64))
    agg = torch.zeros(N, H, dtype=torch.float64).index_add_(0, dst, msg) / deg.clamp(min=1)[:, None]
    out = agg + t["x"] @ t["wroot"].t() + t["bias"]
    (out * t["g"]).sum().backward()
    grads = {k: t[k].grad for k in ("x", "w1", "b1", "w2", "b2", "wroot")}
    # per-element scale of the forward: the same sums over |operands|
    ha = h.detach()
    Wa = (ha @ t["w2"].detach().abs().t() + t["b2"].detach().abs()).view(-1, H, H)
    msga = torch.einsum("ea,eao->eo", t["x"].detach().abs()[src], Wa)
    agga = torch.zeros(N, H, dtype=torch.float64).index_add_(0, dst, msga) / deg.clamp(min=1)[:, None]
    scale = agga + t["x"].detach().abs() @ t["wroot"].detach().abs().t() + t["bias"].detach().abs()
    return out.detach(), grads, scale


def _run(p, ei, N, dev, split):
    old = os.environ.get("QOT_NNCONV_F32_MFMA")
    os.environ["QOT_NNCONV_F32_MFMA"] = "0" if split else "1"
    try:
        t = {k: v.to(dev).clone().requires_grad_(k not in ("g", "ea")) for k, v in p.items()}
        graph = build_graph_index(ei.to(dev), N)
        out = QF.NNConvFn.apply(t["x"], t["ea"], t["w1"], t["b1"], t["w2"], t["b2"], t["wroot"], t["bias"], graph)
        out.backward(t["g"])
        torch.cuda.synchronize()
        return out.detach().cpu(), {k: t[k].grad.cpu() for k in ("x", "w1", "b1", "w2", "b2", "wroot")}
    finally:
        if old is None:
            del os.environ["QOT_NNCONV_F32_MFMA"]
        else:
            os.environ["QOT_NNCONV_F32_MFMA"] = old


def _errs(a, ref, scale=None):
    d = (a.double() - ref).abs()
    m = float(ref.abs().max()) or 1.0
    e = {"max": float(d.max()) / m, "rms": float(d.pow(2).mean().sqrt()) / m}
    if scale is not None:
        e["elem"] = float((d / scale.clamp(min=1e-30)).max())
    return e


def test_split3_planes_reconstruct_exactly(cuda_device):
    """The gather role's split part: hi + mid + lo == x exactly (in fp64) across exponents, signs and magnitudes."""
    dev = cuda_device
    gen = torch.Generator().manual_seed(1)
    n = 1 << 16
    mant = torch.rand(n, generator=gen) + 1.0
    expo = torch.randint(-100, 100, (n,), generator=gen).double()
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    x = (sign * mant * torch.pow(2.0, expo)).float()
    x[:8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1.0e-30, 65504.0])
    xd = x.to(dev)
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    out = torch.empty(n, device=dev)
    planes = torch.empty(3 * n, dtype=torch.int16, device=dev)
    _lib.run_roles([_lib.make_role(_lib.ROLE_GATHER3, [xd, xd, xd, idx, out, idx, planes], [n, 0, n, n])])
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), x)
    bits = planes.cpu().view(3, n).to(torch.int32) & 0xFFFF
    parts = (bits << 16).view(torch.float32).double()
    recon = parts[0] + parts[1] + parts[2]
    assert torch.equal(recon, x.double())
    # hi is x rounded to nearest bf16, and the parts shrink by at least 2^8 each
    assert torch.equal(parts[0].float(), x.bfloat16().float())
    nz = parts[1] != 0
    assert bool((parts[1][nz].abs() <= parts[0][nz].abs() * 2.0 ** -8).all())


@pytest.mark.parametrize("case", ["cfg2", "powerlaw", "isolated", "ragged"])
def test_split_products_against_fp64(cuda_device, case):
    """Forward output and every gradient of the fused H = 64 NNConv: split-bf16 error <= 2x (max) and <= 1.5x (RMS) the
    fp32-MFMA kernels' error against fp64; the forward also per element relative to sum |a| |b|."""
    gen = torch.Generator().manual_seed(7)
    N, ei = _graph(case, gen)
    p = _params(N, ei.shape[1], 4, gen)
    ref_out, ref_g, scale = _ref64(p, ei, N)
    out_s, g_s = _run(p, ei, N, cuda_device, True)
    out_n, g_n = _run(p, ei, N, cuda_device, False)
    checks = [("out", out_s, out_n, ref_out, scale)] + [(k, g_s[k], g_n[k], ref_g[k], None) for k in ref_g]
    for name, a_s, a_n, ref, sc in checks:
        es, en = _errs(a_s, ref, sc), _errs(a_n, ref, sc)
        assert es["max"] <= 2.0 * en["max"] + 1e-7, (case, name, es, en)
        assert es["rms"] <= 1.5 * en["rms"] + 1e-8, (case, name, es, en)
        if sc is not None:
            assert es["elem"] <= 2.0 * en["elem"] + 1e-7, (case, name, es, en)
        assert es["max"] <= 1e-5, (case, name, es)


def test_split_path_is_bitwise_reproducible(cuda_device):
    gen = torch.Generator().manual_seed(3)
    N, ei = _graph("powerlaw", gen)
    p = _params(N, ei.shape[1], 4, gen)
    o1, g1 = _run(p, ei, N, cuda_device, True)
    o2, g2 = _run(p, ei, N, cuda_device, True)
    assert torch.equal(o1, o2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
