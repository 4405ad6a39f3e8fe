"""The operand tile of the split-bf16 NNConv forward at H = 64 (nnconv_mfma64, csrc/nnconv_mfma.hip) written to LDS as bf16
planes, every value split once by the gather thread that holds it, and published in two equal K phases (the default form;
QOT_NNCONV_FWD_SPLIT_AFTER_READ=1 launches the earlier loop: the fp32 image, split after every read by both column-half
waves).

The per-step products are the same in both forms, but a wave now sums other steps, so the outputs differ in the last bits.
Both split forms are therefore held to ONE yardstick: against an fp64 restatement of ``out = bias + A @ Wcat`` the max error
is at most 2x and the RMS error at most 1.5x that of the fp32-MFMA kernel (``qot_nnconv_fused``) on the same inputs (errors
relative to max |reference|, by the rule of tests/test_gpu_nnconv_split_bf16.py as it stands there, absolute terms of one
fp32 rounding included; measured without them, one few-row case misses the bare factor: five rows without edges at D = 3,
max 1.84e-7 against 2 x 0.87e-7, RMS 3.1e-8 against 1.5 x 2.6e-8 -- only the root block is non-zero there and one wave
now sums all four of its steps where two waves summed two each).  Every output buffer is NaN-filled
first, every call is made twice and must repeat bit for bit; a row's result must not depend on its position in the tile
or on the tile's workgroup.  The kernels are called directly on a CSR built here (stable in the edge order, so that a
relabelled graph keeps every row's summation order), and once through ``NNConvFn``."""
import os

import pytest
import torch

from gnn_qot_estimation_amd import _lib
from gnn_qot_estimation_amd import functional as QF
from gnn_qot_estimation_amd.graph import build_graph_index

pytestmark = pytest.mark.gpu

H = 64
ENV = "QOT_NNCONV_FWD_SPLIT_AFTER_READ"
F32 = "QOT_NNCONV_F32_MFMA"


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _edges(case, gen):
    """(N, edge_index [2, E] = (source, destination))."""
    if case == "one_node":
        return 1, torch.zeros(2, 1, dtype=torch.int64)
    if case == "two_tiles":             # the second tile holds one row: 31 rows of absent nodes
        return 33, torch.randint(0, 33, (2, 120), generator=gen)
    if case == "no_edges":
        return 5, torch.zeros(2, 0, dtype=torch.int64)
    if case == "hub":
        # 70 nodes: nodes 2, 5, 8, ... have no in-edges, node 7 has 43 (six gather batches of 8) next to rows of 0..8
        N = 70
        dsts = torch.tensor([j for j in range(N) if j % 3 != 2 and j != 7])
        dst = torch.cat([dsts[torch.randint(0, len(dsts), (200,), generator=gen)], torch.full((43,), 7)])
        return N, torch.stack([torch.randint(0, N, (243,), generator=gen), dst])
    assert case == "carry"              # 1125 tiles: more than the two workgroups per CU of a 304-CU part (608)
    N = 36000
    dst = torch.arange(N).repeat(2)
    return N, torch.stack([torch.randint(0, N, (2 * N,), generator=gen), dst])


def _csr(N, ei, dev):
    """CSR over the destinations, edges of a row in their order in ``ei`` (stable sort)."""
    dst = ei[1]
    order = torch.sort(dst, stable=True)[1]
    deg = torch.bincount(dst, minlength=N)
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = deg.cumsum(0)
    pad = torch.zeros(1, dtype=torch.int64)
    col, eid = torch.cat([ei[0][order], pad]), torch.cat([order, pad])          # (never empty: the kernels take pointers)
    invdeg = 1.0 / deg.clamp(min=1).float()
    return dict(rowptr=rowptr.int().to(dev), col=col.int().to(dev), eid=eid.int().to(dev), invdeg=invdeg.to(dev))


def _inputs(N, E, D, gen, scale=1.0):
    """x and the weights (the three of Wcat) times ``scale``; the bias times scale^2, the size of the products."""
    K = 2 * D
    return dict(x=torch.randn(N, H, generator=gen) * scale, ea=torch.rand(max(E, 1), D, generator=gen),
                w1=torch.randn(K, D, generator=gen) * 0.5, b1=torch.randn(K, generator=gen) * 0.5,
                w2=torch.randn(H * H, K, generator=gen) / 16 * scale, b2=torch.randn(H * H, generator=gen) / 16 * scale,
                wroot=torch.randn(H, H, generator=gen) / 8 * scale, bias=torch.randn(H, generator=gen) * scale * scale)


def _ref64(t, ei, N, csr):
    """out = bias + A @ Wcat in fp64 on the device, A_i = [1/deg_i sum_e h_e[k] x_j (k < K) | 1/deg_i sum_e x_j | x_i]; the
    mean scale is the fp32 1/deg all kernels read."""
    d = {k: v.double() for k, v in t.items()}
    K = d["w1"].shape[0]
    src, dst = ei[0].to(d["x"].device), ei[1].to(d["x"].device)
    E = ei.shape[1]
    h = torch.relu(d["ea"][:E] @ d["w1"].t() + d["b1"])                              # [E, K]
    xs = d["x"][src]                                                               # [E, H]
    blocks = torch.cat([h[:, :, None] * xs[:, None, :], xs[:, None, :]], 1)        # [E, K + 1, H]
    A = torch.zeros(N, K + 1, H, dtype=torch.float64, device=xs.device).index_add_(0, dst, blocks)
    A = A * csr["invdeg"].double()[:, None, None]
    A = torch.cat([A.reshape(N, -1), d["x"]], 1)                                   # [N, (K + 2) H]
    wcat = torch.cat([d["w2"].view(H, H, K).permute(2, 0, 1).reshape(K * H, H), d["b2"].view(H, H), d["wroot"].t()], 0)
    return d["bias"] + A @ wcat


def _pack(t, K):
    with _Env(**{F32: "0"}):             # nnconv_pack writes the planes only for the split form
        wp, _, _, split = QF.nnconv_pack(t["w2"], t["b2"], t["wroot"], H, K)
    torch.cuda.synchronize()
    return wp, split


def _call(form, t, csr, wp, split, N, D, act=None):
    """One forward into a NaN-filled buffer: "presplit" (default), "after_read" or "f32" (the fp32-MFMA kernel)."""
    out = torch.full((N, H), float("nan"), device=t["x"].device)
    P = _lib.ptr
    head = (P(t["x"]), H, P(t["ea"]), P(t["w1"]), P(t["b1"]), P(csr["rowptr"]), P(csr["col"]), P(csr["eid"]),
            P(csr["invdeg"]))
    tail = (P(t["bias"]), P(out), N, H, D) + tuple(QF._act_args(act))
    if form == "f32":
        _lib.call("qot_nnconv_fused", *head, 0, P(wp), *tail)
    else:
        with _Env(**{ENV: "1" if form == "after_read" else "0"}):       # read by the entry point on every call
            _lib.call("qot_nnconv_fused_split", *head, P(split), split.numel() // 3, *tail)
    torch.cuda.synchronize()
    return out


def _errs(a, ref):
    d = (a.double() - ref).abs()
    m = float(ref.abs().max()) or 1.0
    return {"max": float(d.max()) / m, "rms": float(d.pow(2).mean().sqrt()) / m}


def _bits(a):
    return a.view(torch.int32)


def _check_forms(outs, ref, tag, keep=None):
    """The yardstick, for both split forms; ``keep``: the elements compared (all)."""
    sel = (lambda a: a) if keep is None else (lambda a: a[keep])
    en = _errs(sel(outs["f32"]), sel(ref))
    for form in ("presplit", "after_read"):
        es = _errs(sel(outs[form]), sel(ref))
        print(tag, form, es, "f32", en)
        assert not bool(outs[form].isnan().any()), (tag, form)            # every element written
        # the rule of tests/test_gpu_nnconv_split_bf16.py as it stands there: the absolute terms are one fp32 rounding at the
        # largest output (2^-23 = 1.2e-7 of max |reference|) and a tenth of it for the RMS -- the errors of these few-row
        # cases are a handful of such roundings, and a ratio of two of them is quantised more coarsely than the factor
        assert es["max"] <= 2.0 * en["max"] + 1e-7, (tag, form, es, en)
        assert es["rms"] <= 1.5 * en["rms"] + 1e-8, (tag, form, es, en)


_CASES = {}


def _case(name, D, dev, scale=1.0):
    """Inputs, reference and the outputs of the three forms (the split ones twice): computed once, shared, left unchanged."""
    key = (name, D, scale)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(31)
        N, ei = _edges(name, gen)
        t = {k: v.to(dev) for k, v in _inputs(N, ei.shape[1], D, gen, scale).items()}
        csr = _csr(N, ei, dev)
        wp, split = _pack(t, 2 * D)
        outs = {f: _call(f, t, csr, wp, split, N, D) for f in ("presplit", "after_read", "f32")}
        again = {f: _call(f, t, csr, wp, split, N, D) for f in ("presplit", "after_read")}
        _CASES[key] = dict(N=N, outs=outs, again=again, ref=_ref64(t, ei, N, csr))
    return _CASES[key]


def _check_case(c, tag):
    for f, a in c["again"].items():
        assert torch.equal(_bits(a), _bits(c["outs"][f])), (tag, f)
    _check_forms(c["outs"], c["ref"], tag)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["one_node", "two_tiles", "no_edges", "hub", "carry"])
def test_presplit_against_fp64(cuda_device, name, D):
    _check_case(_case(name, D, cuda_device), (name, D))


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("scale", [2.0 ** -20, 2.0 ** 20])
def test_presplit_scaled_operands(cuda_device, scale, D):
    """x and the weights scaled by 2^-20 and 2^20: the splits see other exponents."""
    _check_case(_case("hub", D, cuda_device, scale), ("hub", D, scale))


def test_hub_case_is_what_its_comment_says():
    _, ei = _edges("hub", torch.Generator().manual_seed(31))
    deg = torch.bincount(ei[1], minlength=70)
    assert int(deg[7]) == 43 and not bool(deg[2::3].any()) and int((deg > 0).sum()) > 30


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_rows_do_not_depend_on_tile_or_workgroup(cuda_device, D):
    """The same 32 rows with their in-edges as tile 0 and as tile 5 (another workgroup) of a 7-tile batch: equal bit for bit."""
    dev = cuda_device
    gen = torch.Generator().manual_seed(5)
    nb, nf, N = 32, 170, 202
    blk = torch.stack([torch.randint(0, nb, (150,), generator=gen),
                       torch.cat([torch.randint(0, nb, (130,), generator=gen), torch.full((20,), 9)])])
    fill = torch.randint(0, nf, (2, 500), generator=gen)
    tb = _inputs(nb, 150, D, gen)
    tf = _inputs(nf, 500, D, gen)
    got = {}
    for at in (0, 160):                                     # the block's first node; fillers take the other numbers
        fmap = torch.cat([torch.arange(0, at), torch.arange(at + nb, N)])
        ei = torch.cat([blk + at, fmap[fill]], 1)
        t = {k: v.to(dev) for k, v in tb.items()}
        x = torch.empty(N, H)
        x[at:at + nb], x[fmap] = tb["x"], tf["x"]
        t["x"], t["ea"] = x.to(dev), torch.cat([tb["ea"], tf["ea"]]).to(dev)
        csr = _csr(N, ei, dev)
        wp, split = _pack(t, 2 * D)
        for f in ("presplit", "after_read"):
            got[f, at] = _call(f, t, csr, wp, split, N, D)[at:at + nb].cpu()
    for f in ("presplit", "after_read"):
        assert not bool(got[f, 0].isnan().any())
        assert torch.equal(_bits(got[f, 0]), _bits(got[f, 160])), (f, D)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_rows_do_not_depend_on_tile_row(cuda_device, D):
    """Nodes 0 and 31 of a one-tile graph exchanged (a row moves from tile row 0 to row 31, another one back): every row
    equal bit for bit to what it was under its old number."""
    dev = cuda_device
    gen = torch.Generator().manual_seed(6)
    N = 32
    ei = torch.randint(0, N, (2, 140), generator=gen)
    t0 = _inputs(N, 140, D, gen)
    perm = torch.arange(N)
    perm[0], perm[31] = 31, 0                               # its own inverse
    got = {}
    for moved in (False, True):
        t = {k: v.to(dev) for k, v in t0.items()}
        e = perm[ei] if moved else ei
        if moved:
            t["x"] = t0["x"][perm].to(dev)
        csr = _csr(N, e, dev)
        wp, split = _pack(t, 2 * D)
        for f in ("presplit", "after_read"):
            o = _call(f, t, csr, wp, split, N, D).cpu()
            got[f, moved] = o[perm] if moved else o
    for f in ("presplit", "after_read"):
        assert not bool(got[f, False].isnan().any())
        assert torch.equal(_bits(got[f, False]), _bits(got[f, True])), (f, D)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_fused_activation_and_dropout(cuda_device, D):
    """leaky_relu(0.01) + dropout(0.5) in the epilogue, fixed seed and step: the zeroed elements are the split-after-read
    form's exactly, the kept ones meet the yardstick against 2 leaky_relu(reference)."""
    dev = cuda_device
    gen = torch.Generator().manual_seed(9)
    N, ei = _edges("hub", gen)
    t = {k: v.to(dev) for k, v in _inputs(N, ei.shape[1], D, gen).items()}
    csr = _csr(N, ei, dev)
    wp, split = _pack(t, 2 * D)
    step = torch.tensor([3], dtype=torch.int64, device=dev)
    act = (0.01, 0.5, 1234, step)
    outs = {f: _call(f, t, csr, wp, split, N, D, act) for f in ("presplit", "after_read", "f32")}
    for f in ("presplit", "after_read"):
        assert torch.equal(_bits(_call(f, t, csr, wp, split, N, D, act)), _bits(outs[f])), f
    zero = outs["after_read"] == 0
    assert torch.equal(outs["presplit"] == 0, zero)
    assert torch.equal(outs["f32"] == 0, zero)              # (the mask is a hash of the element's index)
    assert 0.4 < float(zero.float().mean()) < 0.6
    pre = _ref64(t, ei, N, csr)
    ref = torch.where(pre > 0, pre, 0.01 * pre) * 2.0
    _check_forms(outs, ref, ("dropout", D), keep=~zero)


def test_module_path(cuda_device):
    """Through NNConvFn on the library's own graph index: the default form repeats bit for bit and meets the yardstick."""
    dev = cuda_device
    gen = torch.Generator().manual_seed(11)
    N, ei = _edges("hub", gen)
    D = 4
    t = {k: v.to(dev) for k, v in _inputs(N, ei.shape[1], D, gen).items()}
    graph = build_graph_index(ei.to(dev), N)

    def run(**env):
        with _Env(**env):
            o = QF.NNConvFn.apply(t["x"], t["ea"], t["w1"], t["b1"], t["w2"], t["b2"], t["wroot"], t["bias"], graph)
            torch.cuda.synchronize()
        return o.detach()
    outs = {"presplit": run(**{F32: "0", ENV: "0"}), "after_read": run(**{F32: "0", ENV: "1"}), "f32": run(**{F32: "1"})}
    assert torch.equal(_bits(run(**{F32: "0", ENV: "0"})), _bits(outs["presplit"]))
    assert not torch.equal(_bits(outs["f32"]), _bits(outs["presplit"]))      # (three kernels, not one)
    csr = dict(invdeg=graph.invdeg)
    _check_forms(outs, _ref64(t, ei, N, csr), "module")
