"""The BatchNorm kernels (csrc/misc.hip: bn_partial / bn_finalize_* / bn_apply / bn_bwd_apply; the statistics' partials of
csrc/gat.hip's forward epilogue) against the fp64 restatement of tests/bn_cases.py, element by element:
``|got - ref| <= k 2^-24 A`` with the count ``k`` and the magnitude ``A`` derived there.

Every case runs through each path that can take it, against the same reference:

  dense     ``BnFn``:        qot_bn_stats, qot_bn_apply, qot_bn_bwd_reduce, qot_bn_bwd_apply
  rows      ``BnRowsFn``:    idx unique and unsorted, n in {0, 1, about N / 10, N};  training: qot_bn_apply_rows,
                             qot_bn_bwd_reduce_rows, qot_bn_bwd_apply_rows;  eval: qot_rows_scatter + qot_bn_bwd_apply
  folded    ``BnLinearFn``:  relu(bn(x)) W^T with and without the logits epilogue: z, grad_x, grad_weight, grad_bias, grad_lin
  partials  ``GatFn(bn_stats=True)`` on an edge-free graph (self loops only: out = z + bias exactly), then
            ``BnFn(partials=...)``: qot_bn_stats_from_partials, against fp64 statistics of the kernel's own ``out``

with every floating ``torch.empty`` filled with NaN for the duration, each path run twice (bitwise equal), the entry points
that ran asserted from the recorded ``_lib.call`` names and every tensor's worst ``error / bound`` printed before anything is
asserted (``pytest -s``; a record, not a threshold).  A training run is two steps on the same batch: the running statistics
are checked after the second."""
import types

import pytest
import torch

import bn_cases as BC
from helpers import TOL

pytestmark = pytest.mark.gpu

MOMENTUM, EPS = 0.1, 1e-5          # as the models pass them: Python floats, rounded to fp32 on the way into the kernels
_ENTRIES = ("qot_bn_stats", "qot_bn_stats_from_partials", "qot_bn_apply", "qot_bn_bwd_reduce", "qot_bn_bwd_apply",
            "qot_bn_apply_rows", "qot_bn_bwd_reduce_rows", "qot_bn_bwd_apply_rows", "qot_rows_scatter", "qot_gemm_nt",
            "qot_gemm_nt_logits", "qot_gemm_tn_planes", "qot_gat_fwd")


def _record(monkeypatch):
    from gnn_qot_estimation_amd import _lib
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def _nan_filled_empty(monkeypatch):
    """Every floating-point ``torch.empty`` comes back full of NaN: statistics, outputs, gradients and the partials
    workspaces are allocated that way, so an element no kernel writes stays NaN and fails the check."""
    real = torch.empty

    def empty(*a, **kw):
        t = real(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(torch, "empty", empty)


def _leaves(c, dev):
    x, w, b = (t.to(dev).requires_grad_(True) for t in (c.x, c.w, c.b))
    return x, w, b, c.rm0.clone().to(dev), c.rv0.clone().to(dev)


def _statistics(fn, c, res, rm, rv):
    """mean and rstd as the Function saved them (read before a backward frees them); the running buffers by reference."""
    saved = fn.saved_tensors
    res.update(mean=saved[2].clone(), rstd=saved[3].clone())
    if c.training:
        res.update(running_mean=rm, running_var=rv)


def _dense(c, dev):
    from gnn_qot_estimation_amd import functional as QF
    x, w, b, rm, rv = _leaves(c, dev)
    args = (w, b, rm, rv, c.training, MOMENTUM, EPS, c.relu, False, None)
    y = QF.BnFn.apply(x, *args)
    res = dict(y=y.detach())
    _statistics(y.grad_fn, c, res, rm, rv)
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], c.g.to(dev))
    res.update(grad_x=gx, grad_weight=gw, grad_bias=gb)
    for _ in range(c.steps - 1):
        with torch.no_grad():
            res["y_again"] = QF.BnFn.apply(x.detach(), *args)
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in res.items()}


def _rows(c, dev, idx):
    from gnn_qot_estimation_amd import functional as QF
    x, w, b, rm, rv = _leaves(c, dev)
    idx32 = idx.to(torch.int32).to(dev)
    args = (w, b, rm, rv, c.training, MOMENTUM, EPS, c.relu, False, None, idx32)
    y = QF.BnRowsFn.apply(x, *args)
    res = dict(y=y.detach())
    _statistics(y.grad_fn, c, res, rm, rv)
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], c.g[idx].to(dev))
    res.update(grad_x=gx, grad_weight=gw, grad_bias=gb)
    for _ in range(c.steps - 1):
        with torch.no_grad():
            res["y_again"] = QF.BnRowsFn.apply(x.detach(), *args)
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in res.items()}


def _folded(c, dev, logits):
    from gnn_qot_estimation_amd import functional as QF
    x, w, b, rm, rv = _leaves(c, dev)
    lin = c.lin.to(dev).requires_grad_(True)
    att = ()
    if logits:
        gen = torch.Generator().manual_seed(5)
        att = tuple(torch.randn(1, BC.FOLD_OUT // 128, 128, generator=gen).to(dev) for _ in range(2))
    out = QF.BnLinearFn.apply(x, w, b, rm, rv, True, MOMENTUM, EPS, False, None, lin, *att)
    z = out[0] if logits else out
    res = dict(z=z.detach())
    if logits:
        assert out[1].shape == out[2].shape == (c.N, BC.FOLD_OUT // 128) and not bool(torch.isnan(out[1]).any())
    _statistics(z.grad_fn, c, res, rm, rv)
    gx, gw, gb, gl = torch.autograd.grad(z, [x, w, b, lin], c.gz.to(dev))
    res.update(grad_x=gx, grad_weight=gw, grad_bias=gb, grad_lin=gl)
    for _ in range(c.steps - 1):
        with torch.no_grad():
            again = QF.BnLinearFn.apply(x.detach(), w, b, rm, rv, True, MOMENTUM, EPS, False, None, lin.detach(), *att)
            res["z_again"] = again[0] if logits else again
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in res.items()}


def _twice(run, calls):
    first = run()
    ran = tuple(k for k in calls if k in _ENTRIES)
    again = run()
    return first, again, ran


def _check(tag, first, again, ref, ran, want):
    """Figures first (``check_all`` prints every tensor's before it asserts), the other assertions afterwards."""
    names = [k for k in first if not k.endswith("_again")]
    BC.check_all(tag, first, ref, names, global_tol=TOL)
    assert ran == tuple(want), (ran, want)
    for k in first:
        assert torch.equal(first[k], again[k]), (k, "two runs differ")
    for k in first:
        if k.endswith("_again"):                # the second step's output: same batch, same statistics, same bits
            assert torch.equal(first[k], first[k[:-6]]), k


def _subset(ref, idx):
    """The reference of the rows form: ``y`` at the consumed rows."""
    out = dict(ref)
    out["y"] = {k: (v[idx] if v.dim() == 2 else v) for k, v in ref["y"].items()}
    return out


# ------------------------------------------------------------------ dense and rows form
@pytest.mark.parametrize("name", list(BC.CASES))
def test_dense_batchnorm_against_fp64_element_by_element(cuda_device, monkeypatch, name):
    c = BC.bn_case(name)
    ref = BC.bn_reference(name)
    calls = _record(monkeypatch)
    _nan_filled_empty(monkeypatch)
    first, again, ran = _twice(lambda: _dense(c, cuda_device), calls)
    stats = ("qot_bn_stats",) if c.training else ()
    want = stats + ("qot_bn_apply", "qot_bn_bwd_reduce", "qot_bn_bwd_apply") + (stats + ("qot_bn_apply",)) * (c.steps - 1)
    assert set(first) == set(BC.CHECKED) - (set() if c.training else {"running_mean", "running_var"}) | {"y_again"}
    _check(f"{name} dense", first, again, ref, ran, want)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_rows_form_against_fp64_element_by_element(cuda_device, monkeypatch, name):
    c = BC.bn_case(name)
    calls = _record(monkeypatch)
    _nan_filled_empty(monkeypatch)
    for n in BC.rows_counts(c.N):
        ref = BC.bn_reference(name, n)
        idx = ref["idx"]
        assert idx.numel() == n == idx.unique().numel() and (n < 3 or not torch.equal(idx, idx.sort().values))
        calls.clear()
        first, again, ran = _twice(lambda: _rows(c, cuda_device, idx), calls)
        stats = ("qot_bn_stats",) if c.training else ()
        fwd = stats + (("qot_bn_apply_rows",) if n else ())
        bwd = ("qot_bn_bwd_reduce_rows",) if n else ()
        if c.training:
            bwd += ("qot_bn_bwd_apply_rows",)
        else:
            bwd += (("qot_rows_scatter",) if n else ()) + ("qot_bn_bwd_apply",)
        assert first["y"].shape == (n, c.C) and first["grad_x"].shape == (c.N, c.C)
        _check(f"{name} rows n={n}", first, again, _subset(ref, idx), ran, fwd + bwd + fwd * (c.steps - 1))


# ------------------------------------------------------------------ folded into the next projection
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("name", list(BC.FOLD_CASES))
def test_folded_batchnorm_against_fp64_element_by_element(cuda_device, monkeypatch, name, logits):
    c = BC.bn_case(name)
    ref = BC.bn_reference(name)
    for k in ("QOT_LIBRARY_GEMM", "QOT_NO_FUSED_LOGITS"):
        monkeypatch.delenv(k, raising=False)
    calls = _record(monkeypatch)
    _nan_filled_empty(monkeypatch)
    first, again, ran = _twice(lambda: _folded(c, cuda_device, logits), calls)
    fwd = ("qot_bn_stats", "qot_gemm_nt_logits" if logits else "qot_gemm_nt")
    want = fwd + ("qot_gemm_nt", "qot_gemm_tn_planes", "qot_bn_bwd_reduce", "qot_bn_bwd_apply") + fwd * (c.steps - 1)
    assert set(first) == set(BC.FOLD_CHECKED) | {"z_again"}
    _check(f"{name} folded{' + logits' if logits else ''}", first, again, ref, ran, want)


# ------------------------------------------------------------------ statistics from the GATConv epilogue's partials
def _edge_free_graph(N, dev):
    from gnn_qot_estimation_amd.graph import build_graph_index
    graph = build_graph_index(torch.zeros(2, 0, dtype=torch.long, device=dev), N, gat_self_loops=True)
    ar = torch.arange(N + 1, dtype=torch.int32, device=dev)
    assert graph.cap == N and torch.equal(graph.rowptr, ar) and torch.equal(graph.col[:N], ar[:N])
    return graph


def _partials_sizes(HC):
    """small; one more than a resident round; at heads * C = 16 also the size that gives every lane group three rows."""
    from gnn_qot_estimation_amd import _lib
    lib = _lib.load()
    rpb = BC.gat_lanes(HC)[1]
    cap = lib.qot_gat_blocks(1 << 24, 4, HC // 4)
    assert 0 < cap <= 2048
    sizes = {"small": 37, "round": cap * rpb + 1}
    if HC == 16:
        sizes["runs"] = 2 * cap * rpb + 1
    return sizes


# (the small size has fewer than 1000 rows: no outlier row; three rows per lane group are pinned at heads * C = 16)
@pytest.mark.parametrize("HC,size,family", [(HC, size, family) for HC in BC.GAT_WIDTHS for size in ("small", "round", "runs")
                                            for family in ("ordinary", "offset", "outlier")
                                            if (size != "runs" or HC == 16) and (size != "small" or family != "outlier")])
def test_statistics_from_gat_partials_against_fp64(cuda_device, monkeypatch, HC, size, family):
    from gnn_qot_estimation_amd import _lib, functional as QF
    N, dev, lib = _partials_sizes(HC)[size], cuda_device, _lib.load()
    nblk, chunk = lib.qot_gat_blocks(N, 4, HC // 4), lib.qot_gat_chunk_rows(N, 4, HC // 4)
    run, ks, k_merge = BC.gat_chain(N, HC, nblk)
    rpb = BC.gat_lanes(HC)[1]
    assert chunk == run * rpb and run == {"small": 1, "round": 2, "runs": 3}[size], (N, nblk, chunk, run)
    z = BC.partials_input(N, HC, family).to(dev)
    gen = torch.Generator().manual_seed(HC)
    att = [torch.randn(1, 4, HC // 4, generator=gen).to(dev) for _ in range(2)]
    bias = (torch.randn(HC, generator=gen) * 0.5).to(dev)
    w, b = torch.ones(HC, device=dev), torch.zeros(HC, device=dev)
    rm0, rv0 = torch.randn(HC, generator=gen) * 0.5, 0.5 + torch.rand(HC, generator=gen)
    graph = _edge_free_graph(N, dev)
    calls = _record(monkeypatch)
    _nan_filled_empty(monkeypatch)
    steps = 2

    def once():
        out, part = QF.GatFn.apply(z, att[0], att[1], bias, graph, 0.2, True)
        rm, rv = rm0.clone().to(dev), rv0.clone().to(dev)
        res = {}
        for _ in range(steps):
            y = QF.BnFn.apply(out.detach().requires_grad_(True), w, b, rm, rv, True, MOMENTUM, EPS, False, False, (part, bias))
        saved = y.grad_fn.saved_tensors
        res.update(out=out, mean=saved[2], rstd=saved[3], running_mean=rm, running_var=rv)
        torch.cuda.synchronize()
        return {k: v.detach().cpu() for k, v in res.items()}
    first, again, ran = _twice(once, calls)
    assert torch.equal(first["out"], (z + bias).cpu())                  # self loops only: softmax weight 1, out = z + bias
    ref = BC.stats_reference(first.pop("out").double(), ks, k_merge, rm0, rv0, steps)
    again.pop("out")
    want = ("qot_gat_fwd",) + ("qot_bn_stats_from_partials", "qot_bn_apply") * steps
    _check(f"partials hc={HC} n={N} run={run} {family}", first, again, ref, ran, want)


# ------------------------------------------------------------------ column isolation, refusals
def test_a_nan_and_an_inf_stay_in_their_columns(cuda_device, monkeypatch):
    """One NaN in column 1 and one +Inf in column 6 of ``x``: every other column of every output is bitwise what the clean
    run gave (statistics, running statistics, output, all three gradients)."""
    c = BC.bn_case("n129_c20_train_lin")
    dirty = types.SimpleNamespace(**vars(c))
    dirty.x = c.x.clone()
    dirty.x[5, 1] = float("nan")
    dirty.x[77, 6] = float("inf")
    _nan_filled_empty(monkeypatch)
    a, b = _dense(c, cuda_device), _dense(dirty, cuda_device)
    keep = torch.tensor([j not in (1, 6) for j in range(c.C)])
    for k in a:
        assert torch.equal(a[k][..., keep], b[k][..., keep]), k
        assert not bool(torch.isnan(a[k]).any())
    assert bool(torch.isnan(b["mean"][1])) and not bool(torch.isfinite(b["mean"][6]))


@pytest.mark.parametrize("C", [1028, 6])
@pytest.mark.parametrize("training", [True, False])
def test_unsupported_widths_are_refused(cuda_device, C, training):
    """More than 1024 columns, or a width that is no multiple of 4: the package's error, no launch."""
    from gnn_qot_estimation_amd import _lib, functional as QF
    dev = cuda_device
    x = torch.randn(8, C, device=dev, requires_grad=True)
    w, b, rm, rv = torch.ones(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.ones(C, device=dev)
    if training or C == 6:
        with pytest.raises(_lib.QotError):
            QF.BnFn.apply(x, w, b, rm, rv, training, MOMENTUM, EPS, True, False, None)
    else:           # eval mode reduces nothing in the forward: the backward's column sums refuse
        y = QF.BnFn.apply(x, w, b, rm, rv, False, MOMENTUM, EPS, True, False, None)
        with pytest.raises(_lib.QotError):
            y.sum().backward()
    assert bool((rm == 0).all()) and bool((rv == 1).all())
