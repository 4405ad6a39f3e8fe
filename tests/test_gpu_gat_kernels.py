"""Every GATConv kernel of csrc/gat.hip (``gat_logits_kernel``, the forward walk, the two backward walks, ``gat_att_grad``;
dense and thin instantiations) against the fp64 restatement of tests/gat_cases.py, element by element: ``|got - ref| <=
k 2^-24 A`` with the count ``k`` and the magnitude ``A`` derived there.

Each kernel is checked at its own stage: ``QF.GatFn.apply(z, ..., a_src=, a_dst=)`` and ``QF.GatThinFn.apply(x, W, ...)`` are
called directly with drawn fp32 inputs on an index whose CSR order is asserted to be the host's; the thin form's
reference is taken from the logits the kernels themselves used (``logits_sink``), which are checked against ``x (W^T att)``
with a bound of their own.  Checked per element: ``out``, ``stats`` (``m`` bit for bit, ``denom``), ``grad_z`` or
``grad_lin``, ``grad_att_src``, ``grad_att_dst``, ``grad_bias``.  Exact: isolated destinations, destinations whose only
in-edge is their self loop.

The entry points that ran are asserted from the recorded ``_lib.call`` names; every floating ``torch.empty`` is filled with
NaN for the duration; each (case, form) runs twice (bitwise equal); every tensor's worst ``error / bound`` is printed
before anything is asserted (``pytest -s``; a record, not a threshold).  The walk cases take their row count from the
device, so that every lane group walks at least three destinations whatever occupancy the kernels get.

On record (MI355X, 256 CUs): the forward's grid cap ``min(occupancy, 8) x CUs`` is 4 workgroups per CU at C = 4, 8, 16, 32
and 128, 7 at C = 64 and 3 at C = 256 (1024, 1792 and 768 workgroups); the walk cases then give 7 destinations per lane
group (4 at C = 64, 9 at C = 256).  The slowest case is the C = 256 walk: about 0.1 s for both runs of the kernels and 3 s
for its fp64 reference.  Every case passed; the worst ``error / bound`` per width (``m`` is bitwise everywhere; ``logits``: the
logit kernel, ``thin a``: the thin form's logits):

    C     out    denom  grad_z  grad_lin  grad_att_src  grad_att_dst  grad_bias  logits  thin a
    4     0.076  0.067  0.089   0.012     0.003         0.006         0.037      0.296   0.127
    8     0.072  0.059  0.112   0.015     0.004         0.006         0.052      0.317   0.065
    16    0.071  0.076  0.085   0.026     0.006         0.003         0.088      0.210   0.040
    32    0.077  0.080  0.075   0.014     0.004         0.001         0.084      0.108   0.026
    64    0.088  0.078  0.061   0.014     0.003         0.001         0.050      0.065   0.012
    128   0.081  0.061  0.092   0.033     0.001         0.001         0.062      0.056   0.006
    256   0.082  0.058  0.088   0.018     0.002         0.001         0.081      0.036   0.002
"""
import time

import pytest
import torch

import gat_cases as G
from helpers import TOL

pytestmark = pytest.mark.gpu

WANT = {"dense": ("qot_gat_fwd", "qot_gat_bwd_dst", "qot_gat_bwd_src", "qot_gat_att_grad"),
        "thin": ("qot_gat_fwd_thin", "qot_gat_bwd_dst_thin", "qot_gat_bwd_src")}
_RUNS = {}
EPS = torch.tensor(1e-16, dtype=torch.float32)


def _record(monkeypatch):
    from gnn_qot_estimation_amd import _lib
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def _nan_filled_empty(monkeypatch):
    """Every floating-point ``torch.empty`` comes back full of NaN: an element no kernel writes stays NaN and fails."""
    real = torch.empty

    def empty(*a, **kw):
        t = real(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(torch, "empty", empty)


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _case(name, dev):
    return G.gat_case(name, _cus(dev) if name in G.WALK else G.TRIP_CUS)


def _index(c, dev):
    """The device index of the case's edge list; its CSR order must be the host's (stable by destination, the inserted self
    loop last), on which the planted positions and the count of new maxima rest."""
    from gnn_qot_estimation_amd.graph import build_graph_index
    graph = build_graph_index(c.ei.to(dev), c.N, gat_self_loops=c.loops)
    assert torch.equal(graph.rowptr.long().cpu(), c.ix.rowptr)
    assert torch.equal(graph.col[:c.E].long().cpu(), c.ix.col) and torch.equal(graph.eid[:c.E].long().cpu(), c.ix.eid)
    return graph


def _once(c, form, dev, graph):
    from gnn_qot_estimation_amd import functional as QF
    att_s = c.att_src.to(dev).requires_grad_(True)
    att_d = c.att_dst.to(dev).requires_grad_(True)
    bias = c.bias.to(dev).requires_grad_(True)
    sink = []
    if form == "dense":
        lead = c.z.to(dev).requires_grad_(True)
        out = QF.GatFn.apply(lead, att_s, att_d, bias, graph, G.NS, False, c.a_src.to(dev), c.a_dst.to(dev), sink)
        stats = out.grad_fn.saved_tensors[3]
    else:
        lead = c.w.to(dev).requires_grad_(True)
        out = QF.GatThinFn.apply(c.x.to(dev), lead, att_s, att_d, bias, graph, G.NS, False, sink)
        stats = out.grad_fn.saved_tensors[4]
    out.backward(c.g.to(dev))
    torch.cuda.synchronize()
    res = dict(out=out, m=stats[:, :, 0], denom=stats[:, :, 1], grad_att_src=att_s.grad, grad_att_dst=att_d.grad,
               grad_bias=bias.grad, a_src=sink[-1][0], a_dst=sink[-1][1])
    res["grad_z" if form == "dense" else "grad_lin"] = lead.grad
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _run(name, form, dev, monkeypatch):
    key = (name, form)
    if key not in _RUNS:
        c = _case(name, dev)
        calls = _record(monkeypatch)
        graph = _index(c, dev)
        calls.clear()
        _nan_filled_empty(monkeypatch)
        t0 = time.perf_counter()
        first = _once(c, form, dev, graph)
        ran = tuple(k for k in calls if k.startswith("qot_gat_"))
        again = _once(c, form, dev, graph)
        _RUNS[key] = dict(case=c, first=first, again=again, ran=ran, seconds=time.perf_counter() - t0)
    return _RUNS[key]


def _check(tag, got, ref, form):
    """Per element for every tensor, and the global figure ``max|got - ref| <= TOL max|ref|`` on top.  ``grad_att_src`` and
    ``grad_att_dst`` are sums of ``ds = alpha (dalpha - delta) lrelu'``, which is analytically ZERO wherever a destination
    has one in-edge or all its ``raw`` on one side of 0 (the softmax is shift invariant): the reference is then 0 or a
    small remainder and the kernel's value is rounding noise inside its per-element bound, for which ``max|ref|`` is no
    scale.  Their global figure is taken as the project takes it for such gradients (``helpers.grad_compare``): relative
    to ``max(own magnitude, 1e-3 x the largest gradient of the case)``."""
    att = ("grad_att_src", "grad_att_dst")
    G.check_all(tag, got, ref, tuple(k for k in G.CHECKED[form] if k not in att), global_tol=TOL)
    G.check_all(tag, got, ref, att, global_tol=float("inf"))
    gmax = max(float(ref[k]["value"].abs().max()) for k in G.CHECKED[form] if k.startswith("grad"))
    for k in att:
        err = float((got[k].double().reshape(ref[k]["value"].shape) - ref[k]["value"]).abs().max())
        scale = max(float(ref[k]["value"].abs().max()), 1e-3 * gmax)
        print(f"{tag} {k}: global on max(own, 1e-3 largest gradient) {err / scale if scale else err:.3e}")
        assert err <= TOL * scale, (tag, k, err, scale)


@pytest.mark.parametrize("name,form", G.RUNS)
def test_kernels_against_fp64_element_by_element(cuda_device, monkeypatch, name, form):
    run = _run(name, form, cuda_device, monkeypatch)
    c, first, again = run["case"], run["first"], run["again"]
    tag = f"{name} {form}"
    t0 = time.perf_counter()
    if form == "thin":
        # the stage in front: x (W_h^T att_h) of qot_skinny_linear_fwd; the walk is then judged on ITS input
        G.check_all(tag, first, G.thin_logits_reference(c), ("a_src", "a_dst"), global_tol=TOL)
        ref = G.reference(c, "thin", logits=(first["a_src"], first["a_dst"]))
    else:
        assert torch.equal(first["a_src"], c.a_src) and torch.equal(first["a_dst"], c.a_dst)
        ref = G.reference(c, "dense") if name in G.WALK else G.host_reference(name, "dense")
    print(f"{tag}: N {c.N} E {c.E}  kernels twice {run['seconds']:.2f} s  fp64 reference {time.perf_counter() - t0:.2f} s")
    _check(tag, first, ref, form)
    # which kernels ran
    assert run["ran"] == WANT[form], (tag, run["ran"])
    # two runs, the same bits
    for k in first:
        assert torch.equal(first[k], again[k]), (tag, k, "two runs differ")
    # exact: the running maximum everywhere; isolated destinations; destinations whose only in-edge is the self loop
    assert torch.equal(first["m"], ref["m"]["value"].float()), (tag, "m")
    iso = ref["isolated"]
    assert torch.equal(first["out"][iso], c.bias[None, :].expand(int(iso.sum()), -1)), (tag, "isolated: out == bias")
    assert bool((first["m"][iso] == 0).all()) and bool((first["denom"][iso] == EPS).all()), (tag, "isolated: stats")
    only_loop = torch.zeros(c.N, dtype=torch.bool)
    if c.E:
        only_loop = (c.ix.deg == 1) & (c.ix.col[c.ix.rowptr[:-1].clamp(max=c.E - 1)] == torch.arange(c.N))
    if bool(only_loop.any()):
        one = (torch.ones((), dtype=torch.float32) + EPS)
        assert bool((first["denom"][only_loop] == one).all()), (tag, "self loop only: denom")
        if form == "dense":
            z = c.z[only_loop]
            assert torch.equal(first["out"][only_loop], z * (1.0 / one) + c.bias), (tag, "self loop only: out")
    if form == "dense":
        # a node that is nobody's source and has no in-edge of its own: no contribution to grad_z at all
        dead = (c.ix.outdeg == 0) & iso
        assert bool((first["grad_z"][dead] == 0).all()), (tag, "grad_z of an isolated, unread node")


@pytest.mark.parametrize("name", [n for n, cfg in G.CASES.items() if not cfg["loops"] and cfg["family"] != "walk"])
def test_isolated_destinations_leave_zero_rows_in_the_logit_gradients(cuda_device, monkeypatch, name):
    """The backward walks called on their own (the autograd functions keep ``grad_a`` and ``delta`` to themselves): an
    isolated destination has ``delta = grad_a_dst = 0``, a node without out-edges ``grad_a_src = 0`` and a zero row of the
    source pass's ``grad_z``; every other element is written (no NaN left)."""
    from gnn_qot_estimation_amd import _lib
    dev = cuda_device
    c = _case(name, dev)
    graph = _index(c, dev)
    N, H, HC = c.N, G.HEADS, c.HC
    z, g = c.z.to(dev), c.g.to(dev)
    a_s, a_d = c.a_src.to(dev), c.a_dst.to(dev)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    out, stats = nan(N, HC), nan(N, H, 2)
    _lib.call("qot_gat_fwd", z, a_s, a_d, c.bias.to(dev), graph.rowptr, graph.col, out, stats, N, H, c.C, G.NS, None)
    gad, gas, delta, gz, escr = nan(N, H), nan(N, H), nan(N, H), nan(N, HC), nan(max(graph.cap, 1), H, 2)
    _lib.call("qot_gat_bwd_dst", g, z, a_s, a_d, stats, graph.rowptr, graph.col, gad, escr, delta, N, H, c.C, G.NS, None, None)
    _lib.call("qot_gat_bwd_src", g, a_s, a_d, escr, delta, graph.rowptr_t, graph.col_t, graph.pos_t, gz, gas, N, H, c.C, G.NS,
              None, None, None)
    torch.cuda.synchronize()
    iso, leaf = c.ix.deg == 0, c.ix.outdeg == 0
    assert bool(iso.any())
    gad, gas, delta, gz = (t.cpu() for t in (gad, gas, delta, gz))
    assert not any(bool(torch.isnan(t).any()) for t in (gad, gas, delta, gz, out.cpu()))
    assert bool((gad[iso] == 0).all()) and bool((delta[iso] == 0).all()), name
    assert bool((gas[leaf] == 0).all()) and bool((gz[leaf] == 0).all()), name


@pytest.mark.parametrize("C", G.WIDTHS)
def test_logit_kernel_against_fp64(cuda_device, monkeypatch, C):
    """``qot_gat_logits``: ``GatFn`` without logits handed in forms them from ``z``; a C-term dot per head."""
    from gnn_qot_estimation_amd import functional as QF
    dev = cuda_device
    c = _case(f"degrees_noloop_c{C}", dev)
    graph = _index(c, dev)
    calls = _record(monkeypatch)
    _nan_filled_empty(monkeypatch)

    def once():
        sink = []
        with torch.no_grad():
            QF.GatFn.apply(c.z.to(dev), c.att_src.to(dev), c.att_dst.to(dev), c.bias.to(dev), graph, G.NS, False, None, None, sink)
        torch.cuda.synchronize()
        return dict(a_src=sink[-1][0].cpu(), a_dst=sink[-1][1].cpu())
    first, again = once(), once()
    G.check_all(f"logits c{C}", first, G.logits_reference(c), global_tol=TOL)
    assert tuple(k for k in calls if k.startswith("qot_gat_")) == ("qot_gat_logits", "qot_gat_fwd") * 2
    for k in first:
        assert torch.equal(first[k], again[k]), k


def test_shapes_reach_the_places_they_are_chosen_for(cuda_device):
    """Every walk case: at least three destinations per lane group of the forward, the grid at its cap; the holes cases:
    an isolated destination inside a lane group's run, between two destinations that share a source.  Prints the cap per
    width: the forward kernel's occupancy on this device."""
    from gnn_qot_estimation_amd import _lib
    lib = _lib.load()
    cus = _cus(cuda_device)
    for C in G.WIDTHS:
        cap = lib.qot_gat_blocks(1 << 24, G.HEADS, C)
        print(f"forward grid cap C = {C}: {cap} workgroups = {cap / cus:g} x {cus} CUs (RPB {G.rpb(C)}, EB {G.eb(C)})")
        assert cap <= min(8 * cus, 2048)
    for name in G.WALK:
        c = _case(name, cuda_device)
        C = c.C
        N = 3 * min(8 * cus, 2048) * G.rpb(C) + G.rpb(C) + 1
        assert c.N == N, name
        run = lib.qot_gat_chunk_rows(N, G.HEADS, C) // G.rpb(C)
        print(f"{name}: N {N}  destinations per lane group {run}")
        assert run >= 3, name
        assert lib.qot_gat_blocks(N, G.HEADS, C) == lib.qot_gat_blocks(1 << 24, G.HEADS, C), name
        if c.cfg.get("holes"):
            i = torch.arange(1, N - 1)
            deg = c.ix.deg
            first = c.ix.col[c.ix.rowptr[:-1].clamp(max=c.E - 1)]
            mid = (deg[i] == 0) & (deg[i - 1] > 0) & (deg[i + 1] > 0) & ((i - 1) // run == (i + 1) // run)
            assert bool(mid.any()), name
            k = int(i[mid][0])
            left = set(c.ix.col[c.ix.rowptr[k - 1]:c.ix.rowptr[k]].tolist())
            right = set(c.ix.col[c.ix.rowptr[k + 1]:c.ix.rowptr[k + 2]].tolist())
            assert left & right and int(first[k - 1]) != int(first[k + 1]), name


def test_thin_form_refusals(cuda_device):
    """K = 6 is the largest that fits at C = 256 (static and dynamic LDS add up to exactly 64 KB); K outside 1 .. 8 and a
    ``W^T`` that does not fit are refused by the entry point itself."""
    from gnn_qot_estimation_amd import _lib
    lib = _lib.load()
    assert lib.qot_gat_thin_supported(4, 256, 6) == 1 and lib.qot_gat_thin_supported(4, 256, 7) == 0
    for C in G.WIDTHS:
        for K in range(0, 10):
            assert lib.qot_gat_thin_supported(4, C, K) == int(G.thin_fits(C, K)), (C, K)
    dev = cuda_device
    c = _case("degrees_c16", dev)
    graph = _index(c, dev)
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    for C, K in ((16, 0), (16, 9), (256, 7)):
        HC = 4 * C
        with pytest.raises(_lib.QotError) as err:
            _lib.call("qot_gat_fwd_thin", f(c.N, max(K, 1)), K, f(HC, max(K, 1)), f(c.N, 4), f(c.N, 4), f(HC), graph.rowptr, graph.col,
                      f(c.N, HC), f(c.N, 4, 2), c.N, 4, C, G.NS, None)
        assert "status -1:" in str(err.value), str(err.value)          # QOT_ERR_UNSUPPORTED (include/qot_gnn.h)
