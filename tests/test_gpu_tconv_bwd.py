"""The TransformerConv backward kernels against the fp64 restatement of tests/tconv_bwd_cases.py, element by element:
``|got - ref| <= bound`` with the bound derived there.  csrc/tconv.hip: ``qot_tconv_bwd_dst`` and ``qot_tconv_bwd_src`` in node
mode and in tile mode (the forms node, table, scores and tile of the forward's case table); csrc/tconv_rows.hip:
``qot_tconv_bwd_dst_rows`` and ``qot_tconv_bwd_src_rows``; csrc/edge_grad.hip: ``qot_tconv_edge_attr_grad``.

Every kernel is judged on the fp32 bits it reads.  The product's own forward runs first (``QF.TConvFn.apply``); ``stats``, the
activated output ``y`` and (scores, rows) the score matrix are taken from what it saved, a fixed cotangent ``g`` is drawn, and
the reference is formed from those bits.  Two routes per case:
  1. what the product runs: ``torch.autograd.grad(out, (qkvs, edge_attr, w_edge), g)``: ``grad_qkvs``, ``grad_w_edge``,
     ``grad_edge_attr``, and the recorded ``_lib.call`` names;
  2. the C ABI directly, for what autograd hides: ``escr``, ``delta``, ``pds``, ``pal``, the per-node rows (node mode) or the
     partial table rows (tile mode: summed in fp64 here); row form: ``escr = (a, ds)``, ``delta``, ``grad_skip``, the part
     rows ``[grad T_skip | grad M | grad P]``, ``grad T_v`` and the lin_edge partials, with ``parts = 1`` and ``min(B, 8)``.
     The source pass is judged once more on the bits the destination pass left.  Every buffer is sized by the library's
     own functions exactly as ``TConvFn.backward`` / ``_tconv_backward_rows`` do, and every tensor behind a pointer stays
     alive in a local until the device has been waited for.

Switches cleared and set through ``monkeypatch``; every floating ``torch.empty`` NaN-filled; each case runs twice (the same
bits in every tensor: no kernel here adds in an order that varies); every tensor's worst ``error / bound`` is printed before
anything is asserted (``pytest -s``; a record, not a threshold).  The global figure ``helpers.TOL`` is asserted beside the
bounds, except in the sharp family for the tensors built on ``ds = a (da - delta)`` (``CANCELLING`` in tests/tconv_bwd_cases.py
says why: no fp32 evaluation reaches it there).

The graph form (csrc/tconv_graph.hip, ``tconv_bwd_graph_kernel``): a direct call of ``qot_tconv_bwd_graph`` with the forward's
``alpha``, ``ea_csr`` and ``aa`` and the case's ``t4`` as stage inputs, its ``qot_tconv_bwd_graph_blocks(B)`` partial rows summed in
fp64 here and the row ``[gTv | gTs | gM | gP | gWe]`` checked per element; through autograd (launch groups off, so that the entry
points are recorded) the bias gradients and ``grad_w_edge``, which do not depend on the projection weights.  ``gM`` is added
into its fp32 LDS image with ``atomicAdd`` (csrc/tconv_graph.hip:550, ``ATOMIC_GRAPH_GM`` in tests/grad_scale_cases.py): no
bit-for-bit claim for ``gM`` and for what is computed from it (grad T_q, grad T_k: the query and key halves of ``grad_b`` here).
``qot_table_project_bwd_scores`` is then called on its own, on a drawn row ``S`` of that layout, with the tables and parameters
of the forward suite's ``PREPARE_CASES``."""
import pytest
import torch

import tconv_bwd_cases as Bw
import tconv_fwd_cases as T
from helpers import TOL

pytestmark = pytest.mark.gpu

_SWITCHES = ("QOT_TCONV_ROWS_PARTS", "QOT_NO_TCONV_SCORES", "QOT_NO_TCONV_GRAPH", "QOT_NO_TCONV_ROWS", "QOT_NO_TCONV_TILE",
             "QOT_NO_TCONV_FWD_ROWS", "QOT_NO_LAUNCH_GROUPS", "QOT_NO_TABLE_GEMM", "QOT_LIBRARY_GEMM")
FWD_WANT = {"node": ("qot_tconv_fwd",), "table": ("qot_tconv_fwd",), "scores": ("qot_gemm_nt", "qot_tconv_fwd_scores"),
            "rows": ("qot_gemm_nt", "qot_tconv_fwd_rows"), "tile": ("qot_tconv_fwd_tile",)}
_ENTRIES = ("qot_gemm_nt", "qot_tconv_fwd", "qot_tconv_fwd_scores", "qot_tconv_fwd_rows", "qot_tconv_fwd_tile", "qot_tconv_fwd_graph",
            "qot_tconv_bwd_dst", "qot_tconv_bwd_src", "qot_tconv_bwd_dst_rows", "qot_tconv_bwd_src_rows", "qot_tconv_bwd_graph",
            "qot_tconv_edge_attr_grad")
PER_DST = ("qot_tconv_edge_attr_grad", "qot_tconv_bwd_dst", "qot_tconv_bwd_src")
ROWS = ("qot_tconv_edge_attr_grad", "qot_tconv_bwd_dst_rows", "qot_tconv_bwd_src_rows")
_RUNS = {}
TCONVFN_CASES = [n for n, cfg in Bw.CASES.items() if cfg["form"] != "graph"]          # what runs through QF.TConvFn


def _set_env(monkeypatch, env):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


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


def _act(c, dev):
    if c.p > 0:
        return (c.slope, c.p, c.seed, torch.tensor([c.step], dtype=torch.int64, device=dev))
    return (c.slope, 0.0, 0, None)


def _index(c, dev):
    """The device index of the case's batch; its CSR order must be the host's (stable by destination)."""
    from gnn_qot_estimation_amd.graph import graph_index_for, table_maps_for
    batch = c.batch.to(dev)
    graph = graph_index_for(batch, c.N)
    maps = table_maps_for(batch, graph)
    assert (maps is not None) == c.table_mode
    assert torch.equal(graph.rowptr.long().cpu(), c.ix.rowptr) and torch.equal(graph.eid[:c.E].long().cpu(), c.ix.eid)
    # the CSC the source pass walks holds every slot once, under its source
    pos_t = graph.pos_t[:c.E].long().cpu()
    assert torch.equal(pos_t.sort().values, torch.arange(c.E))
    assert torch.equal(torch.diff(graph.rowptr_t.long().cpu()), c.csc.outdeg)
    return batch, graph, maps


def _act_args(c, y, step):
    return (y, float(c.slope), float(c.p if step is not None else 0.0), int(c.seed if c.p > 0 else 0), step)


def _direct_per_destination(c, dev, graph, maps, qk, ea, we, stats, y, g, step):
    """``qot_tconv_bwd_dst`` then ``qot_tconv_bwd_src`` with buffers of this test, laid out as ``TConvFn.backward`` does."""
    from gnn_qot_estimation_amd import _lib
    lib = _lib.load()
    H, D, N = c.H, c.D, c.N
    H4 = 4 * H
    f32 = dict(dtype=torch.float32, device=dev)
    assert qk.is_contiguous() and qk.shape == (c.V, H4) and g.is_contiguous() and y.is_contiguous() and stats.shape == (N, 2)
    rpb = int(lib.qot_tconv_rows_per_block(H))
    assert rpb == T.rpb(H)
    escr = torch.empty(max(graph.cap, 1), 2, **f32)
    delta, pds, pal = torch.empty(N, **f32), torch.empty(N, D, **f32), torch.empty(N, D, **f32)
    gwe = torch.empty(H * D, **f32)
    q0 = qk.data_ptr()
    if maps is not None:
        B, n = (int(v) for v in maps[3])
        assert B * n == N and n <= c.V
        gb = (B + rpb - 1) // rpb
        gpart = torch.empty(gb, n, H4, **f32)
        gskip = torch.empty(N, H, **f32)
        gnode = None
        tile = (n, B, gpart)
        gq_p, gs_p, gk_p, gv_p, ldg = None, gskip.data_ptr(), None, None, H
        rowmap, colf, colf_t = maps[0], maps[1], maps[2]
        ws_rows, blocks = n * gb * rpb, n * gb
    else:
        gnode = torch.empty(N, H4, **f32)
        gpart = gskip = None
        tile = (0, 0, None)
        base = gnode.data_ptr()
        gq_p, gs_p, gk_p, gv_p, ldg = base, base + 4 * 3 * H, base + 4 * H, base + 4 * 2 * H, H4
        rowmap, colf, colf_t = None, graph.col, None
        ws_rows, blocks = N, (N + rpb - 1) // rpb
    assert int(lib.qot_tconv_bwd_dst_blocks(N, H, tile[0], tile[1])) == blocks
    ws = torch.empty(int(lib.qot_tconv_bwd_dst_workspace_floats(ws_rows, H, D)), **f32)
    assert ws.numel() >= (blocks + (blocks + Bw.WEDGE_GROUP - 1) // Bw.WEDGE_GROUP) * H * D
    assert graph.rowptr.numel() == N + 1 and graph.rowptr_t.numel() == N + 1 and colf.numel() >= c.E
    _lib.call("qot_tconv_bwd_dst", g, q0, q0 + 4 * H, q0 + 8 * H, H4, ea, we, stats, graph.rowptr, colf, graph.eid, rowmap,
              gq_p, gs_p, ldg, escr, delta, pds, pal, *_act_args(c, y, step), gwe, ws, *tile, N, H, D)
    _lib.call("qot_tconv_bwd_src", gs_p, ldg, q0, H4, escr, delta, graph.rowptr_t, graph.col_t, graph.pos_t, colf_t,
              gk_p, gv_p, ldg, *tile, N, H)
    torch.cuda.synchronize()
    res = dict(a=escr[:c.E, 0], da=escr[:c.E, 1], delta=delta, pds=pds, pal=pal, gwe=gwe.view(H, D))
    if gnode is not None:
        res.update(gq=gnode[:, :H], gk=gnode[:, H:2 * H], gv=gnode[:, 2 * H:3 * H], gskip=gnode[:, 3 * H:])
    else:
        res.update(gskip=gskip, gpart=gpart)
    res["blocks"] = torch.tensor(blocks)
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _direct_rows(c, dev, graph, maps, qk, ea, we, stats, y, g, step, scores, parts):
    """``qot_tconv_bwd_dst_rows`` then ``qot_tconv_bwd_src_rows``, buffers as ``functional._tconv_backward_rows`` sizes them."""
    from gnn_qot_estimation_amd import _lib
    lib = _lib.load()
    H, D, N = c.H, c.D, c.N
    H4 = 4 * H
    B, n = (int(v) for v in maps[3])
    assert B * n == N and n == c.V == qk.shape[0] and 1 <= parts <= B and lib.qot_tconv_rows_supported(n, H, D)
    assert scores.shape == (n, n) and scores.is_contiguous() and qk.is_contiguous()
    npad, ldrow = int(lib.qot_tconv_rows_npad(n)), int(lib.qot_tconv_rows_ld(n, H, D))
    assert ldrow >= H + npad + D
    f32 = dict(dtype=torch.float32, device=dev)
    escr = torch.empty(max(graph.cap, 1), 2, **f32)
    delta, gskip = torch.empty(N, **f32), torch.empty(N, H, **f32)
    drows = torch.empty(parts, n * ldrow, **f32)
    wparts = torch.empty(parts * n, H * D, **f32)
    vrows = torch.empty(parts, n * H, **f32)
    q0 = qk.data_ptr()
    _lib.call("qot_tconv_bwd_dst_rows", g, q0, q0 + 8 * H, H4, ea, we, stats, graph.rowptr, maps[1], graph.eid, scores,
              scores.shape[1], gskip, escr, delta, *_act_args(c, y, step), n, B, parts, drows, wparts, H, D)
    _lib.call("qot_tconv_bwd_src_rows", gskip, escr, graph.rowptr_t, graph.col_t, graph.pos_t, n, B, parts, vrows, H)
    torch.cuda.synchronize()
    S = drows.double().sum(0).view(n, ldrow)                   # the slices, summed in fp64 on the host
    res = dict(a=escr[:c.E, 0], ds=escr[:c.E, 1], delta=delta, gskip=gskip, gTs=S[:, :H], gM=S[:, H:H + n],
               gP=S[:, H + npad:H + npad + D], gTv=vrows.double().sum(0).view(n, H), gwe_g=wparts.double().sum(0).view(H, D),
               pad=drows.view(parts, n, ldrow)[:, :, H + n:H + npad], tail=drows.view(parts, n, ldrow)[:, :, H + npad + D:])
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _once(c, form, dev, graph, maps, batch, calls):
    from gnn_qot_estimation_amd import functional as QF
    del calls[:]
    qkvs = c.qkvs.to(dev).requires_grad_(True)
    ea = batch.edge_attr.detach().clone().requires_grad_(True)
    we = c.w_edge.to(dev).requires_grad_(True)
    g = c.g.to(dev)
    act = _act(c, dev)
    out = QF.TConvFn.apply(qkvs, ea, we, graph, maps, act)
    stats = out.grad_fn.saved_tensors[3]
    scores = out.grad_fn.scores
    gq, gea, gwe = torch.autograd.grad(out, (qkvs, ea, we), g)
    torch.cuda.synchronize()
    res = dict(stats=stats, y=out, grad_qkvs=gq, gea=gea, gwe=gwe)
    if scores is not None:
        res["scores"] = scores
    res = {k: v.detach().cpu().clone() for k, v in res.items()}
    ran = tuple(k for k in calls if k in _ENTRIES)
    del calls[:]
    qk, ead, wed, y = qkvs.detach(), ea.detach(), we.detach(), out.detach()
    if form == "rows":
        assert scores is not None
        res["direct"] = {parts: _direct_rows(c, dev, graph, maps, qk, ead, wed, stats, y, g, act[3], scores, parts)
                         for parts in sorted({1, min(c.B, 8)})}
    else:
        res["direct"] = _direct_per_destination(c, dev, graph, maps, qk, ead, wed, stats, y, g, act[3])
    return res, ran, tuple(k for k in calls if k in _ENTRIES)


def _run(name, dev, monkeypatch):
    if name not in _RUNS:
        c = Bw.bwd_case(name)
        form = c.cfg["form"]
        _set_env(monkeypatch, Bw.env_of(name))
        if c.cfg.get("lift"):           # a size rule of the dispatcher, not a limit of the kernels (tests/tconv_fwd_cases.py)
            from gnn_qot_estimation_amd import functional as QF
            monkeypatch.setattr(QF, "tconv_scores_ok", lambda qkvs, maps, num_nodes: maps is not None)
        calls = _record(monkeypatch)
        batch, graph, maps = _index(c, dev)
        _nan_filled_empty(monkeypatch)
        first, ran, ran_direct = _once(c, form, dev, graph, maps, batch, calls)
        again, _, _ = _once(c, form, dev, graph, maps, batch, calls)
        _RUNS[name] = dict(case=c, form=form, first=first, again=again, ran=ran, ran_direct=ran_direct)
    return _RUNS[name]


def _same_bits(tag, a, b):
    for k in a:
        if isinstance(a[k], dict):
            _same_bits(f"{tag} {k}", a[k], b[k])
        else:
            assert torch.equal(a[k], b[k]), (tag, k, "two runs differ")


def _act_backward32(c, g, y):
    """``g_i`` behind the activation, in the kernels' fp32 order: ``g * (keep ? keep_scale : 0) * (y > 0 ? 1 : slope)``."""
    ks = torch.tensor(c.ks, dtype=torch.float32)
    return g * (c.keep.float() * ks) * torch.where(y > 0, torch.ones(()), torch.tensor(c.slope, dtype=torch.float32))


@pytest.mark.parametrize("name", TCONVFN_CASES)
def test_backward_against_fp64_element_by_element(cuda_device, monkeypatch, name):
    run = _run(name, cuda_device, monkeypatch)
    c, form, first = run["case"], run["form"], run["first"]
    H, n = c.H, c.n
    stage = dict(m=first["stats"][:, 0], denom=first["stats"][:, 1], y=first["y"], g=c.g)
    ref = Bw.reference(c, form, stage, scores=first.get("scores"), slices=min(c.B, 8))
    # route 1: what autograd returns
    if form == "rows":
        got = dict(grad_qkvs_rows=first["grad_qkvs"], gwe_rows=first["gwe"], gea=first["gea"])
        Bw.check(c, f"{name} autograd", got, ref, ("grad_qkvs_rows", "gwe_rows", "gea"), TOL)
    else:
        Bw.check(c, f"{name} autograd", first, ref, ("grad_qkvs", "gwe", "gea"), TOL)
    # route 2: the entry points themselves
    iso, no_out = ref["isolated"], ref["no_out"]
    gact = _act_backward32(c, c.g, first["y"])
    if form == "rows":
        # the part rows are judged against the least favourable number of slices; what a destination computes does not depend
        # on the slices: the same bits in escr, delta and grad_skip, so the source pass's inputs are one set
        d1 = first["direct"][1]
        src = dict(a=d1["a"], da=d1["ds"], delta=torch.zeros(c.N), gskip=d1["gskip"])
        refs = Bw.reference(c, form, stage, scores=first["scores"], src_stage=src)
        for parts, d in first["direct"].items():
            Bw.check(c, f"{name} rows parts={parts}", d, ref, ("a", "ds", "delta", "gskip", "gTs", "gM", "gP", "gTv", "gwe_g"),
                     TOL)
            for k in ("a", "ds", "delta", "gskip"):
                assert torch.equal(d[k], d1[k]), (name, parts, k)
            Bw.check(c, f"{name} rows parts={parts} source pass on its inputs", d, refs, ("gTv",), TOL)
            assert bool((d["pad"] == 0).all()) and bool((d["tail"] == 0).all()), (name, "padding columns of the part rows")
            assert bool((d["delta"][iso] == 0).all()) and torch.equal(d["gskip"], gact)
    else:
        d = first["direct"]
        names = ("a", "da", "delta", "pds", "pal", "gskip", "gwe")
        src = dict(a=d["a"], da=d["da"], delta=d["delta"], gskip=d["gskip"])
        refs = Bw.reference(c, form, stage, src_stage=src)
        if c.table_mode:
            table = d["gpart"].double().sum(0)                 # [n, 4H]: the groups of graphs, summed in fp64 on the host
            got = dict(d, grad_qkvs=torch.cat([table, table.new_zeros(c.V - n, 4 * H)], 0))
            got.update(gk_table=got["grad_qkvs"][:, H:2 * H], gv_table=got["grad_qkvs"][:, 2 * H:3 * H])
            Bw.check(c, f"{name} direct", got, ref, names + ("grad_qkvs",), TOL)
            Bw.check(c, f"{name} direct source pass on its inputs", got, refs, ("gk_table", "gv_table"), TOL)
        else:
            got = d
            Bw.check(c, f"{name} direct", got, ref, names + ("gq", "gk", "gv"), TOL)
            Bw.check(c, f"{name} direct source pass on its inputs", got, refs, ("gk", "gv"), TOL)
            # exact: a source without out-edges, an isolated destination
            assert int(no_out.sum()) >= 1 and bool((d["gk"][no_out] == 0).all()) and bool((d["gv"][no_out] == 0).all())
            assert bool((d["gq"][iso] == 0).all())
            assert bool((first["grad_qkvs"][:, H:3 * H][no_out] == 0).all()) and bool((first["grad_qkvs"][:, :H][iso] == 0).all())
        assert bool((d["delta"][iso] == 0).all()) and bool((d["pds"][iso] == 0).all()) and bool((d["pal"][iso] == 0).all())
        assert torch.equal(d["gskip"], gact), (name, "gskip is the activation backward of g")
    assert int(iso.sum()) >= 1
    assert bool((gact[~c.keep] == 0).all())
    # table rows no node refers to
    if c.table_mode and c.V > n:
        assert bool((first["grad_qkvs"][n:] == 0).all())
    # which kernels ran: the forward's form, then the backward's entry points
    fwd = FWD_WANT[form]
    assert run["ran"] == fwd + (ROWS if form == "rows" else PER_DST), (name, run["ran"])
    assert run["ran_direct"] == (ROWS[1:] * len(first["direct"]) if form == "rows" else PER_DST[1:]), (name, run["ran_direct"])
    # two runs, the same bits in every tensor
    _same_bits(name, first, run["again"])


def test_every_entry_point_ran_in_both_routes(cuda_device, monkeypatch):
    """``qot_tconv_bwd_dst`` and ``qot_tconv_bwd_src`` in node mode and in tile mode, the row form's two passes: each in the
    product route (recorded names) and in a direct stage call; the shapes reach the places they are chosen for."""
    modes = {"node": 0, "tile": 0, "rows": 0}
    for name in TCONVFN_CASES:
        run = _run(name, cuda_device, monkeypatch)
        c = run["case"]
        if run["form"] == "rows":
            assert run["ran"][-2:] == ROWS[1:] == run["ran_direct"][:2] and set(run["first"]["direct"]) == {1, min(c.B, 8)}
            modes["rows"] += 1
        else:
            assert run["ran"][-2:] == PER_DST[1:] == run["ran_direct"]
            modes["tile" if c.table_mode else "node"] += 1
            assert ("gpart" in run["first"]["direct"]) == c.table_mode
    assert all(v >= 2 for v in modes.values()), modes
    wedge = _run("node_h256_d1_wedge", cuda_device, monkeypatch)
    assert int(wedge["first"]["direct"]["blocks"]) == 2 * Bw.WEDGE_GROUP + 1          # the two-level lin_edge sum ran
    for name in ("tile_h64_d4_b33", "tile_h64_d4_n70"):
        d = _run(name, cuda_device, monkeypatch)["first"]["direct"]
        assert d["gpart"].shape[0] == -(-Bw.CASES[name]["B"] // T.rpb(64)) >= 2       # a ragged last group of graphs


# ------------------------------------------------------------------ the graph form
_GRUNS = {}
GRAPH_CASES = [n for n, cfg in Bw.CASES.items() if cfg["form"] == "graph"]
GRAPH_WANT = ("qot_tconv_fwd_graph", "qot_tconv_bwd_graph", "qot_table_project_bwd_scores")


def _row_layout(n, H, D):
    """``tg_row`` of csrc/tconv_graph_dev.hpp: (ldm, off_gv, off_gs, off_gm, off_gp, off_gwe, len)."""
    pad4 = lambda v: (v + 3) & ~3                                       # noqa: E731
    ldm = pad4(n)
    off_gm = 2 * n * H
    off_gp = off_gm + n * ldm
    off_gwe = pad4(off_gp + n * D)
    return ldm, 0, n * H, off_gm, off_gp, off_gwe, pad4(off_gwe + H * D)


def _graph_once(c, dev, graph, maps, batch, calls):
    from gnn_qot_estimation_amd import _lib, functional as QF
    lib = _lib.load()
    H, D, n, N = c.H, c.D, c.n, c.N
    del calls[:]
    t4 = c.qkvs.to(dev)
    M, P = T.host_lookup(c, "graph")
    ldm = int(lib.qot_tconv_graph_ldm(n))
    Mp = torch.zeros(n, ldm)
    Mp[:, :n] = M
    table = torch.zeros(c.V, H, device=dev, requires_grad=True)           # its shape is all the forward reads
    plan = QF.tconv_graph_plan(table, H, D, graph, maps)
    assert plan is not None and plan[0] == n and plan[1] == c.B
    we = c.w_edge.to(dev).requires_grad_(True)
    ws = [torch.zeros(H, H, device=dev, requires_grad=True) for _ in range(4)]
    bs = [torch.zeros(H, device=dev, requires_grad=True) for _ in range(4)]
    ea = batch.edge_attr
    g = c.g.to(dev)
    act = _act(c, dev)
    out = QF.TConvGraphFn.apply(table, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], ws[3], bs[3], we, ea, (t4, Mp.to(dev), P.to(dev)),
                                graph, maps, plan, act)
    saved = out.grad_fn.saved_tensors
    alpha, ea_csr, aa = saved[7], saved[8], saved[9]
    grads = torch.autograd.grad(out, [table] + bs + [we], g)
    torch.cuda.synchronize()
    res = dict(alpha=alpha[:c.E], aa=aa[:N], y=out, grad_table=grads[0], grad_b=torch.cat(grads[1:5]), gwe=grads[5])
    res = {k: v.detach().cpu().clone() for k, v in res.items()}
    ran = tuple(k for k in calls if k in _ENTRIES + ("qot_table_project_bwd_scores",))
    # the entry point itself: sized as TConvGraphFn.backward sizes it, n, B and max_e from the product's own plan
    blocks, rowlen = int(lib.qot_tconv_bwd_graph_blocks(c.B)), int(lib.qot_tconv_graph_row_floats(n, H, D))
    assert rowlen == _row_layout(n, H, D)[6] and 1 <= blocks <= c.B
    assert lib.qot_tconv_graph_supported(n, plan[2], H, D) and t4.is_contiguous() and t4.shape == (c.V, 4 * H) and n <= c.V
    assert alpha.numel() >= max(c.E, 1) and ea_csr.shape == (max(c.E, 1), D) and aa.shape == (max(N, 1), D)
    y = out.detach()
    wed = we.detach()
    partials = torch.empty(blocks, rowlen, dtype=torch.float32, device=dev)
    _lib.call("qot_tconv_bwd_graph", g, *_act_args(c, y, act[3]), t4, 4 * H, wed, ea_csr, alpha, aa, graph.rowptr, maps[1],
              graph.row, graph.rowptr_t, graph.col_t, graph.pos_t, partials, n, c.B, plan[2], H, D)
    torch.cuda.synchronize()
    res["partials"] = partials.cpu().clone()
    res["plan"] = torch.tensor(plan)
    return res, ran


def _graph_run(name, dev, monkeypatch):
    if name not in _GRUNS:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count if Bw.CASES[name]["B"] == "trips" else T.TRIP_CUS
        c = Bw.bwd_case(name, cus)
        _set_env(monkeypatch, dict(Bw.env_of(name), QOT_NO_LAUNCH_GROUPS="1"))
        calls = _record(monkeypatch)
        batch, graph, maps = _index(c, dev)
        _nan_filled_empty(monkeypatch)
        first, ran = _graph_once(c, dev, graph, maps, batch, calls)
        again, _ = _graph_once(c, dev, graph, maps, batch, calls)
        _GRUNS[name] = dict(case=c, cus=cus, first=first, again=again, ran=ran)
    return _GRUNS[name]


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_graph_form_backward_against_fp64_element_by_element(cuda_device, monkeypatch, name):
    run = _graph_run(name, cuda_device, monkeypatch)
    c, first, again = run["case"], run["first"], run["again"]
    H, D, n = c.H, c.D, c.n
    ldm, off_gv, off_gs, off_gm, off_gp, off_gwe, rowlen = _row_layout(n, H, D)
    stage = dict(y=first["y"], g=c.g, alpha=first["alpha"], aa=first["aa"], m=c.stats[:, 0], denom=c.stats[:, 1])
    ref = Bw.reference_graph(c, stage)
    S = first["partials"].double().sum(0)                       # the workgroups' partial rows, summed in fp64 on the host
    gm = S[off_gm:off_gm + n * ldm].view(n, ldm)
    got = dict(gTv=S[off_gv:off_gv + n * H].view(n, H), gTs=S[off_gs:off_gs + n * H].view(n, H), gM=gm[:, :n],
               gP=S[off_gp:off_gp + n * D].view(n, D), gwe_g=S[off_gwe:off_gwe + H * D].view(H, D))
    Bw.check(c, f"{name} direct", got, ref, ("gTv", "gTs", "gM", "gP", "gwe_g"), TOL)
    Bw.check(c, f"{name} autograd", first, ref, ("grad_b", "gwe"), TOL)
    # exact: padding columns of gM, rows of grad T_v no out-edge feeds, the table rows no node refers to (zero weights here:
    # the whole table gradient), an empty batch
    pm = first["partials"][:, off_gm:off_gm + n * ldm].view(-1, n, ldm)
    assert bool((pm[:, :, n:] == 0).all()), (name, "padding columns of gM")
    assert bool((got["gTv"][ref["no_out_rows"]] == 0).all())
    assert bool((first["grad_table"] == 0).all())
    if c.E == 0:
        for k in ("gTv", "gM", "gP", "gwe_g"):
            assert bool((got[k] == 0).all()), (name, k)
        assert bool((first["gwe"] == 0).all()) and bool((first["grad_b"][:3 * H] == 0).all())
    assert run["ran"] == GRAPH_WANT, (name, run["ran"])
    # two runs: the same bits, except gM (csrc/tconv_graph.hip:550: atomicAdd into the LDS image) and what is computed from it
    free = torch.zeros(rowlen, dtype=torch.bool)              # (the row's alignment padding is written by nobody)
    for off, length in ((off_gv, n * H), (off_gs, n * H), (off_gp, n * D), (off_gwe, H * D)):
        free[off:off + length] = True
    assert not bool(torch.isnan(first["partials"][:, free]).any())
    assert torch.equal(first["partials"][:, free], again["partials"][:, free]), (name, "two runs differ")
    for k in ("alpha", "aa", "y", "gwe", "grad_table"):
        assert torch.equal(first[k], again[k]), (name, k, "two runs differ")
    assert torch.equal(first["grad_b"][2 * H:], again["grad_b"][2 * H:]), (name, "grad_b of value and skip: two runs differ")


def test_graph_form_shapes_reach_the_places_they_are_chosen_for(cuda_device, monkeypatch):
    """More graphs than workgroups (a workgroup walks several graphs, the next-graph prefetch runs), one graph, a graph of
    more than 1024 edges, no edges at all, the largest graph."""
    from gnn_qot_estimation_amd import _lib
    trips = _graph_run("graph_h16_d8_n5_trips", cuda_device, monkeypatch)
    cus = torch.cuda.get_device_properties(cuda_device).multi_processor_count
    assert trips["case"].B == 4 * cus + 3 and trips["first"]["partials"].shape[0] == _lib.load().qot_tconv_bwd_graph_blocks(4 * cus + 3)
    assert trips["first"]["partials"].shape[0] < trips["case"].B
    assert _graph_run("graph_h64_d4_b1", cuda_device, monkeypatch)["first"]["partials"].shape[0] == 1
    assert int(_graph_run("graph_h32_d3_n40_big", cuda_device, monkeypatch)["first"]["plan"][2]) > 1024
    assert _graph_run("graph_h128_d3_e0", cuda_device, monkeypatch)["case"].E == 0
    assert _graph_run("graph_h16_d4_n128", cuda_device, monkeypatch)["case"].n == 128


@pytest.mark.parametrize("name", list(T.PREPARE_CASES))
def test_projection_backward_from_a_summed_row_against_fp64(cuda_device, monkeypatch, name):
    """``qot_table_project_bwd_scores`` on its own: a drawn row ``S`` (padding columns of gM zero, as the kernel leaves them), ``t4``
    (the fp64 projection rounded to fp32), the table, the four weights and ``w_edge`` in; ``grad_table``, ``grad_w``, ``grad_b``
    and ``grad_w_edge`` against fp64 with dot-product bounds."""
    from gnn_qot_estimation_amd import _lib
    lib = _lib.load()
    pc = T.prepare_case(name)
    H, D, n, V = pc.H, pc.D, pc.n, pc.V
    dev = cuda_device
    _set_env(monkeypatch, {})
    layout = _row_layout(n, H, D)
    ldm, off_gm, rowlen = layout[0], layout[3], layout[6]
    assert rowlen == int(lib.qot_tconv_graph_row_floats(n, H, D)) and ldm == int(lib.qot_tconv_graph_ldm(n))
    gen = torch.Generator().manual_seed(5000 + H + D + n)
    S = torch.randn(rowlen, generator=gen)
    S[off_gm:off_gm + n * ldm].view(n, ldm)[:, n:] = 0
    sd = pc.state
    w4 = torch.cat([sd[f"{k}.weight"] for k in T._LINS], 0)
    b4 = torch.cat([sd[f"{k}.bias"] for k in T._LINS], 0)
    t4 = (pc.table.double() @ w4.double().t() + b4.double()).float()
    ref = Bw.project_bwd_reference(pc, S, t4, layout[:6])
    calls = _record(monkeypatch)
    _nan_filled_empty(monkeypatch)
    dS, dt4, dtab, dwe = S.to(dev), t4.to(dev).contiguous(), pc.table.to(dev).contiguous(), sd["lin_edge.weight"].to(dev).contiguous()
    dw = [sd[f"{k}.weight"].to(dev).contiguous() for k in T._LINS]
    assert dt4.shape == (V, 4 * H) and dtab.shape == (V, H) and dwe.shape == (H, D) and all(w.shape == (H, H) for w in dw) and n <= V

    def once():
        gt = torch.empty(V * H, dtype=torch.float32, device=dev)
        gw = torch.empty(4 * H * H, dtype=torch.float32, device=dev)
        gb = torch.empty(4 * H, dtype=torch.float32, device=dev)
        gwe = torch.empty(H, D, dtype=torch.float32, device=dev)
        _lib.call("qot_table_project_bwd_scores", dS, dt4, dwe, dtab, dw[0], dw[1], dw[2], dw[3], gt, gw, gb, gwe, V, n, H, D)
        torch.cuda.synchronize()
        return dict(grad_table=gt.view(V, H).cpu(), grad_w=gw.view(4 * H, H).cpu(), grad_b=gb.cpu(), grad_w_edge=gwe.cpu())
    first, again = once(), once()
    Bw.check_all(f"project backward {name}", first, ref, ("grad_table", "grad_w", "grad_b", "grad_w_edge"), global_tol=TOL)
    assert bool((first["grad_table"][n:] == 0).all())
    assert calls == ["qot_table_project_bwd_scores"] * 2
    for k in first:
        assert torch.equal(first[k], again[k]), k
