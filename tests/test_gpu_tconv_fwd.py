"""Every TransformerConv forward kernel (csrc/tconv.hip: per-destination in node and table mode, its score-matrix variant,
the tile form; csrc/tconv_rows.hip: the row form; csrc/tconv_graph.hip: the graph form) against the fp64 restatement of
tests/tconv_fwd_cases.py, element by element: ``|got - ref| <= k 2^-24 A`` with the count ``k`` and the magnitude ``A``
derived there.

Each kernel is checked at its own stage: ``QF.TConvFn.apply(qkvs, ...)`` and ``QF.TConvGraphFn.apply(..., pre = (t4, M, P))``
are called directly with drawn fp32 inputs, and the reference is taken from exactly those bits (scores and rows: from the
kernel's own ``scores``, which is checked against ``q k^T`` with a dot-product bound of its own; the graph form's ``t4``,
``M`` and ``P`` from ``tconv_graph_prepare`` likewise, in a test of their own).  Checked per element: ``out``, ``stats``
(running maximum, denominator), and what the graph form leaves for its backward (``alpha`` in edge order, ``aa``;
``ea_csr`` bit for bit).  Exact: an isolated destination's output and statistics, dropped elements.

The form is forced through the ``QOT_NO_TCONV_*`` switches and the entry point that ran is asserted from the recorded
``_lib.call`` names; every floating ``torch.empty`` is filled with NaN for the duration; each (case, form) runs twice
(bitwise equal); every tensor's worst ``error / bound`` is printed before anything is asserted (``pytest -s``; a record,
not a threshold).  One end-to-end check per form (table and parameters in, fp64 oracle, ``helpers.TOL``) shows that the
stages are wired together; it is not the sharp check.  The backward kernels are checked the same way in
tests/test_gpu_tconv_bwd.py."""
import pytest
import torch
import torch.nn.functional as F

import tconv_fwd_cases as T
from helpers import TOL

pytestmark = pytest.mark.gpu

_SWITCHES = ("QOT_TCONV_ROWS_PARTS", "QOT_NO_TCONV_SCORES", "QOT_NO_TCONV_GRAPH", "QOT_NO_TCONV_ROWS", "QOT_NO_TCONV_TILE",
             "QOT_NO_TCONV_FWD_ROWS", "QOT_NO_LAUNCH_GROUPS", "QOT_NO_TABLE_GEMM", "QOT_LIBRARY_GEMM")
_ENTRIES = ("qot_tconv_fwd", "qot_tconv_fwd_scores", "qot_tconv_fwd_rows", "qot_tconv_fwd_tile", "qot_tconv_fwd_graph",
            "qot_gemm_nt", "qot_table_scores", "qot_table_project_fwd")
WANT = {"node": ("qot_tconv_fwd",), "table": ("qot_tconv_fwd",), "scores": ("qot_gemm_nt", "qot_tconv_fwd_scores"),
        "rows": ("qot_gemm_nt", "qot_tconv_fwd_rows"), "tile": ("qot_tconv_fwd_tile",), "graph": ("qot_tconv_fwd_graph",)}
_RUNS = {}


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


def _case(name, dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count if T.CASES[name]["B"] == "trips" else T.TRIP_CUS
    return T.tconv_case(name, cus), cus


def _index(c, dev):
    """The device index of the case's batch; its CSR order must be the host's (stable by destination), on which the planted
    positions and the count of new maxima rest."""
    from gnn_qot_estimation_amd.graph import graph_index_for, table_maps_for
    batch = c.batch.to(dev)
    graph = graph_index_for(batch, c.N)
    maps = table_maps_for(batch, graph)
    assert (maps is not None) == c.table_mode
    eid, rowptr = graph.eid[:c.E].long().cpu(), graph.rowptr.long().cpu()
    assert torch.equal(rowptr, c.ix.rowptr) and torch.equal(eid, c.ix.eid)
    return batch, graph, maps, eid


def _act(c, dev):
    if c.p > 0:
        return (c.slope, c.p, c.seed, torch.tensor([c.step], dtype=torch.int64, device=dev))
    return (c.slope, 0.0, 0, None)


def _once(c, form, dev, graph, maps, batch):
    from gnn_qot_estimation_amd import _lib, functional as QF
    H, D = c.H, c.D
    qkvs = c.qkvs.to(dev).requires_grad_(True)
    ea, we = batch.edge_attr, c.w_edge.to(dev)
    res = {}
    if form == "graph":
        M, P = T.host_lookup(c, "graph")
        ldm = _lib.load().qot_tconv_graph_ldm(c.n)
        Mp = torch.zeros(c.n, ldm)
        Mp[:, :c.n] = M
        table = torch.zeros(c.V, H, device=dev, requires_grad=True)           # its shape is all the forward reads
        plan = QF.tconv_graph_plan(table, H, D, graph, maps)
        assert plan is not None and _lib.load().qot_tconv_graph_supported(c.n, int(graph.sizes[1]), H, D)
        wz, bz = torch.zeros(H, H, device=dev), torch.zeros(H, device=dev)
        out = QF.TConvGraphFn.apply(table, wz, bz, wz, bz, wz, bz, wz, bz, we, ea, (qkvs.detach(), Mp.to(dev), P.to(dev)),
                                    graph, maps, plan, _act(c, dev))
        saved = out.grad_fn.saved_tensors
        res.update(alpha=saved[7][:c.E], ea_csr=saved[8][:c.E], aa=saved[9][:c.N])
        res["plan"] = torch.tensor(plan)
    else:
        out = QF.TConvFn.apply(qkvs, ea, we, graph, maps, _act(c, dev))
        stats = out.grad_fn.saved_tensors[3]
        res.update(m=stats[:, 0], denom=stats[:, 1])
        if out.grad_fn.scores is not None:
            res["scores"] = out.grad_fn.scores
    res["out"] = out
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _run(name, form, dev, monkeypatch):
    key = (name, form)
    if key not in _RUNS:
        c, cus = _case(name, dev)
        _set_env(monkeypatch, T.env_of(name, form))
        if c.cfg.get("lift"):           # a size rule of the dispatcher, not a limit of the kernels (see the case table)
            from gnn_qot_estimation_amd import functional as QF
            monkeypatch.setattr(QF, "tconv_scores_ok", lambda qkvs, maps, num_nodes: maps is not None)
        calls = _record(monkeypatch)
        batch, graph, maps, eid = _index(c, dev)
        calls.clear()
        _nan_filled_empty(monkeypatch)
        first = _once(c, form, dev, graph, maps, batch)
        ran = tuple(k for k in calls if k in _ENTRIES)
        again = _once(c, form, dev, graph, maps, batch)
        _RUNS[key] = dict(case=c, cus=cus, first=first, again=again, ran=ran, eid=eid)
    return _RUNS[key]


def _to_edge_order(t, eid):
    return torch.empty_like(t).index_copy_(0, eid, t)


RUNS = [(name, form) for name in T.CASES for form in T.forms_of(name)]


@pytest.mark.parametrize("name,form", RUNS)
def test_forward_against_fp64_element_by_element(cuda_device, monkeypatch, name, form):
    run = _run(name, form, cuda_device, monkeypatch)
    c, first, again = run["case"], run["first"], run["again"]
    tag = f"{name} {form}"
    if form == "graph":
        ref = T.host_reference(name, "graph", run["cus"])
        ref = dict(ref, alpha={k: (_to_edge_order(v, c.ix.eid) if v.dim() == 1 and v.numel() == c.E else v)
                               for k, v in ref["alpha"].items()})
        got = dict(first, alpha=_to_edge_order(first["alpha"], run["eid"]))
        names = ("out", "alpha", "aa")
    else:
        if "scores" in first:
            # the stage in front: T_q T_k^T of qot_gemm_nt, an H-term dot; the attention kernel is then judged on ITS input
            T.check_all(tag, first, T.scores_reference(c), ("scores",), global_tol=TOL)
            ref = T.reference(c, form, lookup=first["scores"])
        else:
            ref = T.host_reference(name, form, run["cus"])
        got, names = first, ("out", "m", "denom")
    T.check_all(tag, got, ref, names, global_tol=TOL)
    # which kernel ran
    assert run["ran"] == WANT[form], (tag, run["ran"])
    assert ("scores" in first) == (form in ("scores", "rows"))
    # two runs, the same bits
    for k in first:
        assert torch.equal(first[k], again[k]), (tag, k, "two runs differ")
    # exact: isolated destinations, dropped elements, the edge features in slot order
    iso = ref["isolated"]
    skip = c.qkvs[c.rows[iso], 3 * c.H:]
    keep = c.keep[iso].float() * float(torch.tensor(c.ks, dtype=torch.float32))
    assert torch.equal(first["out"][iso], F.leaky_relu(skip, c.slope) * keep), (tag, "isolated destination")
    assert bool((first["out"][~c.keep] == 0).all()), (tag, "dropped elements")
    if form == "graph":
        assert torch.equal(first["ea_csr"], c.edge_attr[run["eid"]]), (tag, "ea_csr")
        assert bool((first["aa"][iso] == 0).all())
    else:
        assert bool((first["m"][iso] == 0).all()) and bool((first["denom"][iso] == torch.tensor(1e-16, dtype=torch.float32)).all())


@pytest.mark.parametrize("name", [n for n, cfg in T.CASES.items() if cfg["form"] == "rows"])
def test_rows_form_equals_the_scores_form_bit_for_bit(cuda_device, monkeypatch, name):
    """csrc/tconv_rows.hip: "Same arithmetic, same order: bit-equal outputs"."""
    rows, scores = _run(name, "rows", cuda_device, monkeypatch), _run(name, "scores", cuda_device, monkeypatch)
    assert rows["ran"] == WANT["rows"] and scores["ran"] == WANT["scores"]
    for k in ("out", "m", "denom", "scores"):
        assert torch.equal(rows["first"][k], scores["first"][k]), (name, k)


def test_shapes_reach_the_places_they_are_chosen_for(cuda_device, monkeypatch):
    """The trip case has more graphs than 4 x CUs (a second, ragged trip of workgroup 0 in the graph form), the big case a
    graph of more than 1024 edges (a second staging trip of 256 x 4 edges), the rows cases a second round per lane group."""
    run = _run("graph_h16_d8_n5_trips", "graph", cuda_device, monkeypatch)
    c, cus = run["case"], run["cus"]
    assert c.B == 4 * cus + 3 and cus == torch.cuda.get_device_properties(cuda_device).multi_processor_count
    big = _run("graph_h32_d3_n40_big", "graph", cuda_device, monkeypatch)
    assert int(big["first"]["plan"][2]) > 1024
    for name, cfg in T.CASES.items():
        if name in ("rows_h64_d5_b137", "rows_h256_d5_b41"):
            per = -(-cfg["B"] // 8)                         # graphs per slice: RPB + 2
            assert (per - 1) // T.rpb(cfg["H"]) == 1, name
        if cfg["form"] == "tile" and cfg["n"] > 12:
            assert 4 * T.rpb(cfg["H"]) < cfg["n"] < 8 * T.rpb(cfg["H"]), name


# ------------------------------------------------------------------ the stage in front of the graph form
@pytest.mark.parametrize("name", list(T.PREPARE_CASES))
def test_graph_form_inputs_against_fp64(cuda_device, monkeypatch, name):
    """``(t4, M, P)`` of ``tconv_graph_prepare`` (qot_table_project_fwd, qot_table_scores) from the parameters."""
    import gnn_qot_estimation_amd as q
    pc = T.prepare_case(name)
    ref = T.prepare_reference(pc)
    dev = cuda_device
    _set_env(monkeypatch, {})
    conv = q.nn.TransformerConv(pc.H, pc.H, edge_dim=pc.D)
    conv.load_state_dict(pc.state, strict=True)
    conv.to(dev)
    table = pc.table.to(dev)
    calls = _record(monkeypatch)
    _nan_filled_empty(monkeypatch)

    def once():
        t4, M, P = conv.prepare_graph_form(table, (pc.n, 1, 0))
        torch.cuda.synchronize()
        return dict(t4=t4.cpu(), M=M.cpu(), P=P.cpu())
    first, again = once(), once()
    got = dict(first, M=first["M"][:, :pc.n])
    T.check_all(f"prepare {name}", got, ref, ("t4", "M", "P"), global_tol=TOL)
    assert tuple(k for k in calls if k in _ENTRIES) == ("qot_table_project_fwd", "qot_table_scores") * 2
    assert first["M"].shape[1] == (pc.n + 3) // 4 * 4 and bool((first["M"][:, pc.n:] == 0).all())
    for k in first:
        assert torch.equal(first[k], again[k]), k


# ------------------------------------------------------------------ end to end, once per form
@pytest.mark.parametrize("form", T.FORMS)
def test_end_to_end_from_table_and_parameters(cuda_device, monkeypatch, form):
    """Table and parameters in, ``leaky_relu(conv(table[node_ids], ...))`` out, against the fp64 oracle at the project's bar
    (helpers.TOL): the stages are wired together."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import functional as QF
    from gnn_qot_estimation_amd.graph import cached_i32, graph_index_for, table_maps_for
    e = T.e2e_case(form)
    c = e.case
    dev = cuda_device
    _set_env(monkeypatch, {} if form == "graph" else T.env_of(c.name, form))
    conv = q.nn.TransformerConv(c.H, c.H, edge_dim=c.D)
    conv.load_state_dict(e.state, strict=True)
    conv.to(dev)
    table = e.table.to(dev)
    batch = c.batch.to(dev)
    calls = _record(monkeypatch)
    graph = graph_index_for(batch, c.N)
    maps = table_maps_for(batch, graph)
    act = (c.slope, 0.0, 0, None)
    with torch.no_grad():
        if form == "node":
            assert maps is None
            out = conv(QF.EmbedFn.apply(table, cached_i32(batch, "node_ids")), batch.edge_index, batch.edge_attr, graph=graph, act=act)
        elif form == "graph":
            plan = conv.graph_form(table, graph, maps)
            assert plan is not None
            out = conv.forward_table_graph(table, batch.edge_attr, graph, maps, plan, conv.prepare_graph_form(table, plan), act=act)
        else:
            out = conv.forward_table(table, batch.edge_attr, graph, maps, act=act)
    torch.cuda.synchronize()
    got = out.double().cpu()
    err = float((got - e.ref).abs().max() / e.ref.abs().max())
    print(f"end to end {form} ({c.name}): max|err| / max|ref| = {err:.3e}")
    assert {k for k in calls if k.startswith("qot_tconv_fwd")} == {WANT[form][-1]}, calls
    assert err <= TOL
