"""Host-side checks of tests/tconv_fwd_cases.py: the fp64 restatement agrees with both oracles, the case table plants what
it says, the same chain in fp32 stays inside every bound, and every planted defect leaves one.  No GPU."""
import types

import pytest
import torch
import torch.nn.functional as F

import tconv_fwd_cases as T

CHECKED = ("out", "m", "denom", "alpha", "aa")


def _from_parameters(H, D, seed):
    """A node-mode namespace of ``tconv_case``'s form whose ``qkvs`` is the fp64 projection of random features."""
    from oracle import sparse as O
    base = T.tconv_case(f"node_h{H}_d{D}")
    torch.manual_seed(seed)
    conv = O.TransformerConv(H, H, edge_dim=D).double()
    with torch.no_grad():
        for p in conv.parameters():
            if p.dim() == 1 and p.abs().max() == 0:
                p.uniform_(-0.1, 0.1)
    x = torch.randn(base.N, H, dtype=torch.float64)
    with torch.no_grad():
        qkvs = torch.cat([lin(x) for lin in (conv.lin_query, conv.lin_key, conv.lin_value, conv.lin_skip)], 1)
    c = types.SimpleNamespace(**dict(vars(base), qkvs=qkvs, w_edge=conv.lin_edge.weight.detach().clone()))
    return c, conv, x


@pytest.mark.parametrize("H,D", [(16, 1), (64, 4), (256, 5)])
def test_restatement_equals_both_oracles_in_fp64(H, D):
    from oracle import dense64
    c, conv, x = _from_parameters(H, D, 31 + H)
    got = T._evaluate(c, torch.float64)["out"]
    with torch.no_grad():
        sparse = F.leaky_relu(conv(x, c.ei, c.edge_attr.double()), T.SLOPE32)
    dense = F.leaky_relu(dense64.transformer_conv(conv.state_dict(), "", x, c.ei, c.edge_attr), T.SLOPE32)
    scale = float(sparse.abs().max())
    for name, ref in (("oracle.sparse", sparse), ("oracle.dense64", dense)):
        err = float((got - ref).abs().max()) / scale
        print(f"h{H} d{D} {name}: {err:.3e}")
        assert err <= 1e-12, (name, err)


def test_widths_cover_every_h_and_d():
    used = {(c["H"], c["D"]) for c in T.CASES.values()}
    assert used == set(T.WIDTHS)
    assert {h for h, _ in used} == {16, 32, 64, 128, 256} and {d for _, d in used} == {1, 3, 4, 5, 8}
    for form in T.FORMS:
        mine = [c for c in T.CASES.values() if c["form"] == form]
        assert any(c["p"] == 0.5 for c in mine) and any(c["family"] == "sharp" for c in mine), form


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_table_plants_what_it_says(name):
    c = T.tconv_case(name)
    cfg = c.cfg
    deg = c.ix.deg
    if cfg.get("empty"):
        assert c.E == 0
        return
    # eid is not the identity, duplicates and self loops (asserted in tconv_case as well)
    assert not torch.equal(c.ix.eid, torch.arange(c.E))
    # one graph of the batch has no edges at all (a single graph aside)
    per_graph = torch.zeros(c.B, dtype=torch.long).index_add_(0, c.batch.batch, deg)
    assert c.B == 1 or int((per_graph == 0).sum()) == 1
    # the in-degree set per BT: every class somewhere in the batch; in every graph with edges where n >= 12
    classes = set(T.degree_classes(c.H))
    live_nodes = int((per_graph[c.batch.batch] > 0).sum())
    want = classes if live_nodes >= 12 else set(T.degree_classes(c.H)[:live_nodes])       # (node mode at H = 256: 8 nodes)
    assert want <= set(deg.tolist()), (name, want - set(deg.tolist()))
    if c.n is not None and c.n >= 12:
        for g in range(c.B):
            if per_graph[g] and not (cfg.get("big") and g == 2):
                assert classes <= set(deg[c.batch.batch == g].tolist()), (name, g)
    # the spread limits of the family
    live = c.spread[deg >= 2]
    print(f"{name}: spread {float(live.min()):.2f} .. {float(live.max()):.2f}")
    if c.family == "sharp":
        assert 40.0 <= float(live.min()) and float(live.max()) <= 60.0
        # the place of the maximum: first, middle, last in CSR order, by destination
        s = T._evaluate(c, torch.float64)["s"]
        seen = set()
        for i in torch.nonzero(deg >= 3).view(-1).tolist():
            a, b = int(c.ix.rowptr[i]), int(c.ix.rowptr[i + 1])
            place = int(torch.argmax(s[a:b]))
            assert place == (0, (b - a) // 2, b - a - 1)[i % 3], (name, i)
            seen.add(i % 3)
        assert seen == {0, 1, 2}
        ref = T.host_reference(name, cfg["form"])
        if cfg["form"] != "graph":
            assert float(ref["nrec"].max()) >= 1          # a later edge carries the maximum somewhere
    else:
        assert float(live.max()) <= 16.0
    if cfg.get("big"):
        assert int(per_graph.max()) > 1024


@pytest.mark.parametrize("name", list(T.CASES))
def test_fp32_restatement_is_inside_every_bound(name):
    c = T.tconv_case(name)
    for form in T.forms_of(name):
        ref = T.host_reference(name, form)
        lookup = T.host_lookup(c, form)
        got = T._evaluate(c, torch.float32, lookup=lookup)
        T.check_all(f"{name} {form} fp32", got, ref, CHECKED, global_tol=float("inf"))


# defect -> (case, form, tensor): ordinary-family cases
NAMED = {
    "second_batch_first_edge_dropped": ("node_h64_d4", "node", "out"),
    "no_rescale_on_new_max": ("table_h32_d8_b5_v12", "table", "out"),
    "edge_term_unscaled": ("tile_h64_d4_n70", "tile", "out"),
    "value_edge_term_missing": ("rows_h128_d8_b9", "rows", "out"),
    "features_by_slot": ("graph_h16_d4_n128", "graph", "alpha"),
    "isolated_not_skip": ("scores_h32_d3_v16", "scores", "out"),
    "table_row_is_node": ("table_h256_d1_b3_v16", "table", "out"),
    "mask_numbered_at_table_row": ("drop_table_h64_d5_v16", "table", "out"),
    "weight_off_1e-4": ("graph_h64_d4_b1", "graph", "alpha"),
}


@pytest.mark.parametrize("defect", list(T.DEFECTS))
def test_every_defect_leaves_its_bound(defect):
    name, form, tensor = NAMED[defect]
    c = T.tconv_case(name)
    assert c.family == "ordinary"
    if defect == "table_row_is_node":
        assert c.V > c.n
    if defect == "mask_numbered_at_table_row":
        assert c.p == 0.5
    ref = T.host_reference(name, form)
    lookup = T.host_lookup(c, form)
    got = T._evaluate(c, torch.float64, defect=defect, lookup=lookup)
    f = T.compare(got[tensor], ref[tensor])
    print(f"{defect} on {name} {form} {tensor}: error/bound {f['ratio']:.3e}")
    assert not f["inside"] and f["ratio"] > 1.0, (defect, f)


@pytest.mark.parametrize("name,form", [(n, f) for n, cfg in T.CASES.items() if cfg["family"] == "ordinary" and not cfg.get("empty")
                                       for f in T.forms_of(n)])
def test_a_weight_off_by_1e_4_leaves_the_lookup_forms_bound(name, form):
    """Required of every ordinary case in the lookup forms, in a tensor the GPU test checks there: the denominator (scores,
    rows; ``qe = We^T q`` is an H-term dot in those kernels too, and its companion is most of the logit's bound at D = 8:
    ``out`` alone separates 1e-4 only at small D) or ``alpha`` (graph).  In the dot forms every figure is a record."""
    c = T.tconv_case(name)
    ref = T.host_reference(name, form)
    got = T._evaluate(c, torch.float64, defect="weight_off_1e-4", lookup=T.host_lookup(c, form))
    f = {k: T.compare(got[k], ref[k])["ratio"] for k in ("out", "denom", "alpha")}
    print(f"weight_off_1e-4 on {name} {form}: error/bound out {f['out']:.3e} denom {f['denom']:.3e} alpha {f['alpha']:.3e}")
    if form in T.LOOKUP_FORMS:
        assert f["alpha" if form == "graph" else "denom"] > 1.0, f


@pytest.mark.parametrize("name", list(T.PREPARE_CASES))
def test_prepare_reference_in_fp32_is_inside_its_bounds(name):
    pc = T.prepare_case(name)
    ref = T.prepare_reference(pc)
    sd = pc.state
    w4 = torch.cat([sd[f"{k}.weight"] for k in T._LINS], 0)
    b4 = torch.cat([sd[f"{k}.bias"] for k in T._LINS], 0)
    t4 = pc.table @ w4.t() + b4
    rs = 1.0 / pc.H ** 0.5
    got = dict(t4=t4, M=(t4[:pc.n, :pc.H] @ t4[:pc.n, pc.H:2 * pc.H].t()) * rs, P=(t4[:pc.n, :pc.H] @ sd["lin_edge.weight"]) * rs)
    T.check_all(f"prepare {name} fp32", got, ref, global_tol=float("inf"))
    bad = dict(got, M=got["M"] * pc.H ** 0.5)
    assert not T.compare(bad["M"], ref["M"])["inside"]


def test_end_to_end_references_exist_for_every_form():
    assert set(T.E2E) == set(T.FORMS)
    for form in T.FORMS:
        e = T.e2e_case(form)
        assert e.ref.shape == (e.case.N, e.case.H) and e.case.cfg["form"] == form and e.case.p == 0.0
