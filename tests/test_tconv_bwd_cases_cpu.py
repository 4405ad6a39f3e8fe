"""Host-side checks of tests/tconv_bwd_cases.py: the fp64 restatement of the backward equals autograd of the forward
restatement, every case plants its in-degree and out-degree classes, the same chain in fp32 stays inside every bound, and
every planted defect leaves the bound it is named with.  No GPU."""
import types

import pytest
import torch

import tconv_bwd_cases as Bw
import tconv_fwd_cases as T

STAGE = ("a", "da", "delta", "pds", "pal", "gq", "gk", "gv", "gskip")
PRODUCT = ("grad_qkvs", "gwe", "gea")
ROWS = ("ds", "gM", "gP", "gTs", "gTv", "gwe_g", "grad_qkvs_rows", "gwe_rows")


GRAPH = ("gM", "gP", "gTs", "gTv", "gwe_g", "grad_b", "gwe")


def _checked(form):
    if form == "graph":
        return GRAPH
    return STAGE + PRODUCT + (ROWS if form == "rows" else ())


@pytest.mark.parametrize("name", ["node_h16_d1", "table_h256_d1_b3_v16", "scores_h64_d4_v16", "tile_h32_d8_n5", "rows_h64_d4_b4",
                                  "drop_node_h32_d3", "drop_table_h64_d5_v16", "drop_rows_h128_d3_b9", "sharp_node_h64_d4",
                                  "sharp_scores_h64_d5_v16", "sharp_rows_h256_d1_b9", "graph_h64_d5_v16",
                                  "drop_graph_h32_d8_v16", "sharp_graph_h16_d4_n12"])
def test_restatement_equals_fp64_autograd(name):
    """``sum(out * g)`` of the forward restatement (tests/tconv_fwd_cases.py ``_evaluate``), differentiated by autograd with
    respect to ``qkvs``, ``w_edge`` and ``edge_attr`` in fp64, against the backward chain written out here."""
    base = Bw.bwd_case(name)
    leaves = [t.double().requires_grad_(True) for t in (base.qkvs, base.w_edge, base.edge_attr)]
    c = types.SimpleNamespace(**dict(vars(base), qkvs=leaves[0], w_edge=leaves[1], edge_attr=leaves[2]))
    fwd = T._evaluate(c, torch.float64)
    want = torch.autograd.grad((fwd["out"] * base.g.double()).sum(), leaves)
    stage = dict(m=fwd["m"].detach(), denom=fwd["denom"].detach(), y=fwd["out"].detach(), g=base.g)
    if c.cfg["form"] == "graph":          # the graph form's backward starts from the forward's weights and sum alpha ea
        stage.update(alpha=fwd["alpha"].detach(), aa=fwd["aa"].detach())
    with torch.no_grad():
        got = Bw._evaluate(c, torch.float64, stage)
        # the row form looks the dense part of the logit up in T_q T_k^T: the same chain.  (Not in the sharp rows case: its
        # logits reach 7e3 with |q| up to 2e4, and the fp64 rounding of the looked-up product alone moves grad_k by 1e-8.)
        scores = None
        if c.cfg["form"] == "rows" and c.family != "sharp":
            scores = leaves[0][:, :c.H] @ leaves[0][:, c.H:2 * c.H].t()
            got = Bw._evaluate(c, torch.float64, stage, scores=scores)
    for k, ref in zip(PRODUCT, (want[0], want[1], want[2])):
        err = float((got[k] - ref).abs().max() / ref.abs().max())
        print(f"{name} {k}: {err:.3e}")
        assert err <= 1e-12, (name, k, err)
    if scores is not None or c.cfg["form"] == "graph":
        # the row and graph forms' table-level sums give the same table gradient: grad T_q = rs (grad M T_k + grad P We^T), grad T_k = rs
        # grad M^T T_q (csrc/tconv_rows.hip, header)
        H, rs = c.H, 1.0 / c.H ** 0.5
        tq, tk = leaves[0][:c.n, :H].detach(), leaves[0][:c.n, H:2 * H].detach()
        g4 = torch.cat([rs * (got["gM"] @ tk + got["gP"] @ leaves[1].detach().t()), rs * (got["gM"].t() @ tq), got["gTv"],
                        got["gTs"]], 1)
        assert float((g4 - want[0][:c.n]).abs().max() / want[0].abs().max()) <= 1e-12
        assert bool((want[0][c.n:] == 0).all())


def test_widths_cover_every_h_and_d():
    for forms in (Bw.PER_DST_FORMS, ("graph",)):
        used = {(c["H"], c["D"]) for c in Bw.CASES.values() if c["form"] in forms}
        assert {h for h, _ in used} == {16, 32, 64, 128, 256} and {d for _, d in used} == {1, 3, 4, 5, 8}, forms
    assert {c["H"] for c in Bw.CASES.values() if c["form"] == "rows"} == {64, 128, 256}
    for form in Bw.FORMS:
        mine = [c for c in Bw.CASES.values() if c["form"] == form]
        assert any(c["p"] == 0.5 for c in mine) and any(c["family"] == "sharp" for c in mine), form
    # both modes of the per-destination kernels, one ordinary and one sharp case each
    for forms in (("node",), ("table", "scores", "tile")):
        fam = {c["family"] for c in Bw.CASES.values() if c["form"] in forms}
        assert fam == {"ordinary", "sharp"}


@pytest.mark.parametrize("name", list(Bw.CASES))
def test_case_table_plants_what_it_says(name):
    c = Bw.bwd_case(name)
    f = T.tconv_case(name) if name in T.CASES else T.build_case(name, Bw.CASES[name])
    b = T.bt(c.H)
    if c.cfg.get("empty"):
        assert c.E == 0
        return
    # what stays of the forward case: destinations (hence in-degrees), edge order, features, the self loops
    assert torch.equal(c.ei[1], f.ei[1]) and torch.equal(c.ix.deg, f.ix.deg) and torch.equal(c.edge_attr, f.edge_attr)
    loops = f.ei[0] == f.ei[1]
    assert bool(loops.any()) and torch.equal(c.ei[0][loops], f.ei[0][loops])
    assert not torch.equal(c.ix.eid, torch.arange(c.E))
    assert torch.unique(c.ei, dim=1).shape[1] < c.E                      # duplicates
    live = [d for d in T.degree_classes(c.H) if d <= int(c.ix.deg.max())]
    assert set(live[:5]) <= set(c.ix.deg.tolist())                       # the in-degrees around BT are the forward's
    # out-degrees: 0, 1, BT - 1, BT, BT + 1 and more than 2 BT, somewhere in the batch
    p = Bw.planted(c)
    assert {0, 1, b - 1, b, b + 1} <= p.outdeg, (name, p.outdeg)
    assert max(p.outdeg) > 2 * b
    # duplicates in a CSR row and in a CSC row
    assert p.one_source.numel() >= 1 and p.one_destination.numel() >= 1, name
    # the spread limits of the family
    spread = c.spread[c.ix.deg >= 2]
    print(f"{name}: E {c.E}  out-degrees up to {max(p.outdeg)}  spread {float(spread.min()):.2f} .. {float(spread.max()):.2f}")
    if c.family == "sharp":
        assert 40.0 <= float(spread.min()) and float(spread.max()) <= 60.0
    else:
        assert float(spread.max()) <= 16.0
    cfg = c.cfg
    if cfg.get("big"):
        assert int(torch.diff(c.batch.edge_ptr).max()) > 1024
    if cfg["form"] == "tile" or name == "tile_h64_d4_b33":
        assert c.B % T.rpb(c.H) == 1                                       # a ragged last group of graphs
    if name == "node_h256_d1_wedge":
        assert -(-c.N // T.rpb(c.H)) == 2 * Bw.WEDGE_GROUP + 1             # 257 workgroups: the two-level lin_edge sum


def _src_stage32(c, r64):
    """What the destination pass would leave for the source pass, as fp32 bits."""
    return dict(a=r64["a"].float(), da=r64["da"].float(), delta=r64["delta"].float(), gskip=r64["gskip"].float())


@pytest.mark.parametrize("name", list(Bw.CASES))
def test_fp32_restatement_is_inside_every_bound(name):
    c = Bw.bwd_case(name)
    form = c.cfg["form"]
    ref = Bw.host_reference(name)
    scores = Bw.host_scores(c) if form == "rows" else None
    got = Bw._evaluate(c, torch.float32, scores=scores)
    got.update(grad_qkvs_rows=got["grad_qkvs"], gwe_rows=got["gwe"], grad_b=got["grad_qkvs"][:c.n or c.N].sum(0))
    Bw.check_all(f"{name} fp32", got, ref, _checked(form), global_tol=float("inf"))
    if form == "graph":
        return
    # the source pass alone, from given bits
    src = _src_stage32(c, Bw._evaluate(c, torch.float64, scores=scores))
    ref_s = Bw.reference(c, form, scores=scores, src_stage=src)
    got_s = Bw._evaluate(c, torch.float32, scores=scores, src_stage=src)
    Bw.check_all(f"{name} fp32 source pass", got_s, ref_s, ("gk", "gv") + (("gTv",) if form == "rows" else ()), global_tol=float("inf"))


# defect -> (case, tensor): ordinary-family cases, tensors the GPU test checks
NAMED = {
    "delta_left_out": ("node_h64_d4", "pds"),
    "grad_k_unscaled": ("table_h32_d8_b5_v12", "grad_qkvs"),
    "grad_q_edge_term_unscaled": ("scores_h256_d5_v16", "grad_qkvs"),
    "da_edge_term_missing": ("node_h16_d1", "da"),
    "grad_w_edge_q_term_missing": ("table_h256_d1_b3_v16", "gwe"),
    "grad_w_edge_g_term_missing": ("node_h64_d4", "gwe"),
    "slope_from_sign_of_g": ("node_h16_d1", "gskip"),
    "mask_numbered_at_table_row": ("drop_table_h64_d5_v16", "gskip"),
    "features_by_slot": ("tile_h64_d4_b33", "pal"),
    "dst_edge_at_bt_dropped": ("node_h64_d4", "delta"),
    "src_edge_at_bt_dropped": ("tile_h64_d4_n70", "grad_qkvs"),
    "src_reads_escr_at_csc_slot": ("node_h32_d3", "gv"),
    "tile_last_group_dropped": ("tile_h64_d4_b33", "grad_qkvs"),
    "colf_is_node": ("table_h256_d1_b3_v16", "a"),
    "weight_off_1e-4": ("node_h64_d4", "a"),
}


@pytest.mark.parametrize("defect", list(Bw.DEFECTS))
def test_every_defect_leaves_its_bound(defect):
    name, tensor = NAMED[defect]
    c = Bw.bwd_case(name)
    assert c.family == "ordinary"
    if defect == "colf_is_node":
        assert c.V > c.n
    if defect == "mask_numbered_at_table_row":
        assert c.p == 0.5 and c.table_mode
    if defect in ("dst_edge_at_bt_dropped", "src_edge_at_bt_dropped"):
        assert int(c.ix.deg.max()) > T.bt(c.H) and int(c.csc.outdeg.max()) > T.bt(c.H)
    ref = Bw.host_reference(name)
    got = Bw._evaluate(c, torch.float64, defect=defect)
    f = Bw.compare(got[tensor], ref[tensor])
    print(f"{defect} on {name} {tensor}: error/bound {f['ratio']:.3e}")
    assert not f["inside"] and f["ratio"] > 1.0, (defect, f)


@pytest.mark.parametrize("name", [n for n, cfg in Bw.CASES.items() if cfg["family"] == "ordinary"])
def test_a_weight_off_by_1e_4_leaves_the_bound_of_the_weight_and_of_the_gradient(name):
    """Required of every ordinary case: the weight itself (``escr``, which the direct stage call checks) and ``grad_qkvs`` (what
    autograd returns) both separate a weight that is off by 1e-4; the other figures are a record.  (``gwe`` and ``gea`` do not:
    one weight of a destination moves a sum over all N destinations, or a row whose bound carries the H-term companions
    of ``We^T q`` and ``We^T g``, by less than their bounds.)"""
    c = Bw.bwd_case(name)
    form = c.cfg["form"]
    ref = Bw.host_reference(name)
    got = Bw._evaluate(c, torch.float64, defect="weight_off_1e-4", scores=Bw.host_scores(c) if form == "rows" else None)
    names = GRAPH[:5] if form == "graph" else ("a", "delta", "pal", "grad_qkvs", "gwe", "gea")
    f = {k: Bw.compare(got[k], ref[k])["ratio"] for k in names}
    print(f"weight_off_1e-4 on {name}: error/bound " + "  ".join(f"{k} {v:.3g}" for k, v in f.items()))
    if form == "graph":          # alpha is a stage input there: the weight is seen where it is used, in grad T_v
        assert c.cfg.get("empty") or f["gTv"] > 1.0, f
    else:
        assert f["a"] > 1.0 and f["grad_qkvs"] > 1.0, f


def test_global_figure_is_within_reach_of_fp32_wherever_the_gpu_test_asserts_it():
    """The same chain in fp32 on the CPU meets ``helpers.TOL`` for every tensor and case where the GPU test asserts it, and
    misses it in the sharp family for tensors of ``CANCELLING`` (which is why those are judged per element alone there)."""
    from helpers import TOL
    missed = {}
    for name, cfg in Bw.CASES.items():
        c = Bw.bwd_case(name)
        form = cfg["form"]
        ref = Bw.host_reference(name)
        got = Bw._evaluate(c, torch.float32, scores=Bw.host_scores(c) if form == "rows" else None)
        got.update(grad_qkvs_rows=got["grad_qkvs"], gwe_rows=got["gwe"], grad_b=got["grad_qkvs"][:c.n or c.N].sum(0))
        for k in _checked(form):
            glob = Bw.compare(got[k], ref[k])["glob"]
            if c.family == "sharp" and k in Bw.CANCELLING:
                if glob > TOL:
                    missed[(name, k)] = glob
            else:
                assert glob <= TOL, (name, k, glob)
    print({k: f"{v:.2e}" for k, v in missed.items()})
    assert ("sharp_rows_h256_d1_b9", "grad_qkvs") in missed and {n for n, _ in missed} >= {"sharp_node_h64_d4", "sharp_scores_h64_d5_v16"}
