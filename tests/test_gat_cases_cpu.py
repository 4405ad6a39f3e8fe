"""Host-side checks of tests/gat_cases.py: the fp64 restatement agrees with the oracle's GATConv (forward and gradients), the
case table plants what it says, the same chain in fp32 stays inside every bound, and every planted defect leaves one.
No GPU."""
import types

import pytest
import torch

import gat_cases as G


# ------------------------------------------------------------------ the restatement is the operator
@pytest.mark.parametrize("C", G.WIDTHS)
def test_restatement_equals_the_oracle_in_fp64(C):
    """``oracle.sparse.GATConv`` in fp64 from the case's ``x`` and parameters: ``out`` and the gradients of ``lin.weight``,
    ``att_src``, ``att_dst`` and ``bias``, in both forms (dense: ``z`` and the logits taken from the oracle's projection,
    ``grad_lin = grad_z^T x``).  The oracle's slope is the double 0.2."""
    from oracle import sparse as O
    base = G.gat_case(f"degrees_c{C}")
    conv = O.GATConv(base.K, C, heads=G.HEADS).double()
    with torch.no_grad():
        conv.lin.weight.copy_(base.w.double())
        conv.att_src.copy_(base.att_src.double()[None])
        conv.att_dst.copy_(base.att_dst.double()[None])
        conv.bias.copy_(base.bias.double())
    x = base.x.double()
    out = conv(x, base.ei)
    (out * base.g.double()).sum().backward()
    z = (x @ base.w.double().t()).detach()
    z3 = z.view(base.N, G.HEADS, C)
    logits = ((z3 * base.att_src.double()).sum(-1), (z3 * base.att_dst.double()).sum(-1))
    want = dict(out=out.detach(), grad_lin=conv.lin.weight.grad, grad_att_src=conv.att_src.grad[0],
                grad_att_dst=conv.att_dst.grad[0], grad_bias=conv.bias.grad)
    for form in G.FORMS:
        c = types.SimpleNamespace(**dict(vars(base), z=z))
        got = G._evaluate(c, torch.float64, form=form, logits=logits, ns=0.2, pin=False)
        if form == "dense":
            got["grad_lin"] = got["grad_z"].t() @ x
        for k, ref in want.items():
            err = float((got[k] - ref).abs().max()) / float(ref.abs().max())
            print(f"c{C} {form} {k}: {err:.3e}")
            assert err <= 1e-12, (form, k, err)


def test_host_logit_is_the_restatements_logit():
    """``s`` as the kernels form it in fp32 is what ``_evaluate`` pins in every dtype, and ``m`` follows bit for bit."""
    c = G.gat_case("logits_c16")
    _, s32 = G.host_logit(c)
    for dtype in (torch.float32, torch.float64):
        r = G._evaluate(c, dtype, backward=False)
        m = torch.full((c.N, G.HEADS), -float("inf")).scatter_reduce(0, c.ix.row[:, None].expand(-1, G.HEADS), s32, "amax")
        assert torch.equal(r["m"].float(), m)


# ------------------------------------------------------------------ the table plants what it says
def test_widths_and_forms_are_covered():
    for fam in ("degrees", "logits", "walk"):
        assert {cfg["C"] for cfg in G.CASES.values() if cfg["family"] == fam} == set(G.WIDTHS), fam
    pairs = {(cfg["C"], cfg["kind"]) for cfg in G.CASES.values() if cfg["family"] == "walk" and not cfg.get("holes")}
    assert pairs == {(4, "chain"), (16, "band"), (32, "chain"), (64, "hubs"), (128, "chain"), (256, "chain"), (128, "shuffled_chain")}
    assert {G.eb(C) for C in G.WIDTHS} == {2, 3} and {G.lph(C) for C in G.WIDTHS} == {1, 2, 4, 8, 16, 32, 64}
    assert {cfg["K"] for cfg in G.CASES.values() if "thin" in cfg["forms"]} == {1, 5, 6, 8}
    # the largest K at C = 256: static and dynamic LDS add up to exactly 64 KB
    assert G.thin_fits(256, 6) and not G.thin_fits(256, 7)
    assert G.rpb(256) * G.eb(256) * 1024 * 4 + G.eb(256) * G.nv(256) * 256 * 4 + 6 * 1024 * 4 == 64 * 1024
    for name, cfg in G.CASES.items():
        assert cfg["forms"], name
        if cfg["family"] in ("degrees", "walk", "empty") and cfg["K"] == 5:
            assert cfg["forms"] == G.FORMS, name


@pytest.mark.parametrize("name", [n for n, cfg in G.CASES.items() if cfg["family"] == "degrees"])
def test_degrees_family_plants_its_degrees(name):
    c = G.gat_case(name)
    ix, deg = c.ix, c.ix.deg.tolist()
    src_of = lambda i: ix.col[ix.rowptr[i]:ix.rowptr[i + 1]].tolist()
    left, mid, right, shared = G.SHARED
    if c.loops:
        # one self loop more everywhere; the input's two self loops of node 17 are dropped for the inserted one
        assert deg == [d + 1 if i != 17 else 2 for i, d in enumerate(G.DEGS)]
        assert all(src_of(i)[-1] == i for i in range(c.N)) and src_of(17) == [6, 17]
        assert [i for i in range(c.N) if deg[i] == 1] == list(G.ISOLATED)          # the self loop is their only in-edge
    else:
        assert deg == list(G.DEGS) and set(range(10)) <= set(deg)
        assert [i for i in range(c.N) if deg[i] == 0] == list(G.ISOLATED)
        assert G.ISOLATED[0] == 0 and G.ISOLATED[-1] == c.N - 1 and G.ISOLATED[2] == G.ISOLATED[1] + 1
        assert src_of(17) == [17, 17, 6] and deg[mid] == 0
    assert src_of(15)[:2] == [5, 5]
    # the isolated destination sits between two that share a source, and their first sources differ
    assert shared in src_of(left) and shared in src_of(right) and src_of(left)[0] != src_of(right)[0]
    # every raggedness of the last batch at this width's EB, and the wide destinations' planted positions
    assert {d % G.eb(c.C) for d in deg} == set(range(G.eb(c.C)))
    for wide in (14, 16):
        assert deg[wide] > 40 and src_of(wide)[2] == src_of(wide)[3] == G.STRONG
    assert not torch.equal(ix.eid, torch.arange(c.E))            # the input is not sorted by destination
    if "dense" in c.cfg["forms"]:
        assert int((c.a_src >= c.a_src[G.STRONG]).sum()) == G.HEADS          # the largest logit of every head


@pytest.mark.parametrize("C", G.WIDTHS)
def test_logits_family_plants_its_orders(C):
    c = G.gat_case(f"logits_c{C}")
    ref = G.host_reference(c.name, "dense")
    raw, s = G.host_logit(c)
    seen = set()
    for d, pat, leaves in c.plan:
        L = len(leaves)
        a, b = int(c.ix.rowptr[d]), int(c.ix.rowptr[d + 1])
        assert b - a == L + 1 and c.ix.col[a:b].tolist() == leaves + [d]
        sd, rd, nrec = s[a:b].double(), raw[a:b], ref["nrec"][d]
        seen.add(pat)
        if pat == "increasing":
            assert bool((sd[1:] > sd[:-1]).all()) and nrec.tolist() == [L] * G.HEADS          # every edge a new maximum
        elif pat == "decreasing":
            assert bool((sd[1:] < sd[:-1]).all()) and nrec.tolist() == [0] * G.HEADS
        elif pat == "equal":
            assert bool((sd == sd[0]).all()) and nrec.tolist() == [0] * G.HEADS
        elif pat == "one_low":
            gap = torch.cat([sd[:1], sd[2:]]).min(0).values - sd[1]
            assert bool((gap >= 59.9).all()) and bool((gap <= 61.0).all()) and nrec.tolist() == [L - 1] * G.HEADS
        elif pat == "straddle":
            assert bool((rd > 0).any(0).all()) and bool((rd < 0).any(0).all())
            assert nrec.tolist() == [2 if L == 7 else 1] * G.HEADS
        elif pat == "heads":
            m = ref["m"]["value"][d]
            assert 75.0 <= float(m.max() - m.min()) <= 85.0
    assert seen == set(G.PATTERNS)


@pytest.mark.parametrize("name", G.WALK)
def test_walk_cases_walk(name):
    """At the host's stand-in: N as the formula says, several destinations per lane group even where the grid is at
    ``min(8 CUs, 2048)``, and what the chain is there for."""
    c = G.gat_case(name)
    C, ix = c.C, c.ix
    cap = min(8 * G.TRIP_CUS, 2048)
    assert c.N == 3 * cap * G.rpb(C) + G.rpb(C) + 1
    chunk = -(-(-(-c.N // cap)) // G.rpb(C)) * G.rpb(C)
    assert chunk // G.rpb(C) == G.HOST_RUN >= 3
    places = G.walk_places(ix, C, G.HOST_RUN)
    src_of = lambda i: set(ix.col[ix.rowptr[i]:ix.rowptr[i + 1]].tolist())
    if c.cfg["kind"] == "chain" and not c.cfg.get("holes"):
        assert all(src_of(i) & src_of(i + 1) for i in range(c.N - 1))          # consecutive destinations share a source
        assert int(places["prefetched"].sum()) >= c.N // 2
        # (EB = 2: the first batches (i - 1, i + 1) and (i, i + 2) share nothing; the holes case puts the self loops first)
        assert int(places["cached"].sum()) >= (c.N if G.eb(C) == 3 else 0)
    if c.cfg["kind"] == "shuffled_chain":
        assert int(places["cached"].sum()) < c.N // 8                       # plain loads nearly everywhere
    if c.cfg.get("holes"):
        deg = ix.deg.tolist()
        inside = [i for i in range(1, c.N - 1) if deg[i] == 0 and deg[i - 1] and deg[i + 1]
                  and (i - 1) // G.HOST_RUN == (i + 1) // G.HOST_RUN and src_of(i - 1) & src_of(i + 1)]
        pairs = [i for i in range(1, c.N - 2) if deg[i] == 0 and deg[i + 1] == 0 and (i - 1) // G.HOST_RUN == (i + 2) // G.HOST_RUN]
        assert inside and pairs and deg[0] == 0 and deg[-1] == 0
        assert int(places["cached"].sum()) >= c.N // 4 and int(places["prefetched"].sum()) >= c.N // 4


# ------------------------------------------------------------------ the bounds hold for fp32, and are sharp
@pytest.mark.parametrize("name,form", G.RUNS)
def test_fp32_restatement_is_inside_every_bound(name, form):
    """A condition on the bounds, not a measurement: the same chain in fp32 on the host."""
    c = G.gat_case(name)
    ref = G.host_reference(name, form)
    got = G._evaluate(c, torch.float32, form=form)
    G.check_all(f"{name} {form} fp32", got, ref, G.CHECKED[form] + (("alpha",) if c.E else ()), global_tol=float("inf"))


def test_logit_bounds_hold_for_fp32():
    for C in G.WIDTHS:
        c = G.gat_case(f"degrees_c{C}")
        z3 = c.z.view(c.N, G.HEADS, C)
        got = dict(a_src=(z3 * c.att_src).sum(-1), a_dst=(z3 * c.att_dst).sum(-1))
        G.check_all(f"logits c{C} fp32", got, G.logits_reference(c), global_tol=float("inf"))
        a_s, a_d = G.host_thin_logits(c)
        G.check_all(f"thin logits c{C} fp32", dict(a_src=a_s, a_dst=a_d), G.thin_logits_reference(c), global_tol=float("inf"))
        bad = dict(a_src=got["a_src"] * (1 + 1e-5), a_dst=got["a_dst"])
        assert not G.compare(bad["a_src"], G.logits_reference(c)["a_src"])["inside"]


def _worst(name, form, defect):
    c = G.gat_case(name)
    ref = G.host_reference(name, form)
    got = G._evaluate(c, torch.float64, defect=defect, form=form)
    return {k: G.compare(got[k], ref[k])["ratio"] for k in G.CHECKED[form]}


# defect -> (small case, form)
NAMED = {
    "ragged_tail_slot_accumulated": ("degrees_c64", "dense"),
    "second_batch_first_edge_dropped": ("degrees_c256", "dense"),
    "no_rescale_on_new_max": ("logits_c32", "dense"),
    "self_loop_missing": ("degrees_c8", "thin"),
    "slope_on_the_positive_side": ("logits_c4", "dense"),
    "bias_inside_the_normalisation": ("degrees_c16", "dense"),
    "isolated_not_bias": ("degrees_noloop_c128", "dense"),
    "thin_w_untransposed": ("thin_c256_k6", "thin"),
    "weight_off_1e-4": ("degrees_c32", "thin"),
    "delta_not_subtracted": ("degrees_c4", "dense"),
    "logit_gradient_not_returned_to_grad_z": ("degrees_c128", "thin"),
    "stale_row_after_empty_destination": ("degrees_noloop_c16", "dense"),
    # the LDS image and the prefetch serve nothing where a lane group walks one destination: walk cases (small on the host)
    "cached_logit_of_head0": ("walk_c32_chain", "dense"),
    "prefetch_one_destination_late": ("walk_c256_chain", "thin"),
}
WALK_NAMED = [("cached_logit_of_head0", "walk_c4_chain", "thin"), ("cached_logit_of_head0", "walk_c32_chain", "thin"),
              ("cached_logit_of_head0", "walk_c256_chain_holes", "dense"), ("prefetch_one_destination_late", "walk_c128_chain", "dense"),
              ("prefetch_one_destination_late", "walk_c64_hubs", "dense"),
              ("stale_row_after_empty_destination", "walk_c8_chain_holes", "dense"),
              ("stale_row_after_empty_destination", "walk_c256_chain_holes", "thin")]


@pytest.mark.parametrize("defect", list(G.DEFECTS))
def test_every_defect_leaves_its_bound(defect):
    name, form = NAMED[defect]
    f = _worst(name, form, defect)
    print(f"{defect} on {name} {form}: error/bound " + "  ".join(f"{k} {v:.3e}" for k, v in f.items()))
    assert max(f.values()) > 1.0, (defect, f)


@pytest.mark.parametrize("defect,name,form", WALK_NAMED)
def test_cache_and_prefetch_defects_leave_a_walk_cases_bound(defect, name, form):
    assert defect in G.WALK_DEFECTS and name in G.WALK
    f = _worst(name, form, defect)
    print(f"{defect} on {name} {form}: error/bound " + "  ".join(f"{k} {v:.3e}" for k, v in f.items()))
    assert max(f["out"], f["denom"]) > 1.0, (defect, f)


@pytest.mark.parametrize("name,form", [(n, f) for n in G.ORDINARY for f in G.CASES[n]["forms"]])
def test_a_weight_off_by_1e_4_leaves_the_bound_of_denom_or_out(name, form):
    """The sharpness requirement, on every ordinary small case."""
    f = _worst(name, form, "weight_off_1e-4")
    print(f"weight_off_1e-4 on {name} {form}: error/bound out {f['out']:.3e} denom {f['denom']:.3e}")
    assert max(f["out"], f["denom"]) > 1.0, f
