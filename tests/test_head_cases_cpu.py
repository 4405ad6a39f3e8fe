"""Host-side checks of tests/head_cases.py, the cases and bounds tests/test_gpu_head.py holds the read-out kernels to:

  conditions   every case keeps every element at least 4 bounds away from the chain's three kinks, so that no element has to
               be left out of any comparison; both Huber branches, both signs of ``pre`` and of ``df`` occur; the planted
               graph sizes sit where the case tables say, and the trip cases make workgroups loop;
  restatement  the plain-tensor fp64 chain equals ``oracle.sparse.global_mean_pool`` -> the oracle's ``mlp`` with restated
               masks -> ``F.smooth_l1_loss`` through fp64 autograd, outputs and all gradients, to 1e-12;
  soundness    the same chain in torch float32 on the CPU stays inside ``k 2^-24 A`` on every case and every tensor (and,
               as a condition on the inputs, within a quarter of the global bar 1e-5 on the tensors the GPU test checks);
  sharpness    each planted defect of ``head_cases.DEFECTS`` in that float32 chain breaks the bound."""
import pytest
import torch
import torch.nn.functional as F

import head_cases as HC


def _sizes(c):
    return c.cnt.tolist()


# ------------------------------------------------------------------ conditions
@pytest.mark.parametrize("name", list(HC.CASES))
def test_every_element_is_far_from_every_kink(name):
    c = HC.head_case(name)
    m = HC.margins(c)
    worst = {k: float(v.min()) for k, v in m.items()}
    print(f"{name}: B {c.B} N {c.N} redraw rounds {c.rounds} margins {worst}")
    assert c.rounds < 32
    assert all(w >= HC.MARGIN for w in worst.values()), worst
    ref = HC.head_reference(c)
    quad, pre, df = ref["quad"], ref["pre"]["value"], ref["df"]["value"]
    assert bool(quad.any()) and bool((~quad).any())
    assert bool((pre > 0).any()) and bool((pre < 0).any())
    assert bool((df > 0).any()) and bool((df < 0).any())
    # the exact zeros among the node rows (slope at 0), also at kept positions of the fold
    assert bool(((c.x == 0) & c.in_keep).any())
    assert c.x.dtype == c.y.dtype == torch.float32 and c.N == int(c.ptr[-1]) < 100000


@pytest.mark.parametrize("name", list(HC.SMALL_CASES))
def test_small_cases_plant_what_the_table_says(name):
    c = HC.head_case(name)
    s = _sizes(c)
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129, 300} <= set(s) and 35 <= c.B <= 45
    assert s[0] == 0 and s[-1] == 0 and int(c.ptr[c.B - 1]) == int(c.ptr[c.B]) == c.N
    pairs = list(zip(s, s[1:]))
    assert (0, 0) in pairs and ((0, 300) in pairs or (300, 0) in pairs)
    GB = HC.graphs_per_pass(c.H)
    assert GB == 1 or c.B % GB != 0


def test_small_cases_cover_every_setting_at_every_width():
    for H in HC.WIDTHS:
        cs = [c for c in HC.SMALL_CASES.values() if c["H"] == H]
        assert {(c["O"], c["beta"]) for c in cs} == {(O, b) for O in (1, 3, 8) for b in (1.0, 0.25)}
        assert {(c["p"], c["fold"], c["in_p"]) for c in cs} == {(p, f, ip) for p in (0.0, 0.5)
                                                                 for f, ip in ((False, 0.0), (True, 0.0), (True, 0.5))}


@pytest.mark.parametrize("H", HC.WIDTHS)
def test_trip_cases_make_workgroups_loop(H):
    """B = GB (3 * 512) + GB + r: one pass into the fourth trip, with dead slots in the last pass (as the constants of
    csrc/head.hip stand; the GPU test asserts the same from the exported block counts)."""
    B, GB = HC.TRIP_B[H], HC.graphs_per_pass(H)
    assert B == {16: 24599, 32: 12299, 64: 6149, 128: 2051}[H]
    if GB > 1:
        assert B // GB == 3 * HC.HEAD_BLOCKS + 1 and 0 < B % GB < GB
    npass = -(-B // GB)
    for train, blocks in ((True, min(HC.HEAD_BLOCKS, npass)), (False, min(HC.HEAD_BLOCKS, B))):
        t = HC.trips(B, H, blocks, train)
        assert max(t.values()) >= 4 and len(set(t.values())) >= 2, (train, sorted(set(t.values())))
    seen = {}
    for v in range(4):
        c = HC.head_case(next(n for n, k in HC.TRIP_CASES.items() if k["H"] == H and k["variant"] == v))
        s = _sizes(c)
        assert set(s) <= {0, 1, 2, 3} | set(HC.BIG) and c.B == B
        for j, start in enumerate(HC.trip_places(H, B)):
            assert s[start] in HC.BIG, (v, start)
            seen.setdefault(j, set()).add(s[start])
    # every place has seen each of the four sizes (places that coincide at GB = 1 take the later place's size)
    places = HC.trip_places(H, B)
    for j, start in enumerate(places):
        if start not in places[j + 1:]:
            assert seen[j] == set(HC.BIG), (j, seen[j])


# ------------------------------------------------------------------ the restatement against fp64 autograd
def _autograd(c):
    from oracle import sparse as O
    f64 = torch.float64
    m = O.TopologicalGNN(num_nodes=2, hidden_channels=c.H, out_channels=c.O, edge_dim=1, dropout_p=c.p).double()
    with torch.no_grad():
        for p, v in ((m.mlp[0].weight, c.w0), (m.mlp[0].bias, c.b0), (m.mlp[3].weight, c.w3), (m.mlp[3].bias, c.b3)):
            p.copy_(v.double())
    m.mlp[1].negative_slope = HC._slope32(c.slope)
    x = c.x.double()
    res = {}
    if c.fold:
        # a pre-activation whose dropout(leaky_relu(.)) is x: the gradient asked for is the one wrt it
        s = HC._slope32(c.in_slope)
        z = (torch.where(x > 0, x, x / s) / float(c.in_ks)).requires_grad_(True)
        leaf = z
        x = F.leaky_relu(z, s) * c.in_keep.to(f64) * float(c.in_ks)
        assert float((x.detach() - c.x.double()).abs().max()) <= 1e-15 * float(c.x.abs().max())
    else:
        leaf = x.requires_grad_(True)
    pool = O.global_mean_pool(x, c.batch, c.B)
    h = m._drop(m.mlp[1](m.mlp[0](pool)), m.mlp[2], {"head": c.keep}, "head")
    out = m.mlp[3](h)
    loss = F.smooth_l1_loss(out, c.y.double(), beta=c.beta)
    go, = torch.autograd.grad(loss, out, retain_graph=True)
    gx, gw0, gb0, gw3, gb3 = torch.autograd.grad(loss, [leaf, m.mlp[0].weight, m.mlp[0].bias, m.mlp[3].weight,
                                                        m.mlp[3].bias])
    res.update(pool=pool, h=h, out=out, grad_out=go, loss=loss, gx=gx, gw0=gw0, gb0=gb0, gw3=gw3, gb3=gb3)
    if c.fold:
        res["gbias"] = gx.sum(0)
    return {k: v.detach() for k, v in res.items()}


@pytest.mark.parametrize("name", list(HC.SMALL_CASES) + [n for n, k in HC.TRIP_CASES.items() if k["H"] in (16, 128)
                                                          and k["variant"] == 1])
def test_restatement_equals_the_oracle_through_autograd(name):
    c = HC.head_case(name)
    assert 0 in _sizes(c)                       # empty graphs are part of it
    ref, auto = HC.head_reference(c), _autograd(c)
    worst = {}
    for k, v in auto.items():
        r = ref[k]["value"]
        worst[k] = float((v.reshape(r.shape) - r).abs().max()) / float(r.abs().max())       # on the tensor's own scale
    print(name, worst)
    assert all(w <= 1e-12 for w in worst.values()), worst
    assert abs(float(ref["loss_rows"]["value"].sum()) - float(auto["loss"])) <= 1e-12 * float(auto["loss"])


# ------------------------------------------------------------------ soundness and sharpness of the bound
@pytest.mark.parametrize("name", list(HC.CASES))
def test_float32_chain_stays_inside_the_bound(name):
    c = HC.head_case(name)
    ref = HC.head_reference(c)
    got = HC._evaluate(c, torch.float32)
    names = [k for k in ref if k != "quad"]
    assert set(HC.CHECKED) - {"gbias"} <= set(names) and (("gbias" in names) == c.fold)
    assert torch.equal(got["quad"], ref["quad"])
    # the global figure of the checked tensors is a property of the INPUTS here: grad_out = (out - y) / beta / (B O) on the
    # scale of 1 / (B O) carries out's rounding times 1 / beta, so a case is only fit for the GPU test's global bar of 1e-5
    # if plain float32 meets a quarter of it (else the case gets other inputs, never a wider bar)
    HC.check_all(name + " fp32", got, ref, names, global_tol=float("inf"))
    HC.check_all(name + " fp32 (conditioning)", got, ref, [k for k in names if k in HC.CHECKED], global_tol=HC.GLOBAL_TOL / 4)


# which case shows which defect (each is the first small case at H = 64 that can show it: the defect of the head's mask
# needs p > 0, the fold's slope a fold, the rest show on any case), and one tensor that breaks there
DEFECT_CASES = {
    "pool_skips_last_row": ("small_h64_o3_beta1.0_p0.0_nofold", "out"),
    "count_not_clamped": ("small_h64_o3_beta1.0_p0.0_nofold", "out"),
    "gw0_skips_graph": ("small_h64_o3_beta1.0_p0.0_nofold", "gw0"),
    "head_mask_shifted": ("small_h64_o8_beta0.25_p0.5_nofold", "out"),
    "fold_slope_at_zero": ("small_h64_o3_beta0.25_p0.0_fold0.0", "gx"),
    "inv_n_of_last_pass": ("small_h64_o3_beta1.0_p0.0_nofold", "grad_out"),
}


@pytest.mark.parametrize("defect", list(HC.DEFECTS))
def test_planted_defects_break_the_bound(defect):
    """``DEFECT_CASES`` names, for each defect, the small case that catches it and a tensor it breaks on.  Observed:
    a pool without the last of 300 rows breaks pool, h, out, loss_rows and gW0 (one part in 300 of one graph: the
    gradients behind a linear-branch graph do not move); the unclamped count turns everything of the empty graphs into
    NaN (grad_x has no row of theirs); a graph's term missing from gW0 breaks gW0 alone; the shifted mask breaks h and
    everything behind it; the fold's slope at y == 0 breaks grad_x and the bias gradient; the last pass's own 1 / (B O)
    breaks grad_out, the loss and every gradient that graph 40 (empty: pool 0, no row) takes part in."""
    assert set(DEFECT_CASES) == set(HC.DEFECTS)
    name, tensor = DEFECT_CASES[defect]
    c = HC.head_case(name)
    ref = HC.head_reference(c)
    got = HC._evaluate(c, torch.float32, defect)
    names = [k for k in ref if k != "quad"]
    broken = [k for k in names if not HC.compare(got[k], ref[k])["inside"]]
    print(f"{defect} on {name}: breaks {broken}")
    assert tensor in broken, (defect, name, broken)
    # and only the checked tensors count: at least one of those the GPU test sees must break
    assert set(broken) & set(HC.CHECKED), broken
