"""Host-side checks of tests/bn_cases.py, the cases and bounds tests/test_gpu_bn.py holds the BatchNorm kernels to:

  restatement  the plain-tensor fp64 chain equals ``F.batch_norm`` (+ ``relu``, + the next projection) through fp64 autograd:
               output, running statistics after two steps and every gradient, dense and rows form, to 1e-12;
  conditions   every element is at least 4 bounds from the ReLU kink after fewer than 32 rounds, no element of the ordinary
               data lies beyond Z = 4 sigma (the contract of the variance bound rests on it), the table plants the shapes,
               families, twins and chunkings it says;
  soundness    the same chain in torch float32 on the CPU, with centred (two-pass) statistics, stays inside ``k 2^-24 A`` on
               every case and every tensor, the outlier-first cases included: the bounds are attainable in fp32;
  sharpness    each planted defect of ``bn_cases.DEFECTS`` in that float32 chain breaks a named tensor in a named case."""
import pytest
import torch
import torch.nn.functional as F

import bn_cases as BC

ROWS_CASES = ["n65_c128_train_relu", "n129_c516_train_lin", "n64_c20_train_relu", "n4099_c128_eval_relu", "n129_c344_eval_lin",
              "outlier_n4099_c128"]


# ------------------------------------------------------------------ the restatement against fp64 autograd
def _autograd(c, rows=None):
    f64 = torch.float64
    x = c.x.double().requires_grad_(True)
    w, b = c.w.double().requires_grad_(True), c.b.double().requires_grad_(True)
    rm, rv = c.rm0.double().clone(), c.rv0.double().clone()
    y = F.batch_norm(x, rm, rv, w, b, c.training, BC.MOMENTUM, BC.EPS)
    for _ in range(c.steps - 1):
        with torch.no_grad():
            F.batch_norm(x, rm, rv, w, b, c.training, BC.MOMENTUM, BC.EPS)
    if c.relu:
        y = F.relu(y)
    res = dict(y=y)
    leaves = [x, w, b]
    if c.cfg["kind"] == "fold":
        lin = c.lin.double().requires_grad_(True)
        leaves.append(lin)
        out, g = y @ lin.t(), c.gz.double()
        res["z"] = out
    else:
        out, g = y, c.g.double()
        if rows is not None:
            keep = torch.zeros(c.N, 1, dtype=f64)
            keep[BC.rows_index(c, rows)] = 1
            g = g * keep
    grads = torch.autograd.grad(out, leaves, g)
    res.update(grad_x=grads[0], grad_weight=grads[1], grad_bias=grads[2])
    if c.cfg["kind"] == "fold":
        res["grad_lin"] = grads[3]
    if c.training:
        res.update(running_mean=rm, running_var=rv)
    return {k: v.detach() for k, v in res.items()}


def _same_as_autograd(name, rows=None):
    c = BC.bn_case(name)
    ref, auto = BC.bn_reference(name, rows), _autograd(c, rows)
    worst = {}
    for k, v in auto.items():
        r = ref[k]["value"]
        scale = float(r.abs().max())
        worst[k] = float((v.reshape(r.shape) - r).abs().max()) / (scale if scale > 0 else 1.0)
    print(name, rows, worst)
    assert all(e <= 1e-12 for e in worst.values()), worst


@pytest.mark.parametrize("name", [n for n, k in BC.ALL_CASES.items() if k["kind"] != "outlier"])
def test_restatement_equals_batch_norm_through_autograd(name):
    _same_as_autograd(name)


@pytest.mark.parametrize("name", ROWS_CASES)
def test_rows_form_restatement_equals_autograd_with_a_zero_filled_gradient(name):
    c = BC.bn_case(name)
    for n in BC.rows_counts(c.N):
        _same_as_autograd(name, n)


# ------------------------------------------------------------------ conditions
@pytest.mark.parametrize("name", list(BC.ALL_CASES))
def test_every_element_is_far_from_the_kink_and_within_z(name):
    c = BC.bn_case(name)
    m = BC.margins(name)
    z = BC.max_z(name)
    print(f"{name}: N {c.N} C {c.C} nudge rounds {c.rounds} worst margin {float(m.min()):.3g} max z {z:.3f}")
    assert c.rounds < 32
    assert float(m.min()) >= BC.MARGIN
    if c.training:              # (eval mode normalises with the running statistics: no contract on the batch's own)
        assert z <= BC.Z
    mask = BC.bn_reference(name)["mask"]
    if c.relu and c.N > 3:
        assert bool(mask.any()) and bool((~mask).any())
        assert not bool(mask[:, c.C - 1].any())            # the dead column: y = 0 exactly, mask off
    assert c.x.dtype == c.g.dtype == torch.float32 and c.x.shape == (c.N, c.C)


def test_case_table_plants_what_it_says():
    ns, cs = {}, {}
    for k in BC.CASES.values():
        if k["kind"] == "typical":
            ns.setdefault(k["N"], set()).add(k["C"])
            cs.setdefault(k["C"], set()).add(k["N"])
    assert set(ns) == {2, 3, 63, 64, 65, 129, 4099, 131073} and set(cs) == {4, 20, 128, 344, 516, 1024}
    assert ns.pop(131073) == {20}
    assert all(len(v) >= 2 for v in ns.values()) and all(len(v) >= 3 for v in cs.values())
    # what each width pins: (RPB, idle threads)
    for C, (rpb, idle) in {4: (256, 0), 20: (51, 1), 128: (8, 0), 344: (2, 84), 516: (1, 127), 1024: (1, 0)}.items():
        assert BC.chunking(64, C)[2] == rpb and 256 - rpb * (C // 4) == idle
    # N = 65: a second workgroup with a shorter chunk; 129, 4099: ragged chunks
    assert BC.chunking(64, 4)[:2] == (1, 64) and BC.chunking(65, 4)[:2] == (2, 33) and BC.chunking(63, 4)[:2] == (1, 63)
    assert BC.chunking(129, 4)[:2] == (3, 43) and BC.chunking(4099, 4)[:2] == (65, 64)
    # the grid capped at 2048, chunk 65 > RPB = 51 (a second trip), trailing workgroups empty
    nblk, chunk, rpb = BC.chunking(131073, 20)
    assert (nblk, chunk, rpb) == (2048, 65, 51) and -(-131073 // chunk) < nblk
    settings = {(k["training"], k["relu"]) for k in BC.CASES.values()}
    assert settings == {(True, True), (True, False), (False, True), (False, False)}
    for name, k in BC.CASES.items():
        c = BC.bn_case(name)
        assert c.steps == 2 and bool((c.rm0 != 0).all()) and bool((c.rv0 != 1).all())
        assert bool((c.w[:-1].abs() >= 0.75).all()) and bool((c.b[:-1].abs() >= 0.25).all()) and c.w[-1] == 0 == c.b[-1]
        fams = {BC.family(j) for j in range(c.C)}
        assert fams == {"ordinary", "offset", "constant", "tiny"}
        if c.training:
            ref = BC.bn_reference(name)
            const = [j for j in range(c.C) if BC.family(j) == "constant"]
            assert bool((ref["var"]["value"][const] == 0).all())
            assert bool((ref["rstd"]["value"][const] == 1.0 / torch.sqrt(torch.tensor(BC.EPS, dtype=torch.float64))).all())


@pytest.mark.parametrize("name", [n for n, k in BC.CASES.items() if k["kind"] == "outlier"])
def test_outlier_first_cases_are_row_swaps_of_their_twins(name):
    c, t = BC.bn_case(name), BC.bn_case(BC.CASES[name]["twin"])
    assert torch.equal(c.x[0], t.x[1]) and torch.equal(c.x[1], t.x[0]) and torch.equal(c.x[2:], t.x[2:])
    assert torch.equal(c.g[0], t.g[1]) and torch.equal(c.g[2:], t.g[2:])
    ref, tref = BC.bn_reference(name), BC.bn_reference(t.name)
    for s in BC.STATS:
        assert ref[s] is tref[s]
    # row 0 sits at the level the table says, in units of the other rows' sigma
    rest = c.x[1:].double()
    lv = (c.x[0].double() - rest.mean(0)).abs() / rest.std(0, unbiased=False).clamp_min(1e-300)
    cols = [j for j in range(c.C) if BC.family(j) == "ordinary"]
    seen = set()
    for j in cols:
        want = BC.outlier_level(c.cfg, j)
        assert 0.5 * want <= float(lv[j]) <= 2 * want, (j, float(lv[j]), want)
        seen.add(want)
    assert seen == set(BC.LEVELS) or c.C < 12
    # and the y / grad_x references are the twin's with the rows swapped back
    assert torch.allclose(ref["y"]["value"][0], tref["y"]["value"][1], rtol=1e-12, atol=0)


def test_all_three_outlier_levels_occur():
    seen = set()
    for name, k in BC.CASES.items():
        if k["kind"] == "outlier":
            seen |= {BC.outlier_level(k, j) for j in range(k["C"]) if BC.family(j) == "ordinary"}
    assert seen == set(BC.LEVELS)
    assert BC.outlier_level(BC.CASES["outlier_n65_c4"], 0) == 1e4


# ------------------------------------------------------------------ soundness and sharpness of the bound
def _names(c, ref):
    return [k for k in ref if k not in ("mask", "idx")]


@pytest.mark.parametrize("name", list(BC.ALL_CASES))
def test_float32_chain_with_centred_statistics_stays_inside_the_bound(name):
    c = BC.bn_case(name)
    ref = BC.bn_reference(name)
    got = BC._evaluate(c, torch.float32)
    names = _names(c, ref)
    assert set(BC.FOLD_CHECKED if c.cfg["kind"] == "fold" else BC.CHECKED) - (set() if c.training else {"running_mean", "running_var"}) <= set(names)
    assert torch.equal(got["mask"], ref["mask"])
    BC.check_all(name + " fp32", got, ref, names, global_tol=float("inf"))


@pytest.mark.parametrize("name", ROWS_CASES)
def test_float32_rows_form_stays_inside_the_bound(name):
    c = BC.bn_case(name)
    for n in BC.rows_counts(c.N):
        ref = BC.bn_reference(name, n)
        got = BC._evaluate(c, torch.float32, rows=n)
        BC.check_all(f"{name} rows {n} fp32", got, ref, _names(c, ref), global_tol=float("inf"))


# which case shows which defect, and a tensor that breaks there (rows: the rows form with that many consumed rows)
DEFECT_CASES = {
    "chunk_last_row_skipped": ("n4099_c516_train_relu", None, "mean"),
    "running_var_biased": ("n65_c128_train_relu", None, "running_var"),
    "rows_inv_n_consumed": ("n65_c128_train_relu", 6, "grad_x"),
    "relu_mask_at_zero": ("n65_c128_train_relu", None, "grad_bias"),
    "partial_from_neighbour": ("n65_c128_train_relu", None, "mean"),
    "variance_not_clamped": ("n4099_c516_train_relu", None, "rstd"),
}


@pytest.mark.parametrize("defect", list(BC.DEFECTS))
def test_planted_defects_break_the_bound(defect):
    assert set(DEFECT_CASES) == set(BC.DEFECTS)
    name, rows, tensor = DEFECT_CASES[defect]
    c = BC.bn_case(name)
    ref = BC.bn_reference(name, rows)
    got = BC._evaluate(c, torch.float32, defect, rows=rows)
    clean = BC._evaluate(c, torch.float32, rows=rows)
    names = _names(c, ref)
    assert all(BC.compare(clean[k], ref[k])["inside"] for k in names)
    broken = [k for k in names if not BC.compare(got[k], ref[k])["inside"]]
    print(f"{defect} on {name}: breaks {broken}")
    assert tensor in broken, (defect, name, broken)
    assert set(broken) & set(BC.CHECKED), broken
    if defect == "variance_not_clamped":        # the clamp is what the constant columns need: a negative variance there
        const = [j for j in range(c.C) if BC.family(j) == "constant"]
        assert bool((got["var"][const] < 0).any())


# ------------------------------------------------------------------ the inputs of the partials path
@pytest.mark.parametrize("HC", BC.GAT_WIDTHS)
def test_partials_inputs_keep_the_contract(HC):
    """No element beyond Z sigma (the planted rows aside), an outlier every 1000th row of the ordinary columns, and the lane
    groups' runs as ``gat_chain`` counts them for a grid of 1024 workgroups."""
    N = 2049
    for fam in ("ordinary", "offset", "outlier"):
        x = BC.partials_input(N, HC, fam).double()
        assert x.shape == (N, HC)
        mean = x.mean(0)
        sigma = ((x - mean) ** 2).mean(0).sqrt()
        dev = (x - mean).abs()
        if fam == "outlier":
            plain = BC.partials_input(N, HC, "offset").double()
            moved = (x != plain)
            cols = torch.tensor([BC.family(j) == "ordinary" for j in range(HC)])
            assert torch.equal(moved.any(1).nonzero().view(-1), torch.tensor([999, 1999]))
            assert torch.equal(moved[999], cols) and torch.equal(moved[1999], cols)
            assert bool(((x - plain)[999, cols] / plain[:, cols].std(0) >= 50).all())
            dev[moved] = 0
        assert bool((dev <= BC.Z * sigma).all())
    rpb = BC.gat_lanes(HC)[1]
    assert rpb == {16: 64, 128: 8, 1024: 4}[HC]
    for n, run in ((37, 1), (1024 * rpb + 1, 2), (2 * 1024 * rpb + 1, 3)):
        assert BC.gat_chain(n, HC, min(1024, -(-n // rpb)))[0] == run
