"""GPU: K candidate lightpaths scored in one launch (``LightpathPredictor.what_if`` / ``qot_lightpath_infer_whatif``).

The call is DEFINED through ``infer.materialise_lightpath_what_if``: ``out[k]`` is the row of ``predict(batch)`` that belongs
to the candidate's node in the explicitly built batch, and the kernel runs ``predict``'s own row code with the same sums in
the same order, so the comparison is ``torch.equal``: there is no tolerance to choose.  Beside it, the oracle's and the
engine's eval forward of the materialised batch at the suite's ``TOL``.  The candidates are
``infer_lightpath_whatif_cases.CANDIDATES`` (44 on the 16 graphs of the mixed batch, one call).  What is computed once per
shape -- models, predictor, the materialised batch and its rows -- is shared by the tests and only read."""
import functools

import pytest
import torch

import gnn_qot_estimation_amd as q
import infer_lightpath_whatif_cases as WC
from gnn_qot_estimation_amd import _lib, infer
from helpers import TOL, rel_err

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _setup(C, F, O, lut, device):
    ref = WC.oracle_model(F, C, O, lut)
    hip = WC.engine_model(ref, device)
    pred = q.LightpathPredictor(hip)
    w = WC.build(F, lut)
    data, kw = WC.args(w, device)
    mat, node_new = infer.materialise_lightpath_what_if(data, lut, **kw)
    rows = torch.searchsorted(hip._lut_rows(mat), node_new)
    assert torch.equal(hip._lut_rows(mat)[rows], node_new)
    return ref, hip, pred, w, data, mat, rows, pred(mat)[0][rows]


def _call(pred, w, device, data=None, **over):
    data, kw = WC.args(w, device, data)
    return pred.what_if(data, **{**kw, **over})


@pytest.mark.parametrize("C,F,O,lut", WC.SHAPES)
def test_what_if_is_predicts_row_of_the_materialised_batch_bit_for_bit(cuda_device, C, F, O, lut):
    ref, hip, pred, w, data, mat, rows, want = _setup(C, F, O, lut, cuda_device)
    out, lb = _call(pred, w, cuda_device, data)
    pred.check_status()
    K = len(w.cands)
    assert tuple(out.shape) == (K, O) and out.dtype == torch.float32 and out.grad_fn is None and not out.requires_grad
    assert out.device == want.device and bool(torch.isfinite(out).all())
    for k, c in enumerate(w.cands):
        assert torch.equal(out[k], want[k]), (k, c.name)
    assert torch.equal(lb, data.batch[w.node.to(cuda_device)]) and lb.dtype == torch.int64
    again, lb2 = _call(pred, w, cuda_device, data)                          # reproducible
    assert torch.equal(out, again) and torch.equal(lb, lb2)
    # the edits matter: the rows of the 150-star's hub (no edit, features, 63 / 64 / 65 additions, 32 removals ...) differ
    hub = WC.PTR[WC.STAR150]
    rows_of_hub = {tuple(out[k].tolist()) for k in range(K) if int(w.node[k]) == hub}
    assert len(rows_of_hub) >= 6, len(rows_of_hub)
    # what the cases call the same graph is the same row; a dropped or added message is another
    same = lambda a, b: torch.equal(out[WC.index(a)], out[WC.index(b)])    # noqa: E731
    no_edit = [c.name for c in w.cands].index("no edit") + WC.LUT_ROWS.index(WC.PTR[WC.TRIPLE])
    for name in ("add: the node itself", "drop: no message"):
        assert torch.equal(out[WC.index(name)], out[no_edit]), name
    for name in ("add: a sender again", "drop: a message", "drop: every message"):
        assert not torch.equal(out[WC.index(name)], out[no_edit]), name
    assert not same("drop: offset 0 of 64", "drop: offset 63 of 64")
    # pointer arrays handed over as device tensors (one read each) give the same launch
    dev = lambda v: torch.tensor(v, device=cuda_device)                    # noqa: E731
    out_d, lb_d = _call(pred, w, cuda_device, data, add_ptr=dev(w.add_ptr), drop_ptr=dev(w.drop_ptr))
    assert torch.equal(out_d, out) and torch.equal(lb_d, lb)
    pred.check_status()


@pytest.mark.parametrize("C,F,O,lut", WC.SHAPES)
def test_what_if_matches_the_oracle_and_the_engine_on_the_materialised_batch(cuda_device, C, F, O, lut):
    ref, hip, pred, w, data, mat, rows, _ = _setup(C, F, O, lut, cuda_device)
    out, _ = _call(pred, w, cuda_device, data)
    pred.check_status()
    with torch.no_grad():
        oracle = ref(mat.to("cpu"))[0][rows.cpu()]
        own = hip(mat)[0][rows]
    e_or, e_en = rel_err(out, oracle), rel_err(out, own)
    print(f"C {C} F {F} O {O} lut {lut}: what_if vs oracle {e_or:.3e}, vs the engine's eval forward {e_en:.3e}")
    assert e_or <= TOL, e_or
    assert e_en <= TOL, e_en


@pytest.mark.parametrize("C,F,O,lut", WC.SHAPES)
def test_no_edit_candidates_are_predicts_rows(cuda_device, C, F, O, lut):
    """The existing kernel is untouched: candidates without an edit are ``predict(data)``'s rows, with ``node=None`` (row
    k is LUT row k) and with the nodes given, in any order and repeated."""
    ref, hip, pred, w, data, _, _, _ = _setup(C, F, O, lut, cuda_device)
    base, base_b = pred(data)
    out, lb = pred.what_if(data)
    assert torch.equal(out, base) and torch.equal(lb, base_b)
    # ... also when empty lists say so, and when the rows' own features are handed back
    luts = hip._lut_rows(data)
    L = luts.shape[0]
    none = torch.zeros(0, dtype=torch.long, device=cuda_device)
    out, lb = pred.what_if(data, x_lut=data.x[luts], add_src=none, add_ptr=[0] * (L + 1), drop=none, drop_ptr=[0] * (L + 1))
    assert torch.equal(out, base) and torch.equal(lb, base_b)
    order = torch.tensor([5, 0, L - 1, 5, 10, 10, 3], device=cuda_device)
    out, lb = pred.what_if(data, node=luts[order])
    assert torch.equal(out, base[order]) and torch.equal(lb, base_b[order])
    # no candidate: no launch
    out, lb = pred.what_if(data, node=none)
    assert tuple(out.shape) == (0, O) and tuple(lb.shape) == (0,) and out.dtype == torch.float32
    with pytest.raises(ValueError, match=f"the arguments name 3 candidates, the batch has {L} LUT rows"):
        pred.what_if(data, x_lut=WC.fresh_rows(3, F, lut).to(cuda_device))
    pred.check_status()


@pytest.mark.parametrize("C,F,O,lut", [WC.SHAPES[0], WC.SHAPES[2]])
def test_a_candidates_row_does_not_depend_on_the_other_candidates(cuda_device, C, F, O, lut):
    ref, hip, pred, w, data, _, _, want = _setup(C, F, O, lut, cuda_device)
    ks = [WC.index(n) for n in ("combined: adjacent, second", "drop: 32 on the 150-star", "add: 65 on the 150-star",
                                "one node: features", "drop: a repeat", "the batch's last node", "add: behind a slice of 64",
                                "combined: two LUTs, first")] + [3]
    nine, _ = _call(pred, WC.pick(w, ks), cuda_device, data)
    assert torch.equal(nine, want[ks])
    for where in (0, 1, 2, 8):                                              # alone
        alone, lb = _call(pred, WC.pick(w, [ks[where]]), cuda_device, data)
        assert tuple(alone.shape) == (1, O) and torch.equal(alone[0], nine[where]), where
        assert lb.tolist() == [int(w.data.batch[w.node[ks[where]]])]
    # without feature rows (x_lut=None): the candidates that keep their node's row
    keep = [k for k, c in enumerate(w.cands) if not c.fresh]
    out, _ = _call(pred, WC.pick(w, keep, x_lut=False), cuda_device, data)
    assert torch.equal(out, want[keep])
    pred.check_status()


FLAGGED = {"added source in another graph": 1, "added source negative": 1, "added source past the batch": 1,
           "node negative": 2, "node past the batch": 2, "drop position in another graph": 2, "drop position negative": 2,
           "drop position past the batch": 2, "LUT column just below one": 4, "LUT column zero on a plain node": 4}


@pytest.mark.parametrize("kind", list(FLAGGED))
def test_a_flagged_candidate_is_nan_alone(cuda_device, kind):
    """Refused inputs, handled by the kernel's bounds checks: nothing is read through the offending index."""
    C, F, O, lut = WC.SHAPES[2]
    ref, hip, pred, w, data, _, _, want = _setup(C, F, O, lut, cuda_device)
    ks = [WC.index("combined: two LUTs, second"), WC.index("add: 64 on the 150-star"), WC.index("drop: offset 63 of 64"), 2]
    good = WC.pick(w, ks)
    # the bad candidate goes in at position 2: the hub of the 64-star, one added source and one removal
    g = WC.STAR64
    node, src, pos, row = WC.PTR[g], WC.PTR[g] + 3, WC.EPTR[g] + 5, WC.fresh_rows(1, F, lut, seed=9)
    if kind == "added source in another graph":
        src = WC.PTR[g] - 1
    elif kind == "added source negative":
        src = -1
    elif kind == "added source past the batch":
        src = WC.PTR[-1]
    elif kind == "node negative":
        node = -1
    elif kind == "node past the batch":
        node = WC.PTR[-1]
    elif kind == "drop position in another graph":
        pos = WC.EPTR[g + 1]
    elif kind == "drop position negative":
        pos = -1
    elif kind == "drop position past the batch":
        pos = WC.EPTR[-1]
    elif kind == "LUT column just below one":
        row[0, lut] = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
    elif kind == "LUT column zero on a plain node":
        node, row = WC.PTR[g] + 1, w.data.x[WC.PTR[g] + 1:WC.PTR[g] + 2].clone()
    ap, dp = good.add_ptr, good.drop_ptr
    i64 = lambda v: torch.tensor([v], dtype=torch.long)                     # noqa: E731
    bad = WC.WhatIf(good.data, None, torch.cat([good.node[:2], i64(node), good.node[2:]]),
                    torch.cat([good.x_lut[:2], row, good.x_lut[2:]]),
                    torch.cat([good.add_src[:ap[2]], i64(src), good.add_src[ap[2]:]]), ap[:3] + [v + 1 for v in ap[2:]],
                    torch.cat([good.drop[:dp[2]], i64(pos), good.drop[dp[2]:]]), dp[:3] + [v + 1 for v in dp[2:]])
    out, lb = _call(pred, bad, cuda_device, data)
    assert tuple(out.shape) == (5, O) and bool(torch.isnan(out[2]).all())
    assert torch.equal(out[[0, 1, 3, 4]], want[ks])
    assert lb[[0, 1, 3, 4]].tolist() == w.data.batch[w.node[ks]].tolist()
    assert int(lb[2]) == (-1 if kind.startswith("node") else int(w.data.batch[node]))
    with pytest.raises(_lib.QotError, match=r"flagged the batch \(status %d\)" % FLAGGED[kind]):
        pred.check_status()
    pred.check_status()                                                     # raised once, clean afterwards


def test_what_if_follows_parameters_and_running_statistics(cuda_device):
    C, F, O, lut = 20, 5, 3, 1                                              # (a width the engine runs zero-padded)
    ref = WC.oracle_model(F, C, O, lut, seed=1)                             # (a model of its own: it is changed here)
    hip = WC.engine_model(ref, cuda_device)
    pred = q.LightpathPredictor(hip)
    w = WC.build(F, lut)
    data, kw = WC.args(w, cuda_device)
    mat, node_new = infer.materialise_lightpath_what_if(data, lut, **kw)
    rows = torch.searchsorted(hip._lut_rows(mat), node_new)
    before, _ = pred.what_if(data, **kw)
    assert torch.equal(before, pred(mat)[0][rows])
    with torch.no_grad():
        hip.conv1.att_src.mul_(1.5)
        hip.mlp[3].weight.mul_(0.5)
    stepped, _ = pred.what_if(data, **kw)
    assert not torch.equal(stepped, before) and torch.equal(stepped, pred(mat)[0][rows])
    buffers = {k: v.clone() for k, v in hip.named_buffers()}
    hip.norm1.module.running_mean.add_(0.25)
    moved, _ = pred.what_if(data, **kw)
    assert not torch.equal(moved, stepped) and torch.equal(moved, pred(mat)[0][rows])
    with torch.no_grad():
        e = rel_err(moved, hip(mat)[0][rows])
    print(f"after the updates: what_if vs the engine's eval forward of the materialised batch {e:.3e}")
    assert e <= TOL, e
    # pure: the call writes no buffer
    buffers["norm1.module.running_mean"] += 0.25
    for k, v in hip.named_buffers():
        assert torch.equal(v, buffers[k]), k
    pred.check_status()
