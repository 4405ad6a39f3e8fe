"""GPU: ``LightpathPredictor.place_impact`` (``csrc/infer_lightpath_place_impact.hip``) against its
definition, bit for bit (``torch.equal``, NaN compared as NaN): ``before`` / ``after`` are the rows ``predict`` gives the
affected lightpath's node in the device-built graphs of ``infer.materialise_retest``'s samples, ``out`` / ``count`` are
``place``'s, ``affected`` / ``n_affected`` the host statement's (``to_graph.placement_impact``); the hand cases of
``impact_cases.py``; overflow of ``max_affected``; refused candidates alone among good ones; independence; capture.  Every
shape is a dozen lightpaths on a 4 x 70 grid, or the smallest that reaches the path it names."""
import numpy as np
import pytest
import torch

import gnn_qot_estimation_amd as q
import impact_cases as IC
import place_cases as PC
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

pytestmark = pytest.mark.gpu
SHAPES = [(32, 3), (20, 1)]                                                    # (C = 20: the engine's padded width)


def _model(device, C=32, O=3, seed=0):
    """An engine model with every parameter and running statistic made to matter."""
    torch.manual_seed(seed)
    hip = q.LightpathGNN(5, C, O, PC.LUT_COL, dropout_p=0.0)
    with torch.no_grad():
        hip.conv1.bias.uniform_(-0.5, 0.5)
        bn = hip.norm1.module
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
    return hip.to(device).eval()


def _same(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(torch.nan_to_num(a, nan=-7.0),
                                                                                   torch.nan_to_num(b, nan=-7.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


def _on(b, device):
    """``(status, samples, values, cells, cell_ptr)`` of a ``place_cases.Batch``: the lists stay on the host."""
    return (b.ns.to_device(device), list(b.samples), torch.from_numpy(b.values).to(device),
            torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64)).to(device), list(b.cell_ptr))


def _impact(pred, args, thr, A=8):
    r = pred.place_impact(*args, PC.FEATS, thr, A)
    K, O, dev = args[2].shape[0], pred.model.mlp[3].out_features, args[0].device
    assert isinstance(r, infer.PlaceImpact)
    want = dict(out=(torch.float32, (K, O)), count=(torch.int64, (K,)), affected=(torch.int64, (K, A)),
                n_affected=(torch.int64, (K,)), before=(torch.float32, (K, A, O)), after=(torch.float32, (K, A, O)))
    for name, (dtype, shape) in want.items():
        t = getattr(r, name)
        assert t.dtype == dtype and tuple(t.shape) == shape and t.device == dev and t.grad_fn is None, name
    return r


def _rows_of(pred, retest, nodes, thr):
    """The rows ``predict`` gives node ``nodes[t]`` of the device-built graph of retest sample ``t``."""
    batch = TG.device_batch(retest, "lightpath", PC.FEATS, None, thr)
    out, _ = pred(batch)
    node = batch.ptr.to(out.device)[:-1] + torch.tensor(nodes, device=out.device)
    luts = pred.model._lut_rows(batch)
    row = torch.searchsorted(luts, node)
    assert torch.equal(luts[row], node)                                        # the retested lightpath's node is a LUT node
    return out[row]


def _definition(pred, b, args, thr, A=8):
    """``(affected, n_affected, before, after, impacts)`` by the definition: the host statement names the affected
    lightpaths and their nodes, ``materialise_retest`` builds one sample per (candidate, affected lightpath) pair -- all
    pairs of the batch in one call -- and ``predict`` scores their device-built graphs."""
    st, samples, values, cells, ptr = args
    K, O, dev = len(samples), pred.model.mlp[3].out_features, st.device
    impacts = [IC.host_impact(b, k, thr) for k in range(K)]
    affected = torch.full((K, A), -1, dtype=torch.int64)
    before = torch.full((K, A, O), float("nan"), dtype=torch.float32, device=dev)
    after = before.clone()
    pairs = [(k, i) for k in range(K) for i in range(min(len(impacts[k]), A))]
    for k, i in pairs:
        affected[k, i] = impacts[k][i][0]
    if pairs:
        ks = [k for k, _ in pairs]
        conns = [impacts[k][i][0] for k, i in pairs]
        which = torch.tensor([k for k, _ in pairs], device=dev), torch.tensor([i for _, i in pairs], device=dev)
        plain = infer.materialise_retest(st, [samples[k] for k in ks], conns)
        before[which] = _rows_of(pred, plain, [impacts[k][i][1] for k, i in pairs], thr)
        pcells = torch.cat([cells[:, ptr[k]:ptr[k + 1]] for k in ks], 1)
        pptr = np.cumsum([0] + [ptr[k + 1] - ptr[k] for k in ks]).tolist()
        with_cand = infer.materialise_retest(st, [samples[k] for k in ks], conns, values[ks], pcells, pptr)
        after[which] = _rows_of(pred, with_cand, [impacts[k][i][2] for k, i in pairs], thr)
    n_affected = torch.tensor([len(imp) for imp in impacts], dtype=torch.int64)
    return affected.to(dev), n_affected.to(dev), before, after, impacts


def _check(pred, b, device, thr, A=8):
    args = _on(b, device)
    clone = args[0].data.clone()
    r = _impact(pred, args, thr, A)
    out, count = pred.place(*args, PC.FEATS, thr)
    assert _same(r.out, out) and torch.equal(r.count, count)
    affected, n_affected, before, after, impacts = _definition(pred, b, args, thr, A)
    assert torch.equal(r.affected, affected) and torch.equal(r.n_affected, n_affected), (r.affected, affected, r.n_affected)
    assert _same(r.before, before), (r.before, before)
    assert _same(r.after, after), (r.after, after)
    assert torch.equal(args[0].data, clone)                                    # the call never writes to the chunk
    pred.check_status()
    return r, impacts


# ------------------------------------------------------------------ 1. the definition, bit for bit
@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("thr", IC.THRESHOLDS)
@pytest.mark.parametrize("C,O", SHAPES)
def test_rows_are_predict_of_the_retest_samples(cuda_device, C, O, thr, flagged):
    pred = q.LightpathPredictor(_model(cuda_device, C, O))
    b = IC.batch(0, flagged=flagged)
    r, impacts = _check(pred, b, cuda_device, thr)
    assert bool(torch.isfinite(r.out).all()) and r.count.tolist() == [1 + flagged] * len(b.samples)
    if thr == 0.12:
        assert sum(len(imp) for imp in impacts) >= len(b.samples)
    # the index lists in every form give the same bits
    st, samples, values, cells, ptr = _on(b, cuda_device)
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda_device)      # noqa: E731
    for s_form, p_form in ((dev(samples), dev(ptr)), (tuple(samples), dev(ptr))):
        again = _impact(pred, (st, s_form, values, cells, p_form), thr)
        assert all(_same(x, y) for x, y in zip(again, r))


# ------------------------------------------------------------------ 2. hand-built candidates
@pytest.mark.parametrize("name", list(IC.HAND))
def test_hand_cases(cuda_device, name):
    c = IC.HAND[name]()
    pred = q.LightpathPredictor(_model(cuda_device))
    r, impacts = _check(pred, IC.as_batch(c), cuda_device, c.thr)
    assert impacts[0] == c.want and r.count.tolist() == [c.count]
    assert r.n_affected.tolist() == [len(c.want)] and r.affected[0, :len(c.want)].tolist() == [t[0] for t in c.want]
    assert bool(torch.isfinite(r.out).all())
    if not c.want:
        assert bool((r.affected == -1).all()) and bool(torch.isnan(r.before).all()) and bool(torch.isnan(r.after).all())


# ------------------------------------------------------------------ 3. a message more changes the row
def test_a_message_more_changes_the_row(cuda_device):
    """``after`` has the candidate's message beside those of ``before``: were the rows not to depend on it, a lost or
    misplaced insertion would go unseen.  ``before`` is ``from_status`` of the retest sample wherever the affected
    lightpath is that sample's first flagged one."""
    pred = q.LightpathPredictor(_model(cuda_device))
    only = IC.as_batch(IC.HAND["the candidate is the only source: before sums no message"]())
    seen, firsts = 0, 0
    for b in (IC.batch(0), IC.batch(0, flagged=True), only):
        args = _on(b, cuda_device)
        r = _impact(pred, args, 0.12)
        for k, s in enumerate(b.samples):
            imp = IC.host_impact(b, k, 0.12)
            for i, (conn, node, _, sources, _) in enumerate(imp[:8]):
                assert bool(torch.isfinite(r.before[k, i]).all()) and bool(torch.isfinite(r.after[k, i]).all())
                assert not torch.equal(r.after[k, i], r.before[k, i]), (k, i)
                seen += 1
                retest = infer.materialise_retest(args[0], [s], [conn])
                count, first, _ = TG.lut_neighbourhood(retest.data[0].cpu().numpy(), b.ns.freq, PC.FI, 0.12)
                if first == conn:
                    rows, counts = pred.from_status(retest, None, PC.FEATS, 0.12)
                    assert torch.equal(rows[0], r.before[k, i]) and int(counts[0]) == count
                    firsts += 1
    assert seen >= 16 and firsts >= 8
    pred.check_status()


# ------------------------------------------------------------------ 4. overflow
def test_more_affected_than_slots_is_no_error(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = IC.batch(0)
    degrees = [len(IC.host_impact(b, k, 0.12)) for k in range(len(b.samples))]
    assert max(degrees) >= 4, degrees                                          # a condition on the inputs
    args = _on(b, cuda_device)
    wide, narrow = _impact(pred, args, 0.12, 8), _impact(pred, args, 0.12, 2)
    assert torch.equal(narrow.n_affected, wide.n_affected) and narrow.n_affected.tolist() == degrees
    for k, n in enumerate(degrees):
        m = min(n, 2)
        assert torch.equal(narrow.affected[k, :m], wide.affected[k, :m]) and bool((narrow.affected[k, m:] == -1).all())
        assert torch.equal(narrow.before[k, :m], wide.before[k, :m]) and torch.equal(narrow.after[k, :m], wide.after[k, :m])
        assert bool(torch.isnan(narrow.before[k, m:]).all()) and bool(torch.isnan(narrow.after[k, m:]).all())
    assert _same(narrow.out, wide.out) and torch.equal(narrow.count, wide.count)
    assert int(pred._status.item()) == 0                                       # nothing is flagged
    _check(pred, b, cuda_device, 0.12, A=2)
    _check(pred, b, cuda_device, 0.12, A=1)
    _check(pred, b, cuda_device, 0.12, A=32)


# ------------------------------------------------------------------ 5. refusals on the device
GOOD = ("the candidate is seen between two sources of the lightpath", "an affected lightpath with sources on links the candidate does not touch")


def _alone(pred, device):
    cases = [IC.HAND[n]() for n in GOOD]
    return cases, [_impact(pred, _on(IC.as_batch(c), device), 0.07) for c in cases]


def _refused(r, k):
    return (bool(torch.isnan(r.out[k]).all()) and int(r.count[k]) == 0 and int(r.n_affected[k]) == 0
            and bool((r.affected[k] == -1).all()) and bool(torch.isnan(r.before[k]).all()) and bool(torch.isnan(r.after[k]).all()))


def _good(r, k, alone):
    return all(_same(t[k], a[0]) for t, a in zip(r, alone))


def _refused_in_the_middle(pred, args, alone, cause):
    r = _impact(pred, args, 0.07)
    assert _refused(r, 1) and _good(r, 0, alone[0]) and _good(r, 2, alone[1])
    assert r.n_affected.tolist() == [1, 0, 1]
    with pytest.raises(_lib.QotError, match=cause):
        pred.check_status()
    pred.check_status()                                                        # clean on the next call


def _join(cases):
    return PC.join([PC.Case(c.ns, c.values, np.asarray(c.cells, dtype=np.int64), 0.07, None, 0) for c in cases])


@pytest.mark.parametrize("name", list(PC.refusals()))
def test_a_refused_candidate_flags_its_row_only(cuda_device, name):
    bit, cause, bad = PC.refusals()[name]
    pred = q.LightpathPredictor(_model(cuda_device))
    cases, alone = _alone(pred, cuda_device)
    args = _on(_join([cases[0], bad, cases[1]]), cuda_device)
    _refused_in_the_middle(pred, args, alone, cause)
    pred.place_impact(*args, PC.FEATS, 0.07)                                   # the word carries that bit and no other
    assert int(pred._status.item()) == getattr(infer, bit)
    pred._status.zero_()


def test_256_lightpaths_already_refuse_the_candidate(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    c, full = PC.crowd(255), PC.crowd(256)
    alone = _impact(pred, _on(PC.as_batch(c), cuda_device), 0.12)
    r = _impact(pred, _on(PC.join([c, full, c]), cuda_device), 0.12)
    assert _refused(r, 1) and _good(r, 0, alone) and _good(r, 2, alone) and r.n_affected.tolist() == [1, 0, 1]
    with pytest.raises(_lib.QotError, match=f"more than {TG.MAX_LIGHTPATHS} lightpaths"):
        pred.check_status()


@pytest.mark.parametrize("sample", [3, -1])
def test_a_sample_number_outside_the_chunk_flags_that_row_only(cuda_device, sample):
    pred = q.LightpathPredictor(_model(cuda_device))
    cases, alone = _alone(pred, cuda_device)
    st, samples, values, cells, ptr = _on(_join([cases[0], cases[0], cases[1]]), cuda_device)
    _refused_in_the_middle(pred, (st, [0, sample, 2], values, cells, ptr), alone, "sample number")


def test_a_bad_slice_of_a_device_cell_ptr_flags_that_row_only(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    cases, alone = _alone(pred, cuda_device)
    st, samples, values, cells, ptr = _on(_join([cases[0], cases[0], cases[1]]), cuda_device)
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda_device)      # noqa: E731
    keep = torch.tensor([0, 2], device=cuda_device)
    _refused_in_the_middle(pred, (st, samples, values, cells[:, keep].contiguous(), dev([0, 1, 1, 2])), alone,
                           "cell_ptr slice that is empty")
    for last in (4, 1, -2):                                                    # M = 3: beyond it, descending, negative
        r = _impact(pred, (st, [0, 2, 1], values[[0, 2, 1]], cells[:, [0, 2, 1]].contiguous(), dev([0, 1, 2, last])), 0.07)
        assert _good(r, 0, alone[0]) and _good(r, 1, alone[1]) and _refused(r, 2)
        with pytest.raises(_lib.QotError, match="cell_ptr slice that is empty, descending or beyond"):
            pred.check_status()


# ------------------------------------------------------------------ 6. independence
def test_a_candidate_depends_on_itself_and_its_sample_alone(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = IC.batch(0)
    st, samples, values, cells, ptr = _on(b, cuda_device)
    whole = _impact(pred, (st, samples, values, cells, ptr), 0.12)
    again = _impact(pred, (st, samples, values, cells, ptr), 0.12)
    assert all(_same(x, y) for x, y in zip(whole, again))
    for order in (list(reversed(range(len(samples)))), [5, 2], [3]):           # permuted; subsets
        ocells = torch.cat([cells[:, ptr[k]:ptr[k + 1]] for k in order], 1)
        optr = np.cumsum([0] + [ptr[k + 1] - ptr[k] for k in order]).tolist()
        part = _impact(pred, (st, [samples[k] for k in order], values[order], ocells, optr), 0.12)
        assert all(_same(x, y[order]) for x, y in zip(part, whole)), order
    # two candidates identical but for the sample give their own samples' rows
    fits = lambda k: not np.any(b.ns.data[1 - samples[k]][:, b.cells[0, ptr[k]:ptr[k + 1]], b.cells[1, ptr[k]:ptr[k + 1]]] != 0)  # noqa: E731
    k = next(k for k in range(len(samples)) if fits(k))                        # its cells are free in the other sample too
    kcells = b.cells[:, ptr[k]:ptr[k + 1]]
    twin = PC.Batch(b.ns, [samples[k], 1 - samples[k]], b.values[[k, k]], np.concatenate([kcells, kcells], 1),
                    [0, kcells.shape[1], 2 * kcells.shape[1]])
    r, impacts = _check(pred, twin, cuda_device, 0.12)
    assert all(_same(x[0], y[k]) for x, y in zip(r, whole))
    assert impacts[0] != impacts[1] and not torch.equal(r.out[0], r.out[1])
    pred.check_status()


# ------------------------------------------------------------------ 7. capture
def test_capture_and_replay_on_overwritten_arguments(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b, b2 = IC.batch(0), PC.batch(1)                                           # the same K and shapes, other contents
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda_device)      # noqa: E731
    st, samples, values, cells, ptr = _on(b, cuda_device)
    M = max(cells.shape[1], b2.cells.shape[1])
    cells = torch.cat([cells, cells.new_zeros(2, M - cells.shape[1])], 1)      # room for the other batch's cells
    samples, ptr = dev(samples), dev(ptr)
    eager = pred.place_impact(st, samples, values, cells, ptr, PC.FEATS, 0.12)  # (the column table is uploaded here)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = pred.place_impact(st, samples, values, cells, ptr, PC.FEATS, 0.12)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same(x, y) for x, y in zip(r, eager))
    assert all(_same(x, y) for x, y in zip(eager, _impact(pred, _on(b, cuda_device), 0.12)))
    st.data.copy_(torch.from_numpy(b2.ns.data))                                # in place: the captured pointers stay
    values.copy_(torch.from_numpy(b2.values))
    cells[:, :b2.cells.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(b2.cells, dtype=np.int64)))
    samples.copy_(dev(b2.samples))
    ptr.copy_(dev(b2.cell_ptr))
    graph.replay()
    torch.cuda.synchronize()
    want = _impact(pred, _on(b2, cuda_device), 0.12)
    assert all(_same(x, y) for x, y in zip(r, want)) and not torch.equal(r.out, eager.out)
    assert not _same(r.before, eager.before)
    pred.check_status()


# ------------------------------------------------------------------ 8. empty input
def test_no_candidates_no_launch(cuda_device, monkeypatch):
    pred = q.LightpathPredictor(_model(cuda_device))
    st, samples, values, cells, ptr = _on(IC.batch(0), cuda_device)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for none in ([], torch.zeros(0, dtype=torch.int64, device=cuda_device)):
        r = pred.place_impact(st, none, values[:0], cells[:, :0], [0], PC.FEATS, 0.05, 4)
        shapes = [tuple(t.shape) for t in r]
        assert shapes == [(0, 3), (0,), (0, 4), (0,), (0, 4, 3), (0, 4, 3)], shapes
        assert [t.dtype for t in r] == [torch.float32, torch.int64, torch.int64, torch.int64, torch.float32, torch.float32]
    monkeypatch.undo()
    assert calls == []
    with pytest.raises(ValueError, match="max_affected"):
        pred.place_impact(st, samples, values, cells, ptr, PC.FEATS, 0.05, 33)
    with pytest.raises(infer.EnvelopeError, match="'osnr' cannot be a feature"):
        pred.place_impact(st, samples, values, cells, ptr, ["freq", "mod_order", "num_spans", "osnr"])
    with pytest.raises(TypeError):
        pred.place_impact(st, samples, values, cells, ptr, release=None)
    pred.check_status()
