"""GPU: ``LightpathPredictor.reroute_impact`` (``csrc/infer_lightpath_reroute_impact.hip``) against its
definition, bit for bit (``torch.equal``, NaN compared as NaN): ``before`` / ``after`` are the rows ``predict`` gives the
affected lightpath's node in the device-built graphs of ``infer.materialise_retest``'s samples (``release=`` for ``after``),
``out`` / ``count`` are ``place(..., release=, release_ptr=)``'s, ``affected`` / ``n_affected`` / ``gains`` / ``lost`` the
host statement's (``to_graph.reroute_impact``); the hand cases of ``reroute_impact_cases.py``; no release against
``place_impact``; overflow of ``max_affected``; refused candidates alone among good ones; independence; capture.  Every
shape is a dozen lightpaths on a 4 x 70 grid, or ``place_cases.crowd``."""
import numpy as np
import pytest
import torch

import gnn_qot_estimation_amd as q
import impact_cases as IC
import place_cases as PC
import release_cases as RC
import reroute_impact_cases as RI
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

pytestmark = pytest.mark.gpu
SHAPES = [(32, 3), (20, 1)]                                                    # (C = 20: the engine's padded width)
FIELDS = dict(out=torch.float32, count=torch.int64, affected=torch.int64, n_affected=torch.int64, before=torch.float32,
              after=torch.float32, gains=torch.bool, lost=torch.int64)


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
    if not a.dtype.is_floating_point:
        return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b)
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(torch.nan_to_num(a, nan=-7.0),
                                                                                   torch.nan_to_num(b, nan=-7.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


def _all_same(r, s):
    return all(_same(x, y) for x, y in zip(r, s))


def _dev(v, device):
    return torch.tensor(np.asarray(v, dtype=np.int64).reshape(-1), dtype=torch.int64, device=device)


def _on(b, device):
    """``((status, samples, values, cells, cell_ptr), {release, release_ptr})`` of a ``release_cases.Batch``: the index
    lists stay on the host."""
    return ((b.ns.to_device(device), list(b.samples), torch.from_numpy(b.values).to(device),
             torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64)).to(device), list(b.cell_ptr)),
            dict(release=_dev(b.release, device), release_ptr=list(b.release_ptr)))


def _impact(pred, args, kw, thr, A=8):
    r = pred.reroute_impact(*args, PC.FEATS, thr, A, **kw)
    K, O, dev = args[2].shape[0], pred.model.mlp[3].out_features, args[0].device
    assert isinstance(r, infer.RerouteImpact) and r._fields == tuple(FIELDS)
    shapes = dict(out=(K, O), count=(K,), affected=(K, A), n_affected=(K,), before=(K, A, O), after=(K, A, O), gains=(K, A),
                  lost=(K, A))
    for name, dtype in FIELDS.items():
        t = getattr(r, name)
        assert t.dtype == dtype and tuple(t.shape) == shapes[name] and t.device == dev and t.grad_fn is None, name
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


def _pairs_lists(b, args, pairs):
    """The lists of one ``materialise_retest`` call over ``pairs`` ``[(k, slot)]``: candidate ``k``'s sample, cells and
    release slice once per pair."""
    st, samples, values, cells, ptr = args
    ks = [k for k, _ in pairs]
    pcells = torch.cat([cells[:, ptr[k]:ptr[k + 1]] for k in ks], 1)
    pptr = np.cumsum([0] + [ptr[k + 1] - ptr[k] for k in ks]).tolist()
    rel = _dev([c for k in ks for c in RC.released(b, k)], st.device)
    rptr = np.cumsum([0] + [len(RC.released(b, k)) for k in ks]).tolist()
    return ks, [samples[k] for k in ks], values[ks], pcells, pptr, rel, rptr


def _definition(pred, b, args, thr, A=8):
    """``RerouteImpact``'s six fields behind ``count`` by the definition, and the host tuples: the host statement names the
    affected lightpaths and their nodes, ``materialise_retest`` builds one sample per (candidate, slot) pair -- all pairs
    of the batch in one call each for ``before`` and ``after`` -- and ``predict`` scores their device-built graphs."""
    st = args[0]
    K, O, dev = len(args[1]), pred.model.mlp[3].out_features, st.device
    impacts = [RI.host_impact(b, k, thr) for k in range(K)]
    affected = torch.full((K, A), -1, dtype=torch.int64)
    lost = affected.clone()
    gains = torch.zeros(K, A, dtype=torch.bool)
    before = torch.full((K, A, O), float("nan"), dtype=torch.float32, device=dev)
    after = before.clone()
    pairs = [(k, i) for k in range(K) for i in range(min(len(impacts[k]), A))]
    for k, i in pairs:
        affected[k, i], gains[k, i], lost[k, i] = impacts[k][i][0], impacts[k][i][5], impacts[k][i][6]
    if pairs:
        ks, psamples, pvalues, pcells, pptr, rel, rptr = _pairs_lists(b, args, pairs)
        conns = [impacts[k][i][0] for k, i in pairs]
        which = torch.tensor([k for k, _ in pairs], device=dev), torch.tensor([i for _, i in pairs], device=dev)
        plain = infer.materialise_retest(st, psamples, conns)
        before[which] = _rows_of(pred, plain, [impacts[k][i][1] for k, i in pairs], thr)
        edited = infer.materialise_retest(st, psamples, conns, pvalues, pcells, pptr, release=rel, release_ptr=rptr)
        after[which] = _rows_of(pred, edited, [impacts[k][i][2] for k, i in pairs], thr)
    n_affected = torch.tensor([len(imp) for imp in impacts], dtype=torch.int64)
    return (affected.to(dev), n_affected.to(dev), before, after, gains.to(dev), lost.to(dev)), impacts


def _check(pred, b, device, thr, A=8):
    args, kw = _on(b, device)
    clone = args[0].data.clone()
    r = _impact(pred, args, kw, thr, A)
    out, count = pred.place(*args, PC.FEATS, thr, **kw)
    assert _same(r.out, out) and torch.equal(r.count, count)
    want, impacts = _definition(pred, b, args, thr, A)
    for name, got, w in zip(r._fields[2:], r[2:], want):
        assert _same(got, w), (name, got, w)
    assert torch.equal(args[0].data, clone)                                    # the call never writes to the chunk
    pred.check_status()
    return r, impacts


# ------------------------------------------------------------------ 1. the definition, bit for bit
@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("thr", RI.THRESHOLDS)
@pytest.mark.parametrize("C,O", SHAPES)
def test_rows_are_predict_of_the_retest_samples(cuda_device, C, O, thr, flagged):
    pred = q.LightpathPredictor(_model(cuda_device, C, O))
    b = RI.batch(0, flagged)
    r, impacts = _check(pred, b, cuda_device, thr)
    assert bool(torch.isfinite(r.out).all()) and sum(len(imp) for imp in impacts) >= 2 * len(b.samples)
    (st, samples, values, cells, ptr), kw = _on(b, cuda_device)
    # before is retest's row of the same conn in the unedited sample
    rt = pred.retest(st, samples, r.affected, PC.FEATS, thr)
    assert _same(rt.out, r.before) and torch.equal(rt.conn, r.affected)
    pred.check_status()
    # the index lists in every form give the same bits
    dev = lambda v: _dev(v, cuda_device)                                       # noqa: E731
    for s_form, p_form, r_form in ((dev(samples), dev(ptr), dev(kw["release_ptr"])), (tuple(samples), dev(ptr), tuple(kw["release_ptr"]))):
        again = _impact(pred, (st, s_form, values, cells, p_form), dict(release=kw["release"], release_ptr=r_form), thr)
        assert _all_same(again, r)


# ------------------------------------------------------------------ 2. hand-built candidates
@pytest.mark.parametrize("name", list(RI.HAND))
def test_hand_cases(cuda_device, name):
    c = RI.HAND[name]()
    pred = q.LightpathPredictor(_model(cuda_device))
    r, impacts = _check(pred, RI.as_batch(c), cuda_device, c.thr)
    n = len(c.want)
    assert impacts[0] == c.want and r.count.tolist() == [c.count] and r.n_affected.tolist() == [n]
    assert r.affected[0, :n].tolist() == [t[0] for t in c.want] and r.gains[0, :n].tolist() == [t[5] for t in c.want]
    assert r.lost[0, :n].tolist() == [t[6] for t in c.want]
    assert bool(torch.isfinite(r.out).all()) and bool(torch.isfinite(r.before[0, :n]).all()) and bool(torch.isfinite(r.after[0, :n]).all())
    assert bool((r.affected[0, n:] == -1).all()) and bool((r.lost[0, n:] == -1).all()) and not bool(r.gains[0, n:].any())
    assert bool(torch.isnan(r.before[0, n:]).all()) and bool(torch.isnan(r.after[0, n:]).all())


# ------------------------------------------------------------------ 3. nothing released: place_impact
def test_without_a_release_it_is_place_impact(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    for b in (IC.batch(0), IC.batch(0, flagged=True)):
        K = len(b.samples)
        args = (b.ns.to_device(cuda_device), list(b.samples), torch.from_numpy(b.values).to(cuda_device),
                torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64)).to(cuda_device), list(b.cell_ptr))
        want = pred.place_impact(*args, PC.FEATS, 0.12)
        none = torch.zeros(0, dtype=torch.int64, device=cuda_device)
        for kw in (dict(), dict(release=None, release_ptr=None), dict(release=none, release_ptr=[0] * (K + 1)),
                   dict(release=none, release_ptr=torch.zeros(K + 1, dtype=torch.int64, device=cuda_device))):
            r = _impact(pred, args, kw, 0.12)
            assert _all_same(r[:6], want)
            used = torch.arange(8, device=cuda_device)[None, :] < r.n_affected[:, None]
            assert torch.equal(r.gains, used) and torch.equal(r.lost, torch.where(used, 0, -1))
        assert int(want.n_affected.sum()) >= K
    pred.check_status()


# ------------------------------------------------------------------ 4. the rows depend on the edit
def test_the_rows_depend_on_the_edit(cuda_device):
    """``after`` differs from ``before`` wherever the lightpath gains or loses a source -- were the rows not to depend on
    it, a lost or misplaced message would go unseen -- and a lose-only ``after`` is the row ``retest`` gives the lightpath
    in the sample with the release materialised."""
    pred = q.LightpathPredictor(_model(cuda_device))
    seen = lose_only = 0
    for b in (RI.batch(0), RI.batch(0, True)):
        args, kw = _on(b, cuda_device)
        r = _impact(pred, args, kw, 0.12)
        impacts = [RI.host_impact(b, k, 0.12) for k in range(len(b.samples))]
        pairs = [(k, i) for k, imp in enumerate(impacts) for i in range(len(imp))]
        for k, i in pairs:
            assert bool(r.gains[k, i]) or int(r.lost[k, i]) > 0
            assert not torch.equal(r.after[k, i], r.before[k, i]), (k, i)
            seen += 1
        losers = [(k, i) for k, i in pairs if not impacts[k][i][5]]
        ks, psamples, _, _, _, rel, rptr = _pairs_lists(b, args, losers)
        conns = [impacts[k][i][0] for k, i in losers]
        torn = infer.materialise_retest(args[0], psamples, conns, release=rel, release_ptr=rptr)
        rt = pred.retest(torn, None, _dev(conns, cuda_device)[:, None], PC.FEATS, 0.12)
        for t, (k, i) in enumerate(losers):
            assert torch.equal(rt.out[t, 0], r.after[k, i]), (k, i)
        lose_only += len(losers)
    assert seen >= 40 and lose_only >= 20
    pred.check_status()


# ------------------------------------------------------------------ 5. overflow
def test_more_affected_than_slots_is_no_error(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = RI.batch(0, True)
    degrees = [len(RI.host_impact(b, k, 0.12)) for k in range(len(b.samples))]
    assert max(degrees) >= 4 and max(degrees) <= 8, degrees                    # a condition on the inputs
    args, kw = _on(b, cuda_device)
    wide = _impact(pred, args, kw, 0.12, 8)
    assert wide.n_affected.tolist() == degrees
    for A in (1, 2, 32):
        other = _impact(pred, args, kw, 0.12, A)
        assert torch.equal(other.n_affected, wide.n_affected) and _same(other.out, wide.out) and torch.equal(other.count, wide.count)
        for k, n in enumerate(degrees):
            m = min(n, A)
            for name in ("affected", "before", "after", "gains", "lost"):
                assert torch.equal(getattr(other, name)[k, :m], getattr(wide, name)[k, :m]), (A, k, name)
            assert bool((other.affected[k, m:] == -1).all()) and bool((other.lost[k, m:] == -1).all())
            assert not bool(other.gains[k, m:].any())
            assert bool(torch.isnan(other.before[k, m:]).all()) and bool(torch.isnan(other.after[k, m:]).all())
        assert int(pred._status.item()) == 0                                   # nothing is flagged
    _check(pred, b, cuda_device, 0.12, A=2)
    _check(pred, b, cuda_device, 0.12, A=32)


# ------------------------------------------------------------------ 6. refusals on the device
GOOD = ("a reroute proper: the old neighbours lose, the new one gains", "a released lightpath beside the candidate's new cells")


def _is_refused(r, k):
    return (bool(torch.isnan(r.out[k]).all()) and int(r.count[k]) == 0 and int(r.n_affected[k]) == 0
            and bool((r.affected[k] == -1).all()) and bool((r.lost[k] == -1).all()) and not bool(r.gains[k].any())
            and bool(torch.isnan(r.before[k]).all()) and bool(torch.isnan(r.after[k]).all()))


def _refused(pred, b, device, thr, bit, cause, bad=1, samples=None, release=None, release_ptr=None):
    """Candidate ``bad`` of the three of ``b`` is refused with exactly ``bit``, the other two are what they are alone.
    ``samples``, ``release`` / ``release_ptr``: other lists, the latter on the device."""
    args, kw = _on(b, device)
    alone = {k: _impact(pred, *_on(RC.take(b, [k]), device), thr) for k in set(range(3)) - {bad}}
    assert all(int(a.n_affected[0]) >= 1 and bool(torch.isfinite(a.out).all()) for a in alone.values())
    pred.check_status()
    if samples is not None:
        args = (args[0], samples) + args[2:]
    if release_ptr is not None:
        kw = dict(release=_dev(release, device), release_ptr=_dev(release_ptr, device))
    r = _impact(pred, args, kw, thr)
    assert _is_refused(r, bad)
    for k, a in alone.items():
        assert all(_same(t[k], x[0]) for t, x in zip(r, a)), k
    assert int(pred._status.item()) == bit                                     # that bit and no other
    with pytest.raises(_lib.QotError, match=cause):
        pred.check_status()
    pred.check_status()                                                        # clean on the next call


def _three(middle):
    return RC.join([RI.as_batch(RI.HAND[GOOD[0]]()), RI.as_batch(middle), RI.as_batch(RI.HAND[GOOD[1]]())])


@pytest.mark.parametrize("name", list(PC.refusals()))
def test_a_refused_candidate_flags_its_row_only(cuda_device, name):
    """``place``'s refusals on ``place_cases._one_cell``'s sample (conn 8 on (1, 9), conn 9 on (1, 11), conn 7 on (2, 10)),
    each releasing conn 7: the occupied cell and the taken conn belong to survivors."""
    bit, cause, bad = PC.refusals()[name]
    pred = q.LightpathPredictor(_model(cuda_device))
    middle = RI.Reroute(bad.ns, bad.values, np.asarray(bad.cells, dtype=np.int64), [7], 0.07, None, 0)
    _refused(pred, _three(middle), cuda_device, 0.07, getattr(infer, bit), cause)


def test_a_released_conn_the_sample_does_not_hold(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    middle = RI.HAND[GOOD[0]]()._replace(release=[5, 6])
    _refused(pred, _three(middle), cuda_device, 0.07, infer.LP_PLACE_NO_SUCH_CONN, "released conn_id is no lightpath")


# the three candidates release [5], [5], [6]; the lists below give the good ones those conns and the bad one a bad slice
BAD_SLICES = {
    "descending": (1, [6, 5], [1, 2, 0, 1]),
    "beyond R": (2, [5, 6, 5], [0, 1, 2, 4]),
    "negative": (0, [5, 5, 6], [-1, 1, 2, 3]),
}


@pytest.mark.parametrize("name", list(BAD_SLICES))
def test_a_bad_slice_of_a_device_release_ptr_flags_that_row_only(cuda_device, name):
    bad, release, ptr = BAD_SLICES[name]
    pred = q.LightpathPredictor(_model(cuda_device))
    b = _three(RI.HAND[GOOD[0]]())
    assert [RC.released(b, k) for k in range(3)] == [[5], [5], [6]]
    if bad == 2:
        b = RC.take(b, [0, 2, 1])                                              # the good ones release [5] and [6]: slices 0, 1
    _refused(pred, b, cuda_device, 0.07, infer.LP_PLACE_BAD_RELEASE, "release_ptr slice that is descending", bad,
             release=release, release_ptr=ptr)


def test_a_slice_of_33_is_refused(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    c = RI.HAND["32 releases"]()
    b = RC.join([RI.as_batch(c)] * 3)
    release = list(range(10, 42)) + list(range(10, 43)) + list(range(10, 42))  # 33 conns, all of them in the sample
    args, kw = _on(b, cuda_device)
    with pytest.raises(ValueError, match="LightpathPredictor.reroute_impact: candidate 1 releases 33 lightpaths, at most 32"):
        pred.reroute_impact(*args, PC.FEATS, c.thr, release=_dev(release, cuda_device), release_ptr=[0, 32, 65, 97])
    _refused(pred, b, cuda_device, c.thr, infer.LP_PLACE_BAD_RELEASE, "longer than 32", 1, release=release, release_ptr=[0, 32, 65, 97])


@pytest.mark.parametrize("sample", [3, -1])
def test_a_sample_number_outside_the_chunk_flags_that_row_only(cuda_device, sample):
    pred = q.LightpathPredictor(_model(cuda_device))
    _refused(pred, _three(RI.HAND[GOOD[0]]()), cuda_device, 0.07, infer.LP_STATUS_BAD_SAMPLE, "sample number", samples=[0, sample, 2])


def test_256_lightpaths_with_nothing_released_refuse_the_candidate(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    c = RI.HAND["256 lightpaths, one released"]()
    b = RC.join([RI.as_batch(c), RI.as_batch(c._replace(release=[])), RI.as_batch(c)])
    _refused(pred, b, cuda_device, c.thr, infer.LP_STATUS_TOO_MANY, f"more than {TG.MAX_LIGHTPATHS} lightpaths")


# ------------------------------------------------------------------ 7. independence
def test_a_candidate_depends_on_itself_and_its_sample_alone(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = RI.batch(0)
    K = len(b.samples)
    whole = _impact(pred, *_on(b, cuda_device), 0.12)
    assert _all_same(whole, _impact(pred, *_on(b, cuda_device), 0.12))
    for order in (list(reversed(range(K))), [5, 2], [3]):                      # permuted; subsets
        part = _impact(pred, *_on(RC.take(b, order), cuda_device), 0.12)
        assert all(_same(x, y[order]) for x, y in zip(part, whole)), order
    # two candidates identical but for the sample give their own samples' rows: conn 9 is missing from the second sample
    c = RI.HAND[GOOD[0]]()
    data = c.ns.data.copy()
    data[0, :, 1, 11] = 0.0
    twin = RC.join([RI.as_batch(c), RI.as_batch(c._replace(ns=PC.SK.status(data, c.ns.freq)))])
    assert np.array_equal(twin.values[0], twin.values[1]) and RC.released(twin, 0) == RC.released(twin, 1)
    r, impacts = _check(pred, twin, cuda_device, c.thr)
    assert [t[0] for t in impacts[0]] == [8, 9, 7] and [t[0] for t in impacts[1]] == [8, 7]
    assert torch.equal(r.before[0, 0], r.before[1, 0]) and torch.equal(r.after[0, 2], r.after[1, 1])


# ------------------------------------------------------------------ 8. capture
def test_capture_and_replay_on_overwritten_arguments(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b, b2 = RI.batch(0), RC.lp_batch(1)                                        # the same K and shapes, other contents
    d = lambda v: _dev(v, cuda_device)                                         # noqa: E731
    (st, samples, values, cells, ptr), kw = _on(b, cuda_device)
    M, R = max(cells.shape[1], b2.cells.shape[1]), max(len(b.release), len(b2.release))
    cells = torch.cat([cells, cells.new_zeros(2, M - cells.shape[1])], 1)      # room for the other batch's lists
    rel = torch.cat([kw["release"], kw["release"].new_zeros(R - len(b.release))])
    samples, ptr, rptr = d(samples), d(ptr), d(kw["release_ptr"])
    eager = pred.reroute_impact(st, samples, values, cells, ptr, PC.FEATS, 0.12, release=rel, release_ptr=rptr)
    torch.cuda.synchronize()                                                   # (the column table was uploaded there)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = pred.reroute_impact(st, samples, values, cells, ptr, PC.FEATS, 0.12, release=rel, release_ptr=rptr)
    graph.replay()
    torch.cuda.synchronize()
    assert _all_same(r, eager)
    assert _all_same(eager, _impact(pred, *_on(b, cuda_device), 0.12))         # (the unused tails are not read)
    st.data.copy_(torch.from_numpy(b2.ns.data))                                # in place: the captured pointers stay
    values.copy_(torch.from_numpy(b2.values))
    cells[:, :b2.cells.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(b2.cells, dtype=np.int64)))
    rel[:len(b2.release)].copy_(d(b2.release))
    samples.copy_(d(b2.samples))
    ptr.copy_(d(b2.cell_ptr))
    rptr.copy_(d(b2.release_ptr))
    graph.replay()
    torch.cuda.synchronize()
    want = _impact(pred, *_on(b2, cuda_device), 0.12)
    assert _all_same(r, want) and not torch.equal(r.out, eager.out) and not _same(r.before, eager.before)
    assert int(want.n_affected.sum()) >= 8
    pred.check_status()


# ------------------------------------------------------------------ 9. empty input
def test_no_candidates_no_launch(cuda_device, monkeypatch):
    pred = q.LightpathPredictor(_model(cuda_device))
    (st, samples, values, cells, ptr), kw = _on(RI.batch(0), cuda_device)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for none in ([], torch.zeros(0, dtype=torch.int64, device=cuda_device)):
        for rkw in (dict(), dict(release=kw["release"][:0], release_ptr=[0])):
            r = pred.reroute_impact(st, none, values[:0], cells[:, :0], [0], PC.FEATS, 0.05, 4, **rkw)
            assert [tuple(t.shape) for t in r] == [(0, 3), (0,), (0, 4), (0,), (0, 4, 3), (0, 4, 3), (0, 4), (0, 4)]
            assert [t.dtype for t in r] == list(FIELDS.values())
    monkeypatch.undo()
    assert calls == []
    with pytest.raises(ValueError, match="LightpathPredictor.reroute_impact: max_affected"):
        pred.reroute_impact(st, samples, values, cells, ptr, PC.FEATS, 0.05, 33, **kw)
    with pytest.raises(infer.EnvelopeError, match="LightpathPredictor.reroute_impact: 'osnr' cannot be a feature"):
        pred.reroute_impact(st, samples, values, cells, ptr, ["freq", "mod_order", "num_spans", "osnr"], **kw)
    with pytest.raises(ValueError, match="LightpathPredictor.reroute_impact: release and release_ptr go together"):
        pred.reroute_impact(st, samples, values, cells, ptr, PC.FEATS, release=kw["release"])
    with pytest.raises(TypeError):
        pred.reroute_impact(st, samples, values, cells, ptr, PC.FEATS, 0.05, 8, kw["release"], kw["release_ptr"])   # keyword-only
    pred.check_status()
