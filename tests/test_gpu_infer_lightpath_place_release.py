"""GPU: ``LightpathPredictor.place(..., release=, release_ptr=)`` (``csrc/infer_lightpath_place_release.hip``)
against its definition over ``infer.materialise_placement(..., release=)``'s edited samples, bit for bit (``torch.equal``,
NaN rows compared as NaN): the row of the candidate's node in ``predict(to_graph.device_batch(edited, "lightpath", ...))``
and, where the candidate is the first-seen flagged lightpath of its edited sample, ``from_status(edited)``; empty slices
against plain ``place``; the hand cases of ``release_cases.py``; refused candidates alone among good ones with the exact
status word; independence and capture.  Every shape is a dozen lightpaths on a 4 x 70 grid, or the smallest that reaches
the path it names."""
import numpy as np
import pytest
import torch

import gnn_qot_estimation_amd as q
import place_cases as PC
import release_cases as RC
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


def _dev(v, device):
    return torch.tensor(np.asarray(v, dtype=np.int64).reshape(-1), dtype=torch.int64, device=device)


def _on(b, device):
    """``((status, samples, values, cells, cell_ptr), {release, release_ptr})`` of a ``release_cases.Batch``: the index
    lists stay on the host."""
    return ((b.ns.to_device(device), list(b.samples), torch.from_numpy(b.values).to(device),
             torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64)).to(device), list(b.cell_ptr)),
            dict(release=_dev(b.release, device), release_ptr=list(b.release_ptr)))


def _place(pred, args, kw, thr):
    out, count = pred.place(*args, PC.FEATS, thr, **kw)
    K = args[2].shape[0]
    assert out.dtype == torch.float32 and count.dtype == torch.int64 and out.grad_fn is None and out.device == args[0].device
    assert tuple(out.shape) == (K, pred.model.mlp[3].out_features) and tuple(count.shape) == (K,)
    return out, count


def _via_predict(pred, b, args, kw, thr):
    """The definition: the row ``predict`` gives the candidate's node in the device-built graph of its edited sample, and
    the LUT nodes of that graph."""
    edited = infer.materialise_placement(*args, **kw)
    batch = TG.device_batch(edited, "lightpath", PC.FEATS, None, thr)
    out, lut_batch = pred(batch)
    nodes = [TG.place_lightpath(b.ns.data[s], b.values[k], RC.candidate_cells(b, k), PC.FI, RC.released(b, k))[1]
             for k, s in enumerate(b.samples)]
    node = batch.ptr.to(out.device)[:-1] + torch.tensor(nodes, device=out.device)
    luts = pred.model._lut_rows(batch)
    row = torch.searchsorted(luts, node)
    assert torch.equal(luts[row], node)                                        # the candidate's node is a LUT node
    return out[row], torch.bincount(lut_batch, minlength=len(b.samples)), edited, batch, node


def _check(pred, b, device, thr, first_seen=True):
    args, kw = _on(b, device)
    got, count = _place(pred, args, kw, thr)
    want, want_count, edited, batch, node = _via_predict(pred, b, args, kw, thr)
    assert _same(got, want) and torch.equal(count, want_count), (got, want, count, want_count)
    assert bool(torch.isfinite(got).all())
    status_rows, status_count = pred.from_status(edited, None, PC.FEATS, thr)
    assert torch.equal(status_count, count)
    if first_seen:
        assert _same(got, status_rows)
    pred.check_status()
    return got, count, batch, node


# ------------------------------------------------------------------ 1. the definition, bit for bit
@pytest.mark.parametrize("thr", PC.THRESHOLDS)
@pytest.mark.parametrize("C,O", SHAPES)
def test_rows_are_from_status_and_predict_of_the_edited_samples(cuda_device, C, O, thr):
    pred = q.LightpathPredictor(_model(cuda_device, C, O))
    for seed in (0, 1):
        b = RC.lp_batch(seed)
        got, count, _, _ = _check(pred, b, cuda_device, thr)
        assert count.tolist() == [1] * len(b.samples)
        (st, samples, values, cells, ptr), kw = _on(b, cuda_device)
        rel, rptr = kw["release"], kw["release_ptr"]
        d = lambda v: _dev(v, cuda_device)                                      # noqa: E731
        for s_form, p_form, r_form in ((d(samples), ptr, rptr), (samples, d(ptr), rptr), (samples, ptr, d(rptr)),
                                       (d(samples), d(ptr), d(rptr)), (tuple(samples), tuple(ptr), tuple(rptr)),
                                       (samples, d(ptr), d(rptr))):
            again, cnt = _place(pred, (st, s_form, values, cells, p_form), dict(release=rel, release_ptr=r_form), thr)
            assert torch.equal(again, got) and torch.equal(cnt, count)
        k = 3                                                                  # an int: all candidates in that sample
        one, _ = _place(pred, (st, samples[k], values[k:k + 1], cells[:, ptr[k]:ptr[k + 1]].contiguous(), [0, ptr[k + 1] - ptr[k]]),
                        dict(release=rel[rptr[k]:rptr[k + 1]], release_ptr=[0, rptr[k + 1] - rptr[k]]), thr)
        assert torch.equal(one[0], got[k])


@pytest.mark.parametrize("thr", PC.THRESHOLDS)
def test_rows_in_samples_that_hold_a_flagged_lightpath(cuda_device, thr):
    """The samples hold a lower-numbered flagged lightpath: the candidate's row is still its node's, and the count is the
    flagged survivors plus one."""
    pred = q.LightpathPredictor(_model(cuda_device))
    b = RC.lp_batch(1, flagged=True)
    got, count, batch, node = _check(pred, b, cuda_device, thr, first_seen=False)
    want = [2 - (700 + s in RC.released(b, k)) for k, s in enumerate(b.samples)]
    assert count.tolist() == want


def test_empty_slices_are_plain_place(cuda_device):
    """All-empty release slices through the new entry equal ``place`` without the keywords, bit for bit."""
    pred = q.LightpathPredictor(_model(cuda_device))
    for b, thr in ((PC.batch(0), 0.12), (PC.batch(1, flagged=True), 0.05), (PC.as_batch(PC.HAND["13 cells"]()), 0.12)):
        K = len(b.samples)
        args = (b.ns.to_device(cuda_device), list(b.samples), torch.from_numpy(b.values).to(cuda_device),
                torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64)).to(cuda_device), list(b.cell_ptr))
        want, want_count = pred.place(*args, PC.FEATS, thr)
        none = torch.zeros(0, dtype=torch.int64, device=cuda_device)
        zeros = _dev([0] * (K + 1), cuda_device)
        for rel, rptr in ((none, [0] * (K + 1)), (none, zeros), (_dev([5, 6, 7], cuda_device), zeros)):
            got, count = _place(pred, args, dict(release=rel, release_ptr=rptr), thr)
            assert _same(got, want) and torch.equal(count, want_count)
        pred.check_status()


def test_releasing_a_bystander_leaves_the_row_and_releasing_an_interferer_does_not(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = PC.batch(0)
    cands, near_cands = [], []
    for k, s in enumerate(b.samples):
        near = TG.placement_neighbourhood(b.ns.data[s], b.ns.freq, PC.FI, PC.candidate_cells(b, k), 0.12)
        far = [c for c, _ in RC.lightpaths(b.ns.data[s]) if c not in near]
        cands.append((s, b.values[k], PC.candidate_cells(b, k), far[k % len(far):][:2]))
        near_cands.append((s, b.values[k], PC.candidate_cells(b, k), near[:1]))
    args, kw = _on(RC.pack(b.ns, cands), cuda_device)
    want, want_count = pred.place(*args, PC.FEATS, 0.12)
    got, count = _place(pred, args, kw, 0.12)
    assert torch.equal(got, want) and torch.equal(count, want_count)
    args, kw = _on(RC.pack(b.ns, near_cands), cuda_device)
    got, count = _place(pred, args, kw, 0.12)
    differ = [k for k, c in enumerate(near_cands) if c[3]]
    assert len(differ) >= len(cands) // 2
    for k in range(len(cands)):
        assert torch.equal(got[k], want[k]) == (k not in differ), k
    pred.check_status()


def test_the_builders_covered_rows_differ_from_plain_place(cuda_device):
    """A released interferer that went on sending its message, or a released cell that stayed occupied, would show here."""
    pred = q.LightpathPredictor(_model(cuda_device))
    for seed in (0, 1):
        b = RC.lp_batch(seed)
        args, kw = _on(b, cuda_device)
        got, _ = _place(pred, args, kw, 0.12)
        plain, plain_count = pred.place(*args, PC.FEATS, 0.12)
        assert int(pred._status.item()) == infer.LP_PLACE_OCCUPIED             # the reused cells, and nothing else
        pred._status.zero_()
        seen = [0, 0]
        for k, (interferer, reuse) in enumerate(RC.lp_cover(b)):
            if reuse:
                assert bool(torch.isnan(plain[k]).all()) and int(plain_count[k]) == 0 and bool(torch.isfinite(got[k]).all())
            elif interferer:
                assert not torch.equal(got[k], plain[k]), k
            seen[0] += reuse
            seen[1] += interferer and not reuse
        assert min(seen) >= 2


# ------------------------------------------------------------------ 2. hand-built candidates
@pytest.mark.parametrize("name", list(RC.LP_HAND))
def test_hand_cases(cuda_device, name):
    c = RC.LP_HAND[name]()
    pred = q.LightpathPredictor(_model(cuda_device))
    got, count, batch, node = _check(pred, RC.as_batch(c), cuda_device, c.thr)
    assert count.tolist() == [c.count]
    # the neighbourhood the row was summed over is the host's: the device-built graph has that in-degree at the node
    src, dst = batch.edge_index
    assert int(((dst == node[0]) & (src != node[0])).sum()) == len(c.interferers)


def test_the_cap_of_the_table_counts_survivors(cuda_device):
    """256 lightpaths with one released are accepted (survivors + 1 == 256); with an empty slice the same candidate is
    refused as plain ``place`` refuses it, with that status word."""
    pred = q.LightpathPredictor(_model(cuda_device))
    c = RC.LP_HAND["256 lightpaths, one released"]()
    good, _, batch, node = _check(pred, RC.as_batch(c), cuda_device, c.thr)
    assert int(batch.ptr[1]) == TG.MAX_LIGHTPATHS
    both = RC.join([RC.as_batch(c), RC.as_batch(c._replace(release=[])), RC.as_batch(c)])
    out, count = _place(pred, *_on(both, cuda_device), c.thr)
    assert torch.equal(out[0], good[0]) and torch.equal(out[2], good[0]) and bool(torch.isnan(out[1]).all())
    assert count.tolist() == [1, 0, 1] and int(pred._status.item()) == infer.LP_STATUS_TOO_MANY
    with pytest.raises(_lib.QotError, match=f"more than {TG.MAX_LIGHTPATHS} lightpaths"):
        pred.check_status()
    pred.check_status()


# ------------------------------------------------------------------ 3. refusals on the device
def _refused(pred, b, device, thr, bit, cause, bad=1, release=None, release_ptr=None):
    """Candidate ``bad`` of the three of ``b`` is refused with exactly ``bit``, the other two are the rows they are alone.
    ``release`` / ``release_ptr``: another layout of the lists, on the device."""
    args, kw = _on(b, device)
    alone = {}
    for k in set(range(3)) - {bad}:
        one, n = _place(pred, *_on(RC.take(b, [k]), device), thr)
        alone[k] = (one[0], int(n[0]))
        assert bool(torch.isfinite(one).all()) and int(n[0]) >= 1
    pred.check_status()
    if release_ptr is not None:
        kw = dict(release=_dev(release, device), release_ptr=_dev(release_ptr, device))
    out, count = _place(pred, args, kw, thr)
    assert bool(torch.isnan(out[bad]).all()) and int(count[bad]) == 0
    assert all(torch.equal(out[k], row) and int(count[k]) == n for k, (row, n) in alone.items())
    assert int(pred._status.item()) == bit                                     # that bit and no other
    with pytest.raises(_lib.QotError, match=cause):
        pred.check_status()
    pred.check_status()                                                        # clean on the next call


OWN_CELLS = "reroute with the same conn_id onto its own old cells"             # conn 5 on (1, 10), (2, 10), releasing 5


def _three(middle):
    last = RC.LP_HAND["a new conn_id on a released lightpath's cells"]()        # conn 40 on (1, 9), releasing 8
    return RC.join([RC.as_batch(RC.LP_HAND[OWN_CELLS]()), RC.as_batch(middle), RC.as_batch(last)])


def _other_conn(case):
    v = case.values.copy()
    v[PC.FI["conn_id"]] = 41.0
    return v


REFUSED = {
    "a released conn the sample does not hold": (lambda c: c._replace(release=[5, 6]), "LP_PLACE_NO_SUCH_CONN",
                                                 "released conn_id is no lightpath"),
    "only conns the sample does not hold": (lambda c: c._replace(release=[77], values=_other_conn(c), cells=np.array([[0], [0]])),
                                            "LP_PLACE_NO_SUCH_CONN", "released conn_id is no lightpath"),
    "a cell of a survivor": (lambda c: c._replace(release=[8], values=_other_conn(c)), "LP_PLACE_OCCUPIED", "channel is occupied"),
    "a survivor's conn_id": (lambda c: c._replace(release=[8], cells=np.array([[0], [0]])), "LP_PLACE_CONN_TAKEN",
                             "conn_id is a lightpath of the sample"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_a_refused_candidate_flags_its_row_only(cuda_device, name):
    change, bit, cause = REFUSED[name]
    pred = q.LightpathPredictor(_model(cuda_device))
    _refused(pred, _three(change(RC.LP_HAND[OWN_CELLS]())), cuda_device, 0.07, getattr(infer, bit), cause)


# the three candidates release [5], [5], [8]; the lists below give the good ones those conns and the bad one a bad slice
BAD_SLICES = {
    "descending": (1, [8, 5], [1, 2, 0, 1]),
    "beyond R": (2, [5, 5, 8], [0, 1, 2, 4]),
    "negative": (0, [5, 5, 8], [-1, 1, 2, 3]),
}


@pytest.mark.parametrize("name", list(BAD_SLICES))
def test_a_bad_slice_of_a_device_release_ptr_flags_that_row_only(cuda_device, name):
    bad, release, ptr = BAD_SLICES[name]
    pred = q.LightpathPredictor(_model(cuda_device))
    b = _three(RC.LP_HAND[OWN_CELLS]())
    assert [RC.released(b, k) for k in range(3)] == [[5], [5], [8]]
    if bad == 2:
        b = RC.take(b, [0, 2, 1])                                              # the good ones release [5] and [8]: slices 0, 1
        release = [5, 8, 5]
    _refused(pred, b, cuda_device, 0.07, infer.LP_PLACE_BAD_RELEASE, "release_ptr slice that is descending", bad, release, ptr)


def test_32_releases_are_accepted_and_33_refused(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    c = RC.LP_HAND["32 releases"]()
    _check(pred, RC.as_batch(c), cuda_device, c.thr)
    more = c._replace(release=list(range(10, 43)))                              # 33 conns, all of them in the sample
    b = RC.join([RC.as_batch(c), RC.as_batch(more), RC.as_batch(c)])
    assert b.release_ptr == [0, 32, 65, 97]
    args, kw = _on(b, cuda_device)
    with pytest.raises(ValueError, match="candidate 1 releases 33 lightpaths, at most 32"):
        pred.place(*args, PC.FEATS, c.thr, **kw)
    good = RC.join([RC.as_batch(c)] * 3)                                        # (the rows alone: of a batch the host accepts)
    _refused(pred, good, cuda_device, c.thr, infer.LP_PLACE_BAD_RELEASE, "longer than 32", 1, b.release, b.release_ptr)


def test_host_refusals_on_the_device_side(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    args, kw = _on(RC.lp_batch(0), cuda_device)
    with pytest.raises(ValueError, match="LightpathPredictor.place: release and release_ptr go together"):
        pred.place(*args, PC.FEATS, release=kw["release"])
    with pytest.raises(ValueError, match="LightpathPredictor.place: release is on cpu, the status chunk on cuda"):
        pred.place(*args, PC.FEATS, release=kw["release"].cpu(), release_ptr=kw["release_ptr"])
    with pytest.raises(ValueError, match="non-decreasing from 0 to R = 11"):
        pred.place(*args, PC.FEATS, release=kw["release"], release_ptr=kw["release_ptr"][:-1] + [12])
    with pytest.raises(TypeError):
        pred.place(*args, PC.FEATS, 0.05, kw["release"], kw["release_ptr"])    # keyword-only
    out, count = pred.place(args[0], [], args[2][:0], args[3][:, :0], [0], PC.FEATS, release=kw["release"][:0], release_ptr=[0])
    assert tuple(out.shape) == (0, 3) and tuple(count.shape) == (0,) and count.dtype == torch.int64
    pred.check_status()


# ------------------------------------------------------------------ 4. independence, the chunk is never written
def test_a_row_depends_on_its_candidate_and_its_sample_alone(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = RC.lp_batch(2)
    args, kw = _on(b, cuda_device)
    before = args[0].data.clone()
    whole, count = _place(pred, args, kw, 0.12)
    again, _ = _place(pred, args, kw, 0.12)
    assert torch.equal(whole, again)
    K = len(b.samples)
    for k in range(K):
        alone, one = _place(pred, *_on(RC.take(b, [k]), cuda_device), 0.12)
        assert torch.equal(alone[0], whole[k]) and int(one[0]) == int(count[k]), k
    order = list(reversed(range(K)))                                           # the candidates in another order
    turned, tcount = _place(pred, *_on(RC.take(b, order), cuda_device), 0.12)
    assert torch.equal(turned, whole[order]) and torch.equal(tcount, count[order])
    halves = [_place(pred, *_on(RC.take(b, ks), cuda_device), 0.12)[0] for ks in (range(0, 3), range(3, K))]   # two calls
    assert torch.equal(torch.cat(halves), whole)
    assert torch.equal(args[0].data, before)                                   # the call never writes to the chunk
    pred.check_status()


# ------------------------------------------------------------------ 5. capture
def test_capture_and_replay_on_overwritten_arguments(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b, b2 = RC.lp_batch(0), RC.lp_batch(1)                                     # the same K and shapes, other contents
    d = lambda v: _dev(v, cuda_device)                                         # noqa: E731
    (st, samples, values, cells, ptr), kw = _on(b, cuda_device)
    M, R = max(cells.shape[1], b2.cells.shape[1]), max(len(b.release), len(b2.release))
    cells = torch.cat([cells, cells.new_zeros(2, M - cells.shape[1])], 1)      # room for the other batch's lists
    rel = torch.cat([kw["release"], kw["release"].new_zeros(R - len(b.release))])
    samples, ptr, rptr = d(samples), d(ptr), d(kw["release_ptr"])
    eager, eager_count = pred.place(st, samples, values, cells, ptr, PC.FEATS, 0.12, release=rel, release_ptr=rptr)
    torch.cuda.synchronize()                                                   # (the column table was uploaded there)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, count = pred.place(st, samples, values, cells, ptr, PC.FEATS, 0.12, release=rel, release_ptr=rptr)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(count, eager_count)
    assert torch.equal(eager, _place(pred, *_on(b, cuda_device), 0.12)[0])     # (the unused tails are not read)
    st.data.copy_(torch.from_numpy(b2.ns.data))                                # in place: the captured pointers stay
    values.copy_(torch.from_numpy(b2.values))
    cells[:, :b2.cells.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(b2.cells, dtype=np.int64)))
    rel[:len(b2.release)].copy_(d(b2.release))
    samples.copy_(d(b2.samples))
    ptr.copy_(d(b2.cell_ptr))
    rptr.copy_(d(b2.release_ptr))
    graph.replay()
    torch.cuda.synchronize()
    want, want_count = _place(pred, *_on(b2, cuda_device), 0.12)
    assert torch.equal(out, want) and torch.equal(count, want_count) and not torch.equal(out, eager)
    pred.check_status()
