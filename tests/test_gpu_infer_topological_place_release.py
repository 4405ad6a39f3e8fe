"""GPU: ``TopologicalPredictor.place(..., release=, release_ptr=)`` (``csrc/infer_topological_place_release.hip``, DESIGN.md
4.24) against its definition over ``infer.materialise_placement(..., release=)``'s edited samples -- ``from_status(edited)``
and ``predict(device_batch(edited, "topological"))``, rows and link counts, bit for bit (``torch.equal``) -- and ``links``
against the host statement ``to_graph.placement_links(release=)``, on the batches and the hand cases of
``release_cases.py``; empty slices against plain ``place``; the candidates the device refuses, with the exact status word;
independence, the untouched chunk and capture.  The shapes are 6 x 12 and 4 x 80 channels."""
import numpy as np
import pytest
import torch

import gnn_qot_estimation_amd as q
import release_cases as RC
import topo_place_cases as C
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

pytestmark = pytest.mark.gpu


def _model(device, H=64, O=3, D=4, seed=0):
    """The engine's model with the oracle's state, as tests/test_gpu_infer_topological_place.py builds it."""
    from oracle import sparse as Osp
    torch.manual_seed(seed)
    ref = Osp.TopologicalGNN(TG.NUM_TOPOLOGY_NODES, H, O, D, dropout_p=0.0).eval()
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1 and p.abs().max() == 0:      # zero-init biases: make them matter
                p.uniform_(-0.1, 0.1)
    hip = q.TopologicalGNN(TG.NUM_TOPOLOGY_NODES, H, O, D, dropout_p=0.0)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return hip.to(device).eval()


def _dev(v, device):
    return torch.tensor(np.asarray(v, dtype=np.int64).reshape(-1), dtype=torch.int64, device=device)


def _on(b, device):
    """``((status, samples, values, cells, cell_ptr), {release, release_ptr})`` of a ``release_cases.Batch``: the index
    lists stay on the host."""
    return ((b.ns.to_device(device), list(b.samples), torch.from_numpy(b.values).to(device),
             torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64)).to(device), list(b.cell_ptr)),
            dict(release=_dev(b.release, device), release_ptr=list(b.release_ptr)))


def _place(pred, args, kw):
    out, links = pred.place(*args, C.FEATS, **kw)
    K = args[2].shape[0]
    assert out.dtype == torch.float32 and links.dtype == torch.int64 and out.grad_fn is None and out.device == args[0].device
    assert tuple(out.shape) == (K, pred.model.mlp[3].out_features) and tuple(links.shape) == (K,)
    return out, links


def _host_links(b):
    return [TG.placement_links(b.ns.data[s], b.values[k], RC.candidate_cells(b, k), C.FI, RC.released(b, k))[0].shape[1]
            for k, s in enumerate(b.samples)]


def _check(pred, b, device):
    """The three statements of the definition: ``from_status`` and ``predict`` over the edited samples, the host's count."""
    args, kw = _on(b, device)
    got, links = _place(pred, args, kw)
    edited = infer.materialise_placement(*args, **kw)
    want, want_links = pred.from_status(edited, features_to_consider=C.FEATS)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got, want) and torch.equal(links, want_links), (got, want, links, want_links)
    batch = TG.device_batch(edited, "topological", C.FEATS)
    assert torch.equal(got, pred(batch))
    assert torch.equal(links, (batch.edge_ptr[1:] - batch.edge_ptr[:-1]).to(device=links.device, dtype=torch.int64))
    assert links.tolist() == _host_links(b)
    pred.check_status()
    return got, links


# ------------------------------------------------------------------ 1. the definition, bit for bit
@pytest.mark.parametrize("H,O", [(16, 3), (64, 3), (64, 1)])
def test_rows_are_from_status_and_predict_of_the_edited_samples(cuda_device, H, O):
    pred = q.TopologicalPredictor(_model(cuda_device, H, O))
    b, outcomes = RC.topo_batch()
    got, links = _check(pred, b, cuda_device)
    (st, samples, values, cells, ptr), kw = _on(b, cuda_device)
    rel, rptr = kw["release"], kw["release_ptr"]
    # the builder's outcomes show against plain place of the same candidate: every one of them changes the graph
    legal = [k for k in range(len(samples)) if not np.any(b.ns.data[samples[k]][:, b.cells[0, ptr[k]], b.cells[1, ptr[k]]] != 0)
             and outcomes[k] != RC.TOPO_OUTCOMES[2]]
    plain, plain_links = pred.place(*_on(RC.take(b, legal), cuda_device)[0], C.FEATS)
    pred.check_status()
    assert len(legal) >= 8
    for j, k in enumerate(legal):
        assert not torch.equal(plain[j], got[k]), (k, outcomes[k])
        fewer = int(plain_links[j]) - int(links[k])
        assert fewer == 0 if outcomes[k] == RC.TOPO_OUTCOMES[0] else fewer >= 1, (k, outcomes[k], fewer)
    sole = [k for k in range(len(samples)) if outcomes[k] == RC.TOPO_OUTCOMES[1]]
    unedited_links = pred.from_status(st, [samples[k] for k in sole], C.FEATS)[1]
    assert (unedited_links - links[sole]).tolist() == [0] * len(sole)           # two links fewer, the candidate's two more
    d = lambda v: _dev(v, cuda_device)                                          # noqa: E731
    for s_form, p_form, r_form in ((d(samples), ptr, rptr), (samples, d(ptr), rptr), (samples, ptr, d(rptr)),
                                   (d(samples), d(ptr), d(rptr)), (tuple(samples), tuple(ptr), tuple(rptr))):
        again, again_links = _place(pred, (st, s_form, values, cells, p_form), dict(release=rel, release_ptr=r_form))
        assert torch.equal(again, got) and torch.equal(again_links, links)
    k = 5                                                                      # an int: all candidates in that sample
    one, _ = _place(pred, (st, samples[k], values[k:k + 1], cells[:, ptr[k]:ptr[k + 1]].contiguous(), [0, ptr[k + 1] - ptr[k]]),
                    dict(release=rel[rptr[k]:rptr[k + 1]], release_ptr=[0, rptr[k + 1] - rptr[k]]))
    assert torch.equal(one[0], got[k])


@pytest.mark.parametrize("H", [16, 64])
def test_empty_slices_are_plain_place(cuda_device, H):
    """All-empty release slices through the new entry equal ``place`` without the keywords, bit for bit."""
    pred = q.TopologicalPredictor(_model(cuda_device, H))
    for b in (C.batch(), C.as_batch(C.HAND["255 lightpaths and a candidate on a 256th pair"]())):
        K = len(b.samples)
        args = (b.ns.to_device(cuda_device), list(b.samples), torch.from_numpy(b.values).to(cuda_device),
                torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64)).to(cuda_device), list(b.cell_ptr))
        want, want_links = pred.place(*args, C.FEATS)
        none = torch.zeros(0, dtype=torch.int64, device=cuda_device)
        zeros = _dev([0] * (K + 1), cuda_device)
        for rel, rptr in ((none, [0] * (K + 1)), (none, zeros), (_dev([5, 6, 7], cuda_device), zeros)):
            got, links = _place(pred, args, dict(release=rel, release_ptr=rptr))
            assert torch.equal(got, want) and torch.equal(links, want_links)
        pred.check_status()


def test_releasing_a_lightpath_that_wins_no_pair_leaves_the_row(cuda_device):
    pred = q.TopologicalPredictor(_model(cuda_device))
    b = C.batch()
    cands = []
    for k, s in enumerate(b.samples):
        losers = [c for owners in RC.topo_table(b.ns.data[s]).values() for c, _ in owners[1:]]
        assert losers
        cands.append((s, b.values[k], C.candidate_cells(b, k), losers[:1 + k % 2]))
    args, kw = _on(RC.pack(b.ns, cands), cuda_device)
    want, want_links = pred.place(*args, C.FEATS)
    got, links = _place(pred, args, kw)
    assert torch.equal(got, want) and torch.equal(links, want_links)
    pred.check_status()


# ------------------------------------------------------------------ 2. hand-built candidates
@pytest.mark.parametrize("H", [16, 64])
@pytest.mark.parametrize("name", list(RC.TOPO_HAND))
def test_hand_cases(cuda_device, name, H):
    case = RC.TOPO_HAND[name]()
    pred = q.TopologicalPredictor(_model(cuda_device, H))
    got, links = _check(pred, RC.topo_as_batch(case), cuda_device)
    assert links.tolist() == [case.links]


def test_a_bad_end_node_matters_only_while_its_lightpath_stays(cuda_device):
    pred = q.TopologicalPredictor(_model(cuda_device))
    case = RC.TOPO_HAND["a released lightpath with a bad end node"]()
    args, kw = _on(RC.topo_as_batch(case), cuda_device)
    free, _ = _on(RC.topo_as_batch(case._replace(cells=np.array([[5], [11]]))), cuda_device)   # the same candidate in a free cell
    out, links = pred.place(*free, C.FEATS)                                    # plain place: the sample is refused
    assert bool(torch.isnan(out).all()) and links.tolist() == [0]
    assert int(pred._status.item()) == infer.TOPO_STATUS_BAD_ENDPOINT
    pred._status.zero_()
    out, links = _place(pred, free, dict(release=kw["release"][:0], release_ptr=[0, 0]))       # ... and with nothing released
    assert bool(torch.isnan(out).all()) and int(pred._status.item()) == infer.TOPO_STATUS_BAD_ENDPOINT
    pred._status.zero_()
    out, links = _place(pred, args, kw)
    assert bool(torch.isfinite(out).all()) and links.tolist() == [case.links]
    pred.check_status()


def test_the_cap_of_the_table_counts_survivors(cuda_device):
    """256 lightpaths with one released are accepted (the candidate takes the gone one's table slot); with an empty slice
    the same candidate is refused as plain ``place`` refuses it, with that status word."""
    pred = q.TopologicalPredictor(_model(cuda_device))
    case = RC.TOPO_HAND["256 lightpaths, one released, the candidate in its table slot"]()
    good, _ = _check(pred, RC.topo_as_batch(case), cuda_device)
    free = case._replace(release=[], cells=np.array([[3], [79]]))               # nothing released: a free cell, a full table
    b = RC.join([RC.topo_as_batch(case), RC.topo_as_batch(free), RC.topo_as_batch(case)])
    out, links = _place(pred, *_on(b, cuda_device))
    assert torch.equal(out[0], good[0]) and torch.equal(out[2], good[0]) and bool(torch.isnan(out[1]).all())
    assert links.tolist() == [case.links, 0, case.links] and int(pred._status.item()) == infer.TOPO_STATUS_TOO_MANY
    with pytest.raises(_lib.QotError, match=f"more than {TG.MAX_LIGHTPATHS} lightpaths"):
        pred.check_status()
    pred.check_status()


# ------------------------------------------------------------------ 3. refusals on the device
def _refused(pred, b, device, bit, cause, bad=1, release=None, release_ptr=None):
    """Candidate ``bad`` of the three of ``b`` is refused with exactly ``bit``, the other two are the rows they are alone.
    ``release`` / ``release_ptr``: another layout of the lists, on the device."""
    args, kw = _on(b, device)
    alone = {}
    for k in set(range(3)) - {bad}:
        one, n = _place(pred, *_on(RC.take(b, [k]), device))
        alone[k] = (one[0], int(n[0]))
        assert bool(torch.isfinite(one).all())
    pred.check_status()
    if release_ptr is not None:
        kw = dict(release=_dev(release, device), release_ptr=_dev(release_ptr, device))
    out, links = _place(pred, args, kw)
    assert bool(torch.isnan(out[bad]).all()) and int(links[bad]) == 0
    assert all(torch.equal(out[k], row) and int(links[k]) == n for k, (row, n) in alone.items())
    assert int(pred._status.item()) == bit                                     # that bit and no other
    with pytest.raises(_lib.QotError, match=cause):
        pred.check_status()
    pred.check_status()                                                        # clean on the next call


FIRST, LAST = "the winner released, the loser takes over", "reroute with the same conn_id onto its own old cell"


def _three(middle):
    return RC.join([RC.topo_as_batch(RC.TOPO_HAND[FIRST]()), RC.topo_as_batch(middle), RC.topo_as_batch(RC.TOPO_HAND[LAST]())])


def _with(case, **values):
    v = case.values.copy()
    for name, x in values.items():
        v[C.FI[name]] = x
    return v


# the hand sample holds conn 7 (1 -> 4), 9 (5 -> 2), 3 (2 -> 5) and 0 (6 -> 6); FIRST's candidate is conn 40 on (5, 11), releasing 9
REFUSED = {
    "a released conn the sample does not hold": (lambda c: c._replace(release=[9, 8]), "TOPO_PLACE_NO_SUCH_CONN",
                                                 "released conn_id is no lightpath"),
    "only conns the sample does not hold": (lambda c: c._replace(release=[-9]), "TOPO_PLACE_NO_SUCH_CONN",
                                            "released conn_id is no lightpath"),
    "a cell of a survivor": (lambda c: c._replace(cells=np.array([[5, 3], [11, 4]])), "TOPO_PLACE_OCCUPIED", "channel is occupied"),
    "a survivor's conn_id": (lambda c: c._replace(values=_with(c, conn_id=3.5)), "TOPO_PLACE_CONN_TAKEN",
                             "conn_id is a lightpath of the sample"),
    "a bad end node of the candidate": (lambda c: c._replace(values=_with(c, dst_id=76)), "TOPO_STATUS_BAD_ENDPOINT",
                                        "src_id / dst_id is not an integer"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_a_refused_candidate_flags_its_row_only(cuda_device, name):
    change, bit, cause = REFUSED[name]
    pred = q.TopologicalPredictor(_model(cuda_device))
    _refused(pred, _three(change(RC.TOPO_HAND[FIRST]())), cuda_device, getattr(infer, bit), cause)


# the three candidates release [9], [9], [9]; the lists below give the good ones that conn and the bad one a bad slice
BAD_SLICES = {
    "descending": (1, [9, 9], [1, 2, 0, 1]),
    "beyond R": (2, [9, 9, 9], [0, 1, 2, 4]),
    "negative": (0, [9, 9, 9], [-1, 1, 2, 3]),
}


@pytest.mark.parametrize("name", list(BAD_SLICES))
def test_a_bad_slice_of_a_device_release_ptr_flags_that_row_only(cuda_device, name):
    bad, release, ptr = BAD_SLICES[name]
    pred = q.TopologicalPredictor(_model(cuda_device))
    b = _three(RC.TOPO_HAND[FIRST]())
    assert [RC.released(b, k) for k in range(3)] == [[9], [9], [9]]
    _refused(pred, b, cuda_device, infer.TOPO_PLACE_BAD_RELEASE, "release_ptr slice that is descending", bad, release, ptr)


def test_32_releases_are_accepted_and_33_refused(cuda_device):
    pred = q.TopologicalPredictor(_model(cuda_device))
    case = RC.TOPO_HAND["256 lightpaths, 32 released"]()
    _check(pred, RC.topo_as_batch(case), cuda_device)
    more = case._replace(release=[1000 + 7 * k for k in range(33)])             # 33 conns, all of them in the sample
    b = RC.join([RC.topo_as_batch(case), RC.topo_as_batch(more), RC.topo_as_batch(case)])
    assert b.release_ptr == [0, 32, 65, 97]
    args, kw = _on(b, cuda_device)
    with pytest.raises(ValueError, match="candidate 1 releases 33 lightpaths, at most 32"):
        pred.place(*args, C.FEATS, **kw)
    good = RC.join([RC.topo_as_batch(case)] * 3)                                # (the rows alone: of a batch the host accepts)
    _refused(pred, good, cuda_device, infer.TOPO_PLACE_BAD_RELEASE, "longer than 32", 1, b.release, b.release_ptr)


def test_host_refusals_on_the_device_side(cuda_device):
    pred = q.TopologicalPredictor(_model(cuda_device))
    args, kw = _on(RC.topo_batch()[0], cuda_device)
    R = int(kw["release"].shape[0])
    with pytest.raises(ValueError, match="TopologicalPredictor.place: release and release_ptr go together"):
        pred.place(*args, C.FEATS, release_ptr=kw["release_ptr"])
    with pytest.raises(ValueError, match="TopologicalPredictor.place: release is on cpu, the status chunk on cuda"):
        pred.place(*args, C.FEATS, release=kw["release"].cpu(), release_ptr=kw["release_ptr"])
    with pytest.raises(ValueError, match=f"non-decreasing from 0 to R = {R}"):
        pred.place(*args, C.FEATS, release=kw["release"], release_ptr=kw["release_ptr"][:-1] + [R + 1])
    with pytest.raises(TypeError):
        pred.place(*args, C.FEATS, kw["release"], kw["release_ptr"])           # keyword-only
    out, links = pred.place(args[0], [], args[2][:0], args[3][:, :0], [0], C.FEATS, release=kw["release"][:0], release_ptr=[0])
    assert tuple(out.shape) == (0, 3) and tuple(links.shape) == (0,) and links.dtype == torch.int64
    pred.check_status()


# ------------------------------------------------------------------ 4. independence, the chunk is never written
def test_a_row_depends_on_its_candidate_and_its_sample_alone(cuda_device):
    pred = q.TopologicalPredictor(_model(cuda_device))
    b = RC.take(RC.topo_batch()[0], range(12))
    args, kw = _on(b, cuda_device)
    before = args[0].data.clone()
    whole, links = _place(pred, args, kw)
    again, _ = _place(pred, args, kw)
    assert torch.equal(whole, again)
    K = len(b.samples)
    for k in range(K):
        alone, one = _place(pred, *_on(RC.take(b, [k]), cuda_device))
        assert torch.equal(alone[0], whole[k]) and int(one[0]) == int(links[k]), k
    order = list(reversed(range(K)))                                           # the candidates in another order
    turned, tlinks = _place(pred, *_on(RC.take(b, order), cuda_device))
    assert torch.equal(turned, whole[order]) and torch.equal(tlinks, links[order])
    halves = [_place(pred, *_on(RC.take(b, ks), cuda_device))[0] for ks in (range(0, 5), range(5, K))]         # two calls
    assert torch.equal(torch.cat(halves), whole)
    assert torch.equal(args[0].data, before)                                   # the call never writes to the chunk
    pred.check_status()


# ------------------------------------------------------------------ 5. capture
def test_capture_and_replay_on_overwritten_arguments(cuda_device):
    pred = q.TopologicalPredictor(_model(cuda_device))
    b, b2 = RC.take(RC.topo_batch(0)[0], range(24)), RC.take(RC.topo_batch(1)[0], range(24))   # the same K, other contents
    d = lambda v: _dev(v, cuda_device)                                         # noqa: E731
    (st, samples, values, cells, ptr), kw = _on(b, cuda_device)
    M, R = max(cells.shape[1], b2.cells.shape[1]), max(len(b.release), len(b2.release))
    cells = torch.cat([cells, cells.new_zeros(2, M - cells.shape[1])], 1)      # room for the other batch's lists
    rel = torch.cat([kw["release"], kw["release"].new_zeros(R - len(b.release))])
    samples, ptr, rptr = d(samples), d(ptr), d(kw["release_ptr"])
    eager, eager_links = pred.place(st, samples, values, cells, ptr, C.FEATS, release=rel, release_ptr=rptr)
    torch.cuda.synchronize()                                                   # (the tables were uploaded there)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, links = pred.place(st, samples, values, cells, ptr, C.FEATS, release=rel, release_ptr=rptr)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(links, eager_links)
    assert torch.equal(eager, _place(pred, *_on(b, cuda_device))[0])           # (the unused tails are not read)
    st.data.copy_(torch.from_numpy(b2.ns.data))                                # in place: the captured pointers stay
    values.copy_(torch.from_numpy(b2.values))
    cells[:, :b2.cells.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(b2.cells, dtype=np.int64)))
    rel[:len(b2.release)].copy_(d(b2.release))
    samples.copy_(d(b2.samples))
    ptr.copy_(d(b2.cell_ptr))
    rptr.copy_(d(b2.release_ptr))
    graph.replay()
    torch.cuda.synchronize()
    want, want_links = _place(pred, *_on(b2, cuda_device))
    assert torch.equal(out, want) and torch.equal(links, want_links) and not torch.equal(out, eager)
    pred.check_status()
