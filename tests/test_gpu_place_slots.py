"""GPU: ``LightpathPredictor.place_slots`` (``csrc/infer_lightpath_place_slots.hip``) against its
definition, bit for bit (``torch.equal``, NaN compared as NaN): ``out[route[k], slot[k]]`` is ``place``'s row for the
explicit lists ``infer.materialise_slot_sweep`` builds, every other row NaN, ``free`` the host statement's
(``to_graph.slot_sweep``), ``count`` ``place``'s; independence of ``chunk`` and of the other routes; the hand cases;
refused routes alone among good ones; ``status.data`` untouched; capture.  Every shape is ``place_cases``' 4 x 70 grid."""
import numpy as np
import pytest
import torch

import gnn_qot_estimation_amd as q
import place_slots_cases as SC
import status_infer_cases as SK
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

pytestmark = pytest.mark.gpu
SHAPES = [(32, 3), (20, 1)]                                                    # (C = 20: the engine's padded width)


def _model(device, C=32, O=3, seed=0):
    """An engine model with every parameter and running statistic made to matter."""
    torch.manual_seed(seed)
    hip = q.LightpathGNN(5, C, O, SC.LUT_COL, dropout_p=0.0)
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


def _all_same(r, want):
    return all(_same(x, y) for x, y in zip(r, want))


def _on(b, device):
    """``(status, samples, values, links, link_ptr)`` of ``b`` for a call: the tensors on the device, the lists as lists."""
    return (b.ns.to_device(device), list(b.samples), torch.from_numpy(b.values).to(device),
            torch.from_numpy(np.ascontiguousarray(b.links, dtype=np.int64)).to(device), list(b.link_ptr))


def _sweep(pred, args, thr, **kw):
    r = pred.place_slots(*args, SC.FEATS, thr, **kw)
    st, R = args[0], args[2].shape[0]
    Q, O = st.data.shape[3], pred.model.mlp[3].out_features
    assert isinstance(r, infer.PlaceSlots)
    want = dict(out=(torch.float32, (R, Q, O)), free=(torch.bool, (R, Q)), count=(torch.int64, (R,)))
    for name, (dtype, shape) in want.items():
        t = getattr(r, name)
        assert t.dtype == dtype and tuple(t.shape) == shape and t.device == st.device and t.grad_fn is None, name   # 7.
    return r


def _definition(pred, args, thr, width=1, slot_feature="freq"):
    """``PlaceSlots`` by the definition: the explicit lists of every free (route, start slot), scored by ``place``."""
    st, R = args[0], args[2].shape[0]
    Q, O = st.data.shape[3], pred.model.mlp[3].out_features
    sw = infer.materialise_slot_sweep(*args, width=width, slot_feature=slot_feature)
    rows, count = pred.place(st, sw.samples, sw.values, sw.cells, sw.cell_ptr, SC.FEATS, thr)
    pred.check_status()                                                         # every listed candidate is a legal one
    out = torch.full((R, Q, O), float("nan"), dtype=torch.float32, device=st.device)
    out[sw.route, sw.slot] = rows
    return infer.PlaceSlots(out, sw.free, count), sw


def _check(pred, b, device, thr, width=1, slot_feature="freq", **kw):
    args = _on(b, device)
    clone = args[0].data.clone()
    r = _sweep(pred, args, thr, width=width, slot_feature=slot_feature, **kw)
    want, sw = _definition(pred, args, thr, width, slot_feature)
    assert torch.equal(r.free, want.free), (r.free, want.free)
    assert _same(r.out, want.out), (r.out, want.out)
    assert torch.equal(torch.isnan(r.out).any(2), ~r.free) and torch.equal(torch.isnan(r.out).all(2), ~r.free)
    if sw.route.numel():                                                        # count[r] is place's, at every slot of r
        assert torch.equal(r.count[sw.route], want.count)
    assert torch.equal(args[0].data, clone)                                     # 7. the call never writes to the chunk
    pred.check_status()                                                         # an occupied slot sets no bit
    return r, sw, args


def _host_free(b, width):
    return torch.from_numpy(np.stack([TG.slot_sweep(b.ns.data[s], b.ns.freq, SC.FI, SC.route_links(b, r), 0.05, width)[0]
                                      for r, s in enumerate(b.samples)]))


# ------------------------------------------------------------------ 1. the definition, bit for bit
@pytest.mark.parametrize("slot_feature", ["freq", None])
@pytest.mark.parametrize("width", SC.WIDTHS)
@pytest.mark.parametrize("thr", SC.THRESHOLDS)
@pytest.mark.parametrize("C,O", SHAPES)
def test_rows_are_place_of_the_materialised_sweep(cuda_device, C, O, thr, width, slot_feature):
    pred = q.LightpathPredictor(_model(cuda_device, C, O))
    b = SC.batch(0, flagged=(width == 2))
    r, sw, _ = _check(pred, b, cuda_device, thr, width, slot_feature)
    assert torch.equal(r.free.cpu(), _host_free(b, width))                      # 2. free is the host statement's
    band = r.free[:, SC.BAND0:]
    assert 0.25 <= float(band.float().mean()) <= 0.75                           # free and occupied slots both, in the band
    assert r.count.tolist() == [1 + (width == 2)] * len(b.samples)


def test_the_sweep_sees_the_thresholds_the_slot_and_the_width(cuda_device):
    """Were the rows not to depend on the messages, on the start slot's frequency or on the width, a sweep that found
    nobody, or that scored one slot for all, would go unseen."""
    pred = q.LightpathPredictor(_model(cuda_device))
    args = _on(SC.batch(1), cuda_device)
    near, far = _sweep(pred, args, 0.05), _sweep(pred, args, 0.12)
    assert torch.equal(near.free, far.free) and not _same(near.out, far.out)
    plain = _sweep(pred, args, 0.12, slot_feature=None)
    assert torch.equal(plain.free, far.free) and not _same(plain.out, far.out)
    empty = plain.out[0, :40]                                                   # below the band nobody is near: with
    assert bool(near.free[0, :40].all()) and bool((empty == empty[0]).all())    # equal values the rows are equal,
    assert not bool((far.out[0, :40] == far.out[0, 0]).all())                   # with the slot's frequency they are not
    wide = _sweep(pred, args, 0.12, width=2)
    assert int(wide.free.sum()) < int(far.free.sum()) and bool((wide.free <= far.free).all())
    pred.check_status()


# ------------------------------------------------------------------ 2. free against the host statement
def test_free_is_the_host_statement_on_partly_blocked_slots(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b, width, not_free = SC.blocked_in_parts()
    r, _, _ = _check(pred, b, cuda_device, 0.07, width)
    assert set(torch.nonzero(~r.free[0]).flatten().tolist()) == not_free        # one link only; the second width-slot; Q - 1
    assert torch.equal(r.free.cpu(), _host_free(b, width))
    for w in (1, 3, 8):
        r, _, _ = _check(pred, b, cuda_device, 0.07, w)
        assert torch.equal(r.free.cpu(), _host_free(b, w))
        assert not bool(r.free[0, SC.Q - w + 1:].any()) and bool(r.free[0, SC.Q - w])    # the last w - 1 start slots


# ------------------------------------------------------------------ 3. chunk
@pytest.mark.parametrize("width", SC.WIDTHS)
def test_results_do_not_depend_on_chunk(cuda_device, width):
    pred = q.LightpathPredictor(_model(cuda_device))
    args = _on(SC.batch(2, flagged=True), cuda_device)
    whole = _sweep(pred, args, 0.12, width=width)
    assert bool(whole.free.any()) and not bool(whole.free.all())
    for chunk in (1, 5, 32):                                                    # Q = 70 is ragged for 5 and for 32
        assert _all_same(_sweep(pred, args, 0.12, width=width, chunk=chunk), whole), chunk
    pred.check_status()
    with pytest.raises(ValueError, match="chunk must be None or an int"):
        pred.place_slots(*args, SC.FEATS, 0.12, chunk=33)


# ------------------------------------------------------------------ 4. the other routes
def test_a_route_depends_on_itself_and_its_sample_alone(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = SC.batch(0)
    assert len(set(b.samples)) < len(b.samples)                                 # a condition on the inputs: repeats
    args = _on(b, cuda_device)
    whole = _sweep(pred, args, 0.12, width=2)
    st, samples, values, links, ptr = args
    for r in range(len(samples)):
        alone = _sweep(pred, (st, [samples[r]], values[r:r + 1], links[ptr[r]:ptr[r + 1]], [0, ptr[r + 1] - ptr[r]]), 0.12,
                       width=2)
        assert _all_same(alone, [t[r:r + 1] for t in whole]), r
    # the index arguments in every form give the same bits
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda_device)      # noqa: E731
    for s_form, p_form in ((tuple(samples), tuple(ptr)), (dev(samples), dev(ptr)), (dev(samples), ptr)):
        assert _all_same(_sweep(pred, (st, s_form, values, links, p_form), 0.12, width=2), whole)
    one = _sweep(pred, (st, 1, values, links, ptr), 0.12)
    assert _all_same(one, _sweep(pred, (st, [1] * len(samples), values, links, ptr), 0.12))
    pred.check_status()


# ------------------------------------------------------------------ 5. hand cases
def test_a_sample_without_lightpaths(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = SC.empty_sample()
    r, sw, _ = _check(pred, b, cuda_device, 0.12)
    assert bool(r.free.all()) and r.count.tolist() == [1] and bool(torch.isfinite(r.out).all())
    plain, _, _ = _check(pred, b, cuda_device, 0.12, slot_feature=None)
    assert bool((plain.out == plain.out[0, 0]).all())                           # the self loop only: one row for all slots


def test_a_route_without_a_free_slot_is_no_error(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    r, _, _ = _check(pred, SC.full_route(), cuda_device, 0.12)
    assert not bool(r.free.any()) and bool(torch.isnan(r.out).all()) and r.count.tolist() == [1]
    assert int(pred._status.item()) == 0
    pred.check_status()                                                         # does not raise


def test_a_duplicate_link_changes_nothing(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = SC.batch(0)
    ns, s = b.ns, b.samples[0]
    once = SC.single(ns, [2, 0], b.values[0], s)
    r, _, _ = _check(pred, once, cuda_device, 0.12, 2)
    for links in ([2, 0, 2], [0, 2, 0, 0, 2]):
        twice, _, _ = _check(pred, SC.single(ns, links, b.values[0], s), cuda_device, 0.12, 2)
        assert _all_same(twice, r), links


def test_69_messages_cross_the_64_message_chunk(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b, thr, slot = SC.crowded_link()
    r, sw, _ = _check(pred, b, cuda_device, thr)
    assert torch.nonzero(r.free[0]).flatten().tolist() == [slot] and bool(torch.isfinite(r.out[0, slot]).all())
    assert len(TG.slot_sweep(b.ns.data[0], b.ns.freq, SC.FI, b.links, thr)[1][slot]) == 69
    fewer, _, _ = _check(pred, b, cuda_device, 0.12)                            # four of them: another row
    assert not torch.equal(fewer.out[0, slot], r.out[0, slot])


def test_a_repeated_frequency_names_nobody(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b, thr = SC.repeated_frequency()
    r, _, args = _check(pred, b, cuda_device, thr)
    near = TG.slot_sweep(b.ns.data[0], b.ns.freq, SC.FI, b.links, thr)[1]
    assert near[11] == [8] and near[9] == [8] and near[13] == []
    # start slot 11 sums conn 8's message alone: the row of the same candidate in the sample without conn 9
    data = b.ns.data.copy()
    data[0, :, 1, 12] = 0.0
    without = _sweep(pred, _on(b._replace(ns=SK.status(data, b.ns.freq)), cuda_device), thr)
    assert torch.equal(without.out[0, 11], r.out[0, 11]) and bool(without.free[0, 12]) and not bool(r.free[0, 12])


# ------------------------------------------------------------------ 6. refusals on the device
def _refused(r, k):
    return bool(torch.isnan(r.out[k]).all()) and not bool(r.free[k].any()) and int(r.count[k]) == 0


def _good_routes():
    return SC.single(SC.batch(0).ns, [1, 3], sample=1), SC.blocked_in_parts()[0]


def _among_good(pred, device, bad, cause, bit, thr=0.12):
    """``bad`` (one route) between two good ones: it alone is refused, the others are bit-equal to a run without it."""
    first, last = _good_routes()
    good = _sweep(pred, _on(SC.join([first, last]), device), thr, width=2)
    assert bool(good.free.any()) and not bool(good.free.all()) and int(pred._status.item()) == 0
    st, samples, values, links, ptr = _on(SC.join([first, bad._replace(samples=[0]), last]), device)
    if bad.samples[0] != 0:                                                     # a sample number outside the chunk
        samples[1] = -1 if bad.samples[0] < 0 else int(st.data.shape[0])
    for chunk in (None, 7):
        r = _sweep(pred, (st, samples, values, links, ptr), thr, width=2, chunk=chunk)
        assert _refused(r, 1)
        assert _all_same([t[[0, 2]] for t in r], good)
        assert int(pred._status.item()) == getattr(infer, bit)                  # the word carries that bit and no other
        with pytest.raises(_lib.QotError, match=cause):
            pred.check_status()
        pred.check_status()                                                     # clean on the next call


@pytest.mark.parametrize("name", list(SC.refusals()))
def test_a_refused_route_flags_its_rows_only(cuda_device, name):
    bit, cause, bad = SC.refusals()[name]
    _among_good(q.LightpathPredictor(_model(cuda_device)), cuda_device, bad, cause, bit)


@pytest.mark.parametrize("name,end", [("empty", 6), ("descending", 5), ("beyond M", 9)])
def test_a_bad_slice_of_a_device_link_ptr_flags_that_route_only(cuda_device, name, end):
    pred = q.LightpathPredictor(_model(cuda_device))
    first, last = _good_routes()
    st, samples, values, links, ptr = _on(SC.join([first, last, first, last]), cuda_device)
    assert ptr == [0, 2, 4, 6, 8]
    good = _sweep(pred, (st, samples, values, links, torch.tensor(ptr, device=cuda_device)), 0.12)
    r = _sweep(pred, (st, samples, values, links, torch.tensor(ptr[:4] + [end], device=cuda_device)), 0.12)   # route 3: links[6:end]
    assert _refused(r, 3) and _all_same([t[:3] for t in r], [t[:3] for t in good]) and bool(good.free[3].any())
    assert int(pred._status.item()) == infer.LP_PLACE_BAD_CELL
    with pytest.raises(_lib.QotError, match="place: a link or frequency index outside the sample, or a cell_ptr slice"):
        pred.check_status()
    pred.check_status()


# ------------------------------------------------------------------ 8. capture
def test_capture_and_replay_on_overwritten_arguments(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b, b2 = SC.batch(0), SC.batch(1, flagged=True)                              # the same shapes, other contents
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda_device)      # noqa: E731
    st, _, values, links, _ = _on(b, cuda_device)
    samples, ptr = dev(b.samples), dev(b.link_ptr)
    eager = pred.place_slots(st, samples, values, links, ptr, SC.FEATS, 0.12, width=2)      # (the column table is uploaded here)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = pred.place_slots(st, samples, values, links, ptr, SC.FEATS, 0.12, width=2)
        first_fit = r.free.int().argmax(1)                                      # the README's use: no host read
        best = r.out[..., 0].masked_fill(~r.free, float("-inf")).argmax(1)
    graph.replay()
    torch.cuda.synchronize()
    assert _all_same(r, eager)
    st.data.copy_(torch.from_numpy(b2.ns.data))                                 # in place: the captured pointers stay
    samples.copy_(dev(b.samples[::-1]))
    values.copy_(torch.from_numpy(b2.values))
    graph.replay()
    torch.cuda.synchronize()
    want = _sweep(pred, (b2.ns.to_device(cuda_device), b.samples[::-1], torch.from_numpy(b2.values).to(cuda_device),
                         links, list(b.link_ptr)), 0.12, width=2)
    assert _all_same(r, want) and not _same(r.out, eager.out) and not torch.equal(r.free, eager.free)
    assert r.count.tolist() == [2] * len(b.samples)
    assert torch.equal(first_fit, want.free.int().argmax(1))
    assert torch.equal(best, want.out[..., 0].masked_fill(~want.free, float("-inf")).argmax(1))
    pred.check_status()


# ------------------------------------------------------------------ empty input
def test_no_routes_no_launch(cuda_device, monkeypatch):
    pred = q.LightpathPredictor(_model(cuda_device))
    st, _, values, links, _ = _on(SC.batch(0), cuda_device)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for none in ([], torch.zeros(0, dtype=torch.int64, device=cuda_device)):
        r = pred.place_slots(st, none, values[:0], links[:0], [0], SC.FEATS)
        assert [tuple(t.shape) for t in r] == [(0, SC.Q, 3), (0, SC.Q), (0,)]
        assert [t.dtype for t in r] == [torch.float32, torch.bool, torch.int64]
    monkeypatch.undo()
    assert calls == []
    with pytest.raises(ValueError, match="links is on cpu"):
        pred.place_slots(st, 0, values[:1], links[:1].cpu(), [0, 1], SC.FEATS)
    with pytest.raises(TypeError):
        pred.place_slots(st, 0, values[:1], links[:1], [0, 1], SC.FEATS, 0.05, 2)           # width is keyword-only
    with pytest.raises(TypeError):
        pred.place_slots(st, 0, values[:1], links[:1], [0, 1], release=None)
    pred.check_status()
