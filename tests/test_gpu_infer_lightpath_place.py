"""GPU: ``LightpathPredictor.place`` (``csrc/infer_lightpath_place.hip``) against its definition over
``infer.materialise_placement``'s edited samples, bit for bit (``torch.equal``, NaN rows compared as NaN): the row of the
candidate's node in ``predict(to_graph.device_batch(edited, "lightpath", ...))`` and, where the candidate is the first-seen
flagged lightpath of its edited sample, ``from_status(edited)``; the hand cases of ``place_cases.py``; refused candidates
alone among good ones; independence, parameter following and capture.  Every shape is a dozen lightpaths on a 4 x 70
grid, or the smallest that reaches the path it names."""
import numpy as np
import pytest
import torch

import gnn_qot_estimation_amd as q
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


def _place(pred, args, thr):
    out, count = pred.place(*args, PC.FEATS, thr)
    K = args[2].shape[0]
    assert out.dtype == torch.float32 and count.dtype == torch.int64 and out.grad_fn is None and out.device == args[0].device
    assert tuple(out.shape) == (K, pred.model.mlp[3].out_features) and tuple(count.shape) == (K,)
    return out, count


def _via_predict(pred, b, args, thr):
    """The definition: the row ``predict`` gives the candidate's node in the device-built graph of its edited sample, and
    the LUT nodes of that graph."""
    edited = infer.materialise_placement(*args)
    batch = TG.device_batch(edited, "lightpath", PC.FEATS, None, thr)
    out, lut_batch = pred(batch)
    nodes = [TG.place_lightpath(b.ns.data[s], b.values[k], PC.candidate_cells(b, k), PC.FI)[1] for k, s in enumerate(b.samples)]
    node = batch.ptr.to(out.device)[:-1] + torch.tensor(nodes, device=out.device)
    luts = pred.model._lut_rows(batch)
    row = torch.searchsorted(luts, node)
    assert torch.equal(luts[row], node)                                        # the candidate's node is a LUT node
    return out[row], torch.bincount(lut_batch, minlength=len(b.samples)), edited, batch, node


def _check(pred, b, device, thr, first_seen=True):
    args = _on(b, device)
    got, count = _place(pred, args, thr)
    want, want_count, edited, batch, node = _via_predict(pred, b, args, thr)
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
        b = PC.batch(seed)
        got, count, _, _ = _check(pred, b, cuda_device, thr)
        assert count.tolist() == [1] * len(b.samples)
        st, samples, values, cells, ptr = _on(b, cuda_device)
        dev = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda_device)  # noqa: E731
        for s_form, p_form in ((dev(samples), ptr), (samples, dev(ptr)), (dev(samples), dev(ptr)), (tuple(samples), tuple(ptr))):
            again, _ = _place(pred, (st, s_form, values, cells, p_form), thr)
            assert torch.equal(again, got)
        k = samples.index(samples[0], 1) if samples[0] in samples[1:] else 0    # an int: all candidates in that sample
        one, _ = _place(pred, (st, samples[k], values[k:k + 1], cells[:, ptr[k]:ptr[k + 1]].contiguous(),
                               [0, ptr[k + 1] - ptr[k]]), thr)
        assert torch.equal(one[0], got[k])


def test_the_thresholds_tell_rows_apart(cuda_device):
    """At 0.12 a row has the messages of two slots either side, at 0.05 at most one: rows whose neighbourhoods differ between
    the two must differ, the others must not."""
    pred = q.LightpathPredictor(_model(cuda_device))
    b = PC.batch(0)
    args = _on(b, cuda_device)
    wide, narrow = _place(pred, args, 0.12)[0], _place(pred, args, 0.05)[0]
    differ = 0
    for k, s in enumerate(b.samples):
        n = [TG.placement_neighbourhood(b.ns.data[s], b.ns.freq, PC.FI, PC.candidate_cells(b, k), t) for t in (0.12, 0.05)]
        assert torch.equal(wide[k], narrow[k]) == (n[0] == n[1]), k
        differ += n[0] != n[1]
    assert differ >= len(b.samples) // 2


@pytest.mark.parametrize("thr", PC.THRESHOLDS)
def test_rows_behind_a_flagged_lightpath_of_the_sample(cuda_device, thr):
    """The samples hold a lower-numbered flagged lightpath: count == 2, the candidate's row is still its node's, and
    ``from_status`` of the edited sample answers for the other one."""
    pred = q.LightpathPredictor(_model(cuda_device))
    b = PC.batch(1, flagged=True)
    got, count, batch, node = _check(pred, b, cuda_device, thr, first_seen=False)
    assert count.tolist() == [2] * len(b.samples) and bool((node > batch.ptr.to(node.device)[:-1]).all())
    edited = infer.materialise_placement(*_on(b, cuda_device))
    other, _ = pred.from_status(edited, None, PC.FEATS, thr)
    assert all(not torch.equal(other[k], got[k]) for k in range(len(b.samples)))


# ------------------------------------------------------------------ 2. hand-built candidates
@pytest.mark.parametrize("name", list(PC.HAND))
def test_hand_cases(cuda_device, name):
    c = PC.HAND[name]()
    pred = q.LightpathPredictor(_model(cuda_device))
    got, count, batch, node = _check(pred, PC.as_batch(c), cuda_device, c.thr, first_seen=c.count == 1)
    assert count.tolist() == [c.count]
    # the neighbourhood the row was summed over is the host's: the device-built graph has that in-degree at the node
    src, dst = batch.edge_index
    assert int(((dst == node[0]) & (src != node[0])).sum()) == len(c.interferers)


def test_a_message_more_changes_the_row(cuda_device):
    """A mark lost or doubled by a wave would go unseen if the rows did not depend on it: the 13-cell candidate without
    its last cell's private interferers, or with one lightpath of the sample gone, is another row."""
    pred = q.LightpathPredictor(_model(cuda_device))
    c = PC.HAND["13 cells"]()
    full, _, _, _ = _check(pred, PC.as_batch(c), cuda_device, c.thr)
    gone = c.ns.data.copy()
    conn = gone[0, PC.FI["conn_id"]]
    gone[0][:, conn == c.interferers[-1]] = 0.0                                # the last message of the row
    less, _, _, _ = _check(pred, PC.as_batch(c._replace(ns=PC.SK.status(gone, c.ns.freq))), cuda_device, c.thr)
    assert not torch.equal(full, less)


def test_256_lightpaths_with_the_candidate_are_accepted_257_refused(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    c = PC.crowd(255)
    got, count, batch, node = _check(pred, PC.as_batch(c), cuda_device, c.thr)
    assert int(batch.ptr[1]) == TG.MAX_LIGHTPATHS and int(node[0]) == 255 and count.tolist() == [1]
    full = PC.crowd(256)
    both = PC.join([c, full, c])
    out, count = _place(pred, _on(both, cuda_device), c.thr)
    assert torch.equal(out[0], got[0]) and torch.equal(out[2], got[0]) and bool(torch.isnan(out[1]).all())
    assert count.tolist() == [1, 0, 1]
    with pytest.raises(_lib.QotError, match=f"more than {TG.MAX_LIGHTPATHS} lightpaths"):
        pred.check_status()
    pred.check_status()                                                        # the word was cleared


# ------------------------------------------------------------------ 3. refusals on the device
GOOD = ("one cell", "interferers at slot 64 and above")


def _alone(pred, device, names=GOOD):
    cases = [PC.HAND[n]() for n in names]
    return cases, [_place(pred, _on(PC.as_batch(c), device), 0.12)[0][0] for c in cases]


def _refused_in_the_middle(pred, args, alone, cause):
    out, count = _place(pred, args, 0.12)
    assert bool(torch.isnan(out[1]).all()) and count.tolist() == [1, 0, 1]
    assert torch.equal(out[0], alone[0]) and torch.equal(out[2], alone[1])
    with pytest.raises(_lib.QotError, match=cause):
        pred.check_status()
    pred.check_status()                                                        # clean on the next call


@pytest.mark.parametrize("name", list(PC.refusals()))
def test_a_refused_candidate_flags_its_row_only(cuda_device, name):
    bit, cause, bad = PC.refusals()[name]
    pred = q.LightpathPredictor(_model(cuda_device))
    cases, alone = _alone(pred, cuda_device)
    args = _on(PC.join([cases[0], bad, cases[1]]), cuda_device)
    _refused_in_the_middle(pred, args, alone, cause)
    # the word carries that bit and no other
    pred.place(*args, PC.FEATS, 0.12)
    assert int(pred._status.item()) == getattr(infer, bit)
    pred._status.zero_()


@pytest.mark.parametrize("sample", [3, -1])
def test_a_sample_number_outside_the_chunk_flags_that_row_only(cuda_device, sample):
    pred = q.LightpathPredictor(_model(cuda_device))
    cases, alone = _alone(pred, cuda_device)
    st, samples, values, cells, ptr = _on(PC.join([cases[0], cases[0], cases[1]]), cuda_device)
    _refused_in_the_middle(pred, (st, [0, sample, 2], values, cells, ptr), alone, "sample number")


def test_a_bad_slice_of_a_device_cell_ptr_flags_that_row_only(cuda_device):
    """A ``cell_ptr`` on the device is the kernel's to check: an empty slice in the middle; a slice that runs beyond M or
    descends, at the end."""
    pred = q.LightpathPredictor(_model(cuda_device))
    cases, alone = _alone(pred, cuda_device)
    st, samples, values, cells, ptr = _on(PC.join([cases[0], cases[0], cases[1]]), cuda_device)
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda_device)      # noqa: E731
    keep = torch.tensor([0, 2], device=cuda_device)
    _refused_in_the_middle(pred, (st, samples, values, cells[:, keep].contiguous(), dev([0, 1, 1, 2])), alone,
                           "cell_ptr slice that is empty")
    for last in (4, 1, -2):                                                    # M = 3: beyond it, descending, negative
        out, count = _place(pred, (st, [0, 2, 1], values[[0, 2, 1]], cells[:, [0, 2, 1]].contiguous(), dev([0, 1, 2, last])), 0.12)
        assert torch.equal(out[0], alone[0]) and torch.equal(out[1], alone[1]) and bool(torch.isnan(out[2]).all())
        assert count.tolist() == [1, 1, 0]
        with pytest.raises(_lib.QotError, match="cell_ptr slice that is empty, descending or beyond"):
            pred.check_status()


def test_no_candidates_no_launch_and_host_refusals_on_the_device_side(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    st, samples, values, cells, ptr = _on(PC.batch(0), cuda_device)
    for none in ([], torch.zeros(0, dtype=torch.int64, device=cuda_device)):
        out, count = pred.place(st, none, values[:0], cells[:, :0], [0], PC.FEATS)
        assert tuple(out.shape) == (0, 3) and tuple(count.shape) == (0,) and count.dtype == torch.int64
    with pytest.raises(TypeError, match="DeviceStatus"):
        pred.place(PC.batch(0).ns, samples, values, cells, ptr)
    with pytest.raises(ValueError, match="values is on cpu"):
        pred.place(st, samples, values.cpu(), cells, ptr)
    with pytest.raises(infer.EnvelopeError, match="on the CPU"):
        pred.place(PC.batch(0).ns.to_device("cpu"), samples, values.cpu(), cells.cpu(), ptr)
    with pytest.raises(ValueError, match="finite positive"):
        pred.place(st, samples, values, cells, ptr, freq_threshold=0.0)
    with pytest.raises(ValueError, match="empty slice"):
        pred.place(st, samples, values, cells, [0] + ptr[1:-2] + [ptr[-1], ptr[-1]])
    with pytest.raises(infer.EnvelopeError, match="in_channels"):
        pred.place(st, samples, values, cells, ptr, ["freq"])
    pred.check_status()


# ------------------------------------------------------------------ 4. independence, reproducibility, parameters
def test_a_row_depends_on_its_candidate_and_its_sample_alone(cuda_device):
    hip = _model(cuda_device)
    pred = q.LightpathPredictor(hip)
    b = PC.batch(2)
    st, samples, values, cells, ptr = _on(b, cuda_device)
    before = st.data.clone()
    whole, count = _place(pred, (st, samples, values, cells, ptr), 0.12)
    again, _ = _place(pred, (st, samples, values, cells, ptr), 0.12)
    assert torch.equal(whole, again)
    for k in range(len(samples)):
        alone, one = _place(pred, (st, [samples[k]], values[k:k + 1], cells[:, ptr[k]:ptr[k + 1]].contiguous(),
                                   [0, ptr[k + 1] - ptr[k]]), 0.12)
        assert torch.equal(alone[0], whole[k]) and int(one[0]) == int(count[k]), k
    order = list(reversed(range(len(samples))))                                # the candidates in another order
    rcells = torch.cat([cells[:, ptr[k]:ptr[k + 1]] for k in order], 1)
    rptr = np.cumsum([0] + [ptr[k + 1] - ptr[k] for k in order]).tolist()
    turned, _ = _place(pred, (st, [samples[k] for k in order], values[order], rcells, rptr), 0.12)
    assert torch.equal(turned, whole[order])
    assert torch.equal(st.data, before)                                        # the call never writes to the chunk
    with torch.no_grad():                                                      # a parameter updated in place is seen
        hip.mlp[3].bias.add_(0.25)
        hip.norm1.module.running_mean.mul_(0.5)
    moved, _, _, _ = _check(pred, b, cuda_device, 0.12)
    assert not torch.equal(moved, whole)
    pred.check_status()


# ------------------------------------------------------------------ 5. capture
def test_capture_and_replay_on_overwritten_arguments(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    b, b2 = PC.batch(0), PC.batch(1)                                           # the same K and shapes, other contents
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda_device)      # noqa: E731
    st, samples, values, cells, ptr = _on(b, cuda_device)
    M = max(cells.shape[1], b2.cells.shape[1])
    cells = torch.cat([cells, cells.new_zeros(2, M - cells.shape[1])], 1)      # room for the other batch's cells
    samples, ptr = dev(samples), dev(ptr)
    eager, eager_count = pred.place(st, samples, values, cells, ptr, PC.FEATS, 0.12)   # (the column table is uploaded here)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, count = pred.place(st, samples, values, cells, ptr, PC.FEATS, 0.12)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(count, eager_count)
    assert torch.equal(eager, _place(pred, _on(b, cuda_device), 0.12)[0])       # (the unused tail of cells is not read)
    st.data.copy_(torch.from_numpy(b2.ns.data))                                # in place: the captured pointers stay
    values.copy_(torch.from_numpy(b2.values))
    cells[:, :b2.cells.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(b2.cells, dtype=np.int64)))
    samples.copy_(dev(b2.samples))
    ptr.copy_(dev(b2.cell_ptr))
    graph.replay()
    torch.cuda.synchronize()
    want, want_count = _place(pred, _on(b2, cuda_device), 0.12)
    assert torch.equal(out, want) and torch.equal(count, want_count) and not torch.equal(out, eager)
    pred.check_status()
