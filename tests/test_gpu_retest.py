"""GPU: ``LightpathPredictor.retest`` (``csrc/infer_lightpath_retest.hip``) against its definition, bit for
bit (``torch.equal``, NaN compared as NaN): ``out[g, i]`` is the row ``predict`` gives the lightpath's node in the
device-built graph of ``infer.materialise_retest``'s sample, ``conn`` / ``n`` the host statement's
(``to_graph.retest_neighbourhood``), ``count`` ``from_status``'s; ``place_impact``'s ``before``; named mode against gathered
all-mode rows; independence of ``chunk`` and ``max_lightpaths``; refused samples alone among good ones; capture.  Every
shape is a dozen lightpaths on a 4 x 70 grid, or the smallest that reaches the path it names."""
import numpy as np
import pytest
import torch

import gnn_qot_estimation_amd as q
import impact_cases as IC
import place_cases as PC
import retest_cases as RC
import status_infer_cases as SK
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

pytestmark = pytest.mark.gpu
SHAPES = [(32, 3), (20, 1)]                                                    # (C = 20: the engine's padded width)
NAN = float("nan")


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


def _all_same(r, want):
    return all(_same(x, y) for x, y in zip(r, want))


def _retest(pred, st, thr, samples=None, conns=None, M=256, **kw):
    r = pred.retest(st, samples, conns, RC.FEATS, thr, M, **kw)
    G = st.data.shape[0] if samples is None else len(samples)
    M = M if conns is None else conns.shape[1]
    O, dev = pred.model.mlp[3].out_features, st.device
    assert isinstance(r, infer.Retest)
    want = dict(out=(torch.float32, (G, M, O)), conn=(torch.int64, (G, M)), n=(torch.int64, (G,)), count=(torch.int64, (G,)))
    for name, (dtype, shape) in want.items():
        t = getattr(r, name)
        assert t.dtype == dtype and tuple(t.shape) == shape and t.device == dev and t.grad_fn is None, name
    return r


def _rows_of(pred, retest, nodes, thr):
    """The rows ``predict`` gives node ``nodes[t]`` of the device-built graph of retest sample ``t``."""
    batch = TG.device_batch(retest, "lightpath", RC.FEATS, None, thr)
    out, _ = pred(batch)
    node = batch.ptr.to(out.device)[:-1] + torch.tensor(nodes, device=out.device)
    luts = pred.model._lut_rows(batch)
    row = torch.searchsorted(luts, node)
    assert torch.equal(luts[row], node)                                        # the retested lightpath's node is a LUT node
    return out[row]


def _definition(pred, ns, st, thr, M=256):
    """``(out, conn, n, count)`` by the definition: the host statement names each sample's lightpaths and their nodes,
    ``materialise_retest`` builds one sample per (sample, lightpath) pair -- all pairs in one call -- and ``predict`` scores
    their device-built graphs."""
    G, O, dev = ns.data.shape[0], pred.model.mlp[3].out_features, st.device
    hosts = [RC.host(ns, g, thr) for g in range(G)]
    conn = torch.full((G, M), -1, dtype=torch.int64)
    out = torch.full((G, M, O), NAN, dtype=torch.float32, device=dev)
    pairs = [(g, i) for g in range(G) for i in range(min(len(hosts[g]), M))]
    for g, i in pairs:
        conn[g, i] = hosts[g][i][0]
    if pairs:
        which = torch.tensor([g for g, _ in pairs], device=dev), torch.tensor([i for _, i in pairs], device=dev)
        plain = infer.materialise_retest(st, [g for g, _ in pairs], [hosts[g][i][0] for g, i in pairs])
        out[which] = _rows_of(pred, plain, [hosts[g][i][1] for g, i in pairs], thr)
    n = torch.tensor([len(h) for h in hosts], dtype=torch.int64)
    count = torch.tensor([TG.lut_neighbourhood(ns.data[g], ns.freq, RC.FI, thr)[0] for g in range(G)], dtype=torch.int64)
    return infer.Retest(out, conn.to(dev), n.to(dev), count.to(dev)), hosts


def _check(pred, ns, device, thr, M=256, **kw):
    st = ns.to_device(device)
    clone = st.data.clone()
    r = _retest(pred, st, thr, M=M, **kw)
    want, hosts = _definition(pred, ns, st, thr, M)
    assert torch.equal(r.conn, want.conn) and torch.equal(r.n, want.n) and torch.equal(r.count, want.count), (r, want)
    assert _same(r.out, want.out), (r.out, want.out)
    assert torch.equal(st.data, clone)                                         # 8. the call never writes to the chunk
    pred.check_status()
    return r, hosts, st


def _gather(whole, samples, conns):
    """Named mode stated through all-mode rows: slot (g, i) is the row of conn ``conns[g, i]`` in sample ``samples[g]``."""
    G, M = conns.shape
    out = torch.full((G, M) + tuple(whole.out.shape[2:]), NAN, dtype=torch.float32, device=whole.out.device)
    conn = torch.full((G, M), -1, dtype=torch.int64, device=whole.out.device)
    for g, s in enumerate(samples):
        have = whole.conn[s].tolist()
        for i, c in enumerate(conns[g].tolist()):
            if c != -1 and c in have:
                out[g, i], conn[g, i] = whole.out[s, have.index(c)], c
    sel = torch.tensor(list(samples), device=whole.out.device)
    return infer.Retest(out, conn, whole.n[sel], whole.count[sel])


def _join(datas, freq):
    return SK.status(np.concatenate(datas), freq)


# ------------------------------------------------------------------ 1. the definition, bit for bit
@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("thr", RC.THRESHOLDS)
@pytest.mark.parametrize("C,O", SHAPES)
def test_rows_are_predict_of_the_retest_samples(cuda_device, C, O, thr, flagged):
    pred = q.LightpathPredictor(_model(cuda_device, C, O))
    ns = RC.samples(flagged)
    r, hosts, st = _check(pred, ns, cuda_device, thr)
    for g, h in enumerate(hosts):
        assert bool(torch.isfinite(r.out[g, :len(h)]).all()) and bool(torch.isnan(r.out[g, len(h):]).all())
        assert bool((r.conn[g, len(h):] == -1).all()) and 10 <= len(h) <= 13
    assert r.count.tolist() == [int(flagged)] * 2
    # the sample numbers in every form give the same bits
    for form in ([0, 1], (0, 1), torch.tensor([0, 1], device=cuda_device)):
        assert _all_same(_retest(pred, st, thr, form), r)
    back = _retest(pred, st, thr, [1, 0, 1])
    assert _all_same(back, [t[[1, 0, 1]] for t in r])


@pytest.mark.parametrize("name", list(RC.HAND))
def test_hand_cases(cuda_device, name):
    c = RC.HAND[name]()
    pred = q.LightpathPredictor(_model(cuda_device))
    r, hosts, _ = _check(pred, c.ns, cuda_device, c.thr)
    assert hosts[0] == c.want and r.n.tolist() == [len(c.want)] and r.count.tolist() == [c.count]
    assert r.conn[0, :len(c.want)].tolist() == [t[0] for t in c.want]
    if not c.want:
        assert bool((r.conn == -1).all()) and bool(torch.isnan(r.out).all())


def test_a_message_changes_the_row(cuda_device):
    """Two lightpaths with equal features but for their neighbourhoods get different rows: were the rows not to depend on
    the messages, a retest that found nobody would go unseen."""
    data, freq = PC.grid()
    data[0, :, 0, 5] = SK.vec(8, 64, 70000, 9, freq[5])
    data[0, :, 0, 6] = SK.vec(7, 4, 30000, 1, freq[6])
    data[0, :, 2, 5] = SK.vec(9, 64, 70000, 9, freq[5])                       # conn 8's twin, alone on its link
    pred = q.LightpathPredictor(_model(cuda_device))
    r, hosts, _ = _check(pred, SK.status(data, freq), cuda_device, 0.07)
    assert hosts[0] == [(8, 0, [7]), (7, 1, [8]), (9, 2, [])]
    assert not torch.equal(r.out[0, 0], r.out[0, 2])


# ------------------------------------------------------------------ 2. count and the flagged lightpath's row are from_status's
def test_count_and_the_flagged_row_are_from_status(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    seen = 0
    for ns, thr in ((RC.samples(True), 0.12), (RC.samples(True), 0.05), (RC.samples(False), 0.12),
                    (RC.HAND["the sample's flagged lightpath, retested itself and as a source"]().ns, 0.07)):
        st = ns.to_device(cuda_device)
        r = _retest(pred, st, thr)
        rows, count = pred.from_status(st, None, RC.FEATS, thr)
        assert torch.equal(r.count, count)
        for g in range(ns.data.shape[0]):
            _, first, _ = TG.lut_neighbourhood(ns.data[g], ns.freq, RC.FI, thr)
            if first is None:
                assert bool(torch.isnan(rows[g]).all())
            else:
                assert torch.equal(r.out[g, r.conn[g].tolist().index(first)], rows[g])
                seen += 1
    assert seen == 5
    pred.check_status()


# ------------------------------------------------------------------ 3. place_impact's before
@pytest.mark.parametrize("flagged", [False, True])
def test_before_of_place_impact_is_the_retest_row(cuda_device, flagged):
    pred = q.LightpathPredictor(_model(cuda_device))
    b = IC.batch(0, flagged=flagged)
    st = b.ns.to_device(cuda_device)
    values = torch.from_numpy(b.values).to(cuda_device)
    cells = torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64)).to(cuda_device)
    imp = pred.place_impact(st, list(b.samples), values, cells, list(b.cell_ptr), RC.FEATS, 0.12, 8)
    whole = _retest(pred, st, 0.12)
    seen = 0
    for k, s in enumerate(b.samples):
        have = whole.conn[s].tolist()
        for i in range(min(int(imp.n_affected[k]), 8)):
            assert torch.equal(imp.before[k, i], whole.out[s, have.index(int(imp.affected[k, i]))]), (k, i)
            seen += 1
    assert seen >= 16
    # named mode takes place_impact's own tables: the affected conns, -1 padded, of each candidate's sample
    named = _retest(pred, st, 0.12, list(b.samples), imp.affected)
    assert _same(named.out, imp.before) and torch.equal(named.conn, imp.affected)
    pred.check_status()


# ------------------------------------------------------------------ 4. named mode
def test_named_mode_is_the_gathered_all_mode_rows(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    ns = RC.samples(True)
    st = ns.to_device(cuda_device)
    whole = _retest(pred, st, 0.12)
    have = [whole.conn[g, :int(whole.n[g])].tolist() for g in range(2)]
    rng = np.random.default_rng(0)
    dev = lambda rows: torch.tensor(rows, dtype=torch.int64, device=cuda_device)    # noqa: E731
    pad = lambda row, M: list(row) + [-1] * (M - len(row))                          # noqa: E731
    M = max(len(h) for h in have)
    tables = {
        "every conn, permuted": ([0, 1], [pad(rng.permutation(h).tolist(), M) for h in have]),
        "subsets, the samples swapped": ([1, 0], [have[1][2:5], have[0][7:4:-1]]),
        "a conn named three times": ([0, 0], [[have[0][3], have[0][1], have[0][3], have[0][3]], [have[0][0]] * 4]),
        "-1 slots first, between and last": ([0, 1], [[-1, have[0][2], -1, have[0][0], -1], [-1, -1, -1, -1, have[1][4]]]),
        "only -1": ([1], [[-1, -1, -1]]),
        "one slot": ([1, 0], [[have[1][-1]], [have[0][-1]]]),
        "more slots than one chunk holds": ([0, 1], [pad((h * 4)[:40], 40) for h in have]),
    }
    for name, (samples, rows) in tables.items():
        conns = dev(rows)
        keep = conns.clone()
        r = _retest(pred, st, 0.12, samples, conns)
        assert _all_same(r, _gather(whole, samples, conns)), name
        assert torch.equal(conns, keep) and int(pred._status.item()) == 0, name
    # a conn the sample does not hold, alone between good ones: that slot only, and the new bit alone
    missing = next(c for c in have[1] if c not in have[0])                          # a lightpath of the OTHER sample
    conns = dev([[have[0][1], missing, have[0][2]], have[1][:3]])
    r = _retest(pred, st, 0.12, [0, 1], conns)
    assert _all_same(r, _gather(whole, [0, 1], conns))
    assert r.conn[0].tolist() == [have[0][1], -1, have[0][2]] and bool(torch.isnan(r.out[0, 1]).all())
    assert bool(torch.isfinite(r.out[0, [0, 2]]).all()) and bool(torch.isfinite(r.out[1]).all())
    assert int(pred._status.item()) == infer.LP_RETEST_NO_SUCH_CONN == 4096
    with pytest.raises(_lib.QotError, match="retest: a named conn_id is no lightpath of the sample"):
        pred.check_status()
    pred.check_status()                                                              # clean on the next call
    with pytest.raises(ValueError, match="conns has 2 rows, samples names 3 samples"):
        pred.retest(st, [0, 1, 0], conns, RC.FEATS, 0.12)


# ------------------------------------------------------------------ 5. chunk
@pytest.mark.parametrize("case", ["random", "255 lightpaths"])
def test_results_do_not_depend_on_chunk(cuda_device, case):
    pred = q.LightpathPredictor(_model(cuda_device))
    ns, thr = (RC.samples(True), 0.12) if case == "random" else (RC.HAND[case]().ns, 0.12)
    st = ns.to_device(cuda_device)
    whole = _retest(pred, st, thr)
    assert (case == "random" or whole.n.tolist() == [255]) and bool(torch.isfinite(whole.out[0, 0]).all())
    have = whole.conn[0, :int(whole.n[0])].tolist()
    conns = torch.tensor([(have[::-1] * 4)[:37] + [-1, have[0], -1]] * st.data.shape[0], dtype=torch.int64, device=cuda_device)
    named = _retest(pred, st, thr, None, conns)
    for chunk in (1, 5, 32):
        assert _all_same(_retest(pred, st, thr, chunk=chunk), whole), chunk
        assert _all_same(_retest(pred, st, thr, M=37, chunk=chunk), [whole.out[:, :37], whole.conn[:, :37], whole.n, whole.count]), chunk
        assert _all_same(_retest(pred, st, thr, None, conns, chunk=chunk), named), chunk
    if case == "random":                                       # (sample 1 does not hold sample 0's conns)
        assert int(pred._status.item()) == infer.LP_RETEST_NO_SUCH_CONN
        pred._status.zero_()
    pred.check_status()
    with pytest.raises(ValueError, match="chunk must be None or an int"):
        pred.retest(st, None, None, RC.FEATS, thr, chunk=33)


# ------------------------------------------------------------------ 6. max_lightpaths
def test_more_lightpaths_than_slots_is_no_error(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    ns = RC.samples(True)
    st = ns.to_device(cuda_device)
    wide = _retest(pred, st, 0.12, M=256)
    assert int(wide.n.min()) > 7                                                # a condition on the inputs: n > M below
    for M in (1, 7):
        narrow = _retest(pred, st, 0.12, M=M)
        assert torch.equal(narrow.n, wide.n) and torch.equal(narrow.count, wide.count)
        assert torch.equal(narrow.conn, wide.conn[:, :M]) and torch.equal(narrow.out, wide.out[:, :M])
        assert bool(torch.isfinite(narrow.out).all())
    assert int(pred._status.item()) == 0                                        # nothing is flagged
    _check(pred, ns, cuda_device, 0.12, M=7)
    _check(pred, ns, cuda_device, 0.12, M=1)
    for M in (0, 257, True):
        with pytest.raises(ValueError, match="max_lightpaths must be an int in"):
            pred.retest(st, None, None, RC.FEATS, 0.12, M)


# ------------------------------------------------------------------ 7. refusals on the device
def _refused(r, g):
    return (bool(torch.isnan(r.out[g]).all()) and bool((r.conn[g] == -1).all()) and int(r.n[g]) == 0 and int(r.count[g]) == 0)


def _refusal_cases():
    ns = RC.samples(True)
    nan_conn, big_conn = ns.data[0:1].copy(), ns.data[0:1].copy()
    l, f = np.argwhere(np.any(ns.data[0] != 0, axis=0))[5]
    nan_conn[0, RC.FI["conn_id"], l, f] = np.nan
    big_conn[0, RC.FI["conn_id"], l, f] = 2.0 ** 60
    return {"a NaN conn_id": (nan_conn, None, "LP_STATUS_BAD_CONN", "conn_id is not finite"),
            "a conn_id beyond 2^53": (big_conn, None, "LP_STATUS_BAD_CONN", "conn_id is not finite"),
            "256 lightpaths are none too many": (PC.crowd(256).ns.data, None, None, None),
            "more than 256 lightpaths": (_too_many(), None, "LP_STATUS_TOO_MANY", f"more than {TG.MAX_LIGHTPATHS} lightpaths"),
            "a sample number at S": (ns.data[0:1], [0, 3, 2], "LP_STATUS_BAD_SAMPLE", "sample number"),
            "a negative sample number": (ns.data[0:1], [0, -1, 2], "LP_STATUS_BAD_SAMPLE", "sample number")}


def _too_many():
    data, _ = PC.grid()
    for k in range(257):
        data[0, :, k // PC.Q, k % PC.Q] = SK.vec(10 + k, fval=193.0)
    return data


@pytest.mark.parametrize("name", ["a NaN conn_id", "a conn_id beyond 2^53", "256 lightpaths are none too many",
                                  "more than 256 lightpaths", "a sample number at S", "a negative sample number"])
def test_a_refused_sample_flags_its_rows_only(cuda_device, name):
    middle, samples, bit, cause = _refusal_cases()[name]
    pred = q.LightpathPredictor(_model(cuda_device))
    ns = RC.samples(True)
    good = _retest(pred, ns.to_device(cuda_device), 0.12, M=16)
    st = _join([ns.data[0:1], middle, ns.data[1:2]], ns.freq).to_device(cuda_device)
    have = [good.conn[g, :3].tolist() for g in range(2)]
    conns = torch.tensor([have[0], have[0], have[1]], dtype=torch.int64, device=cuda_device)
    for named in (None, conns):
        for chunk in (None, 2):
            r = _retest(pred, st, 0.12, samples, named, M=16, chunk=chunk)
            want = good if named is None else infer.Retest(good.out[:, :3], good.conn[:, :3], good.n, good.count)
            assert _all_same([t[0] for t in r], [t[0] for t in want]) and _all_same([t[2] for t in r], [t[1] for t in want])
            if bit is None:                                                     # the cap itself is legal
                assert int(r.n[1]) == 256 and int(r.count[1]) == 0
                if named is None:
                    assert bool(torch.isfinite(r.out[1]).all()) and int(pred._status.item()) == 0
                pred._status.zero_()                                            # (named: sample 0's conns are not the crowd's)
                continue
            assert _refused(r, 1)
            assert int(pred._status.item()) == getattr(infer, bit)              # the word carries that bit and no other
            with pytest.raises(_lib.QotError, match=cause):
                pred.check_status()
            pred.check_status()                                                 # clean on the next call


# ------------------------------------------------------------------ 9. capture
def test_capture_and_replay_on_overwritten_arguments(cuda_device):
    pred = q.LightpathPredictor(_model(cuda_device))
    ns, ns2 = RC.samples(False), RC.samples(True)                              # the same shapes, other contents
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda_device)      # noqa: E731
    st, samples = ns.to_device(cuda_device), dev([0, 1, 0])
    eager = pred.retest(st, samples, None, RC.FEATS, 0.12, 16)                  # (the column table is uploaded here)
    conns = eager.conn[:, [3, 0, 5, 3]].clone()
    eager_named = pred.retest(st, samples, conns, RC.FEATS, 0.12)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = pred.retest(st, samples, None, RC.FEATS, 0.12, 16)
        rn = pred.retest(st, samples, conns, RC.FEATS, 0.12)
    graph.replay()
    torch.cuda.synchronize()
    assert _all_same(r, eager) and _all_same(rn, eager_named)
    assert _all_same(rn, _gather(_retest(pred, st, 0.12), [0, 1, 0], conns))
    st.data.copy_(torch.from_numpy(ns2.data))                                  # in place: the captured pointers stay
    samples.copy_(dev([1, 1, 0]))
    want = _retest(pred, ns2.to_device(cuda_device), 0.12, [1, 1, 0], M=16)
    conns.copy_(want.conn[:, [1, 2, 2, 0]])
    graph.replay()
    torch.cuda.synchronize()
    assert _all_same(r, want) and not _same(r.out, eager.out) and r.count.tolist() == [1, 1, 1]
    assert _all_same(rn, _gather(_retest(pred, ns2.to_device(cuda_device), 0.12), [1, 1, 0], conns))
    assert bool(torch.isfinite(rn.out).all())
    pred.check_status()


# ------------------------------------------------------------------ 10. empty input
def test_no_samples_no_launch(cuda_device, monkeypatch):
    pred = q.LightpathPredictor(_model(cuda_device))
    st = RC.samples().to_device(cuda_device)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    for none in ([], torch.zeros(0, dtype=torch.int64, device=cuda_device)):
        for conns, M in ((None, 4), (torch.zeros(0, 6, dtype=torch.int64, device=cuda_device), 6)):
            r = pred.retest(st, none, conns, RC.FEATS, 0.05, 4)
            assert [tuple(t.shape) for t in r] == [(0, M, 3), (0, M), (0,), (0,)]
            assert [t.dtype for t in r] == [torch.float32, torch.int64, torch.int64, torch.int64]
    monkeypatch.undo()
    assert calls == []
    with pytest.raises(infer.EnvelopeError, match="'osnr' cannot be a feature"):
        pred.retest(st, None, None, ["freq", "mod_order", "num_spans", "osnr"])
    with pytest.raises(ValueError, match="conns is on cpu"):
        pred.retest(st, None, torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(TypeError):
        pred.retest(st, None, None, RC.FEATS, 0.05, 16, 4)                      # chunk is keyword-only
    with pytest.raises(TypeError):
        pred.retest(st, release=None)
    pred.check_status()
