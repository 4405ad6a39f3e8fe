"""CPU-side checks of ``LightpathPredictor.place_impact`` (``csrc/infer_lightpath_place_impact.hip``): the
host statement ``to_graph.placement_impact`` on the hand cases of ``impact_cases.py`` and against ``lut_neighbourhood`` of
the retest samples; the definition ``infer.materialise_retest`` against a numpy restatement; the refusals that need no
device, through ``infer.lightpath_place_impact_args``; the new entry declared, bound, built and answering its envelope
before any launch."""
import os

import numpy as np
import pytest
import torch

import impact_cases as IC
import place_cases as PC
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = [PC.FI[n] for n in ("osnr", "snr", "ber")]


def _cpu_status(ns):
    data, freq = torch.from_numpy(ns.data), torch.from_numpy(np.asarray(ns.freq, dtype=np.float64))
    return TG.DeviceStatus(data, torch.from_numpy(ns.target), freq, ns.lp_feat, ns.metric)


def _tensors(b):
    return torch.from_numpy(b.values), torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64))


def _retest(sample, conn, values=None, cells=None):
    """The definition in three lines of numpy."""
    out = sample.copy()
    if values is not None:
        out[:, cells[0], cells[1]] = np.where(np.isin(np.arange(len(values)), LABELS), 0.0, values)[:, None]
    mine = np.any(out != 0, axis=0) & (np.trunc(out[PC.FI["conn_id"]]) == conn)
    out[LABELS] = np.where(mine, -1.0, out[LABELS])
    return out


# ------------------------------------------------------------------ the host statement
@pytest.mark.parametrize("name", list(IC.HAND))
def test_hand_cases_on_the_host(name):
    c = IC.HAND[name]()
    sample = c.ns.data[0]
    got = TG.placement_impact(sample, c.ns.freq, IC.FI, c.values, c.cells, c.thr)
    assert got == c.want
    assert [t[0] for t in got] == TG.placement_neighbourhood(sample, c.ns.freq, IC.FI, c.cells, c.thr)
    assert int(c.values[IC.FI["conn_id"]]) == IC.CAND


@pytest.mark.parametrize("thr", IC.THRESHOLDS)
@pytest.mark.parametrize("flagged", [False, True])
def test_placement_impact_on_the_random_candidates(flagged, thr):
    """The conn list is ``placement_neighbourhood``'s; the sources are ``lut_neighbourhood``'s of the retest sample where
    the lightpath is its first flagged one; ``sources_after`` is ``sources_before`` with the candidate inserted at its
    first-seen position, which is the count of first channels below the smallest cell."""
    b = IC.batch(0, flagged=flagged)
    Q = b.ns.data.shape[3]
    for k, s in enumerate(b.samples):
        sample, cells, own = b.ns.data[s], PC.candidate_cells(b, k), int(b.values[k][IC.FI["conn_id"]])
        got = IC.host_impact(b, k, thr)
        assert [t[0] for t in got] == TG.placement_neighbourhood(sample, b.ns.freq, IC.FI, cells, thr)
        link_idx, freq_idx, vec = TG._occupied(sample)
        conn = vec[IC.FI["conn_id"]].astype(np.int64)
        first = np.sort(np.unique(conn, return_index=True)[1])
        order = [int(conn[i]) for i in first]
        pos = int(np.sum((link_idx[first] * Q + freq_idx[first]) < int(np.min(cells[0] * Q + cells[1]))))
        assert pos == TG.place_lightpath(sample, b.values[k], cells, IC.FI)[1]
        for c, node_before, node_after, before, after in got:
            assert node_before == order.index(c) and node_after == node_before + (node_before >= pos)
            at = sum(order.index(x) < pos for x in before)
            assert after == before[:at] + [own] + before[at:], (k, c)
            if not flagged:                                 # c is the only flagged lightpath of its retest samples
                assert TG.lut_neighbourhood(_retest(sample, c), b.ns.freq, IC.FI, thr) == (1, c, before)
                assert TG.lut_neighbourhood(_retest(sample, c, b.values[k], cells), b.ns.freq, IC.FI, thr) == (1, c, after)


def test_placement_impact_refuses_what_place_lightpath_refuses():
    c = IC.HAND["the candidate is the only source: before sums no message"]()
    with pytest.raises(ValueError, match=r"\(link 1, slot 11\) is occupied"):
        TG.placement_impact(c.ns.data[0], c.ns.freq, IC.FI, c.values, np.array([[1], [11]]), c.thr)
    taken = c.values.copy()
    taken[IC.FI["conn_id"]] = 8.0
    with pytest.raises(ValueError, match="conn_id 8 is a lightpath of the sample"):
        TG.placement_impact(c.ns.data[0], c.ns.freq, IC.FI, taken, c.cells, c.thr)


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize("flagged", [False, True])
def test_materialise_retest_is_the_numpy_restatement(flagged):
    b = IC.batch(0, flagged=flagged)
    st = _cpu_status(b.ns)
    values, cells = _tensors(b)
    before = st.data.clone()
    pairs = [(k, t[0]) for k in range(len(b.samples)) for t in IC.host_impact(b, k, 0.12)]
    ks, conns = [k for k, _ in pairs], [c for _, c in pairs]
    samples = [b.samples[k] for k in ks]
    plain = infer.materialise_retest(st, samples, conns)
    ptr = np.cumsum([0] + [b.cell_ptr[k + 1] - b.cell_ptr[k] for k in ks]).tolist()
    pcells = torch.cat([cells[:, b.cell_ptr[k]:b.cell_ptr[k + 1]] for k in ks], 1)
    with_cand = infer.materialise_retest(st, torch.tensor(samples), torch.tensor(conns), values[ks], pcells, ptr)
    assert isinstance(plain, TG.DeviceStatus) and tuple(plain.data.shape) == (len(pairs),) + tuple(st.data.shape[1:])
    changed = 0
    for t, (k, c) in enumerate(pairs):
        sample = b.ns.data[b.samples[k]]
        assert np.array_equal(plain.data[t].numpy(), _retest(sample, c)), t
        assert np.array_equal(with_cand.data[t].numpy(), _retest(sample, c, b.values[k], PC.candidate_cells(b, k))), t
        changed += not np.array_equal(plain.data[t].numpy(), sample)
        cand = with_cand.data[t][:, pcells[0, ptr[t]], pcells[1, ptr[t]]].numpy()
        assert (cand[LABELS] == 0.0).all() and cand[IC.FI["conn_id"]] == b.values[k][IC.FI["conn_id"]]
    # measured lightpaths became lightpaths under test; the samples' own (conn 700 + s, place_cases.dense_sample) stay as they are
    assert changed == sum(c < 700 for _, c in pairs) and (changed < len(pairs)) == flagged
    assert torch.equal(st.data, before) and torch.equal(plain.target, st.target[samples])
    one = infer.materialise_retest(st, samples[0], conns[:1])                 # an int
    assert torch.equal(one.data, plain.data[:1])
    with pytest.raises(ValueError, match="materialise_retest: samples names 1 samples, conns 2"):
        infer.materialise_retest(st, [0], [1, 2])
    with pytest.raises(ValueError, match="materialise_retest: cells and cell_ptr go with values"):
        infer.materialise_retest(st, [0], [1], None, cells)
    with pytest.raises(ValueError, match="materialise_retest: cell_ptr must be non-decreasing"):
        infer.materialise_retest(st, samples[:1], conns[:1], values[:1], cells, [1, 2])
    with pytest.raises(TypeError, match="materialise_retest takes a DeviceStatus"):
        infer.materialise_retest(b.ns, samples, conns)


# ------------------------------------------------------------------ refusals without a device
def test_refusals_before_any_launch():
    b = IC.batch(0)
    st = _cpu_status(b.ns)
    values, cells = _tensors(b)
    K, M = values.shape[0], cells.shape[1]

    def args(**kw):
        return infer.lightpath_place_impact_args(kw.pop("status", st), kw.pop("F", 5), kw.pop("lut", PC.LUT_COL),
                                                 kw.pop("samples", b.samples), kw.pop("values", values),
                                                 kw.pop("cells", cells), kw.pop("cell_ptr", b.cell_ptr), **kw)

    who = "LightpathPredictor.place_impact"
    with pytest.raises(TypeError, match=who + " takes a DeviceStatus"):
        args(status=b.ns)
    with pytest.raises(infer.EnvelopeError, match="on the CPU"):             # everything is in order but the device
        args()
    assert infer.PLACE_MAX_AFFECTED == 32
    for A in (1, 8, 32):
        with pytest.raises(infer.EnvelopeError, match="on the CPU"):
            args(max_affected=A)
    for A in (0, 33, -1, True, False, 8.0, None, "8"):
        with pytest.raises(ValueError, match=who + r": max_affected must be an int in 1 \.\.\. 32") as e:
            args(max_affected=A)
        assert not isinstance(e.value, infer.EnvelopeError)
    for label in ("osnr", "snr", "ber"):
        with pytest.raises(infer.EnvelopeError, match=f"{who}: '{label}' cannot be a feature"):
            args(features_to_consider=["freq", "mod_order", "num_spans", label])
    # every refusal of lightpath_place_args, under the new name
    bad = {
        r"values must be a float64 tensor \[K, 10\]": [dict(values=values.float()), dict(values=values[:, :9]),
                                                        dict(values=values[0]), dict(values=b.values)],
        r"cells must be an int64 tensor \[2, M\]": [dict(cells=cells.int()), dict(cells=cells.t().contiguous()),
                                                    dict(cells=cells[0]), dict(cells=b.cells)],
        "samples must be an int, a sequence or a 1-d int64 tensor": [
            dict(samples=torch.tensor(b.samples, dtype=torch.int32)), dict(samples=torch.tensor(b.samples)[:-1]),
            dict(samples=torch.tensor([b.samples])), dict(samples=None), dict(samples=True)],
        f"samples names {K - 1} candidates, values has {K} rows": [dict(samples=b.samples[:-1])],
        f"cell_ptr must be a sequence or a 1-d int64 tensor of K \\+ 1 = {K + 1}": [
            dict(cell_ptr=torch.tensor(b.cell_ptr, dtype=torch.int32)), dict(cell_ptr=torch.tensor(b.cell_ptr)[:-1]),
            dict(cell_ptr=torch.tensor([b.cell_ptr]))],
        f"cell_ptr must hold K \\+ 1 = {K + 1} offsets": [dict(cell_ptr=b.cell_ptr[:-1]), dict(cell_ptr=b.cell_ptr + [M])],
        f"cell_ptr must be non-decreasing from 0 to M = {M}": [
            dict(cell_ptr=[1] + b.cell_ptr[1:]), dict(cell_ptr=b.cell_ptr[:-1] + [M - 1]), dict(cell_ptr=b.cell_ptr[:-1] + [M + 1]),
            dict(cell_ptr=[0, b.cell_ptr[2], b.cell_ptr[1]] + b.cell_ptr[3:])],
        "candidate 1 has an empty slice of cells": [dict(cell_ptr=[0, b.cell_ptr[1], b.cell_ptr[1]] + b.cell_ptr[3:])],
        "freq_threshold must be a finite positive number": [dict(freq_threshold=t) for t in (0.0, -0.05, float("inf"), float("nan"), "0.05", None, True)],
    }
    for msg, cases in bad.items():
        for kw in cases:
            with pytest.raises(ValueError, match=who + ": " + msg) as e:
                args(**kw)
            assert not isinstance(e.value, infer.EnvelopeError), (msg, kw)
    with pytest.raises(infer.EnvelopeError, match=who + ".*in_channels"):
        args(F=6)
    with pytest.raises(infer.EnvelopeError, match=who + ".*is_lut_index"):
        args(lut=0)
    with pytest.raises(infer.EnvelopeError, match="in_channels"):
        args(features_to_consider=["freq", "mod_order"])
    renamed = [("hops" if n == "num_spans" else n) for n in TG.LP_FEAT]
    with pytest.raises(infer.EnvelopeError, match="'num_spans'"):
        args(status=TG.DeviceStatus(st.data, st.target, st.freq, renamed, st.metric))
    # the method takes no release= keyword
    import inspect
    assert list(inspect.signature(infer.LightpathPredictor.place_impact).parameters) == [
        "self", "status", "samples", "values", "cells", "cell_ptr", "features_to_consider", "freq_threshold", "max_affected"]
    assert infer.PlaceImpact._fields == ("out", "count", "affected", "n_affected", "before", "after")


# ------------------------------------------------------------------ the layers agree
def test_entry_is_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    name = "qot_lightpath_infer_place_impact"
    assert f"int {name}(" in hdr and name in _lib.SIGNATURES and "#define QOT_PLACE_MAX_AFFECTED 32 " in hdr
    place_sig, sig = _lib.SIGNATURES["qot_lightpath_infer_place"], _lib.SIGNATURES[name]
    assert sig[0] == place_sig[0]
    # the place entry's arguments up to M, then affected, n_affected, before, after, max_affected, the stream
    assert sig[1][:len(place_sig[1]) - 1] == place_sig[1][:-1] and len(sig[1]) == len(place_sig[1]) + 5
    import ctypes
    assert sig[1][-6:] == [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p]
    mk = open(os.path.join(ROOT, "gnn_qot_estimation_amd", "csrc", "Makefile")).read()
    assert " infer_lightpath_place_impact.hip " in mk
    csrc = os.path.join(ROOT, "gnn_qot_estimation_amd", "csrc")
    shared = open(os.path.join(csrc, "infer_lightpath_status_dev.hpp")).read()
    # the shared routines are stated once, in the header, and neither kernel restates them or the phases they share
    # (the candidate's argument struct is both models': sg::PlaceArgs of status_scan_dev.hpp, which the header includes)
    scan = open(os.path.join(csrc, "status_scan_dev.hpp")).read()
    assert '#include "status_scan_dev.hpp"' in shared
    for piece in ("bool channel_conn(", "void lp_mark_slots(", "int lp_stage_marked(", "int lp_place_scan(", "struct PlaceArgs {"):
        assert (scan if piece == "struct PlaceArgs {" else shared).count(piece) == 1
        for f in ("infer_lightpath_place.hip", "infer_lightpath_place_impact.hip"):
            src = open(os.path.join(csrc, f)).read()
            assert '#include "infer_lightpath_status_dev.hpp"' in src and piece not in src, (f, piece)
    src = open(os.path.join(csrc, "infer_lightpath_place_impact.hip")).read()
    for used in ("lp_place_scan<false>(", "lp_mark_slots(", "lp_stage_marked(", "sg_feature(", "sg_feature_vec(", "lp_row<false, LpStaged>("):
        assert used in src, used
    assert "discover(" in shared


def test_entry_answers_the_envelope_before_any_launch():
    """Sizes and the envelope are answered without a pointer being looked at; K == 0 is QOT_OK without a launch."""
    lib = _lib.load()

    def rc(K=0, S=4, P=10, L=4, Q=70, F=5, C=32, O=3, heads=4, lut=1, rows=(0, 7, 8, 9), ncol=5, thr=0.05, N=0, M=0, A=8):
        none = [None] * 6
        return lib.qot_lightpath_infer_place_impact(*none, 0, N, 0, K, None, None, None, None, 0.2, None, None, None, None,
                                                    1e-5, None, None, None, None, 0.01, None, None, F, C, O, heads, lut, None,
                                                    None, None, None, S, P, L, Q, *rows, None, ncol, thr, None, None, None, M,
                                                    None, None, None, None, A, None)
    OK, UNSUPPORTED, BADARG = 0, -1, -2                                       # include/qot_gnn.h: QOT_OK, QOT_ERR_*
    assert rc() == OK and rc(M=7) == OK and rc(A=1) == OK and rc(A=32) == OK
    codes = {name: rc(**kw) for name, kw in {
        "a batch beside the status": dict(N=3), "K < 0": dict(K=-1), "P < 1": dict(P=0), "Q < 1": dict(Q=0),
        "ncol != F": dict(ncol=4), "a row outside P": dict(rows=(0, 7, 8, 10)), "threshold 0": dict(thr=0.0),
        "threshold nan": dict(thr=float("nan")), "M < 0": dict(M=-1), "no pointers with K > 0": dict(K=2, M=2),
        "max_affected 0": dict(A=0), "max_affected 33": dict(A=33), "max_affected < 0": dict(A=-1)}.items()}
    assert all(c == BADARG for c in codes.values()), codes
    outside = {name: rc(**kw) for name, kw in {
        "F": dict(F=17, ncol=17), "C": dict(C=257), "O": dict(O=9), "heads": dict(heads=2), "lut": dict(lut=5),
        "Q above the cap": dict(Q=1025), "L * Q": dict(L=1 << 22, Q=1024)}.items()}
    assert all(c == UNSUPPORTED for c in outside.values()), outside
