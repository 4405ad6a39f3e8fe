"""CPU-side checks of ``LightpathPredictor.place`` (``csrc/infer_lightpath_place.hip``): the host statements
of a candidate -- ``to_graph.place_lightpath`` (the edited sample, the candidate's node) against ``create_lightpath_graph``,
``to_graph.placement_neighbourhood`` (stated on the UNEDITED sample plus the cells) against ``lut_neighbourhood`` of the
edited sample; ``infer.materialise_placement`` against ``place_lightpath``; the refusals that need no device, through
``infer.lightpath_place_args``; the new entry declared, bound, built and answering its envelope before any launch."""
import os

import numpy as np
import pytest
import torch

import place_cases as PC
import status_infer_cases as SK
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _candidates(b):
    for k, s in enumerate(b.samples):
        yield k, b.ns.data[s], b.values[k], PC.candidate_cells(b, k)


def _cpu_status(ns):
    data, freq = torch.from_numpy(ns.data), torch.from_numpy(np.asarray(ns.freq, dtype=np.float64))
    return TG.DeviceStatus(data, torch.from_numpy(ns.target), freq, ns.lp_feat, ns.metric)


def _tensors(b):
    return torch.from_numpy(b.values), torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64))


# ------------------------------------------------------------------ the definition on the host
@pytest.mark.parametrize("thr", PC.THRESHOLDS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_placement_neighbourhood_is_lut_neighbourhood_of_the_edited_sample(seed, thr):
    """Where the candidate is the first-seen flagged lightpath of its edited sample (here: the only one)."""
    b = PC.batch(seed)
    some = 0
    for k, sample, values, cells in _candidates(b):
        edited, _ = TG.place_lightpath(sample, values, cells, PC.FI)
        count, conn, want = TG.lut_neighbourhood(edited, b.ns.freq, PC.FI, thr)
        assert (count, conn) == (1, int(values[PC.FI["conn_id"]]))
        got = TG.placement_neighbourhood(sample, b.ns.freq, PC.FI, cells, thr)
        assert got == want, (k, got, want)
        some += len(got) >= 2
    assert thr != 0.12 or 2 * some >= len(b.samples)


@pytest.mark.parametrize("name", list(PC.HAND))
def test_hand_cases_on_the_host(name):
    c = PC.HAND[name]()
    sample = c.ns.data[0]
    assert TG.placement_neighbourhood(sample, c.ns.freq, PC.FI, c.cells, c.thr) == c.interferers
    edited, node = TG.place_lightpath(sample, c.values, c.cells, PC.FI)
    count, conn, inter = TG.lut_neighbourhood(edited, c.ns.freq, PC.FI, c.thr)
    assert count == c.count
    own = int(c.values[PC.FI["conn_id"]])
    if c.count == 1:
        assert conn == own and inter == c.interferers
    else:                                                   # the row from_status gives is another lightpath's
        assert conn != own and node > 0


@pytest.mark.parametrize("flagged", [False, True])
def test_place_lightpath_names_the_node_of_the_host_built_graph(flagged):
    b = PC.batch(1, flagged=flagged)
    for k, sample, values, cells in _candidates(b):
        edited, node = TG.place_lightpath(sample, values, cells, PC.FI)
        assert not np.shares_memory(edited, sample) and np.array_equal(sample, b.ns.data[b.samples[k]])
        assert np.array_equal(edited[:, cells[0], cells[1]], np.tile(values[:, None], (1, cells.shape[1])))
        changed = np.any(edited != sample, axis=0)
        assert int(changed.sum()) == len({(int(l), int(q)) for l, q in cells.T})
        G = TG.create_lightpath_graph(0, PC.FEATS, SK.status(edited[None], b.ns.freq))
        names = list(G.nodes)
        assert names[node] == f"lightpath_{int(values[PC.FI['conn_id']])}" and G.nodes[names[node]]["is_lut"] == 1
        assert (node > 0) if flagged else True              # the sample's flagged lightpath is seen first
        assert sum(d["is_lut"] for _, d in G.nodes(data=True)) == 1 + int(flagged)


def test_place_lightpath_refuses_occupied_cells_taken_conns_and_cells_outside():
    c = PC.HAND["one cell"]()
    sample = c.ns.data[0]
    with pytest.raises(ValueError, match=r"\(link 1, slot 11\) is occupied"):
        TG.place_lightpath(sample, c.values, np.array([[1, 1], [10, 11]]), PC.FI)
    taken = c.values.copy()
    taken[PC.FI["conn_id"]] = 9.6                             # truncates to conn 9
    with pytest.raises(ValueError, match="conn_id 9 is a lightpath of the sample"):
        TG.place_lightpath(sample, taken, c.cells, PC.FI)
    for cells in ([[PC.L], [10]], [[0], [PC.Q]], [[-1], [0]]):
        with pytest.raises(ValueError, match="outside the 4 links x 70 frequency slots"):
            TG.place_lightpath(sample, c.values, np.array(cells), PC.FI)
        with pytest.raises(ValueError, match="outside the 4 links x 70 frequency slots"):
            TG.placement_neighbourhood(sample, c.ns.freq, PC.FI, np.array(cells), c.thr)
    with pytest.raises(ValueError, match=r"cells must be \[2, m\]"):
        TG.place_lightpath(sample, c.values, np.zeros((2, 0), dtype=np.int64), PC.FI)


def test_materialise_placement_is_place_lightpath_per_candidate():
    b = PC.batch(2)
    st = _cpu_status(b.ns)
    values, cells = _tensors(b)
    before = st.data.clone()
    forms = (b.samples, torch.tensor(b.samples)), (b.cell_ptr, torch.tensor(b.cell_ptr))
    for samples in forms[0]:
        for ptr in forms[1]:
            ed = infer.materialise_placement(st, samples, values, cells, ptr)
            assert isinstance(ed, TG.DeviceStatus) and tuple(ed.data.shape) == (len(b.samples),) + tuple(st.data.shape[1:])
            for k, sample, v, c in _candidates(b):
                assert np.array_equal(ed.data[k].numpy(), TG.place_lightpath(sample, v, c, PC.FI)[0]), k
            assert torch.equal(ed.target, st.target[b.samples]) and torch.equal(st.data, before)
    one = infer.materialise_placement(st, b.samples[0], values[:1], cells[:, :b.cell_ptr[1]], b.cell_ptr[:2])   # an int
    assert torch.equal(one.data, ed.data[:1])
    none = infer.materialise_placement(st, [], values[:0], cells[:, :0], [0])
    assert tuple(none.data.shape) == (0,) + tuple(st.data.shape[1:])


# ------------------------------------------------------------------ refusals without a device
def test_refusals_before_any_launch():
    b = PC.batch(0)
    st = _cpu_status(b.ns)
    values, cells = _tensors(b)
    K, M = values.shape[0], cells.shape[1]

    def args(**kw):
        return infer.lightpath_place_args(kw.pop("status", st), kw.pop("F", 5), kw.pop("lut", PC.LUT_COL),
                                          kw.pop("samples", b.samples), kw.pop("values", values), kw.pop("cells", cells),
                                          kw.pop("cell_ptr", b.cell_ptr), **kw)

    with pytest.raises(TypeError, match="LightpathPredictor.place takes a DeviceStatus"):
        args(status=b.ns)
    # everything is in order but the device: lightpath_status_args names the CPU chunk last
    with pytest.raises(infer.EnvelopeError, match="on the CPU"):
        args()
    for samples in (0, torch.tensor(b.samples), tuple(b.samples)):
        with pytest.raises(infer.EnvelopeError, match="on the CPU"):
            args(samples=samples, cell_ptr=torch.tensor(b.cell_ptr))
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
            with pytest.raises(ValueError, match="LightpathPredictor.place: " + msg) as e:
                args(**kw)
            assert not isinstance(e.value, infer.EnvelopeError), (msg, kw)
    # what from_status refuses, through the same routine
    with pytest.raises(infer.EnvelopeError, match="in_channels"):
        args(F=6)
    with pytest.raises(infer.EnvelopeError, match="is_lut_index"):
        args(lut=0)
    with pytest.raises(infer.EnvelopeError, match="in_channels"):
        args(features_to_consider=["freq", "mod_order"])
    renamed = [("hops" if n == "num_spans" else n) for n in TG.LP_FEAT]
    with pytest.raises(infer.EnvelopeError, match="'num_spans'"):
        args(status=TG.DeviceStatus(st.data, st.target, st.freq, renamed, st.metric))
    # materialise_placement checks its lists by the same routine, under its own name
    with pytest.raises(ValueError, match="materialise_placement: cell_ptr must be non-decreasing"):
        infer.materialise_placement(st, b.samples, values, cells, [1] + b.cell_ptr[1:])
    with pytest.raises(TypeError, match="materialise_placement takes a DeviceStatus"):
        infer.materialise_placement(b.ns, b.samples, values, cells, b.cell_ptr)


# ------------------------------------------------------------------ the layers agree
def test_status_bits_header_and_constants_agree():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    names = ("BAD_CELL", "OCCUPIED", "CONN_TAKEN", "NOT_LUT")
    bits = tuple(getattr(infer, "LP_PLACE_" + n) for n in names)
    assert bits == (64, 128, 256, 512)
    for name, bit in zip(names, bits):
        assert f"#define QOT_LP_PLACE_{name} {bit} " in hdr
    older = (1, 2, 4, infer.LP_STATUS_BAD_CONN, infer.LP_STATUS_TOO_MANY, infer.LP_STATUS_BAD_SAMPLE)
    assert len({*older, *bits}) == 10 and all(b & sum(older) == 0 for b in bits)
    assert [b for b, _ in infer.LightpathPredictor._PLACE_CAUSES] == list(bits)
    assert all("place" in infer.LightpathPredictor._FLAGS[1] and text.startswith("place: ")
               for _, text in infer.LightpathPredictor._PLACE_CAUSES)
    # check_status() names a place cause beside the older ones
    pred = infer.LightpathPredictor.__new__(infer.LightpathPredictor)
    infer._DeviceState.__init__(pred)
    pred._status = torch.tensor([infer.LP_PLACE_OCCUPIED | infer.LP_STATUS_BAD_SAMPLE], dtype=torch.int32)
    with pytest.raises(_lib.QotError, match="sample number.*channel is occupied"):
        pred.check_status()
    pred.check_status()


def test_entry_is_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    assert "int qot_lightpath_infer_place(" in hdr and "qot_lightpath_infer_place" in _lib.SIGNATURES
    status_sig, place_sig = _lib.SIGNATURES["qot_lightpath_infer_status"], _lib.SIGNATURES["qot_lightpath_infer_place"]
    assert place_sig[0] == status_sig[0]
    # the status entry's arguments up to the threshold, then values, cells, cell_ptr, M, the stream
    assert place_sig[1][:len(status_sig[1]) - 1] == status_sig[1][:-1] and len(place_sig[1]) == len(status_sig[1]) + 4
    mk = open(os.path.join(ROOT, "gnn_qot_estimation_amd", "csrc", "Makefile")).read()
    assert " infer_lightpath_place.hip " in mk
    csrc = os.path.join(ROOT, "gnn_qot_estimation_amd", "csrc")
    shared = open(os.path.join(csrc, "infer_lightpath_status_dev.hpp")).read()
    for piece in ("bool channel_conn(", "void lp_mark_slots(", "int lp_stage_marked("):
        assert piece in shared
        for f in ("infer_lightpath_status.hip", "infer_lightpath_place.hip"):
            src = open(os.path.join(csrc, f)).read()
            assert '#include "infer_lightpath_status_dev.hpp"' in src and piece not in src, (f, piece)


def test_entry_answers_the_envelope_before_any_launch():
    """Sizes and the envelope are answered without a pointer being looked at; K == 0 is QOT_OK without a launch."""
    lib = _lib.load()

    def rc(K=0, S=4, P=10, L=4, Q=70, F=5, C=32, O=3, heads=4, lut=1, rows=(0, 7, 8, 9), ncol=5, thr=0.05, N=0, M=0):
        none = [None] * 6
        return lib.qot_lightpath_infer_place(*none, 0, N, 0, K, None, None, None, None, 0.2, None, None, None, None, 1e-5,
                                             None, None, None, None, 0.01, None, None, F, C, O, heads, lut, None, None, None,
                                             None, S, P, L, Q, *rows, None, ncol, thr, None, None, None, M, None)
    OK, UNSUPPORTED, BADARG = 0, -1, -2                                       # include/qot_gnn.h: QOT_OK, QOT_ERR_*
    assert rc() == OK and rc(M=7) == OK
    codes = {name: rc(**kw) for name, kw in {
        "a batch beside the status": dict(N=3), "K < 0": dict(K=-1), "P < 1": dict(P=0), "Q < 1": dict(Q=0),
        "ncol != F": dict(ncol=4), "a row outside P": dict(rows=(0, 7, 8, 10)), "threshold 0": dict(thr=0.0),
        "threshold nan": dict(thr=float("nan")), "M < 0": dict(M=-1), "no pointers with K > 0": dict(K=2, M=2)}.items()}
    assert all(c == BADARG for c in codes.values()), codes
    outside = {name: rc(**kw) for name, kw in {
        "F": dict(F=17, ncol=17), "C": dict(C=257), "O": dict(O=9), "heads": dict(heads=2), "lut": dict(lut=5),
        "Q above the cap": dict(Q=1025), "L * Q": dict(L=1 << 22, Q=1024)}.items()}
    assert all(c == UNSUPPORTED for c in outside.values()), outside
