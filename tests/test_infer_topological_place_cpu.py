"""CPU-side checks of ``TopologicalPredictor.place`` (``csrc/infer_topological_place.hip``): the host
statement ``to_graph.placement_links`` against ``create_topological_graph`` of the edited sample ->
``dataset.topological_data_from_graph`` -> ``canonical_link_order``, with the stated outcomes of the hand cases; the
conditions on the random batch; the refusals that need no device, through ``infer.topological_place_args``; the status
bits against the header; the new entry declared, bound, built and answering its envelope before any launch."""
import os

import numpy as np
import pytest
import torch

import status_topo_cases as TK
import topo_place_cases as C
from gnn_qot_estimation_amd import _lib, dataset, infer, to_graph as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the definition on the host
def _host_links(sample, freq):
    """The host builder's directed links of ``sample`` in canonical order, each with the conn_id its attributes carry
    (``conn_id`` has no range in ``FEATURE_RANGES``: it passes through unscaled, and is exact in fp32 here)."""
    ns = TK.status(sample[None], freq)
    d = dataset.topological_data_from_graph(TG.create_topological_graph(0, ["conn_id"], ns), ["conn_id"])
    m = d.edge_index.shape[1]
    ei, ea = TG.canonical_link_order(d.edge_index, torch.tensor([0, m]), d.edge_attr)
    return ei.numpy(), ea[:, 0].numpy().astype(np.int64)


def _compare(b, k):
    sample = b.ns.data[b.samples[k]]
    cells = C.candidate_cells(b, k)
    edited, _ = TG.place_lightpath(sample, b.values[k], cells, C.FI)
    want_ei, want_conn = _host_links(edited, b.ns.freq)
    ei, conn, outcome = TG.placement_links(sample, b.values[k], cells, C.FI)
    assert ei.dtype == np.int64 and conn.dtype == np.int64 and ei.shape == (2, conn.shape[0])
    assert np.array_equal(ei, want_ei), (k, ei, want_ei)
    assert np.array_equal(conn, want_conn), (k, conn, want_conn)              # the winner's attributes, through its conn
    # the outcome, restated from the two graphs: the link count and who carries the candidate's pair
    before = _host_links(sample, b.ns.freq)[0].shape[1]
    mine = int(b.values[k][C.FI["conn_id"]])
    if ei.shape[1] > before:
        assert outcome == "new pair" and ei.shape[1] - before == (1 if b.values[k][C.FI["src_id"]] == b.values[k][C.FI["dst_id"]] else 2)
    else:
        assert outcome == ("takes the pair" if mine in conn.tolist() else "loses the pair")
        if outcome == "loses the pair":
            assert np.array_equal(conn, _host_links(sample, b.ns.freq)[1])
    return ei, conn, outcome


def test_placement_links_on_the_random_batch():
    b = C.batch()                                                             # (asserts the conditions on the inputs)
    assert len(b.samples) == 12 and b.values.shape == (12, C.P) and len(b.ns) == 8 and b.ns.data.shape[2:] == (6, 12)
    outcomes = [_compare(b, k)[2] for k in range(12)]
    assert all(outcomes.count(name) >= 2 for name in C.OUTCOMES), outcomes
    fig = C.figures(b)
    assert [o for o, _, _ in fig] == outcomes
    assert any(loop for _, loop, _ in fig) and any(rev for _, _, rev in fig)
    # conn ids on both sides of the incumbents': on an occupied pair some candidate is above and some below
    sides = set()
    for k, s in enumerate(b.samples):
        inc = C.incumbent(b.ns.data[s], int(b.values[k][C.FI["src_id"]]), int(b.values[k][C.FI["dst_id"]]))
        if inc is not None:
            sides.add(int(b.values[k][C.FI["conn_id"]]) > inc[0])
    assert sides == {True, False}
    assert C.meets_conditions(C.random_batch(C.SEED)) and all(not C.meets_conditions(C.random_batch(s)) for s in range(C.SEED))


@pytest.mark.parametrize("name", list(C.HAND))
def test_placement_links_and_outcomes_on_the_hand_cases(name):
    case = C.HAND[name]()
    ei, _, outcome = _compare(C.as_batch(case), 0)
    assert outcome == case.outcome and ei.shape[1] == case.links


def test_placement_links_names_the_candidate_on_its_pair():
    ei, conn, outcome = TG.placement_links(*(lambda c: (c.ns.data[0], c.values, c.cells, C.FI))(C.HAND["takes the pair"]()))
    assert ei.tolist() == [[0, 1, 3, 4, 5], [3, 4, 0, 1, 5]] and conn.tolist() == [7, 12, 7, 12, 0] and outcome == "takes the pair"
    case = C.HAND["loses the pair"]()
    ei, conn, outcome = TG.placement_links(case.ns.data[0], case.values, case.cells, C.FI)
    assert conn.tolist() == [7, 9, 7, 9, 0] and outcome == "loses the pair"
    case = C.HAND["a self loop in an empty sample"]()
    ei, conn, outcome = TG.placement_links(case.ns.data[0], case.values, case.cells, C.FI)
    assert ei.tolist() == [[32], [32]] and conn.tolist() == [5] and outcome == "new pair"
    with pytest.raises(ValueError, match="occupied"):
        TG.placement_links(case.ns.data[0] + 1.0, case.values, case.cells, C.FI)
    taken = C.HAND["takes the pair"]()
    with pytest.raises(ValueError, match="conn_id 9 is a lightpath of the sample already"):
        TG.placement_links(taken.ns.data[0], TK.vec(9.6, 5, 2), taken.cells, C.FI)
    with pytest.raises(ValueError, match="outside"):
        TG.placement_links(taken.ns.data[0], taken.values, [[6], [0]], C.FI)


# ------------------------------------------------------------------ refusals without a device
def _cpu_status(lp_feat=None):
    ns = TK.chunk()
    data, freq = torch.from_numpy(ns.data), torch.from_numpy(np.asarray(ns.freq, dtype=np.float64))
    target = torch.zeros(data.shape[0], len(ns.metric), dtype=torch.float64)
    return TG.DeviceStatus(data, target, freq, lp_feat or ns.lp_feat, ns.metric)


def test_refusals_before_any_launch():
    st = _cpu_status()
    b = C.batch()
    good = dict(samples=list(b.samples), values=torch.from_numpy(b.values), cells=torch.from_numpy(b.cells),
                cell_ptr=list(b.cell_ptr))

    def args(**kw):
        a = dict(good, **kw)
        return infer.topological_place_args(a.pop("status", st), a.pop("D", 4), a.pop("samples"), a.pop("values"),
                                            a.pop("cells"), a.pop("cell_ptr"), **a)
    with pytest.raises(TypeError, match="DeviceStatus"):
        args(status=TK.chunk())
    for bad in (b.values, torch.from_numpy(b.values).float(), torch.from_numpy(b.values)[:, :9], torch.from_numpy(b.values)[0]):
        with pytest.raises(ValueError, match="values must be a float64 tensor"):
            args(values=bad)
    for bad in (b.cells, torch.from_numpy(b.cells).int(), torch.from_numpy(b.cells).T.contiguous(), torch.from_numpy(b.cells)[0]):
        with pytest.raises(ValueError, match="cells must be an int64 tensor"):
            args(cells=bad)
    for bad in (None, True):
        with pytest.raises(ValueError, match="samples must be an int, a sequence"):
            args(samples=bad)
    with pytest.raises(ValueError, match="samples names 11 candidates, values has 12 rows"):
        args(samples=list(b.samples)[:-1])
    for bad in (torch.zeros(11, dtype=torch.int64), torch.zeros(12, dtype=torch.int32), torch.zeros(12, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="1-d int64 tensor of 12 sample numbers"):
            args(samples=bad)
    with pytest.raises(ValueError, match="K \\+ 1 = 13 offsets"):
        args(cell_ptr=list(b.cell_ptr)[:-1])
    with pytest.raises(ValueError, match="K \\+ 1 = 13 offsets"):
        args(cell_ptr=torch.tensor(b.cell_ptr, dtype=torch.int32))
    M = b.cells.shape[1]
    for bad in ([1] + list(b.cell_ptr)[1:], list(b.cell_ptr)[:-1] + [M + 1], [0, 3, 2] + list(b.cell_ptr)[3:]):
        with pytest.raises(ValueError, match="non-decreasing from 0 to M"):
            args(cell_ptr=bad)
    with pytest.raises(ValueError, match="candidate 1 has an empty slice"):
        args(cell_ptr=[0, b.cell_ptr[1], b.cell_ptr[1]] + list(b.cell_ptr)[3:])
    # ... then everything topological_status_args refuses, a chunk on the CPU last
    with pytest.raises(ValueError, match="edge_dim"):
        args(D=3)
    with pytest.raises(ValueError, match="edge_dim"):
        args(features_to_consider=["freq", "mod_order"])
    for gone in ("conn_id", "src_id", "dst_id", "num_spans"):
        with pytest.raises(ValueError, match=repr(gone)):
            args(status=_cpu_status([("x_" + n if n == gone else n) for n in TG.LP_FEAT]))
    with pytest.raises(IndexError, match="index out of range in self"):
        args(num_embeddings=74)
    with pytest.raises(ValueError, match="TopologicalPredictor.place: the status chunk is on the CPU"):
        args()
    with pytest.raises(ValueError, match="on the CPU"):                       # an int for all K passes the list checks
        args(samples=3)
    with pytest.raises(ValueError, match="on the CPU"):
        args(num_embeddings=75, model_device=torch.device("cuda", 0))


def test_check_model_refusals_come_first():
    import gnn_qot_estimation_amd as q
    pred = object.__new__(infer.TopologicalPredictor)                          # (the constructor refuses a CPU model itself)
    pred.model = q.TopologicalGNN(75, 16, 3, 4, dropout_p=0.0)
    with pytest.raises(ValueError, match="on the CPU"):
        pred.place(TK.chunk(), 0, None, None, None)                            # not the TypeError: the model is named first


# ------------------------------------------------------------------ the status bits, the entry point
def test_status_bits_do_not_collide_and_are_stated_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    bits = (infer.TOPO_PLACE_BAD_CELL, infer.TOPO_PLACE_OCCUPIED, infer.TOPO_PLACE_CONN_TAKEN)
    assert bits == (128, 256, 512)
    for name, bit in zip(("BAD_CELL", "OCCUPIED", "CONN_TAKEN"), bits):
        assert f"#define QOT_TOPO_PLACE_{name} {bit} " in hdr
    older = (1, 2, 4, infer.TOPO_STATUS_BAD_CONN, infer.TOPO_STATUS_TOO_MANY, infer.TOPO_STATUS_BAD_SAMPLE,
             infer.TOPO_STATUS_BAD_ENDPOINT)
    assert len({*older, *bits}) == 10 and min(bits) > max(older)
    assert [bit for bit, _ in infer.TopologicalPredictor._PLACE_CAUSES] == list(bits)
    assert "place" in infer.TopologicalPredictor._FLAGS[1]


def test_check_status_names_the_cause():
    pred = object.__new__(infer.TopologicalPredictor)
    infer._DeviceState.__init__(pred)
    for bit, words in ((infer.TOPO_PLACE_BAD_CELL, "link or frequency index outside the sample"),
                       (infer.TOPO_PLACE_OCCUPIED, "channel is occupied"),
                       (infer.TOPO_PLACE_CONN_TAKEN, "conn_id is a lightpath of the sample already"),
                       (infer.TOPO_STATUS_BAD_ENDPOINT, "src_id / dst_id is not an integer")):
        pred._status = torch.tensor([bit], dtype=torch.int32)
        with pytest.raises(_lib.QotError, match=words):
            pred.check_status()
    pred._status = torch.tensor([infer.TOPO_PLACE_OCCUPIED | infer.TOPO_STATUS_BAD_SAMPLE], dtype=torch.int32)
    with pytest.raises(_lib.QotError, match="sample number.*channel is occupied"):
        pred.check_status()
    pred.check_status()


def test_entry_is_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    assert "int qot_topological_infer_place(" in hdr and "qot_topological_infer_place" in _lib.SIGNATURES
    status_sig, place_sig = _lib.SIGNATURES["qot_topological_infer_status"], _lib.SIGNATURES["qot_topological_infer_place"]
    assert place_sig[0] == status_sig[0]
    # the status entry's arguments up to ncol, then values, cells, cell_ptr, the cell count, the stream
    assert place_sig[1][:len(status_sig[1]) - 1] == status_sig[1][:-1] and len(place_sig[1]) == len(status_sig[1]) + 4
    csrc = os.path.join(ROOT, "gnn_qot_estimation_amd", "csrc")
    assert " infer_topological_place.hip " in open(os.path.join(csrc, "Makefile")).read()
    assert hasattr(_lib.load(), "qot_topological_infer_place")
    # what the two status kernels share is stated once, in the header both include
    shared = open(os.path.join(csrc, "infer_topological_status_dev.hpp")).read()
    for piece in ("struct InferStatusEdges {", "int topo_status_bits(", "size_t kTopoStatusStatic =", "struct TopoStatusArgs {"):
        assert piece in shared
        for f in ("infer_topological_status.hip", "infer_topological_place.hip"):
            src = open(os.path.join(csrc, f)).read()
            assert '#include "infer_topological_status_dev.hpp"' in src and piece not in src, (f, piece)


def test_entry_answers_the_envelope_before_any_launch():
    """Sizes and the envelope are answered without a pointer being looked at; K == 0 is QOT_OK without a launch."""
    lib = _lib.load()

    def rc(K=0, S=4, P=10, L=6, Q=12, H=64, D=4, O=3, N=75, E=0, n_max=75, max_e=512, V=75, rows=(0, 1, 2), ncol=4,
           ei=None, M=0):
        return lib.qot_topological_infer_place(None, ei, None, None, None, N, E, K, n_max, max_e, None, 4 * H, None, 128, None,
                                               V, None, None, None, None, None, None, None, None, None, 0.01, 0.01, None,
                                               H, D, O, None, None, None, None, S, P, L, Q, *rows, None, ncol, None, None,
                                               None, M, None)
    OK, UNSUPPORTED, BADARG = 0, -1, -2                                       # include/qot_gnn.h: QOT_OK, QOT_ERR_*
    assert rc() == OK and rc(M=7) == OK
    for H in (16, 32, 64):                                                     # the whole envelope fits the LDS budget
        for D in (1, 2, 3, 4):
            assert rc(H=H, D=D, ncol=D) == OK, (H, D)
    codes = {name: rc(**kw) for name, kw in {
        "a batch beside the status": dict(E=3), "an edge_index": dict(ei=16), "N != 75": dict(N=74), "n_max != 75": dict(n_max=76),
        "max_e != 512": dict(max_e=511), "K < 0": dict(K=-1), "S < 0": dict(S=-1), "P < 1": dict(P=0), "L < 1": dict(L=0),
        "Q < 1": dict(Q=0), "V < 1": dict(V=0), "ncol != D": dict(ncol=3), "a row outside P": dict(rows=(0, 1, 10)),
        "a negative row": dict(rows=(-1, 1, 2)), "M < 0": dict(M=-1), "no pointers with K > 0": dict(K=2, M=2)}.items()}
    assert all(c == BADARG for c in codes.values()), codes
    outside = {name: rc(**kw) for name, kw in {
        "H": dict(H=48), "D": dict(D=5, ncol=5), "O": dict(O=9), "Q above the cap": dict(Q=1025),
        "L * Q": dict(L=1 << 21, Q=1024), "K": dict(K=1 << 31)}.items()}
    assert all(c == UNSUPPORTED for c in outside.values()), outside
