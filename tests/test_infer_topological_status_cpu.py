"""CPU-side checks of ``TopologicalPredictor.from_status`` (``csrc/infer_topological_status.hip``): the host
statement of the links a row is summed over, ``to_graph.topological_links``, against ``create_topological_graph`` ->
``dataset.topological_data_from_graph`` -> ``canonical_link_order``; the refusals that need no device, through
``infer.topological_status_args``; the status bits against the header; the new entry declared, bound and answering its
envelope before any launch."""
import os

import numpy as np
import pytest
import torch

import status_topo_cases as K
from gnn_qot_estimation_amd import _lib, dataset, infer, to_graph as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the definition on the host
def _host_links(ns, i):
    """The host builder's directed links of sample ``i`` in canonical order, each with the conn_id its attributes carry
    (``conn_id`` has no range in ``FEATURE_RANGES``: it passes through unscaled, and is exact in fp32 here)."""
    d = dataset.topological_data_from_graph(TG.create_topological_graph(i, ["conn_id"], ns), ["conn_id"])
    m = d.edge_index.shape[1]
    ei, ea = TG.canonical_link_order(d.edge_index, torch.tensor([0, m]), d.edge_attr)
    return ei.numpy(), ea[:, 0].numpy().astype(np.int64)


def _compare(ns, links=None):
    for i in range(len(ns)):
        want_ei, want_conn = _host_links(ns, i)
        ei, conn = TG.topological_links(ns.data[i], ns.feature_indexes)
        assert ei.dtype == np.int64 and conn.dtype == np.int64 and ei.shape == (2, conn.shape[0])
        assert np.array_equal(ei, want_ei), (i, ei, want_ei)
        assert np.array_equal(conn, want_conn), (i, conn, want_conn)      # the winner's attributes, through its conn
        if links is not None:
            assert ei.shape[1] == links[i]


def test_topological_links_on_the_chunks():
    _compare(K.chunk(), K.LINKS)
    _compare(K.other_chunk())
    _compare(K.synthetic_chunk())


@pytest.mark.parametrize("name", list(K.HAND))
def test_topological_links_on_the_hand_cases(name):
    ns, links = K.HAND[name]()
    _compare(ns, links)


def test_topological_links_name_the_largest_conn_and_the_canonical_order():
    ns, _ = K.HAND["the builder's hand sample"]()
    ei, conn = TG.topological_links(ns.data[0], ns.feature_indexes)
    assert ei.tolist() == [[0, 1, 3, 4, 5], [3, 4, 0, 1, 5]] and conn.tolist() == [7, 9, 7, 9, 0]
    for order in ((9, 3, 5), (3, 5, 9), (3, 9, 5)):
        ns, _ = K.parallel(order)
        ei, conn = TG.topological_links(ns.data[0], ns.feature_indexes)
        assert ei.tolist() == [[2, 7, 7, 8], [7, 2, 8, 7]] and conn.tolist() == [9, 9, 1, 1]
    ns, _ = K.HAND["an empty sample beside a non-empty one"]()
    ei, conn = TG.topological_links(ns.data[0], ns.feature_indexes)
    assert ei.shape == (2, 0) and conn.shape == (0,)


# ------------------------------------------------------------------ refusals without a device
def _cpu_status(ns=None, lp_feat=None, L=None, Q=None):
    ns = ns or K.chunk()
    data, freq = torch.from_numpy(ns.data), torch.from_numpy(np.asarray(ns.freq, dtype=np.float64))
    if Q is not None:
        data, freq = torch.zeros(1, data.shape[1], L or 1, Q, dtype=torch.float64), torch.arange(Q, dtype=torch.float64)
    target = torch.zeros(data.shape[0], len(ns.metric), dtype=torch.float64)
    return TG.DeviceStatus(data, target, freq, lp_feat or ns.lp_feat, ns.metric)


class _Elsewhere:
    """Stands in for ``status.data`` of a chunk on a second GPU (there is one GPU at most here): what the checks look at."""
    is_cuda = True
    device = torch.device("cuda", 1)

    def __init__(self, shape):
        self.shape = shape


def test_refusals_before_any_launch():
    st = _cpu_status()
    args = lambda **kw: infer.topological_status_args(kw.pop("status", st), kw.pop("D", 4), **kw)
    with pytest.raises(TypeError, match="DeviceStatus"):
        args(status=K.chunk())
    with pytest.raises(ValueError, match="on the CPU"):
        args()
    with pytest.raises(ValueError, match="1024 frequency slots"):
        args(status=_cpu_status(Q=1025))
    with pytest.raises(ValueError, match="on the CPU"):                       # (1024 itself passes that check)
        args(status=_cpu_status(Q=1024))
    huge = _cpu_status()
    huge.data = _Elsewhere((1, 10, 1 << 21, 1024))                             # L * Q == 2^31
    with pytest.raises(ValueError, match="below 2\\^31"):
        args(status=huge)
    with pytest.raises(ValueError, match="edge_dim"):
        args(D=3)
    with pytest.raises(ValueError, match="edge_dim"):
        args(features_to_consider=["freq", "mod_order"])
    renamed = [("hops" if n == "num_spans" else n) for n in TG.LP_FEAT]
    with pytest.raises(ValueError, match="'num_spans'"):
        args(status=_cpu_status(lp_feat=renamed))
    for gone in ("conn_id", "src_id", "dst_id"):
        with pytest.raises(ValueError, match=repr(gone)):
            args(status=_cpu_status(lp_feat=[("x_" + n if n == gone else n) for n in TG.LP_FEAT]))
    for bad in (torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2)):
        with pytest.raises(ValueError, match="1-d int64"):
            args(samples=bad)
    with pytest.raises(ValueError, match="on the CPU"):                       # (a well-formed tensor and a list pass)
        args(samples=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="on the CPU"):
        args(samples=[0, 1])
    with pytest.raises(IndexError, match="index out of range in self"):
        args(num_embeddings=74)
    with pytest.raises(ValueError, match="on the CPU"):                       # (75 rows hold the topology)
        args(num_embeddings=75)
    with pytest.raises(ValueError, match="on the CPU"):
        args(model_device=torch.device("cuda", 0))
    other = _cpu_status()
    other.data = _Elsewhere(tuple(other.data.shape))
    with pytest.raises(ValueError, match="on cuda:1, the model on cuda:0"):
        args(status=other, model_device=torch.device("cuda", 0))
    sa = args(status=other, model_device=torch.device("cuda", 1))             # ... and the same device passes
    assert (sa.S, sa.P, sa.L, sa.Q) == (8, 10, 6, 12) and sa.features == K.FEATS
    assert (sa.conn_row, sa.src_row, sa.dst_row) == (K.FI["conn_id"], K.FI["src_id"], K.FI["dst_id"])


def test_check_model_refusals_come_first():
    """Everything ``_check_model`` refuses is refused by ``from_status`` before the status is looked at."""
    import gnn_qot_estimation_amd as q
    model = q.TopologicalGNN(75, 16, 3, 4, dropout_p=0.0)
    pred = object.__new__(infer.TopologicalPredictor)                          # (the constructor refuses a CPU model itself)
    pred.model = model
    with pytest.raises(ValueError, match="on the CPU"):
        pred.from_status(K.chunk())                                            # not the TypeError: the model is named first


def test_status_bits_do_not_collide_and_are_stated_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    bits = (infer.TOPO_STATUS_BAD_CONN, infer.TOPO_STATUS_TOO_MANY, infer.TOPO_STATUS_BAD_SAMPLE, infer.TOPO_STATUS_BAD_ENDPOINT)
    assert bits == (8, 16, 32, 64)
    for name, bit in zip(("BAD_CONN", "TOO_MANY", "BAD_SAMPLE", "BAD_ENDPOINT"), bits):
        assert f"#define QOT_TOPO_STATUS_{name} {bit} " in hdr
    assert all(b & (1 | 2 | 4) == 0 for b in bits) and len({1, 2, 4, *bits}) == 7     # above the predictor's 1 / 2 / 4
    causes = infer.TopologicalPredictor._CAUSES
    assert [b for b, _ in causes] == list(bits)
    words = dict(TG._SG_CAUSES)
    assert [t for _, t in causes] == [words[TG.SG_BAD_CONN], words[TG.SG_TOO_MANY], words[TG.SG_BAD_SAMPLE],
                                      words[TG.SG_BAD_ENDPOINT]]
    assert "from_status" in infer.TopologicalPredictor._FLAGS[1]
    assert infer.TOPO_STATUS_MAX_LINKS == 2 * TG.MAX_LIGHTPATHS


def test_entry_answers_the_envelope_before_any_launch():
    """Sizes and the envelope are answered without a pointer being looked at; G == 0 is QOT_OK without a launch."""
    assert "qot_topological_infer_status" in _lib.SIGNATURES
    lib = _lib.load()

    def rc(G=0, S=4, P=10, L=6, Q=12, H=64, D=4, O=3, N=75, E=0, n_max=75, max_e=512, V=75, rows=(0, 1, 2), ncol=4,
           ei=None):
        return lib.qot_topological_infer_status(None, ei, None, None, None, N, E, G, n_max, max_e, None, 4 * H, None, 128, None,
                                                V, None, None, None, None, None, None, None, None, None, 0.01, 0.01, None,
                                                H, D, O, None, None, None, None, S, P, L, Q, *rows, None, ncol, None)
    OK, UNSUPPORTED, BADARG = 0, -1, -2                                       # include/qot_gnn.h: QOT_OK, QOT_ERR_*
    assert rc() == OK
    for H in (16, 32, 64):                                                     # the whole envelope fits the LDS budget
        for D in (1, 2, 3, 4):
            assert rc(H=H, D=D, ncol=D) == OK, (H, D)
    codes = {name: rc(**kw) for name, kw in {
        "a batch beside the status": dict(E=3), "an edge_index": dict(ei=16), "N != 75": dict(N=74), "n_max != 75": dict(n_max=76),
        "max_e != 512": dict(max_e=511), "G < 0": dict(G=-1), "S < 0": dict(S=-1), "P < 1": dict(P=0), "L < 1": dict(L=0),
        "Q < 1": dict(Q=0), "V < 1": dict(V=0), "ncol != D": dict(ncol=3), "a row outside P": dict(rows=(0, 1, 10)),
        "a negative row": dict(rows=(-1, 1, 2)), "no pointers with G > 0": dict(G=2)}.items()}
    assert all(c == BADARG for c in codes.values()), codes
    outside = {name: rc(**kw) for name, kw in {
        "H": dict(H=48), "D": dict(D=5, ncol=5), "O": dict(O=9), "Q above the cap": dict(Q=1025),
        "L * Q": dict(L=1 << 21, Q=1024), "G": dict(G=1 << 31)}.items()}
    assert all(c == UNSUPPORTED for c in outside.values()), outside
