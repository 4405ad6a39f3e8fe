"""CPU-side checks of ``LightpathPredictor.from_status`` (``csrc/infer_lightpath_status.hip``): the host
statement of what a row takes of its sample, ``to_graph.lut_neighbourhood``, against ``create_lightpath_graph`` plus the
networkx neighbours of the LUT node; the refusals that need no device, through ``infer.lightpath_status_args``; the new
entry declared, bound and answering its envelope before any launch."""
import os

import numpy as np
import pytest
import torch

import status_infer_cases as K
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the definition on the host
@pytest.mark.parametrize("thr", K.THRESHOLDS)
def test_lut_neighbourhood_on_the_chunk(thr):
    ns = K.chunk()
    degrees = []
    for i in range(len(ns)):
        want = K.host_neighbourhood(ns, i, thr)
        got = TG.lut_neighbourhood(ns.data[i], ns.freq, ns.feature_indexes, thr)
        assert got == want, (i, got, want)
        assert got[0] == 1 and got[1] is not None
        degrees.append(len(got[2]))
    assert degrees == K.IN_DEGREES[thr]


@pytest.mark.parametrize("name", list(K.HAND))
def test_lut_neighbourhood_on_the_hand_cases(name):
    ns, thr, count, degree = K.HAND[name]()
    want = K.host_neighbourhood(ns, 0, thr)
    got = TG.lut_neighbourhood(ns.data[0], ns.freq, ns.feature_indexes, thr)
    assert got == want, (got, want)
    assert got[0] == count and len(got[2]) == degree
    assert (got[1] is None) == (count == 0)


def test_lut_neighbourhood_names_each_interferer_once_and_in_first_seen_order():
    ns, thr, _, _ = K.HAND["an interferer sharing two links and two slots"]()
    assert TG.lut_neighbourhood(ns.data[0], ns.freq, ns.feature_indexes, thr) == (1, 5, [8])
    ns, thr, _, _ = K.HAND["two flagged lightpaths"]()
    assert TG.lut_neighbourhood(ns.data[0], ns.freq, ns.feature_indexes, thr) == (2, 8, [5, 7])
    ns, thr, _, _ = K.hub(65)
    count, conn, inter = TG.lut_neighbourhood(ns.data[0], ns.freq, ns.feature_indexes, thr)
    assert (count, conn) == (1, 1000 - 3 * 32) and inter == [1000 - 3 * k for k in range(66) if k != 32]


# ------------------------------------------------------------------ refusals without a device
def _cpu_status(ns=None, lp_feat=None, Q=None):
    ns = ns or K.chunk()
    data, freq = torch.from_numpy(ns.data), torch.from_numpy(np.asarray(ns.freq, dtype=np.float64))
    if Q is not None:
        data, freq = torch.zeros(1, data.shape[1], 1, Q, dtype=torch.float64), torch.arange(Q, dtype=torch.float64)
    target = torch.zeros(data.shape[0], len(ns.metric), dtype=torch.float64)
    return TG.DeviceStatus(data, target, freq, lp_feat or ns.lp_feat, ns.metric)


def test_refusals_before_any_launch():
    st = _cpu_status()
    args = lambda **kw: infer.lightpath_status_args(kw.pop("status", st), kw.pop("F", 5), kw.pop("lut", K.LUT_COL), **kw)
    with pytest.raises(TypeError, match="DeviceStatus"):
        args(status=K.chunk())
    with pytest.raises(infer.EnvelopeError, match="on the CPU"):
        args()
    with pytest.raises(infer.EnvelopeError, match="1024 frequency slots"):
        args(status=_cpu_status(Q=1025))
    with pytest.raises(infer.EnvelopeError, match="on the CPU"):              # (1024 itself passes that check)
        args(status=_cpu_status(Q=1024))
    with pytest.raises(infer.EnvelopeError, match="in_channels"):
        args(F=6)
    with pytest.raises(infer.EnvelopeError, match="in_channels"):
        args(features_to_consider=["freq", "mod_order"])
    with pytest.raises(infer.EnvelopeError, match="is_lut_index"):
        args(lut=0)
    renamed = [("hops" if n == "num_spans" else n) for n in TG.LP_FEAT]
    with pytest.raises(infer.EnvelopeError, match="'num_spans'"):
        args(status=_cpu_status(lp_feat=renamed))
    for gone in ("conn_id", "osnr", "snr", "ber"):
        with pytest.raises(infer.EnvelopeError, match=repr(gone)):
            args(status=_cpu_status(lp_feat=[("x_" + n if n == gone else n) for n in TG.LP_FEAT]))
    for thr in (0.0, -0.05, float("inf"), float("nan"), "0.05", None, True):
        with pytest.raises(ValueError, match="finite positive"):
            args(freq_threshold=thr)
    for thr in (0.0, float("nan")):                                            # a ValueError proper, not the envelope's
        with pytest.raises(ValueError) as e:
            args(freq_threshold=thr)
        assert not isinstance(e.value, infer.EnvelopeError)


def test_status_bits_do_not_collide_and_are_stated_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    bits = (infer.LP_STATUS_BAD_CONN, infer.LP_STATUS_TOO_MANY, infer.LP_STATUS_BAD_SAMPLE)
    for name, bit in zip(("BAD_CONN", "TOO_MANY", "BAD_SAMPLE"), bits):
        assert f"#define QOT_LP_STATUS_{name} {bit} " in hdr
    assert all(b & (1 | 2 | 4) == 0 for b in bits) and len({1, 2, 4, *bits}) == 6     # above the other kernels' bits
    assert [b for b, _ in infer.LightpathPredictor._CAUSES] == list(bits)


def test_entry_answers_the_envelope_before_any_launch():
    """Sizes and the envelope are answered without a pointer being looked at; G == 0 is QOT_OK without a launch."""
    assert "qot_lightpath_infer_status" in _lib.SIGNATURES
    lib = _lib.load()

    def rc(G=0, S=4, P=10, L=6, Q=12, F=5, C=32, O=3, heads=4, lut=1, rows=(0, 7, 8, 9), ncol=5, thr=0.05, N=0):
        none = [None] * 6
        return lib.qot_lightpath_infer_status(*none, 0, N, 0, G, None, None, None, None, 0.2, None, None, None, None, 1e-5,
                                              None, None, None, None, 0.01, None, None, F, C, O, heads, lut, None, None, None,
                                              None, S, P, L, Q, *rows, None, ncol, thr, None)
    OK, UNSUPPORTED, BADARG = 0, -1, -2                                       # include/qot_gnn.h: QOT_OK, QOT_ERR_*
    assert rc() == OK
    codes = {name: rc(**kw) for name, kw in {
        "a batch beside the status": dict(N=3), "G < 0": dict(G=-1), "P < 1": dict(P=0), "Q < 1": dict(Q=0),
        "ncol != F": dict(ncol=4), "a row outside P": dict(rows=(0, 7, 8, 10)), "threshold 0": dict(thr=0.0),
        "threshold nan": dict(thr=float("nan")), "threshold inf": dict(thr=float("inf")),
        "no pointers with G > 0": dict(G=2)}.items()}
    assert all(c == BADARG for c in codes.values()), codes
    outside = {name: rc(**kw) for name, kw in {
        "F": dict(F=17, ncol=17), "C": dict(C=257), "O": dict(O=9), "heads": dict(heads=2), "lut": dict(lut=5),
        "Q above the cap": dict(Q=1025), "L * Q": dict(L=1 << 22, Q=1024)}.items()}
    assert all(c == UNSUPPORTED for c in outside.values()), outside
