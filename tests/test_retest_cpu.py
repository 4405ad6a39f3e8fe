"""CPU-side checks of ``LightpathPredictor.retest`` (``csrc/infer_lightpath_retest.hip``): the host
statement ``to_graph.retest_neighbourhood`` on the hand cases of ``retest_cases.py`` and against ``lut_neighbourhood`` of the
numpy-flagged sample; ``infer.retest_chunk``; the refusals that need no device, through ``infer.lightpath_retest_args``; the
new entry declared, bound, built and answering its envelope before any launch."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import place_cases as PC
import retest_cases as RC
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = [RC.FI[n] for n in ("osnr", "snr", "ber")]


def _cpu_status(ns):
    data, freq = torch.from_numpy(ns.data), torch.from_numpy(np.asarray(ns.freq, dtype=np.float64))
    return TG.DeviceStatus(data, torch.from_numpy(ns.target), freq, ns.lp_feat, ns.metric)


def _flag(sample, conn):
    """``materialise_retest`` without values, in numpy."""
    out = sample.copy()
    mine = np.any(out != 0, axis=0) & (np.trunc(out[RC.FI["conn_id"]]) == conn)
    out[LABELS] = np.where(mine, -1.0, out[LABELS])
    return out


# ------------------------------------------------------------------ the host statement
@pytest.mark.parametrize("name", list(RC.HAND))
def test_hand_cases_on_the_host(name):
    c = RC.HAND[name]()
    got = RC.host(c.ns, 0, c.thr)
    assert got == c.want
    assert [t[1] for t in got] == list(range(len(got)))
    assert TG.lut_neighbourhood(c.ns.data[0], c.ns.freq, RC.FI, c.thr)[0] == c.count


@pytest.mark.parametrize("thr", RC.THRESHOLDS)
@pytest.mark.parametrize("flagged", [False, True])
def test_retest_neighbourhood_is_lut_neighbourhood_of_the_flagged_sample(flagged, thr):
    """Where the sample has no flagged lightpath of its own, flagging lightpath ``conn`` makes it the first flagged one, and
    ``lut_neighbourhood`` names its sources; the nodes count up; nobody is their own source and the rule is symmetric."""
    ns = RC.samples(flagged)
    seen = 0
    for s in range(ns.data.shape[0]):
        got = RC.host(ns, s, thr)
        assert [t[1] for t in got] == list(range(len(got))) and len({t[0] for t in got}) == len(got) >= 10
        by_conn = {conn: sources for conn, _, sources in got}
        for conn, node, sources in got:
            assert conn not in sources and all(conn in by_conn[x] for x in sources)
            count, first, interferers = TG.lut_neighbourhood(_flag(ns.data[s], conn), ns.freq, RC.FI, thr)
            own = 700 + s                                   # place_cases.dense_sample's flagged lightpath: first seen
            assert count == 1 + (flagged and conn != own)
            if not flagged or conn == own:
                assert (first, interferers) == (conn, sources)
                seen += 1
    assert seen >= (2 if flagged else 20)


def test_the_conditions_on_the_random_inputs():
    for flagged in (False, True):
        ns = RC.samples(flagged)
        degrees = [len(t[2]) for s in range(2) for t in RC.host(ns, s, 0.12)]
        assert sum(d >= 2 for d in degrees) >= 16 and sum(d == 0 for d in degrees) <= 1, degrees


# ------------------------------------------------------------------ the chunk
def test_retest_chunk():
    assert infer.RETEST_MAX_CHUNK == 32 and infer.RETEST_MAX_LIGHTPATHS == 256
    for cus in (1, 64, 256, 304):
        for M in (1, 7, 31, 32, 33, 255, 256):
            last = 0
            for G in (1, 2, 3, 8, 37, 64, 255, 256, 257, 512, 4096):
                c = infer.retest_chunk(G, M, cus)
                assert isinstance(c, int) and 1 <= c <= min(32, M), (G, M, cus, c)
                blocks = -(-M // c)
                assert blocks * c >= M and (c - 1) * blocks < M                # the product covers M; equal shares
                assert c >= last, (G, M, cus)                                  # monotone in G
                last = c
                if G >= cus:                                                   # G alone fills the machine: chunk 32's grid
                    assert blocks == -(-M // 32)
                elif G * M >= cus:                                             # at least one workgroup per CU ...
                    assert G * blocks >= cus
                    assert all(G * -(-M // c2) < cus for c2 in range(c + 1, 33) if -(-M // c2) < blocks)   # ... no smaller grid does
                else:
                    assert c == 1
    assert infer.retest_chunk(1, 256, 256) == 1 and infer.retest_chunk(8, 256, 256) == 8
    assert infer.retest_chunk(64, 256, 256) == 32 and infer.retest_chunk(512, 256, 256) == 32
    assert infer.retest_chunk(0, 256, 256) == 1
    for M in (0, 257, -1):
        with pytest.raises(ValueError, match="retest_chunk: max_lightpaths"):
            infer.retest_chunk(4, M, 256)


# ------------------------------------------------------------------ refusals without a device
def test_refusals_before_any_launch():
    ns = RC.samples()
    st = _cpu_status(ns)
    conns = torch.tensor([[1, 2, -1], [3, 4, 5]])

    def args(**kw):
        return infer.lightpath_retest_args(kw.pop("status", st), kw.pop("F", 5), kw.pop("lut", PC.LUT_COL), **kw)

    who = "LightpathPredictor.retest"
    with pytest.raises(TypeError, match=who + " takes a DeviceStatus"):
        args(status=ns)
    with pytest.raises(infer.EnvelopeError, match="on the CPU"):             # everything is in order but the device
        args()
    for M in (1, 7, 256):
        with pytest.raises(infer.EnvelopeError, match="on the CPU"):
            args(max_lightpaths=M)
    for M in (0, 257, -1, True, False, 8.0, None, "8"):
        with pytest.raises(ValueError, match=who + r": max_lightpaths must be an int in 1 \.\.\. 256") as e:
            args(max_lightpaths=M)
        assert not isinstance(e.value, infer.EnvelopeError)
    for chunk in (None, 1, 5, 32):
        with pytest.raises(infer.EnvelopeError, match="on the CPU"):
            args(chunk=chunk)
    for chunk in (0, 33, -1, True, False, 8.0, "8"):
        with pytest.raises(ValueError, match=who + r": chunk must be None or an int in 1 \.\.\. 32") as e:
            args(chunk=chunk)
        assert not isinstance(e.value, infer.EnvelopeError)
    with pytest.raises(infer.EnvelopeError, match="on the CPU"):
        args(conns=conns, max_lightpaths=0)                                   # ignored beside conns
    for bad in (conns.int(), conns[0], conns[:, :0], torch.zeros(2, 257, dtype=torch.int64), conns.tolist(), conns[None]):
        with pytest.raises(ValueError, match=who + r": conns must be an int64 tensor \[G, M\]") as e:
            args(conns=bad)
        assert not isinstance(e.value, infer.EnvelopeError)
    for label in ("osnr", "snr", "ber"):
        with pytest.raises(infer.EnvelopeError, match=f"{who}: '{label}' cannot be a feature"):
            args(features_to_consider=["freq", "mod_order", "num_spans", label])
    # every refusal of lightpath_status_args, under the new name
    for t in (0.0, -0.05, float("inf"), float("nan"), "0.05", None, True):
        with pytest.raises(ValueError, match=who + ": freq_threshold must be a finite positive number"):
            args(freq_threshold=t)
    with pytest.raises(infer.EnvelopeError, match=who + ".*in_channels"):
        args(F=6)
    with pytest.raises(infer.EnvelopeError, match=who + ".*is_lut_index"):
        args(lut=0)
    with pytest.raises(infer.EnvelopeError, match=who + ".*in_channels"):
        args(features_to_consider=["freq", "mod_order"])
    renamed = [("hops" if n == "num_spans" else n) for n in TG.LP_FEAT]
    with pytest.raises(infer.EnvelopeError, match=who + ".*'num_spans'"):
        args(status=TG.DeviceStatus(st.data, st.target, st.freq, renamed, st.metric))
    wide = TG.DeviceStatus(torch.zeros(1, 10, 1, 1025, dtype=torch.float64), st.target[:1], torch.zeros(1025, dtype=torch.float64),
                           st.lp_feat, st.metric)
    with pytest.raises(infer.EnvelopeError, match=who + ": at most 1024 frequency slots"):
        args(status=wide)
    # the call: chunk is keyword-only, there is no release=
    params = inspect.signature(infer.LightpathPredictor.retest).parameters
    assert list(params) == ["self", "status", "samples", "conns", "features_to_consider", "freq_threshold", "max_lightpaths", "chunk"]
    assert params["chunk"].kind is inspect.Parameter.KEYWORD_ONLY and params["max_lightpaths"].default == 256
    assert infer.Retest._fields == ("out", "conn", "n", "count")


def test_the_status_bit_is_new_and_named():
    taken = [infer.LP_STATUS_BAD_CONN, infer.LP_STATUS_TOO_MANY, infer.LP_STATUS_BAD_SAMPLE, infer.LP_PLACE_BAD_CELL,
             infer.LP_PLACE_OCCUPIED, infer.LP_PLACE_CONN_TAKEN, infer.LP_PLACE_NOT_LUT, infer.LP_PLACE_NO_SUCH_CONN,
             infer.LP_PLACE_BAD_RELEASE, 1, 2, 4]
    bit = infer.LP_RETEST_NO_SUCH_CONN
    assert bit == 4096 and bit not in taken and all(bit & t == 0 for t in taken)
    P = infer.LightpathPredictor
    assert P._RETEST_CAUSES == infer._RETEST_CAUSES == ((4096, "retest: a named conn_id is no lightpath of the sample"),)
    every = P._CAUSES + P._PLACE_CAUSES + P._RELEASE_CAUSES + P._RETEST_CAUSES
    assert len({b for b, _ in every}) == len(every) and "retest" in P._FLAGS[1]
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    assert "#define QOT_LP_RETEST_NO_SUCH_CONN 4096 " in hdr and "#define QOT_LP_RETEST_MAX_CHUNK 32 " in hdr


# ------------------------------------------------------------------ the layers agree
def test_entry_is_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    name = "qot_lightpath_infer_retest"
    assert f"int {name}(" in hdr and name in _lib.SIGNATURES
    status_sig, sig = _lib.SIGNATURES["qot_lightpath_infer_status"], _lib.SIGNATURES[name]
    assert sig[0] == status_sig[0]
    # the status entry's arguments up to freq_threshold, then conns, conn, n, max_lightpaths, chunk, the stream
    assert sig[1][:len(status_sig[1]) - 1] == status_sig[1][:-1] and len(sig[1]) == len(status_sig[1]) + 5
    assert sig[1][-6:] == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    csrc = os.path.join(ROOT, "gnn_qot_estimation_amd", "csrc")
    assert " infer_lightpath_retest.hip " in open(os.path.join(csrc, "Makefile")).read()
    assert hasattr(_lib.load(), name)
    # the rescan of the slotted lightpaths is stated once, in the header, and both kernels call it
    shared = open(os.path.join(csrc, "infer_lightpath_status_dev.hpp")).read()
    assert shared.count("void lp_mark_slotted(") == 1
    for f in ("infer_lightpath_place_impact.hip", "infer_lightpath_retest.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "infer_lightpath_status_dev.hpp"' in src and src.count("lp_mark_slotted(d, st, LQ, ") == 1, f
        assert "void lp_mark_slotted(" not in src and "__ballot(slot" not in src and "lp_mark_slots(d, " not in src, f
    src = open(os.path.join(csrc, "infer_lightpath_retest.hip")).read()
    for used in ("discover(", "lp_stage_marked(", "sg_feature(", "lp_row<false, LpStaged>("):
        assert used in src, used
    assert hasattr(TG, "retest_neighbourhood") and hasattr(infer.LightpathPredictor, "retest")


def test_entry_answers_the_envelope_before_any_launch():
    """Sizes and the envelope are answered without a pointer being looked at; G == 0 is QOT_OK without a launch."""
    lib = _lib.load()

    def rc(G=0, S=4, P=10, L=4, Q=70, F=5, C=32, O=3, heads=4, lut=1, rows=(0, 7, 8, 9), ncol=5, thr=0.05, N=0, M=256, chunk=32):
        none = [None] * 6
        return lib.qot_lightpath_infer_retest(*none, 0, N, 0, G, None, None, None, None, 0.2, None, None, None, None, 1e-5,
                                              None, None, None, None, 0.01, None, None, F, C, O, heads, lut, None, None, None,
                                              None, S, P, L, Q, *rows, None, ncol, thr, None, None, None, M, chunk, None)
    OK, UNSUPPORTED, BADARG = 0, -1, -2                                       # include/qot_gnn.h: QOT_OK, QOT_ERR_*
    assert rc() == OK and rc(M=1) == OK and rc(M=7, chunk=1) == OK and rc(chunk=5) == OK and rc(M=3, chunk=32) == OK
    codes = {name: rc(**kw) for name, kw in {
        "a batch beside the status": dict(N=3), "G < 0": dict(G=-1), "P < 1": dict(P=0), "Q < 1": dict(Q=0),
        "ncol != F": dict(ncol=4), "a row outside P": dict(rows=(0, 7, 8, 10)), "threshold 0": dict(thr=0.0),
        "threshold nan": dict(thr=float("nan")), "no pointers with G > 0": dict(G=2),
        "max_lightpaths 0": dict(M=0), "max_lightpaths 257": dict(M=257), "max_lightpaths < 0": dict(M=-1),
        "chunk 0": dict(chunk=0), "chunk 33": dict(chunk=33), "chunk < 0": dict(chunk=-1)}.items()}
    assert all(c == BADARG for c in codes.values()), codes
    outside = {name: rc(**kw) for name, kw in {
        "F": dict(F=17, ncol=17), "C": dict(C=257), "O": dict(O=9), "heads": dict(heads=2), "lut": dict(lut=5),
        "Q above the cap": dict(Q=1025), "L * Q": dict(L=1 << 22, Q=1024), "the grid": dict(G=(1 << 31) - 1, M=256, chunk=1)}.items()}
    assert all(c == UNSUPPORTED for c in outside.values()), outside
