"""CPU-side checks of ``place(..., release=, release_ptr=)`` of both predictors (``csrc/infer_lightpath_place_release.hip``,
``csrc/infer_topological_place_release.hip``): the host statements ``to_graph.place_lightpath`` /
``placement_neighbourhood`` / ``placement_links`` with ``release=`` against the host builders on the numpy-edited sample
(``release_cases.edit``); ``infer.materialise_placement(release=)`` against that edit; the survivor-order argument the
kernels rest on, checked explicitly; every refusal that needs no device, with its message; the status bits against the
header; the two entries declared, bound, built and answering their envelopes before any launch."""
import os

import numpy as np
import pytest
import torch

import place_cases as PC
import release_cases as RC
import status_topo_cases as TK
from gnn_qot_estimation_amd import _lib, infer, to_graph as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FI = RC.FI
SEEDS = (0, 1, 2)


def _lp_candidates():
    for seed in SEEDS:
        b = RC.lp_batch(seed)
        for k, s in enumerate(b.samples):
            yield b.ns.data[s], b.ns.freq, b.values[k], RC.candidate_cells(b, k), RC.released(b, k)
    b = RC.lp_batch(1, True)
    for k, s in enumerate(b.samples):
        yield b.ns.data[s], b.ns.freq, b.values[k], RC.candidate_cells(b, k), RC.released(b, k)
    for make in RC.LP_HAND.values():
        c = make()
        yield c.ns.data[0], c.ns.freq, c.values, c.cells, c.release


def _topo_candidates():
    for seed in (0, 1):
        b, _ = RC.topo_batch(seed)
        for k, s in enumerate(b.samples):
            yield b.ns.data[s], b.values[k], RC.candidate_cells(b, k), RC.released(b, k)
    for make in RC.TOPO_HAND.values():
        c = make()
        yield c.ns.data[0], c.values, c.cells, c.release


# ------------------------------------------------------------------ the builders' cover
def test_the_seeds_meet_their_cover():
    for seed in SEEDS:
        b = RC.lp_batch(seed)                                                  # (asserts the conditions on the inputs)
        cover = RC.lp_cover(b)
        assert len(b.samples) == 8 and b.ns.data.shape[2:] == (PC.L, PC.Q)
        assert 2 * sum(i for i, _ in cover) >= 8 and 3 * sum(r for _, r in cover) >= 8
    for seed in (0, 1):
        b, outcomes = RC.topo_batch(seed)
        assert all(outcomes.count(name) >= 2 for name in RC.TOPO_OUTCOMES)
        assert b.ns.data.shape[2:] == (6, 12) and max(b.release_ptr[k + 1] - b.release_ptr[k] for k in range(len(outcomes))) >= 2


# ------------------------------------------------------------------ the host statements against the edited sample
def test_place_lightpath_edits_as_numpy_does_and_numbers_the_node_as_the_builder():
    for sample, freq, v, cells, rel in _lp_candidates():
        edited, node = TG.place_lightpath(sample, v, cells, FI, release=rel)
        assert np.array_equal(edited, RC.edit(sample, v, cells, rel))
        G = TG.create_lightpath_graph(0, PC.FEATS, PC.SK.status(edited[None], freq))
        assert list(G.nodes)[node] == f"lightpath_{int(v[FI['conn_id']])}"


@pytest.mark.parametrize("thr", PC.THRESHOLDS)
def test_placement_neighbourhood_is_lut_neighbourhood_of_the_edited_sample(thr):
    checked = 0
    for sample, freq, v, cells, rel in _lp_candidates():
        got = TG.placement_neighbourhood(sample, freq, FI, cells, thr, release=rel)
        edited = RC.edit(sample, v, cells, rel)
        count, conn, want = TG.lut_neighbourhood(edited, freq, FI, thr)
        if conn != int(v[FI["conn_id"]]):                                      # a flagged survivor is seen first: hide it
            hidden = edited.copy()
            flagged = (edited[FI["osnr"]] == -1) & (edited[FI["conn_id"]].astype(np.int64) != int(v[FI["conn_id"]]))
            hidden[FI["osnr"]][flagged] = 20.0
            count, conn, want = TG.lut_neighbourhood(hidden, freq, FI, thr)
        assert conn == int(v[FI["conn_id"]]) and got == want, (got, want)
        assert not set(got) & set(rel)
        checked += bool(set(rel) & set(TG.placement_neighbourhood(sample, freq, FI, cells, thr)))
    assert thr != 0.12 or checked >= 8                                         # released interferers were there to strike


def test_hand_cases_name_their_interferers_and_counts():
    for name, make in RC.LP_HAND.items():
        c = make()
        assert TG.placement_neighbourhood(c.ns.data[0], c.ns.freq, FI, c.cells, c.thr, release=c.release) == c.interferers, name
        edited, _ = TG.place_lightpath(c.ns.data[0], c.values, c.cells, FI, release=c.release)
        assert TG.lut_neighbourhood(edited, c.ns.freq, FI, c.thr)[0] == c.count, name


def test_placement_links_are_topological_links_of_the_edited_sample():
    for sample, v, cells, rel in _topo_candidates():
        ei, conn, outcome = TG.placement_links(sample, v, cells, FI, release=rel)
        want_ei, want_conn = TG.topological_links(RC.edit(sample, v, cells, rel), FI)
        assert np.array_equal(ei, want_ei) and np.array_equal(conn, want_conn)
        assert outcome in ("new pair", "takes the pair", "loses the pair") and not set(rel) & (set(conn.tolist()) - {int(v[FI["conn_id"]])})
    for name, make in RC.TOPO_HAND.items():
        c = make()
        assert TG.placement_links(c.ns.data[0], c.values, c.cells, FI, release=c.release)[0].shape[1] == c.links, name
    c = RC.TOPO_HAND["still loses the pair to the survivor"]()
    assert TG.placement_links(c.ns.data[0], c.values, c.cells, FI, release=c.release)[2] == "loses the pair"
    c = RC.TOPO_HAND["reroute with the same conn_id onto its own old cell"]()
    assert TG.placement_links(c.ns.data[0], c.values, c.cells, FI, release=c.release)[2] == "takes the pair"


def test_release_defaults_leave_the_host_statements_as_they_were():
    b = PC.batch(0)
    for k, s in enumerate(b.samples):
        sample, cells = b.ns.data[s], PC.candidate_cells(b, k)
        assert TG.placement_neighbourhood(sample, b.ns.freq, FI, cells, 0.12) == \
            TG.placement_neighbourhood(sample, b.ns.freq, FI, cells, 0.12, release=[])
        a, b_ = TG.place_lightpath(sample, b.values[k], cells, FI), TG.place_lightpath(sample, b.values[k], cells, FI, ())
        assert np.array_equal(a[0], b_[0]) and a[1] == b_[1]


def test_unknown_and_illegal_releases_raise_on_the_host():
    c = RC.LP_HAND["reroute with the same conn_id onto its own old cells"]()
    sample = c.ns.data[0]
    for call in (lambda r: TG.place_lightpath(sample, c.values, c.cells, FI, release=r),
                 lambda r: TG.placement_neighbourhood(sample, c.ns.freq, FI, c.cells, c.thr, release=r),
                 lambda r: TG.placement_links(sample, c.values, c.cells, FI, release=r)):
        with pytest.raises(ValueError, match="released conn_id 6 is no lightpath of the sample"):
            call([5, 6])
    with pytest.raises(ValueError, match="occupied"):                          # its own cells, nothing released
        TG.place_lightpath(sample, c.values, c.cells, FI)
    with pytest.raises(ValueError, match="conn_id 5 is a lightpath of the sample already"):
        TG.place_lightpath(sample, c.values, [[0], [0]], FI, release=[8])


# ------------------------------------------------------------------ the argument the kernels rest on
def test_survivors_keep_their_first_channel_and_their_relative_order():
    """Releasing zeroes whole channels and the candidate fills channels that are free afterwards: the lightpaths of the
    edited sample other than the candidate are the unedited sample's survivors, with the same first channels, in the
    same order -- so the unedited table without the gone rows is the edited sample's table without the candidate."""
    seen = 0
    for sample, freq, v, cells, rel in _lp_candidates():
        mine = int(v[FI["conn_id"]])
        want = [(c, first) for c, first in RC.lightpaths(sample) if c not in rel]
        got = [(c, first) for c, first in RC.lightpaths(RC.edit(sample, v, cells, rel)) if c != mine]
        assert got == want
        # ... and with it each survivor's feature vector
        assert all(np.array_equal(sample[:, l, q], RC.edit(sample, v, cells, rel)[:, l, q]) for _, (l, q) in want)
        seen += len(rel) > 0
    assert seen >= 20
    for sample, v, cells, rel in _topo_candidates():
        mine = int(v[FI["conn_id"]])
        assert [x for x in RC.lightpaths(RC.edit(sample, v, cells, rel)) if x[0] != mine] == \
            [x for x in RC.lightpaths(sample) if x[0] not in rel]


# ------------------------------------------------------------------ materialise_placement(release=)
def _cpu(b):
    ns = b.ns
    st = TG.DeviceStatus(torch.from_numpy(ns.data), torch.zeros(ns.data.shape[0], len(ns.metric), dtype=torch.float64),
                         torch.from_numpy(np.asarray(ns.freq, dtype=np.float64)), ns.lp_feat, ns.metric)
    return (st, list(b.samples), torch.from_numpy(b.values), torch.from_numpy(np.ascontiguousarray(b.cells, dtype=np.int64)),
            list(b.cell_ptr)), dict(release=torch.from_numpy(b.release), release_ptr=list(b.release_ptr))


def test_materialise_placement_is_the_numpy_edit():
    batches = [RC.lp_batch(s) for s in SEEDS] + [RC.topo_batch(0)[0]] + [RC.as_batch(m()) for m in RC.LP_HAND.values()] + \
        [RC.topo_as_batch(m()) for m in RC.TOPO_HAND.values()]
    for b in batches:
        args, kw = _cpu(b)
        before = args[0].data.clone()
        edited = infer.materialise_placement(*args, **kw)
        want = np.stack([RC.edited(b, k) for k in range(len(b.samples))])
        assert np.array_equal(edited.data.numpy(), want)
        assert torch.equal(args[0].data, before)
        again = infer.materialise_placement(*args, release=kw["release"], release_ptr=torch.tensor(kw["release_ptr"]))
        assert torch.equal(again.data, edited.data)
    args, kw = _cpu(RC.lp_batch(0))
    plain = infer.materialise_placement(*args)
    none = infer.materialise_placement(*args, release=torch.zeros(0, dtype=torch.int64), release_ptr=[0] * 9)
    assert torch.equal(plain.data, none.data) and not torch.equal(plain.data, infer.materialise_placement(*args, **kw).data)


def test_materialise_placement_follows_the_channel_rule():
    """A channel with conn_id 0 and another value != 0 is an occupied channel of conn 0; an all-zero channel is nobody's;
    a NaN conn_id matches nothing."""
    data, freq = PC.grid()
    data[0, FI["freq"], 0, 3] = 193.15                                         # conn 0, occupied
    data[0, :, 1, 4] = PC.SK.vec(9, fval=freq[4])
    data[0, :, 1, 5] = PC.SK.vec(0.7, fval=freq[5])                            # truncates to conn 0
    data[0, :, 2, 6] = PC.SK.vec(np.nan, fval=freq[6])
    c = RC.Case(PC.SK.status(data, freq), PC.SK.vec(5, fval=freq[8], quality=PC.SK.UNDER_TEST), np.array([[3], [8]]), [0], 0.1, [], 1)
    args, kw = _cpu(RC.as_batch(c))
    out = infer.materialise_placement(*args, **kw).data[0].numpy()
    assert not out[:, 0, 3].any() and not out[:, 1, 5].any() and out[:, 1, 4].any() and out[:, 3, 8].any()
    assert np.isnan(out[FI["conn_id"], 2, 6]) and int((out != 0).any(0).sum()) == 3


# ------------------------------------------------------------------ refusals without a device
def test_host_refusals_with_their_messages():
    b = RC.lp_batch(0)
    (st, samples, values, cells, ptr), kw = _cpu(b)
    K, R = len(samples), int(b.release.shape[0])
    rel, rptr = kw["release"], kw["release_ptr"]
    assert infer.place_release_args(st, K, None, None) is None
    ra = infer.place_release_args(st, K, rel, rptr, "x")
    assert ra.R == R and ra.release is rel and ra.release_ptr.tolist() == rptr and ra.release_ptr.dtype == torch.int64
    dev_ptr = torch.tensor(rptr)
    assert infer.place_release_args(st, K, rel, dev_ptr).release_ptr is dev_ptr
    assert infer.place_release_args(st, K, rel[:0], [0] * (K + 1)).R == 0
    assert infer.PLACE_MAX_RELEASE == 32
    bad = {
        "release and release_ptr go together, got only release$": [dict(release_ptr=None)],
        "release and release_ptr go together, got only release_ptr": [dict(release=None)],
        "release must be a 1-d int64 tensor of conn_id values": [dict(release=b.release), dict(release=rel.int()),
                                                                 dict(release=rel[None]), dict(release=rel.double()),
                                                                 dict(release=list(rptr))],
        f"release_ptr must be a sequence or a 1-d int64 tensor of K \\+ 1 = {K + 1} offsets": [
            dict(release_ptr=dev_ptr.int()), dict(release_ptr=dev_ptr[:-1]), dict(release_ptr=dev_ptr[None])],
        f"release_ptr must hold K \\+ 1 = {K + 1} offsets into release, got {K}": [dict(release_ptr=rptr[:-1])],
        f"release_ptr must be non-decreasing from 0 to R = {R}": [
            dict(release_ptr=[1] + rptr[1:]), dict(release_ptr=rptr[:-1] + [R + 1]), dict(release_ptr=rptr[:-1] + [R - 1]),
            dict(release_ptr=[0, rptr[2], rptr[1]] + rptr[3:])],
    }
    for who, call in (("LightpathPredictor.place", lambda **k: infer.place_release_args(st, K, k["release"], k["release_ptr"],
                                                                                        "LightpathPredictor.place")),
                      ("materialise_placement", lambda **k: infer.materialise_placement(st, samples, values, cells, ptr, **k))):
        for msg, cases in bad.items():
            for change in cases:
                with pytest.raises(ValueError, match=f"{who}: {msg}"):
                    call(**dict(kw, **change))
    many = torch.arange(40)
    with pytest.raises(ValueError, match="x: candidate 1 releases 33 lightpaths, at most 32"):
        infer.place_release_args(st, 3, many, [0, 7, 40, 40], "x")
    assert infer.place_release_args(st, 3, many, [0, 8, 40, 40], "x").R == 40                  # 32 are allowed
    with pytest.raises(ValueError, match="at most 32"):                        # a tensor on the host is checked as a list is
        infer.place_release_args(st, 3, many, torch.tensor([0, 7, 40, 40]), "x")
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="release is on cuda:0, the status chunk on cpu"):
            infer.place_release_args(st, K, rel.cuda(), rptr)


def test_the_keywords_are_keyword_only_and_last():
    import inspect
    for cls in (infer.LightpathPredictor, infer.TopologicalPredictor):
        params = list(inspect.signature(cls.place).parameters.values())
        assert [p.name for p in params[-2:]] == ["release", "release_ptr"]
        assert all(p.kind is p.KEYWORD_ONLY and p.default is None for p in params[-2:])
        assert all(p.kind is p.POSITIONAL_OR_KEYWORD for p in params[:-2])
    assert list(inspect.signature(infer.materialise_placement).parameters)[-2:] == ["release", "release_ptr"]
    for fn in (TG.place_lightpath, TG.placement_neighbourhood, TG.placement_links):
        assert inspect.signature(fn).parameters["release"].default == ()


def test_check_model_refusals_still_come_first():
    import gnn_qot_estimation_amd as q
    pred = object.__new__(infer.TopologicalPredictor)
    pred.model = q.TopologicalGNN(75, 16, 3, 4, dropout_p=0.0)
    with pytest.raises(ValueError, match="on the CPU"):
        pred.place(TK.chunk(), 0, None, None, None, release=None, release_ptr=[0])


# ------------------------------------------------------------------ the status bits, the entries
def test_status_bits_header_and_constants_agree():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    assert "#define QOT_PLACE_MAX_RELEASE 32 " in hdr
    for model, cls, older in (("LP", infer.LightpathPredictor, 1023), ("TOPO", infer.TopologicalPredictor, 1023)):
        bits = (getattr(infer, f"{model}_PLACE_NO_SUCH_CONN"), getattr(infer, f"{model}_PLACE_BAD_RELEASE"))
        assert bits == (1024, 2048) and all(b & older == 0 for b in bits)
        assert f"#define QOT_{model}_PLACE_NO_SUCH_CONN 1024 " in hdr and f"#define QOT_{model}_PLACE_BAD_RELEASE 2048 " in hdr
        assert [b for b, _ in cls._RELEASE_CAUSES] == list(bits) and all(t.startswith("place: ") for _, t in cls._RELEASE_CAUSES)
        assert not {b for b, _ in cls._RELEASE_CAUSES} & {b for b, _ in tuple(cls._CAUSES) + tuple(cls._PLACE_CAUSES)}
        pred = cls.__new__(cls)
        infer._DeviceState.__init__(pred)
        for bit, words in zip(bits, ("released conn_id is no lightpath of the sample", "release_ptr slice that is descending")):
            pred._status = torch.tensor([bit], dtype=torch.int32)
            with pytest.raises(_lib.QotError, match=rf"status {bit}\).*{words}"):
                pred.check_status()
        pred._status = torch.tensor([bits[0] | cls._PLACE_CAUSES[1][0]], dtype=torch.int32)
        with pytest.raises(_lib.QotError, match="channel is occupied.*released conn_id"):
            pred.check_status()
        pred.check_status()


def test_entries_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    csrc = os.path.join(ROOT, "gnn_qot_estimation_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    lib = _lib.load()
    for model, dev_hpp in (("lightpath", "infer_lightpath_status_dev.hpp"), ("topological", "infer_topological_status_dev.hpp")):
        name = f"qot_{model}_infer_place_release"
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name)
        place_sig, rel_sig = _lib.SIGNATURES[f"qot_{model}_infer_place"], _lib.SIGNATURES[name]
        # the place entry's arguments up to the cell count, then release, release_ptr, R, the stream
        assert rel_sig[0] == place_sig[0] and rel_sig[1][:len(place_sig[1]) - 1] == place_sig[1][:-1]
        assert rel_sig[1][len(place_sig[1]) - 1:] == [_lib._p, _lib._p, _lib._i64, _lib._p]
        assert f" infer_{model}_place_release.hip " in mk
        src = open(os.path.join(csrc, f"infer_{model}_place_release.hip")).read()
        # both take the shared argument structs; the lightpath kernel runs the sample's scan and the release through the
        # shared candidate scan over status_scan_dev.hpp's LDS struct, the topological kernel keeps its own statement of
        # steps 1 to 3 (its header says why)
        assert f'#include "{dev_hpp}"' in src and "const sg::PlaceArgs pl" in src and "const sg::ReleaseArgs rl" in src
        if model == "lightpath":
            assert "lp_place_scan<true>(" in src and "__shared__ sg::Release rs;" in src
            for piece in ("sg::discover(", "rel[", "found[", "gone_mask["):
                assert piece not in src, piece
        else:
            assert "sg::discover(" in src and "__shared__ int64_t rel[" in src
        for piece in ("void lp_mark_slots(", "int lp_stage_marked(", "int topo_winners(", "void topo_status_forward(",
                      "int lp_place_scan("):
            assert piece not in src                                             # the shared routines are used, not restated
    # the release rule of the shared scan is status_scan_dev.hpp's
    scan = open(os.path.join(csrc, "status_scan_dev.hpp")).read()
    for piece in ("struct PlaceArgs {", "struct ReleaseArgs {", "struct Release {", "int64_t rel[kMaxRelease];",
                  "uint8_t found[kMaxRelease];", "uint8_t gone[kCap];", "unsigned long long gone_mask[kWaves];",
                  "int release_slice(", "void release_load(", "bool release_match(", "int release_gone(",
                  "bool release_unmatched(", "bool release_freed("):
        assert scan.count(piece) == 1, piece
    lp_dev = open(os.path.join(csrc, "infer_lightpath_status_dev.hpp")).read()
    assert lp_dev.count("int lp_place_scan(") == 1 and "template <bool kRelease>" in lp_dev and "sg::discover(" in lp_dev
    for call in ("sg::release_slice(", "sg::release_load(", "sg::release_match(", "sg::release_gone(", "sg::release_unmatched(",
                 "sg::release_freed("):
        assert call in lp_dev, call
    # the lightpath place kernels reach discover() through the scan; the candidate structs of old are gone
    for f in ("infer_lightpath_place.hip", "infer_lightpath_place_impact.hip", "infer_lightpath_place_release.hip"):
        assert "sg::discover(" not in open(os.path.join(csrc, f)).read(), f
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(csrc, f)).read()
            for gone in ("LpPlaceReleaseArgs", "TopoPlaceReleaseArgs", "LpPlaceArgs", "TopoPlaceArgs"):
                assert gone not in text, (f, gone)


def test_entries_answer_their_envelopes_before_any_launch():
    lib = _lib.load()
    OK, UNSUPPORTED, BADARG = 0, -1, -2                                       # include/qot_gnn.h: QOT_OK, QOT_ERR_*

    def lp(K=0, S=4, P=10, L=4, Q=70, F=5, C=32, O=3, heads=4, lut=1, rows=(0, 7, 8, 9), ncol=5, thr=0.05, N=0, M=0, R=0):
        none = [None] * 6
        return lib.qot_lightpath_infer_place_release(*none, 0, N, 0, K, None, None, None, None, 0.2, None, None, None, None,
                                                     1e-5, None, None, None, None, 0.01, None, None, F, C, O, heads, lut, None,
                                                     None, None, None, S, P, L, Q, *rows, None, ncol, thr, None, None, None, M,
                                                     None, None, R, None)

    def topo(K=0, S=4, P=10, L=6, Q=12, H=64, D=4, O=3, N=75, E=0, n_max=75, max_e=512, V=75, rows=(0, 1, 2), ncol=4, M=0, R=0):
        return lib.qot_topological_infer_place_release(None, None, None, None, None, N, E, K, n_max, max_e, None, 4 * H, None,
                                                       128, None, V, None, None, None, None, None, None, None, None, None,
                                                       0.01, 0.01, None, H, D, O, None, None, None, None, S, P, L, Q, *rows,
                                                       None, ncol, None, None, None, M, None, None, R, None)
    for rc in (lp, topo):
        assert rc() == OK and rc(M=7, R=5) == OK
        codes = {name: rc(**kw) for name, kw in {"K < 0": dict(K=-1), "P < 1": dict(P=0), "Q < 1": dict(Q=0), "M < 0": dict(M=-1),
                                                 "R < 0": dict(R=-1), "no pointers with K > 0": dict(K=2, M=2, R=2),
                                                 "a row outside P": dict(rows=(0, 7, 8, 10) if rc is lp else (0, 1, 10))}.items()}
        assert all(c == BADARG for c in codes.values()), codes
        assert rc(Q=1025) == UNSUPPORTED and rc(O=9) == UNSUPPORTED
    assert lp(ncol=4) == BADARG and lp(thr=0.0) == BADARG and lp(N=3) == BADARG and lp(C=257) == UNSUPPORTED
    assert topo(N=74) == BADARG and topo(max_e=511) == BADARG and topo(H=48) == UNSUPPORTED
    for H in (16, 32, 64):                                                     # the whole envelope fits the LDS budget
        for D in (1, 2, 3, 4):
            assert topo(H=H, D=D, ncol=D) == OK, (H, D)
