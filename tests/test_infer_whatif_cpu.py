"""CPU-side checks of the what-if path (``csrc/infer_whatif.hip``, ``TopologicalPredictor.what_if``,
``infer.materialise_what_if``): the entry points are declared, bound and exported; ``materialise_what_if`` -- the definition
the GPU tests compare against -- builds, on CPU tensors, the graphs written out by hand in ``infer_whatif_cases``; a
materialised no-edit candidate is the base graph to the fp64 oracle; every argument refusal comes without a device; the
edge cap is the eval kernel's; the C entry's return codes before any launch."""
import ctypes
import os
import re

import pytest
import torch

import gnn_qot_estimation_amd as q
import infer_whatif_cases as WC
from gnn_qot_estimation_amd import _lib, infer
from helpers import INFER_COMMON_REFUSALS, infer_common_args, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qot_topological_infer_whatif", "qot_topological_infer_whatif_supported", "qot_topological_infer_whatif_max_edges")


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "qot_gnn.h")).read()
    declared = set(re.findall(r"\b(qot_[a-z0-9_]+)\s*\(", hdr))
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(_lib.SIGNATURES[name][1]) == decl.count(",") + 1, name
    # everything qot_topological_infer takes, then add_edge_index, add_edge_attr, add_ptr, A, drop, drop_ptr, R, graph, K,
    # max_add; the stream comes last
    ev, wi = _lib.SIGNATURES["qot_topological_infer"][1], _lib.SIGNATURES["qot_topological_infer_whatif"][1]
    P, I64, INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert wi[:len(ev) - 1] == ev[:-1] and wi[-1] is P
    assert wi[len(ev) - 1:-1] == [P, P, P, I64, P, P, I64, P, I64, INT]
    assert hasattr(q.TopologicalPredictor, "what_if")
    assert infer.WHAT_IF_MAX_DROP == 32 and callable(infer.materialise_what_if) and callable(infer.what_if_edge_cap)
    assert "infer_whatif.hip" in open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()


@pytest.mark.parametrize("n,H,D", [(75, 16, 4), (100, 64, 4), (128, 64, 4), (128, 32, 1), (2, 16, 2), (7, 32, 3)])
def test_edge_cap_is_the_eval_cap(n, H, D):
    lib = _lib.load()
    cap = infer.what_if_edge_cap(n, H, D)
    assert cap == infer.edge_cap(n, H, D) == lib.qot_topological_infer_whatif_max_edges(n, H, D) > 0
    assert lib.qot_topological_infer_whatif_supported(n, cap, H, D, 3) == 1
    assert lib.qot_topological_infer_whatif_supported(n, cap + 1, H, D, 3) == 0
    assert infer.what_if_edge_cap(129, H, D) == -1 and infer.what_if_edge_cap(n, 48, D) == -1


# ------------------------------------------------------------------ materialise_what_if: the definition
@pytest.mark.parametrize("D", [1, 4])
def test_materialise_builds_the_hand_written_graphs(D):
    w = WC.build(D)
    a, kw = WC.args(w)
    got = infer.materialise_what_if(*a, **kw)
    K = len(w.edits)
    assert K == 22 and got.num_graphs == K
    ptr, eptr = got.ptr.tolist(), got.edge_ptr.tolist()
    assert len(ptr) == len(eptr) == K + 1 and ptr[0] == eptr[0] == 0
    assert got.edge_index.dtype == torch.int64 and got.edge_attr.dtype == w.data.edge_attr.dtype
    assert got.x is None and got.num_nodes == ptr[-1] == got.node_ids.shape[0] == got.batch.shape[0]
    assert got.edge_index.shape[1] == eptr[-1] == got.edge_attr.shape[0]
    for k, (c, (n, edges, attr)) in enumerate(zip(w.edits, w.want)):
        assert ptr[k + 1] - ptr[k] == n == (WC.A_N, WC.B_N)[c.graph], c
        assert torch.equal(got.node_ids[ptr[k]:ptr[k + 1]], torch.arange(n)), c
        assert bool((got.batch[ptr[k]:ptr[k + 1]] == k).all()), c
        local = (got.edge_index[:, eptr[k]:eptr[k + 1]] - ptr[k]).t().tolist()      # renumbered to the candidate's block
        assert [tuple(e) for e in local] == [tuple(e) for e in edges], c
        if c.graph == 0:
            assert [tuple(e) for e in local] == WC.A_WANT[c.name], c                # ... and the list written by hand
        assert torch.equal(got.edge_attr[eptr[k]:eptr[k + 1]], attr), c
    assert got.graph_sizes == (WC.B_N, max(len(e) for _, e, _ in w.want))
    # the base batch was only read
    fresh = WC.base_batch(D)
    assert torch.equal(w.data.edge_index, fresh.edge_index) and torch.equal(w.data.edge_attr, fresh.edge_attr)


def test_materialise_takes_tensors_for_the_pointers_and_a_single_graph_without_graph():
    w = WC.build(4)
    a, kw = WC.args(w)
    want = infer.materialise_what_if(*a, **kw)
    got = infer.materialise_what_if(*a[:3], torch.tensor(w.add_ptr), drop=w.drop, drop_ptr=torch.tensor(w.drop_ptr),
                                    graph=w.graph)
    assert torch.equal(got.edge_index, want.edge_index) and torch.equal(got.edge_ptr, want.edge_ptr)
    # B == 1: graph=None means graph 0; no removals: drop / drop_ptr left out; an empty candidate list
    one = q.Batch.from_data_list([q.Data(edge_index=torch.tensor(WC.A_EDGES).t().contiguous(),
                                         edge_attr=torch.ones(len(WC.A_EDGES), 2), node_ids=torch.arange(WC.A_N),
                                         num_nodes=WC.A_N)])
    got = infer.materialise_what_if(one, torch.tensor([[2, 0], [5, 3]]), torch.zeros(2, 2), [0, 1, 1, 2])
    assert got.num_graphs == 3 and got.edge_ptr.tolist() == [0, 13, 25, 38] and got.ptr.tolist() == [0, 7, 14, 21]
    assert got.edge_index[:, 12].tolist() == [2, 5] and got.edge_index[:, 37].tolist() == [14, 17]
    none = infer.materialise_what_if(one, torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 2), [0])
    assert none.num_graphs == 0 and none.num_nodes == 0 and none.edge_index.shape == (2, 0)


def test_materialise_refuses_what_the_kernel_flags():
    w = WC.build(4, WC.edits()[:4])
    a, kw = WC.args(w)
    for bad, msg in ((dict(graph=torch.tensor([0, 1, 2, 1])), "graph must lie in"),
                     (dict(drop=torch.tensor([len(WC.A_EDGES)]), drop_ptr=[0, 1, 1, 1, 1]), "drop position"),
                     (dict(drop=torch.tensor([-1]), drop_ptr=[0, 0, 1, 1, 1]), "drop position")):
        with pytest.raises(ValueError, match=msg):
            infer.materialise_what_if(*a, **{**kw, **bad})
    with pytest.raises(ValueError, match="endpoint outside"):      # candidate 1 aims at graph B; node 3 belongs to graph A
        infer.materialise_what_if(a[0], torch.tensor([[WC.A_N + 2], [3]]), a[2][:1], [0, 0, 1, 1, 1], graph=w.graph)


def test_a_materialised_no_edit_candidate_is_the_base_graph_to_the_oracle():
    ref, _ = WC.models(None, 16)
    data = WC.base_batch(4)
    data.edge_attr = data.edge_attr.double()
    g = torch.tensor([1, 0, 1])
    mat = infer.materialise_what_if(data, torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 4), [0, 0, 0, 0], graph=g)
    with torch.no_grad():
        base, got = ref(data), ref(mat)
    # fp64, the same sums per graph (at most the order of a scatter differs): far below 1e-12
    e = rel_err(got, base[g])
    print(f"no-edit candidates vs the base graphs, fp64 oracle: {e:.3e}")
    assert got.shape == (3, 3) and e <= 1e-12, e


# ------------------------------------------------------------------ refusals without a device
def _ok(A=2, K=2, D=4):
    return dict(edge_dim=D, add_edge_index=torch.zeros(2, A, dtype=torch.long), add_edge_attr=torch.zeros(A, D),
                add_ptr=[0] + [A] * K)


def test_argument_checks_need_no_device():
    w = infer.what_if_args(**_ok(), num_graphs=1)
    assert (w.K, w.A, w.R, w.add_ptr.tolist(), w.drop_ptr, w.max_add) == (2, 2, 0, [0, 2, 2], None, 2)
    w = infer.what_if_args(**_ok(), drop=torch.tensor([3, 1, 3]), drop_ptr=torch.tensor([0, 3, 3]), graph=torch.tensor([1, 0]))
    assert (w.R, w.drop_ptr.tolist()) == (3, [0, 3, 3]) and w.drop_ptr.dtype == torch.int64 and not w.drop_ptr.is_cuda
    assert infer.what_if_args(**_ok(A=0, K=0)).K == 0
    refusals = [
        (dict(add_ptr=[0, 1]), "add_ptr must be non-decreasing from 0 to 2"),
        (dict(add_ptr=[1, 2]), "add_ptr must be non-decreasing from 0 to 2"),
        (dict(add_ptr=[0, 2, 1, 2]), "add_ptr must be non-decreasing"),
        (dict(add_ptr=torch.tensor([0, 3])), "add_ptr must be non-decreasing"),
        (dict(add_ptr=[]), "add_ptr must be a non-empty"),
        (dict(add_ptr=[0.0, 2.0]), "add_ptr must be a non-empty 1-d sequence of integers"),
        (dict(add_edge_attr=torch.zeros(2, 3)), r"add_edge_attr must be \[2, 4\]"),
        (dict(add_edge_attr=torch.zeros(3, 4)), r"add_edge_attr must be \[2, 4\]"),
        (dict(add_edge_attr=None), r"add_edge_attr must be \[2, 4\]"),
        (dict(add_edge_index=torch.zeros(3, 2, dtype=torch.long)), r"add_edge_index must be an integer tensor \[2, A\]"),
        (dict(add_edge_index=torch.zeros(2, 2)), "add_edge_index must be an integer tensor"),
        (dict(drop=torch.tensor([1])), "drop and drop_ptr must be given together"),
        (dict(drop_ptr=[0, 0, 0]), "drop and drop_ptr must be given together"),
        (dict(drop=torch.tensor([1, 2]), drop_ptr=[0, 1, 1]), "drop_ptr must be non-decreasing from 0 to 2"),
        (dict(drop=torch.tensor([1, 2]), drop_ptr=[0, 2]), "add_ptr names 2 candidates, drop_ptr 1"),
        (dict(drop=torch.tensor([1.0]), drop_ptr=[0, 1, 1]), "drop must be a 1-d integer tensor"),
        (dict(drop=torch.arange(33), drop_ptr=[0, 33, 33]), "a candidate removes 33 edges; at most WHAT_IF_MAX_DROP = 32"),
        (dict(num_graphs=2), "graph=None needs a base batch of exactly one graph, this one has 2"),
        (dict(num_graphs=0), "graph=None needs a base batch of exactly one graph"),
        (dict(graph=torch.tensor([0])), r"graph must be an integer tensor \[2\]"),
        (dict(graph=torch.tensor([0.0, 1.0])), "graph must be an integer tensor"),
    ]
    for kw, msg in refusals:
        with pytest.raises(ValueError, match="TopologicalPredictor.what_if: " + msg):
            infer.what_if_args(**{**_ok(), **kw})
    assert infer.what_if_args(**_ok(), drop=torch.arange(32), drop_ptr=[0, 32, 32], graph=torch.tensor([0, 0])).R == 32


def test_what_if_checks_its_arguments_before_the_model_and_the_batch():
    """As ``sample``: a predictor whose model sits on the CPU names a bad argument first, then the CPU model, and reads
    nothing of the batch for either."""
    pred = q.TopologicalPredictor.__new__(q.TopologicalPredictor)
    pred.model, pred._tables, pred._tag, pred._status = q.TopologicalGNN(14, 32, 3, 4), None, None, None
    ok = _ok()
    ok.pop("edge_dim")
    with pytest.raises(ValueError, match="add_ptr must be non-decreasing"):
        pred.what_if(None, ok["add_edge_index"], ok["add_edge_attr"], [0, 1, 3])
    with pytest.raises(ValueError, match=r"add_edge_attr must be \[2, 4\]"):
        pred.what_if(None, ok["add_edge_index"], torch.zeros(2, 1), ok["add_ptr"])
    with pytest.raises(ValueError, match="given together"):
        pred.what_if(None, **ok, drop=torch.tensor([0]))
    with pytest.raises(ValueError, match="graph=None needs a base batch of exactly one graph, this one has 2"):
        pred.what_if(WC.base_batch(4), **ok)
    with pytest.raises(ValueError, match="CPU"):
        pred.what_if(WC.base_batch(4), **ok, graph=torch.tensor([0, 1]))
    assert pred.model.training and pred._tables is None


# ------------------------------------------------------------------ the C entry before any launch
def _c_call(A=4, R=0, K=2, max_add=2, add=1, add_ptr=1, drop=None, drop_ptr=None, graph=1, **kw):
    p = lambda v: ctypes.c_void_p(v)                         # never dereferenced: every call here is answered first
    return _lib.load().qot_topological_infer_whatif(*infer_common_args(**kw), p(add), p(add), p(add_ptr), A, p(drop),
                                                    p(drop_ptr), R, p(graph), K, max_add, None)


# with K = 2 candidates an empty batch is a size that disagrees, not an empty launch
_COMMON = [(kw, code) for kw, code in INFER_COMMON_REFUSALS if kw.get("B", 1) != 0 or code != 0]


@pytest.mark.parametrize("kw,code", _COMMON + [
    (dict(K=0), 0), (dict(K=0, B=0), 0), (dict(K=0, A=0, max_add=0, add=None, add_ptr=None, graph=None, B=3), 0),
    (dict(H=48), -1), (dict(H=48, K=0), -1),                 # the envelope before the empty candidate list
    # sizes that disagree
    (dict(A=-1), -2), (dict(R=-1), -2), (dict(K=-1), -2), (dict(max_add=-1), -2), (dict(max_add=5), -2),
    (dict(R=3), -2), (dict(R=3, drop=1), -2), (dict(R=3, drop_ptr=1), -2),
    (dict(graph=None, B=2), -2), (dict(B=0), -2), (dict(B=0, out=None), -2),
    (dict(add_ptr=None), -2), (dict(add=None), -2),
])
def test_entry_point_return_codes_before_any_launch(kw, code):
    assert _c_call(**kw) == code


def test_the_envelope_is_asked_for_the_base_edges_and_the_additions_together():
    cap = infer.edge_cap(10, 16, 4)
    # (answered by the null `out` when the envelope holds: nothing is launched here)
    assert _c_call(max_e=cap, max_add=0, out=None) == -2 and _c_call(max_e=cap - 2, max_add=2, out=None) == -2
    assert _c_call(max_e=cap, max_add=1, out=None) == -1 and _c_call(max_e=cap - 2, max_add=3, out=None) == -1
