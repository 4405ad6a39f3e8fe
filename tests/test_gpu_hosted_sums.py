"""Sums hosted by the grad-h launch (``qot_nnconv_gradh_host_roles``; csrc/nnconv_gradh64.hip: tail workgroups).

The hosted jobs are the same device bodies over the same partials in the same fixed order as in a ``qot_run_roles`` launch
of their own; only the launch that carries them changes.  So everything here is EQUALITY BIT FOR BIT: the NNConv backward
{adjoint, host-roles + grad-h, sum of grad-h's partials} against {adjoint, grad-h, ``qot_nnconv_bwd_finalize``}, hosted
``SUM_ROWS`` jobs against the same jobs through ``qot_run_roles``, a training step in the default schedule against
``QOT_NO_HOSTED_SUMS=1``, and a captured step against the eager one.  Every output buffer is NaN-filled before a call and
every call is made twice.  Shapes: the smallest at which the tile walk over ``n_main`` workgroups (no longer the whole grid)
or the tail's table lookup can go wrong."""
import os

import pytest
import torch

from gnn_qot_estimation_amd import _lib
from gnn_qot_estimation_amd import functional as QF
from gnn_qot_estimation_amd.graph import build_graph_index

pytestmark = pytest.mark.gpu

H = 64
P = _lib.ptr
SUM, SLAB, GHSUM = _lib.ROLE_SUM_ROWS, _lib.ROLE_NNCONV_SLAB_SUM64, _lib.ROLE_NNCONV_GRADH_SUM64


def _graph(case, gen):
    if case == "one_node":              # main grid 1
        return 1, torch.zeros(2, 1, dtype=torch.int64)
    if case == "two_tiles":             # a one-row second tile
        return 33, torch.randint(0, 33, (2, 120), generator=gen)
    if case == "no_edges":
        return 5, torch.zeros(2, 0, dtype=torch.int64)
    N = 36000                           # "carry": 1125 tiles, more than the two workgroups per CU of a 304-CU part (608)
    return N, torch.randint(0, N, (2, 3 * N), generator=gen)


def _pack(w2, b2, wroot, h, K):
    old = os.environ.get("QOT_NNCONV_F32_MFMA")
    os.environ["QOT_NNCONV_F32_MFMA"] = "0"              # nnconv_pack writes the planes only for the split form
    try:
        return QF.nnconv_pack(w2, b2, wroot, h, K)
    finally:
        if old is None:
            del os.environ["QOT_NNCONV_F32_MFMA"]
        else:
            os.environ["QOT_NNCONV_F32_MFMA"] = old


def _nan(*shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Case:
    """Inputs of one NNConv backward at H = 64 plus two arrays of partials for hosted SUM_ROWS jobs."""

    def __init__(self, name, D, dev):
        gen = torch.Generator().manual_seed(41)
        N, ei = _graph(name, gen)
        K, E = 2 * D, ei.shape[1]
        self.dev, self.D, self.K, self.N, self.E = dev, D, K, N, E
        self.graph = build_graph_index(ei.to(dev), N)
        r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(dev)
        self.x, self.g, self.ea = r(N, H), r(N, H), torch.rand(E, D, generator=gen).to(dev)
        self.w1, self.b1 = r(K, D, scale=0.5), r(K, scale=0.5)
        self.wp, self.wp_adj, self.bp, self.split = _pack(r(H * H, K, scale=1 / 16), r(H * H, scale=1 / 16), r(H, H, scale=1 / 8), H, K)
        self.bsplit = self.split[self.wp.numel():]           # the planes of Wk^T follow those of Wcat in each plane
        lib = _lib.load()
        self.ws = torch.empty(lib.qot_nnconv_adjoint_dw_workspace_floats(D), dtype=torch.float32, device=dev)
        self.wsh = torch.empty(lib.qot_nnconv_gradh_workspace_floats(D), dtype=torch.float32, device=dev)
        self.part_a, self.part_b = r(37, 1000), r(5, 7)      # float4 columns / a row length that is no multiple of 4
        self.gx = torch.empty(N, H, device=dev)

    def adjoint(self):
        self.ws.fill_(float("nan"))
        _lib.call("qot_nnconv_adjoint_dw", P(self.g), H, P(self.x), H, P(self.ea), P(self.w1), P(self.b1), P(self.graph.rowptr_t),
                  P(self.graph.col_t), P(self.graph.eid_t), P(self.graph.invdeg), P(self.wp_adj), P(self.gx),
                  P(_nan(1, dev=self.dev)), 2, P(self.ws), self.N, H, self.D)

    def gradh(self, gw1=None, gb1=None, fused=False):
        self.wsh.fill_(float("nan"))
        common = (P(self.g), H, P(self.x), H, P(self.ea), P(self.w1), P(self.b1), P(self.graph.rowptr), P(self.graph.col),
                  P(self.graph.eid), P(self.graph.invdeg))
        if fused:
            _lib.call("qot_nnconv_gradh_fused", *common, P(self.bp), P(gw1), P(gb1), P(self.wsh), self.N, H, self.D)
        else:
            _lib.call("qot_nnconv_gradh_split", *common, P(self.bsplit), self.split.numel() // 3, P(gw1), P(gb1), P(self.wsh),
                      self.N, H, self.D)

    def outputs(self):
        K, D = self.K, self.D
        return dict(gpar=_nan((K + 2) * H * H, dev=self.dev), gw1=_nan(K * D, dev=self.dev), gb1=_nan(K, dev=self.dev),
                    sum_a=_nan(1000, dev=self.dev), sum_b=_nan(7, dev=self.dev))

    def sum_roles(self, o):
        return [_lib.make_role(SUM, (self.part_a, o["sum_a"]), (37, 1000, 0)), _lib.make_role(SUM, (self.part_b, o["sum_b"]), (5, 7, 0))]

    def reference(self):
        o = self.outputs()
        self.adjoint()
        self.gradh()
        _lib.call("qot_nnconv_bwd_finalize", P(self.ws), P(self.wsh), P(o["gpar"]), P(o["gw1"]), P(o["gb1"]), self.N, H, self.D)
        _lib.run_roles(self.sum_roles(o))
        torch.cuda.synchronize()
        return {k: _bits(v) for k, v in o.items()}

    def hosted(self, fused=False):
        o = self.outputs()
        self.adjoint()
        _lib.host_roles([_lib.make_role(SLAB, (self.ws, None, o["gpar"]), (self.N, self.D))] + self.sum_roles(o))
        self.gradh(fused=fused)
        _lib.run_roles([_lib.make_role(GHSUM, (None, self.wsh, None, o["gw1"], o["gb1"]), (self.N, self.D))])
        torch.cuda.synchronize()
        return {k: _bits(v) for k, v in o.items()}


_CASES = {}


def _case(name, D, dev):
    """Inputs, the reference results and two hosted runs: computed once, shared, left unchanged."""
    if (name, D) not in _CASES:
        c = Case(name, D, dev)
        c.ref, c.h1, c.h2 = c.reference(), c.hosted(), c.hosted()
        _CASES[(name, D)] = c
    return _CASES[(name, D)]


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["one_node", "two_tiles", "no_edges", "carry"])
def test_hosted_backward_equals_the_finalize_launch_bitwise(cuda_device, name, D):
    c = _case(name, D, cuda_device)
    for k, ref in c.ref.items():
        assert not bool(torch.isnan(ref.view(torch.float32)).any()), (name, D, k)            # every entry written
        differ = [int((ref != h[k]).sum()) for h in (c.h1, c.h2)]
        print(name, D, k, "differing words (two hosted runs)", differ)
        assert differ == [0, 0], (name, D, k)
    if c.E > 0:
        assert bool(c.ref["gw1"].view(torch.float32).any()) and bool(c.ref["gpar"].view(torch.float32).any())


def test_the_fp32_form_hosts_too(cuda_device):
    """``qot_nnconv_gradh_fused`` at H = 64 (the fp32-MFMA kernel) carries the jobs as the split forms do: the hosted sums
    have the reference's bits (its gw1 / gb1 are another kernel's and are not compared)."""
    c = _case("two_tiles", 4, cuda_device)
    h = c.hosted(fused=True)
    for k in ("gpar", "sum_a", "sum_b"):
        assert torch.equal(h[k], c.ref[k]), k
    assert not bool(torch.isnan(h["gw1"].view(torch.float32)).any())


def test_hosted_jobs_are_taken_by_one_grad_h_call_only(cuda_device):
    c = _case("two_tiles", 4, cuda_device)
    o = c.outputs()
    _lib.host_roles(c.sum_roles(o))
    c.gradh()
    torch.cuda.synchronize()
    assert torch.equal(_bits(o["sum_a"]), c.ref["sum_a"]) and torch.equal(_bits(o["sum_b"]), c.ref["sum_b"])
    o["sum_a"].fill_(float("nan"))
    o["sum_b"].fill_(float("nan"))
    c.gradh()                                    # no new host-roles call: nothing is carried
    torch.cuda.synchronize()
    assert bool(torch.isnan(o["sum_a"]).all()) and bool(torch.isnan(o["sum_b"]).all())


def test_a_refused_host_roles_call_stores_nothing_and_launches_nothing(cuda_device):
    c = _case("two_tiles", 4, cuda_device)
    o = c.outputs()
    ok = c.sum_roles(o)
    heavy = _lib.make_role(_lib.ROLE_NNCONV_FINALIZE64, (c.ws, c.wsh, o["gpar"], o["gw1"], o["gb1"]), (c.N, c.D))
    null = _lib.make_role(SUM, (c.part_a, None), (37, 1000, 0))
    for bad in ([ok[0]] * (_lib.MAX_ROLES + 1), [ok[0], heavy], [ok[0], null],
                [ok[0], _lib.make_role(GHSUM, (None, c.wsh, None, o["gw1"], o["gb1"]), (c.N, c.D))]):
        with pytest.raises(_lib.QotError):
            _lib.host_roles(bad)
        c.gradh()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(v).all()) for v in o.values())


def test_a_job_that_reads_the_grad_h_workspace_is_refused_before_any_launch(cuda_device):
    c = _case("two_tiles", 4, cuda_device)
    out = _nan(4, dev=cuda_device)
    _lib.host_roles([_lib.make_role(SUM, (c.wsh, out), (2, 4, 0))])
    with pytest.raises(_lib.QotError):
        c.gradh()
    c.gradh()                                    # the refused call dropped the job
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_a_grad_h_call_that_cannot_host_runs_the_jobs_in_a_launch_of_their_own(cuda_device):
    """H = 32: the width-generic grad-h kernel has no tail; the hosted jobs run behind it, same bits."""
    c = _case("two_tiles", 4, cuda_device)
    dev, h, D, K, N = cuda_device, 32, 4, 8, c.N
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    _, _, bp, _ = QF.nnconv_pack(r(h * h, K) / 8, r(h * h) / 8, r(h, h) / 8, h, K)
    x, g = r(N, h), r(N, h)
    ws = torch.empty(max(_lib.load().qot_nnconv_gradh_workspace_floats(D), 1 << 16), dtype=torch.float32, device=dev)
    res = []
    for host in (False, True, True):
        o = c.outputs()
        if host:
            _lib.host_roles(c.sum_roles(o))
        _lib.call("qot_nnconv_gradh_fused", P(g), h, P(x), h, P(c.ea), P(c.w1), P(c.b1), P(c.graph.rowptr), P(c.graph.col),
                  P(c.graph.eid), P(c.graph.invdeg), P(bp), P(o["gw1"]), P(o["gb1"]), P(ws), N, h, D)
        torch.cuda.synchronize()
        res.append({k: _bits(v) for k, v in o.items()})
    assert bool(torch.isnan(res[0]["sum_a"].view(torch.float32)).all())                # (not hosted: untouched)
    for h_ in res[1:]:
        assert torch.equal(h_["sum_a"], c.ref["sum_a"]) and torch.equal(h_["sum_b"], c.ref["sum_b"])
        assert torch.equal(h_["gw1"], res[0]["gw1"]) and torch.equal(h_["gb1"], res[0]["gb1"])


# ------------------------------------------------------------------ one training step, default schedule vs the switch
def _flagship(dev):
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    torch.manual_seed(0)
    return q.TopologicalGNN(100, 64, 3, 4).to(dev).train(), S.topological_batch(2, 6, n=100, e=400).to(dev)


def _nodeless(dev):
    """Graph ids 0 .. 3, id 1 without a node; every node reads a table row of its own (a table gradient row with a single
    term has no summation order)."""
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    graphs = []
    for g, n in enumerate((40, 0, 33, 27)):
        if n == 0:
            graphs.append(q.Data(edge_index=torch.zeros(2, 0, dtype=torch.long), edge_attr=torch.zeros(0, 4),
                                 node_ids=torch.zeros(0, dtype=torch.long), y=torch.zeros(1, 3), num_nodes=0))
            continue
        b = S.topological_batch(2, 1, n=n, e=4 * n, first_graph=g)
        graphs.append(q.Data(edge_index=b.edge_index, edge_attr=b.edge_attr, node_ids=b.node_ids, y=torch.zeros(1, 3), num_nodes=n))
    batch = q.Batch.from_data_list(graphs)
    batch.y = torch.randn(4, 3, generator=torch.Generator().manual_seed(5))
    batch.node_ids = torch.arange(100)
    torch.manual_seed(0)
    return q.TopologicalGNN(100, 64, 3, 4).to(dev).train(), batch.to(dev)


def _step(model, batch):
    batch._qot_cache = {}
    model._qot_step.fill_(7)             # the dropout draws of every compared step are those of counter 7
    model.zero_grad(set_to_none=True)
    out, _, g = model.forward_loss(batch, batch.y.view(-1, 3))
    out.backward(g)
    torch.cuda.synchronize()
    return {k: _bits(p.grad) for k, p in model.named_parameters()}


def _spied_step(model, batch, switch):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("QOT_NO_HOSTED_SUMS", "1" if switch else "0")
        calls, launches = [], []
        real_call, real_run = _lib.call, _lib.run_roles
        mp.setattr(_lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
        mp.setattr(_lib, "run_roles", lambda roles, *a: (launches.append(len(roles)) if roles else None, real_run(roles, *a))[1])
        grads = _step(model, batch)
    return grads, calls, launches


@pytest.mark.parametrize("which", ["flagship", "nodeless"])
def test_training_step_equals_the_unhosted_schedule_bitwise(cuda_device, which):
    model, batch = (_flagship if which == "flagship" else _nodeless)(cuda_device)
    _step(model, batch)                                          # (first-call setup outside the comparison)
    g_def, calls_def, runs_def = _spied_step(model, batch, switch=False)
    g_off, calls_off, runs_off = _spied_step(model, batch, switch=True)
    g_def2, _, _ = _spied_step(model, batch, switch=False)
    for calls in (calls_def, calls_off):
        assert "qot_nnconv_gradh_split" in calls and "qot_nnconv_adjoint_dw" in calls
    assert sorted(calls_def) == sorted(calls_off)                # the same entry points, grad-h later in the pass
    print(which, "qot_run_roles launches: default", runs_def, "switch", runs_off)
    if which == "flagship":
        assert len(runs_def) == len(runs_off) - 1                # the stage-1 launch is gone
    else:
        # No table mode with a node-less graph, hence no stage 2 for the sum of grad-h's partials to ride with: that sum has
        # to follow the grad-h launch, so the epilogue keeps a launch -- of that one job instead of all of stage 1.
        assert len(runs_def) == len(runs_off) and runs_def[-1] == 1 and runs_off[-1] > 1
    for k in g_off:
        assert not bool(torch.isnan(g_off[k].view(torch.float32)).any()), k
        assert torch.equal(g_def[k], g_off[k]) and torch.equal(g_def2[k], g_off[k]), (which, k)


def test_captured_step_replays_the_eager_bits(cuda_device):
    """The step captured with ``torch.cuda.graph`` (default capture mode, one stream: the graph is a chain) and replayed
    twice equals the eager step: the hosted jobs are host state only until the grad-h launch takes them."""
    model, batch = _flagship(cuda_device)
    eager = _step(model, batch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(model, batch)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    y = batch.y.view(-1, 3)
    model.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                # (the forward reads and advances the counter buffer where it lies)
        out, _, g = model.forward_loss(batch, y)
        out.backward(g)
    grads = dict(model.named_parameters())
    for _ in range(2):
        for p in grads.values():
            p.grad.fill_(float("nan"))
        model._qot_step.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for k, p in grads.items():
            assert torch.equal(_bits(p.grad), eager[k]), k
