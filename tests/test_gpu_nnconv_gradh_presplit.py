"""The g tile of the split-bf16 grad-h kernel at H = 64 (nnconv_gradh64, csrc/nnconv_gradh64.hip) written to LDS as three
bf16 planes, split once per tile, with the staged edge features living in the planes' storage after the MFMA phase.

The same values are split by the same routine and meet the same weight planes in the same MFMA order as in the earlier
loop (QOT_GRADH_SPLIT_AFTER_READ=1: the fp32 tile, split after every read), so gw1 and gb1 must be EQUAL BIT FOR BIT
between the two forms, and the default form bit for bit run to run.  ``qot_nnconv_gradh_split`` is called directly, with
the planes of Wk^T from ``functional.nnconv_pack``, at the smallest shapes at which the layout, the aliasing or the added
barrier can go wrong.  (Parity against fp64: tests/test_gpu_nnconv_split_bf16.py.)"""
import os

import pytest
import torch

from gnn_qot_estimation_amd import _lib
from gnn_qot_estimation_amd import functional as QF
from gnn_qot_estimation_amd.graph import build_graph_index

pytestmark = pytest.mark.gpu

H = 64
ENV = "QOT_GRADH_SPLIT_AFTER_READ"


def _graph(case, gen):
    if case == "one_node":
        return 1, torch.zeros(2, 1, dtype=torch.int64)
    if case == "two_tiles":             # the second tile holds one row: 31 plane rows of absent nodes, which must be zero
        return 33, torch.randint(0, 33, (2, 120), generator=gen)
    if case == "no_edges":
        return 5, torch.zeros(2, 0, dtype=torch.int64)
    if case == "gaps":
        # 70 nodes: two full tiles and a 6-row one; nodes 2, 5, 8, ... have no in-edges (their plane rows are written and
        # multiplied but no edge reads the GA rows), inside both full tiles
        N = 70
        dsts = torch.tensor([j for j in range(N) if j % 3 != 2])
        dst = dsts[torch.randint(0, len(dsts), (260,), generator=gen)]
        return N, torch.stack([torch.randint(0, N, (260,), generator=gen), dst])
    if case == "cap":
        # tile 0 holds exactly 256 edges (all staged, kGhCap), tile 1 holds 300 (44 through the overflow path, straight
        # from memory), tile 2 a few
        N = 70
        dst = torch.cat([torch.randint(0, 32, (256,), generator=gen), torch.randint(32, 64, (300,), generator=gen),
                         torch.randint(64, 70, (9,), generator=gen)])
        return N, torch.stack([torch.randint(0, N, (565,), generator=gen), dst])
    N = 36000                           # "carry": 1125 tiles, more than the two workgroups per CU of a 304-CU part (608)
    return N, torch.randint(0, N, (2, 3 * N), generator=gen)


def _call(c, after_read):
    """gw1, gb1 of one call of qot_nnconv_gradh_split; the switch is read by the entry point on every call."""
    dev, D, K, N = c["dev"], c["D"], 2 * c["D"], c["N"]
    gw1 = torch.full((K, D), float("nan"), device=dev)
    gb1 = torch.full((K,), float("nan"), device=dev)
    graph, P = c["graph"], _lib.ptr
    old = os.environ.get(ENV)
    os.environ[ENV] = "1" if after_read else "0"
    try:
        _lib.call("qot_nnconv_gradh_split", P(c["g"]), H, P(c["x"]), H, P(c["ea"]), P(c["w1"]), P(c["b1"]), P(graph.rowptr),
                  P(graph.col), P(graph.eid), P(graph.invdeg), P(c["bsplit"]), c["split"].numel() // 3, P(gw1), P(gb1),
                  P(c["ws"]), N, H, D)
        torch.cuda.synchronize()
    finally:
        if old is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = old
    return gw1.cpu(), gb1.cpu()


_CASES = {}


def _case(name, D, dev, gscale=1.0):
    """Inputs and the results of default / split-after-read / default again: computed once, shared, left unchanged."""
    key = (name, D, gscale)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(23)
        N, ei = _graph(name, gen)
        K, E = 2 * D, ei.shape[1]
        c = dict(dev=dev, D=D, N=N, E=E, graph=build_graph_index(ei.to(dev), N),
                 x=torch.randn(N, H, generator=gen).to(dev), g=(torch.randn(N, H, generator=gen) * gscale).to(dev),
                 ea=torch.rand(E, D, generator=gen).to(dev), w1=(torch.randn(K, D, generator=gen) * 0.5).to(dev),
                 b1=(torch.randn(K, generator=gen) * 0.5).to(dev))
        w2 = (torch.randn(H * H, K, generator=gen) / 16).to(dev)
        b2 = (torch.randn(H * H, generator=gen) / 16).to(dev)
        wroot = (torch.randn(H, H, generator=gen) / 8).to(dev)
        old = os.environ.get("QOT_NNCONV_F32_MFMA")
        os.environ["QOT_NNCONV_F32_MFMA"] = "0"          # nnconv_pack writes the planes only for the split form
        try:
            wp, _, _, split = QF.nnconv_pack(w2, b2, wroot, H, K)
        finally:
            if old is None:
                del os.environ["QOT_NNCONV_F32_MFMA"]
            else:
                os.environ["QOT_NNCONV_F32_MFMA"] = old
        c["split"], c["bsplit"] = split, split[wp.numel():]      # the planes of Wk^T follow those of Wcat in each plane
        c["ws"] = torch.empty(_lib.load().qot_nnconv_gradh_workspace_floats(D), dtype=torch.float32, device=dev)
        c["new"] = _call(c, False)
        c["old"] = _call(c, True)
        c["again"] = _call(c, False)
        _CASES[key] = c
    return _CASES[key]


def _check(c, tag):
    (w_new, b_new), (w_old, b_old), (w_again, b_again) = c["new"], c["old"], c["again"]
    print(tag, "gw1 max |.|", float(w_new.abs().max()), "gb1 max |.|", float(b_new.abs().max()),
          "differing words vs split-after-read", int((w_new.view(torch.int32) != w_old.view(torch.int32)).sum()) +
          int((b_new.view(torch.int32) != b_old.view(torch.int32)).sum()))
    assert not bool(w_new.isnan().any()) and not bool(b_new.isnan().any()), tag          # every entry written
    assert torch.equal(w_new.view(torch.int32), w_old.view(torch.int32)), tag
    assert torch.equal(b_new.view(torch.int32), b_old.view(torch.int32)), tag
    assert torch.equal(w_new.view(torch.int32), w_again.view(torch.int32)), tag
    assert torch.equal(b_new.view(torch.int32), b_again.view(torch.int32)), tag
    if c["E"] == 0:
        assert not bool(w_new.any()) and not bool(b_new.any()), tag
    else:
        assert bool(w_new.any()), tag            # (not two forms that both return nothing)


SHAPES = [("one_node", 4), ("two_tiles", 4), ("no_edges", 4), ("gaps", 1), ("gaps", 2), ("gaps", 3), ("gaps", 4),
          ("cap", 4), ("cap", 1), ("carry", 4)]


@pytest.mark.parametrize("name,D", SHAPES)
def test_presplit_equals_split_after_read_bitwise(cuda_device, name, D):
    _check(_case(name, D, cuda_device), (name, D))


@pytest.mark.parametrize("gscale", [2.0 ** 20, 2.0 ** -20])
def test_presplit_scaled_g_bitwise(cuda_device, gscale):
    """g scaled by 2^20 and 2^-20: the splits see other exponents."""
    _check(_case("gaps", 4, cuda_device, gscale), ("gaps", 4, gscale))


def test_staged_edge_counts_of_cap_case():
    """The "cap" graph is what its comment says: 256 in-edges in tile 0 (the staging capacity), more in tile 1."""
    gen = torch.Generator().manual_seed(23)
    _, ei = _graph("cap", gen)
    per_tile = torch.bincount(ei[1] // 32, minlength=3)
    assert per_tile.tolist() == [256, 300, 9]
