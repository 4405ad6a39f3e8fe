"""Cases, fp64 restatement and per-element error bounds of the TransformerConv forward (tests/test_tconv_fwd_cases_cpu.py,
tests/test_gpu_tconv_fwd.py): logits -> edge softmax -> ``sum alpha (v_j + We ea) + skip`` -> ``dropout(leaky_relu(.))``, in
the six forms behind ``nn.TransformerConv``: the per-destination kernel in node and in table mode, its score-matrix variant,
the row form, the tile form and the graph form.

Every form is checked AT ITS OWN STAGE: the attention kernels take the fp32 rows ``qkvs = [q | k | v | skip]`` (graph
form: ``(t4, M, P)``; scores and rows: also the kernel's own ``scores = T_q T_k^T``) as inputs, and ``reference`` restates
the chain in fp64 from exactly those bits.  The products in front (``qot_gemm_nt``, ``qot_table_scores``,
``qot_table_project_fwd``) have plain dot-product bounds of their own (``scores_reference``, ``prepare_reference``).

Companions as in tests/head_cases.py: a magnitude ``A >= |value|`` and a count ``k``; the assertion is ``|got - ref| <=
k 2^-24 A`` per element (``head_cases.compare`` / ``check_all``).  A sum of n operands counts ``max k_i + n - 1`` over
``sum A_i``, a product ``k_x + k_y + 1`` over ``A_x A_y``, a stage input has ``k = 0`` and ``A = |value|``.

The logit's count per form, as read from the kernels (``logit_count``):
  * per-destination (csrc/tconv.hip, ``tconv_fwd_kernel``): ``qi = scale4(rs, ld4(q ...))`` with ``rs = rsqrtf(H)``: 2 (the
    factor and the product); ``dotv<NV>(qi, kr[u])``: products of ``qi`` (2 + 0 + 1 = 3), four of them added on one lane
    (counted 4), then ``group_sum<TPR>``: ``log2(H / 4)`` steps; ``qe[d] = group_sum<TPR>(t)`` is the same tree over
    ``qi We``; ``s = fmaf(qe[d], ee[d], s)``: products of a computed operand (+ 1) and D additions:
    k = 3 + 4 + log2(H / 4) + 1 + D = 8 + log2(H / 4) + D  over  A = rs (<|q|, |k|> + <|q| |We|, |ea|>);
  * tile (``tconv_fwd_tile_kernel``): the same dot, written to ``srow`` and read back: the same count;
  * scores and rows (``tconv_fwd_kernel<., ., MT>``: ``mym = rs * Mtab[...]``, csrc/tconv_rows.hip: ``sM[t] = rs *
    Mtab[...]``): the lookup costs 2, the ``qe`` tree is the longer operand: the same k over
    A = rs (|scores| + <|q| |We|, |ea|>);
  * graph (csrc/tconv_graph.hip, stage A: ``s = mv; s = fmaf(pr[d], ev[d], s)``): k = D + 1 over A = |M| + <|P|, |ea|>.

The softmax.  Let ``b_i`` be the largest logit bound among the in-edges of destination ``i``.
  * A weight ``p_e = exp(s_e - m)`` carries the relative error ``2 b_i + (2 |s_e - m| + C0 + 3 r_i) u``: ``s_e`` and ``m``
    are each off by ``b_i``; ``s - mn`` is rounded (``|x| u`` on the result) and ``__expf`` scales its argument by ``log2 e``
    (another ``|x| u``), the instruction itself is inside ``C0 u``.  The per-destination, scores, rows and tile forms
    keep a running maximum: a weight formed against an earlier maximum is later multiplied by ``sc = __expf(m - mn)``
    once per arrival of a new maximum; the arguments of those factors add up to ``s_e - m`` (already counted), each
    factor adds its instruction's error and two roundings: ``3 r_i u`` with ``r_i`` the number of new maxima after the
    first in CSR order (a logit within ``2 b_i`` of the running maximum counts as one).  The graph form makes two passes:
    ``r_i = 0``.
  * ``alpha_e`` adds the destination's worst weight error and ``(deg + C0) u`` (the denominator's chain and the division).
  * ``pre = sum alpha (v_j + We ea_e) + skip``: ``sum_e alpha_e rel(alpha_e) (|v_j| + |We| |ea_e|)`` plus
    ``(deg + D + 3 + C0) u A_pre``.  leaky_relu and the mask are 1-Lipschitz in ``pre``: the bound of ``pre`` (and two
    roundings) carries to ``out`` times ``keep_scale``; no margin from the kink is needed, a dropped element's bound is 0.
  * An isolated destination has ``m = 0`` and ``denom = 1e-16f`` as the kernels leave them, and ``out = act(skip_i)``.

Nothing here touches the GPU; every case and host reference is built once and shared."""
import functools
import math
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import gnn_qot_estimation_amd as q
from head_cases import C0, U, check_all, compare      # noqa: F401  (re-exported: the checks are the head's)
from oracle import dropout as OD

SLOPE = 0.01
SLOPE32 = float(np.float32(SLOPE))          # what the kernels receive: ``float slope``
SEED = (1 << 63) + 0x5DEECE66D       # all 64 bits in use
STEP = 7
EPS32 = float(np.float32(1e-16))
FORMS = ("node", "table", "scores", "rows", "tile", "graph")
LOOKUP_FORMS = ("scores", "rows", "graph")
ONLINE_FORMS = ("node", "table", "scores", "rows", "tile")
# a dozen (H, D) pairs: every H, every D; D == 4 (the graph form's float4 path) and D > 4 (the rows form's own path) among them
WIDTHS = ((16, 1), (16, 4), (16, 8), (32, 3), (32, 8), (64, 1), (64, 4), (64, 5), (128, 3), (128, 8), (256, 1), (256, 5))


def rpb(H):
    """Destinations per workgroup (``tconv_rpb``)."""
    return 256 // (H // 4)


def bt(H):
    """In-edges prefetched per batch (``BT`` of the per-destination kernels)."""
    return min(H // 4, 16)


def degree_classes(H):
    """The planted in-degrees, those around the batch size ``BT`` first: a graph of fewer than 12 nodes takes a run of this
    list (rotating with the graph), a larger one all of it."""
    b = bt(H)
    return [0, 1, b - 1, b, b + 1, 2 * b, 2 * b + 3, 3 * b + 1, 2, 3, 4, 5]


# ------------------------------------------------------------------ case table
def _c(form, H, D, n, B, V=None, family="ordinary", p=0.0, env=(), **kw):
    assert (H, D) in WIDTHS, (H, D)
    return dict(form=form, H=H, D=D, n=n, B=B, V=V if V is not None else n, family=family, p=p, env=dict(env), **kw)


_NO_TILE = {"QOT_NO_TCONV_TILE": "1"}
_TABLE = {"QOT_NO_TCONV_GRAPH": "1", "QOT_NO_TCONV_TILE": "1", "QOT_NO_TCONV_SCORES": "1"}
_SCORES = dict(_NO_TILE, QOT_NO_TCONV_FWD_ROWS="1")
_TILE = {"QOT_NO_TCONV_GRAPH": "1"}


def _cases():
    out = {}
    # node mode: N = 2 RPB + 3 nodes in graphs of unequal sizes (no table): the last workgroup is partly empty
    for H, D in ((16, 1), (32, 3), (64, 4), (128, 8), (256, 5)):
        out[f"node_h{H}_d{D}"] = _c("node", H, D, None, None, N=2 * rpb(H) + 3)
    # per-destination kernel in table mode: n = 12, B n no multiple of RPB; one case with more table rows than nodes
    for H, D, B, V in ((16, 4, 7, 12), (32, 8, 5, 12), (64, 5, 3, 12), (128, 3, 3, 12), (256, 1, 3, 16)):
        out[f"table_h{H}_d{D}_b{B}_v{V}"] = _c("table", H, D, 12, B, V, env=_TABLE)
    # score matrix: V = 16 != n = 12 (never the rows form), N = 72 >= 4 V; one case with V == n and the rows form switched off
    for H, D in ((32, 3), (64, 4), (128, 8), (256, 5)):
        out[f"scores_h{H}_d{D}_v16"] = _c("scores", H, D, 12, 6, 16, env=_NO_TILE)
    out["scores_h64_d1_v12"] = _c("scores", 64, 1, 12, 4, 12, env=_SCORES)
    # rows: fewer graphs than the 8 slices; per = 2 with three empty slices; 8 RPB + 9 graphs (a second round per lane group
    # and the graph-ahead prefetch)
    # (B = 3 gives N = 36 < 4 V: the dispatcher's size rule ``functional.tconv_scores_ok`` would send it to the per-destination
    # kernel; the kernels have no such limit, and the GPU test lifts the rule for this case -- ``lift``; B = 4 is the
    # smallest batch the dispatcher itself sends to the rows form)
    out["rows_h64_d4_b3"] = _c("rows", 64, 4, 12, 3, env=_NO_TILE, lift=True)
    out["rows_h64_d4_b4"] = _c("rows", 64, 4, 12, 4, env=_NO_TILE)
    out["rows_h128_d8_b9"] = _c("rows", 128, 8, 12, 9, env=_NO_TILE)
    out["rows_h256_d1_b9"] = _c("rows", 256, 1, 12, 9, env=_NO_TILE)
    out["rows_h64_d5_b137"] = _c("rows", 64, 5, 12, 8 * rpb(64) + 9, env=_NO_TILE)
    out["rows_h256_d5_b41"] = _c("rows", 256, 5, 12, 8 * rpb(256) + 9, env=_NO_TILE)
    # tile: B = RPB + 1 (dead lane groups); n = 4 RPB + 6 (a second, ragged j0 round of the score row); n = 5
    out["tile_h64_d4_n70"] = _c("tile", 64, 4, 4 * rpb(64) + 6, rpb(64) + 1, env=_TILE)
    out["tile_h256_d5_n22"] = _c("tile", 256, 5, 4 * rpb(256) + 6, rpb(256) + 1, env=_TILE)
    out["tile_h32_d8_n5"] = _c("tile", 32, 8, 5, rpb(32) + 1, env=_TILE)
    out["tile_h128_d3_n12"] = _c("tile", 128, 3, 12, rpb(128) + 1, env=_TILE)
    # graph: n = 128; n = 70 > G = 64 destinations of a stage-C round; n = 5 at G = 4; B = 1; a graph of more than 1024
    # edges (second staging trip); more graphs than 4 x CUs (later-graph trips, ragged last trip); E = 0; V > n
    out["graph_h16_d4_n128"] = _c("graph", 16, 4, 128, 3)
    out["graph_h16_d1_n70"] = _c("graph", 16, 1, 70, 3)
    out["graph_h256_d5_n5"] = _c("graph", 256, 5, 5, 6)
    out["graph_h64_d4_b1"] = _c("graph", 64, 4, 12, 1)
    out["graph_h32_d3_n40_big"] = _c("graph", 32, 3, 40, 3, big=1)
    out["graph_h16_d8_n5_trips"] = _c("graph", 16, 8, 5, "trips")
    out["graph_h128_d3_e0"] = _c("graph", 128, 3, 12, 2, empty=True)
    out["graph_h64_d5_v16"] = _c("graph", 64, 5, 12, 3, 16)
    # dropout at p = 0.5, one per form (table mode included: the mask is numbered by node, not by table row)
    out["drop_node_h32_d3"] = _c("node", 32, 3, None, None, N=2 * rpb(32) + 3, p=0.5)
    out["drop_table_h64_d5_v16"] = _c("table", 64, 5, 12, 3, 16, p=0.5, env=_TABLE)
    out["drop_scores_h128_d8_v16"] = _c("scores", 128, 8, 12, 6, 16, p=0.5, env=_NO_TILE)
    out["drop_rows_h128_d3_b9"] = _c("rows", 128, 3, 12, 9, p=0.5, env=_NO_TILE)
    out["drop_tile_h16_d8_n12"] = _c("tile", 16, 8, 12, rpb(16) + 1, p=0.5, env=_TILE)
    out["drop_graph_h32_d8_v16"] = _c("graph", 32, 8, 12, 5, 16, p=0.5)
    # sharp softmax, one per form
    out["sharp_node_h64_d4"] = _c("node", 64, 4, None, None, N=2 * rpb(64) + 3, family="sharp")
    out["sharp_table_h32_d3"] = _c("table", 32, 3, 12, 5, family="sharp", env=_TABLE)
    out["sharp_scores_h64_d5_v16"] = _c("scores", 64, 5, 12, 6, 16, family="sharp", env=_NO_TILE)
    out["sharp_rows_h256_d1_b9"] = _c("rows", 256, 1, 12, 9, family="sharp", env=_NO_TILE)
    out["sharp_tile_h128_d3_n12"] = _c("tile", 128, 3, 12, rpb(128) + 1, family="sharp", env=_TILE)
    out["sharp_graph_h16_d4_n12"] = _c("graph", 16, 4, 12, 3, family="sharp")
    return out


CASES = _cases()
TRIP_CUS = 2        # host stand-in for the device's multi_processor_count in the "trips" case


def forms_of(name):
    """The forms a case runs in: its own, and for a rows case also the scores form (same bits promised)."""
    form = CASES[name]["form"]
    return (form, "scores") if form == "rows" else (form,)


def env_of(name, form):
    cfg = CASES[name]
    return dict(cfg["env"], QOT_NO_TCONV_FWD_ROWS="1") if (cfg["form"] == "rows" and form == "scores") else dict(cfg["env"])


# ------------------------------------------------------------------ graphs
def _graph_edges(n, H, rot, gen, extra=0):
    """``(src, dst)`` of one graph, in an order that is NOT sorted by destination: node r has in-degree
    ``degree_classes(H)[(r + rot) % 12]`` (r < 12; later nodes 3 .. 5), plus ``extra``; the first in-edge of every third
    destination is a self loop, the second in-edge of every other destination of in-degree >= 3 repeats its first."""
    classes = degree_classes(H)
    src, dst = [], []
    for r in range(n):
        deg = (classes[(r + rot) % 12] if r < 12 else int(torch.randint(3, 6, (1,), generator=gen))) + extra
        s = torch.randint(0, n, (deg,), generator=gen).tolist()
        if deg >= 1 and r % 3 == 1:
            s[0] = r
        if deg >= 3 and r % 2 == 0:
            s[1] = s[0]
        src += s
        dst += [r] * deg
    perm = torch.randperm(len(src), generator=gen)
    return torch.tensor([src, dst], dtype=torch.long).view(2, -1)[:, perm]


def _sizes(cfg, cus):
    """``[(n, rotation, extra in-degree, has edges)]`` per graph."""
    if cfg["form"] == "node":
        N = cfg["N"]
        sizes = [12] * (N // 12) + ([N % 12] if N % 12 else [])
        if len(sizes) == 1:
            sizes = [N - 3, 3]
        assert len(set(sizes)) > 1 and sum(sizes) == N           # unequal sizes: no table mode
        return [(s, g, 0, g != len(sizes) - 1 if len(sizes) == 2 else g != 1) for g, s in enumerate(sizes)]
    B = 4 * cus + 3 if cfg["B"] == "trips" else cfg["B"]
    n = cfg["n"]
    out = []
    for g in range(B):
        rot = (g - (g > 1)) * n % 12 if n < 12 else g          # (graph 1 has no edges: its run goes to the next)
        has = not cfg.get("empty") and (B == 1 or g != 1)
        out.append((n, rot, 26 if (cfg.get("big") and g == 2) else 0, has))
    return out


def _index(ei, N):
    """Host CSR of ``edge_index`` in the device build's order (stable by destination: csrc/graph_prep.hip)."""
    src, dst = ei[0], ei[1]
    eid = torch.argsort(dst, stable=True)
    deg = torch.bincount(dst, minlength=N)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])
    row = dst[eid]
    pos = torch.arange(ei.shape[1]) - rowptr[row]
    return types.SimpleNamespace(eid=eid, deg=deg, rowptr=rowptr, row=row, col=src[eid], pos=pos)


def _unit_rows(R, H, gen):
    return torch.randn(R, 4 * H, generator=gen)


def _logits64(c, qkvs):
    """fp64 logits per CSR slot from ``qkvs`` (the H-term dot), and the per-destination spread."""
    r = _evaluate(types.SimpleNamespace(**dict(vars(c), qkvs=qkvs, p=0.0, ks=1.0, keep=torch.ones(c.N, c.H, dtype=torch.bool))),
                  torch.float64)
    lo = torch.full((c.N,), float("inf"), dtype=torch.float64).scatter_reduce(0, c.ix.row, r["s"], "amin")
    spread = torch.where(c.ix.deg > 0, r["m"] - lo, torch.zeros((), dtype=torch.float64))
    return r["s"], spread


@functools.lru_cache(maxsize=None)
def tconv_case(name, cus=TRIP_CUS):
    return build_case(name, CASES[name], cus)


def build_case(name, cfg, cus=TRIP_CUS):
    """The case ``name`` of a table entry ``cfg`` (tests/tconv_bwd_cases.py has entries of its own)."""
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))          # by name: adding a case moves no other
    H, D = cfg["H"], cfg["D"]
    sizes = _sizes(cfg, cus)
    sharp = cfg["family"] == "sharp"
    graphs = []
    for g, (n, rot, extra, has) in enumerate(sizes):
        if sharp and cfg["form"] != "node" and g > 0 and has:
            ei, ea = graphs[0].edge_index, graphs[0].edge_attr       # one graph, repeated: a table row has ONE spread
        elif has:
            ei = _graph_edges(n, H, 0 if sharp else rot, gen, extra)
            ea = torch.rand(ei.shape[1], D, generator=gen)
        else:
            ei, ea = torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, D)
        graphs.append(q.Data(edge_index=ei.clone(), edge_attr=ea.clone(), node_ids=torch.arange(n), num_nodes=n))
    table_mode = cfg["form"] != "node"
    N = sum(s[0] for s in sizes)
    c = types.SimpleNamespace(name=name, cfg=cfg, H=H, D=D, N=N, n=cfg["n"], B=len(sizes), V=cfg["V"] if table_mode else N,
                              table_mode=table_mode, slope=SLOPE, p=cfg["p"], seed=SEED + 17 * len(name), step=STEP,
                              family=cfg["family"])
    c.w_edge = (torch.rand(H, D, generator=gen) * 2 - 1) / D ** 0.5           # PyG's Linear(D, H, bias=False) initialisation
    qkvs = _unit_rows(c.V, H, gen)
    for attempt in range(2):
        c.batch = q.Batch.from_data_list(graphs)
        c.ei, c.edge_attr = c.batch.edge_index, c.batch.edge_attr
        c.E = c.ei.shape[1]
        c.ix = _index(c.ei, N)
        c.rows = (torch.arange(N) % c.n) if table_mode else torch.arange(N)      # node -> row of qkvs (node_ids)
        if not sharp or attempt == 1:
            break
        # sharp: the largest logit of destination i goes first, to the middle or last in CSR order (i % 3) by exchanging
        # two in-edges' (source, features); then q's rows are scaled (below) -- a positive factor keeps the place
        s, _ = _logits64(c, qkvs)
        for g0 in ([0] if table_mode else range(len(graphs))):
            lo_node = int(c.batch.ptr[g0])
            gr = graphs[g0]
            for i in range(lo_node, lo_node + sizes[g0][0]):
                a, b = int(c.ix.rowptr[i]), int(c.ix.rowptr[i + 1])
                if b - a < 2:
                    continue
                top = a + int(torch.argmax(s[a:b]))
                want = (a, a + (b - a) // 2, b - 1)[i % 3]
                e1, e2 = (int(c.ix.eid[top]) - int(c.batch.edge_ptr[g0]), int(c.ix.eid[want]) - int(c.batch.edge_ptr[g0]))
                for t in (gr.edge_index[0], gr.edge_attr):
                    t[[e1, e2]] = t[[e2, e1]]
        if table_mode:
            graphs = [q.Data(edge_index=graphs[0].edge_index.clone(), edge_attr=graphs[0].edge_attr.clone(),
                             node_ids=gr.node_ids, num_nodes=gr.num_nodes) if sz[3] else gr for gr, sz in zip(graphs, sizes)]
    if sharp:
        _, spread = _logits64(c, qkvs)
        per_row = torch.zeros(c.V, dtype=torch.float64).scatter_reduce(0, c.rows, spread, "amax")
        target = 42.0 + 16.0 * torch.rand(c.V, generator=gen, dtype=torch.float64)
        fac = torch.where(per_row > 0, target / per_row.clamp_min(1e-30), torch.ones((), dtype=torch.float64))
        qkvs = qkvs.clone()
        qkvs[:, :H] = (qkvs[:, :H].double() * fac[:, None]).float()
    c.qkvs = qkvs
    c.keep = OD.keep_mask(c.seed, c.step, (N, H), c.p)
    c.ks = float(OD.keep_scale(c.p)) if c.p > 0 else 1.0
    # what the host asserts of every case: the index is not the identity, duplicates and self loops are there
    if c.E:
        assert not torch.equal(c.ix.eid, torch.arange(c.E)), name
        assert bool((c.ei[0] == c.ei[1]).any()), name
        assert torch.unique(c.ei, dim=1).shape[1] < c.E, name
    s, spread = _logits64(c, c.qkvs)
    c.spread = spread
    if sharp:
        assert float(spread.max()) <= 60.0 and float(spread[c.ix.deg >= 2].min()) >= 40.0, (name, spread)
    else:
        assert float(spread.max()) <= 16.0, (name, float(spread.max()))
    return c


def host_lookup(c, form):
    """The lookup tensors of a lookup form as the stage in front would leave them: fp64 products rounded to fp32."""
    H = c.H
    t = c.qkvs.double()
    tq, tk = t[:, :H], t[:, H:2 * H]
    if form in ("scores", "rows"):
        return (tq @ tk.t()).float()
    if form == "graph":
        rs = 1.0 / math.sqrt(H)
        return ((tq[:c.n] @ tk[:c.n].t()) * rs).float(), ((tq[:c.n] @ c.w_edge.double()) * rs).float()
    return None


# ------------------------------------------------------------------ the chain, in any dtype
DEFECTS = {
    "second_batch_first_edge_dropped": "the in-edge at CSR position BT is dropped",
    "no_rescale_on_new_max": "no rescale of the running sums when a new maximum arrives",
    "edge_term_unscaled": "1 / sqrt(H) applied to <q, k> only",
    "value_edge_term_missing": "We (sum alpha ea) left out of the output",
    "features_by_slot": "ea read at the CSR slot instead of eid[slot]",
    "isolated_not_skip": "an isolated destination gets 0",
    "table_row_is_node": "row i % V instead of node_ids[i]",
    "mask_numbered_at_table_row": "the dropout index taken from the table row",
    "weight_off_1e-4": "one weight per destination multiplied by 1 + 1e-4",
}


def _segsum(x, row, N):
    return torch.zeros((N,) + tuple(x.shape[1:]), dtype=x.dtype).index_add_(0, row, x)


def _segmax(x, row, N):
    return torch.full((N,), -float("inf"), dtype=x.dtype).scatter_reduce(0, row, x, "amax")


def _evaluate(c, dtype, defect=None, lookup=None):
    """The chain in plain tensor operations in ``dtype``, per CSR slot; ``lookup``: ``scores [V, V]`` or ``(M, P)``, read as
    the form reads it; ``defect``: one of DEFECTS planted."""
    assert defect is None or defect in DEFECTS
    H, D, N = c.H, c.D, c.N
    ix = c.ix
    t, we, ea = c.qkvs.to(dtype), c.w_edge.to(dtype), c.edge_attr.to(dtype)
    rs = 1.0 / math.sqrt(H)
    rows = c.rows
    if defect == "table_row_is_node":
        rows = torch.arange(N) % c.V
    ri, rj = rows[ix.row], c.rows[ix.col]
    e = ea[torch.arange(c.E)] if defect == "features_by_slot" else ea[ix.eid]
    tq, tk, tv, ts = t[:, :H], t[:, H:2 * H], t[:, 2 * H:3 * H], t[:, 3 * H:]
    if isinstance(lookup, tuple):
        M, P = (x.to(dtype) for x in lookup)
        dense, edge = M[ri, rj], (P[ri] * e).sum(-1)
    else:
        dense = (lookup.to(dtype)[ri, rj] if lookup is not None else (tq[ri] * tk[rj]).sum(-1)) * rs
        edge = (((tq @ we) * rs)[ri] * e).sum(-1)
    if defect == "edge_term_unscaled":
        edge = edge * math.sqrt(H)
    s = dense + edge
    live = torch.ones(c.E, dtype=torch.bool)
    if defect == "second_batch_first_edge_dropped":
        live = ix.pos != bt(H)
    s_live = torch.where(live, s, torch.full((), -float("inf"), dtype=dtype))
    m = _segmax(s_live, ix.row, N)
    has = m > -float("inf")
    m = torch.where(has, m, torch.zeros((), dtype=dtype))
    p = torch.where(live, (s - m[ix.row]).exp(), torch.zeros((), dtype=dtype))
    if defect == "no_rescale_on_new_max":        # every weight stays relative to the maximum of its own time
        run = s.clone()
        for k in range(1, c.E):
            if ix.row[k] == ix.row[k - 1]:
                run[k] = torch.maximum(run[k - 1], s[k])
        p = (s - run).exp()
    if defect == "weight_off_1e-4":
        p = torch.where((ix.pos == 0) & (ix.deg[ix.row] >= 2), p * (1 + 1e-4), p)
    denom = _segsum(p, ix.row, N) + EPS32
    alpha = p / denom[ix.row]
    aa = _segsum(alpha[:, None] * e, ix.row, N)
    pre = _segsum(alpha[:, None] * tv[rj], ix.row, N) + ts[rows]
    if defect != "value_edge_term_missing":
        pre = pre + aa @ we.t()
    if defect == "isolated_not_skip":
        pre = pre * has.to(dtype)[:, None]
    keep = c.keep
    if defect == "mask_numbered_at_table_row":
        keep = OD.keep_mask(c.seed, c.step, (c.V, H), c.p)[rows]
    act = torch.where(pre > 0, pre, pre * float(np.float32(c.slope)))
    out = act * (keep.to(dtype) * c.ks)
    return dict(s=s, m=m, p=p, denom=denom, alpha=alpha, aa=aa, pre=pre, out=out)


def logit_count(form, H, D):
    return D + 1 if form == "graph" else 8 + int(math.log2(H // 4)) + D


def _new_maxima(s, bs, ix):
    """Per destination: arrivals of a new running maximum after the first in CSR order (within ``2 b`` counts)."""
    r = torch.zeros(ix.deg.numel(), dtype=torch.float64)
    sl, rowl, bl = s.tolist(), ix.row.tolist(), bs.tolist()
    runv = 0.0
    for k in range(len(sl)):
        if k == 0 or rowl[k] != rowl[k - 1]:
            runv = sl[k]
            continue
        if sl[k] > runv - 2 * bl[k]:
            r[rowl[k]] += 1
        runv = max(runv, sl[k])
    return r


def reference(c, form, lookup=None):
    """``{quantity: dict(value, A, k, bound)}`` in fp64 for case ``c`` in ``form``; ``lookup``: the tensors a lookup form
    reads (default: ``host_lookup``).  ``alpha`` is per CSR slot; ``out``, ``m``, ``denom``, ``aa`` per node."""
    assert form in FORMS
    if form in LOOKUP_FORMS and lookup is None:
        lookup = host_lookup(c, form)
    r = _evaluate(c, torch.float64, lookup=lookup if form in LOOKUP_FORMS else None)
    H, D, N, ix = c.H, c.D, c.N, c.ix
    f64 = torch.float64
    t, we, ea = c.qkvs.double().abs(), c.w_edge.double().abs(), c.edge_attr.double().abs()[ix.eid]
    rs = 1.0 / math.sqrt(H)
    ri, rj = c.rows[ix.row], c.rows[ix.col]
    tq, tk, tv, ts = t[:, :H], t[:, H:2 * H], t[:, 2 * H:3 * H], t[:, 3 * H:]
    if form == "graph":
        a_s = lookup[0].double().abs()[ri, rj] + (lookup[1].double().abs()[ri] * ea).sum(-1)
    else:
        dense = lookup.double().abs()[ri, rj] if form in LOOKUP_FORMS else (tq[ri] * tk[rj]).sum(-1)
        a_s = rs * (dense + ((tq @ we)[ri] * ea).sum(-1))
    ks = float(logit_count(form, H, D))
    bs = ks * U * a_s
    deg = ix.deg.double()
    b_i = torch.zeros(N, dtype=f64).scatter_reduce(0, ix.row, bs, "amax")
    nrec = _new_maxima(r["s"], bs, ix) if form in ONLINE_FORMS else torch.zeros(N, dtype=f64)
    x = (r["s"] - r["m"][ix.row]).abs()
    relp = 2 * b_i[ix.row] + (2 * x + C0 + 3 * nrec[ix.row]) * U
    relmax = torch.zeros(N, dtype=f64).scatter_reduce(0, ix.row, relp, "amax")
    rela = relp + relmax[ix.row] + (deg[ix.row] + C0) * U
    alpha = r["alpha"]
    msg_a = tv[rj] + ea @ we.t()
    a_pre = _segsum(alpha[:, None] * msg_a, ix.row, N) + ts[c.rows]
    k_pre = deg + D + 3 + C0
    b_pre = _segsum((alpha * rela)[:, None] * msg_a, ix.row, N) + (k_pre * U)[:, None] * a_pre
    keep = c.keep.double() * c.ks
    b_out = keep * (b_pre + 2 * U * a_pre)
    a_aa = _segsum(alpha[:, None] * ea, ix.row, N)
    b_aa = _segsum((alpha * rela)[:, None] * ea, ix.row, N) + ((deg + C0) * U)[:, None] * a_aa
    rel_den = relmax + (deg + C0) * U
    iso = ix.deg == 0

    def entry(value, bound, k):
        k = torch.as_tensor(k, dtype=f64)
        k = k[:, None] if (k.dim() == 1 and bound.dim() == 2) else (k if k.numel() else torch.zeros((), dtype=f64))
        return dict(value=value, bound=bound, k=k, A=bound / (k * U))
    ref = dict(out=entry(r["out"], b_out, k_pre + 2), m=entry(r["m"], b_i, ks),
               denom=entry(r["denom"], torch.where(iso, torch.zeros((), dtype=f64), r["denom"] * rel_den), deg + C0),
               alpha=entry(alpha, alpha * rela, deg[ix.row] + C0), aa=entry(r["aa"], b_aa, deg + C0),
               pre=entry(r["pre"], b_pre, k_pre), s=entry(r["s"], bs, ks))
    ref["isolated"] = iso
    ref["nrec"] = nrec
    return ref


@functools.lru_cache(maxsize=None)
def host_reference(name, form, cus=TRIP_CUS):
    """``reference`` with the host's lookup tensors (cached)."""
    return reference(tconv_case(name, cus), form)


def stats_of(res):
    """``[N, 2]`` as the kernels leave it: running maximum (0 when isolated), denominator."""
    return torch.stack([res["m"], res["denom"]], 1)


# ------------------------------------------------------------------ the products in front
def scores_reference(c):
    """``scores = T_q T_k^T`` of ``qot_gemm_nt`` (fp32 MFMA, H products per element in any order): k = H + C0."""
    H = c.H
    t = c.qkvs.double()
    value = t[:, :H] @ t[:, H:2 * H].t()
    A = t[:, :H].abs() @ t[:, H:2 * H].abs().t()
    k = torch.tensor(float(H + C0), dtype=torch.float64)
    return dict(scores=dict(value=value, A=A, k=k, bound=k * U * A))


PREPARE_CASES = {"h16_d4_n5_v5": (16, 4, 5, 5), "h32_d3_n40_v40": (32, 3, 40, 40), "h64_d4_n70_v70": (64, 4, 70, 70),
                 "h128_d8_n12_v16": (128, 8, 12, 16), "h256_d5_n5_v16": (256, 5, 5, 16), "h64_d1_n128_v128": (64, 1, 128, 128)}
_LINS = ("lin_query", "lin_key", "lin_value", "lin_skip")


@functools.lru_cache(maxsize=None)
def prepare_case(name):
    """A table ``[V, H]`` and PyG-initialised parameters (biases drawn, not zero) for ``tconv_graph_prepare``."""
    from oracle import sparse as O
    H, D, n, V = PREPARE_CASES[name]
    torch.manual_seed(8000 + H + D + n)
    conv = O.TransformerConv(H, H, edge_dim=D)
    table = torch.randn(V, H)
    return types.SimpleNamespace(name=name, H=H, D=D, n=n, V=V, table=table, state={k: v.detach().clone() for k, v in
                                                                                     conv.state_dict().items()})


def prepare_reference(pc):
    """``t4 = table W^T + b`` (``qot_table_project_fwd``: the bias and H products on one chain, k = H + 1), ``M`` and ``P`` of
    ``table_scores_body`` (csrc/tconv_graph_dev.hpp): ``tq`` as t4's; ``u = Wk^T tq`` and ``beta = <tq, bk>`` are H products
    of a computed operand (k = (H + 2) + H - 1); ``M = (beta + <emb, u>) rs`` adds H + 1 operands of k = 2 H + 2 and the
    factor (2): k = 3 H + 4; ``P = (tq We) rs``: k = 2 H + 3.  ``C0`` once for each."""
    H, D, n = pc.H, pc.D, pc.n
    sd = {k: v.double() for k, v in pc.state.items()}
    tab = pc.table.double()
    w4 = torch.cat([sd[f"{k}.weight"] for k in _LINS], 0)
    b4 = torch.cat([sd[f"{k}.bias"] for k in _LINS], 0)
    we = sd["lin_edge.weight"]
    rs = 1.0 / math.sqrt(H)
    t4 = tab @ w4.t() + b4
    a_t4 = tab.abs() @ w4.abs().t() + b4.abs()
    tq, tk, a_tq = t4[:n, :H], t4[:n, H:2 * H], a_t4[:n, :H]
    a_u = a_tq @ sd["lin_key.weight"].abs()
    a_m = rs * (a_tq @ sd["lin_key.bias"].abs()[:, None] + a_u @ tab[:n].abs().t())
    val = dict(t4=t4, M=(tq @ tk.t()) * rs, P=(tq @ we) * rs)
    comp = dict(t4=(a_t4, H + 1 + C0), M=(a_m, 3 * H + 4 + C0), P=(rs * (a_tq @ we.abs()), 2 * H + 3 + C0))
    ref = {}
    for k_, (A, k) in comp.items():
        k = torch.tensor(float(k), dtype=torch.float64)
        ref[k_] = dict(value=val[k_], A=A, k=k, bound=k * U * A)
        assert bool((A * (1 + 1e-12) >= val[k_].abs()).all()), k_
    return ref


# ------------------------------------------------------------------ end to end, from a table and parameters
E2E = {"node": "node_h32_d3", "table": "table_h64_d5_b3_v12", "scores": "scores_h64_d4_v16", "rows": "rows_h128_d8_b9",
       "tile": "tile_h64_d4_n70", "graph": "graph_h16_d1_n70"}


@functools.lru_cache(maxsize=None)
def e2e_case(form):
    """The batch of ``E2E[form]`` with an embedding table and PyG-initialised parameters; ``ref``:
    ``leaky_relu(oracle.sparse.TransformerConv(table[node_ids], ...))`` in fp64."""
    import copy
    from oracle import sparse as O
    c = tconv_case(E2E[form])
    torch.manual_seed(9000 + c.H + c.D)
    conv = O.TransformerConv(c.H, c.H, edge_dim=c.D)
    with torch.no_grad():
        for p in conv.parameters():
            if p.dim() == 1 and p.abs().max() == 0:
                p.uniform_(-0.1, 0.1)
    table = torch.randn(c.V, c.H)
    with torch.no_grad():
        x = table.double()[c.batch.node_ids]
        ref = F.leaky_relu(copy.deepcopy(conv).double()(x, c.ei, c.edge_attr.double()), SLOPE32)
    return types.SimpleNamespace(case=c, table=table, state=conv.state_dict(), ref=ref)
