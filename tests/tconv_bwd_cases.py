"""Cases, fp64 restatement and per-element error bounds of the TransformerConv backward (tests/test_tconv_bwd_cases_cpu.py,
tests/test_gpu_tconv_bwd.py): the per-destination kernels of csrc/tconv.hip (``tconv_bwd_dst_kernel``, ``tconv_bwd_src_kernel``,
in node mode and in tile mode) behind the forms ``node``, ``table``, ``scores`` and ``tile`` of tests/tconv_fwd_cases.py, the
row form's passes (csrc/tconv_rows.hip) and the edge-feature gradient (csrc/edge_grad.hip).

Every kernel is judged AT ITS OWN STAGE, on the fp32 bits it reads: the rows ``qkvs = [q | k | v | skip]``, the edge features,
``w_edge``, the cotangent ``g``, and what the product's own forward saved -- ``stats = (m, denom)`` and the activated output
``y`` (host stand-ins: the fp64 forward of tests/tconv_fwd_cases.py rounded to fp32).  The source pass is judged twice: on
the chain from those inputs (what autograd returns) and on the ``escr``, ``delta`` and ``grad_skip`` bits the destination pass
left (``src_stage``).

Cases: the forward case table's shapes, widths, families and dropout, with the SOURCES re-dealt (``_redeal``): in-degrees,
self loops, the edge order and the edge features stay as the forward case has them, out-degrees take planted classes around
the source pass's batch ``BT = min(H / 4, 16)``: 0, 1, BT - 1, BT, BT + 1 and 2 BT + 1 (spread over the graphs of a batch
where one graph cannot hold them), one destination fed by a single source and one source feeding a single destination.

The chain (``_evaluate``), for destination i and in-edge e = (j -> i), rs = 1 / sqrt(H), ``g_i`` behind the activation:
    a_e = exp(s_e - m_i) / denom_i        da_e = <g_i, v_j + We ea_e>        delta_i = sum a da        ds_e = a_e (da_e - delta_i)
    gq_i = rs (sum ds k_j + We sum ds ea)     gk_j = rs sum ds q_i     gv_j = sum a g_i     gskip_i = g_i
    gWe = sum_i rs q_i (x) pd_i + g_i (x) p2_i     gea_e = rs ds_e We^T q_i + a_e We^T g_i
    gM[r_i, r_j] += ds_e      gP[r] += sum ds ea      (row form)
tests/test_tconv_bwd_cases_cpu.py shows that this equals ``torch.autograd.grad`` of the forward restatement in fp64.

Bounds.  As in tests/head_cases.py the assertion is ``|got - ref| <= bound`` per element with ``bound = k 2^-24 A``; here
every quantity carries ``(mag, b)``: a magnitude (of a sum: the sum of its terms' magnitudes, so cancellation never shrinks
it -- ``gq``, ``pd``, ``ds``, the ``grad M`` entries all are differences ``A1 - delta A2``) and the error bound ``b``, combined
by three rules (u = 2^-24): a stage input has b = 0; a product has ``b = b_x mag_y + mag_x b_y + u mag_x mag_y`` (``k_x + k_y +
1``); a sum of n terms in ANY order ``b = sum b_i + (n - 1) u sum mag_i`` (``max k_i + n - 1``).  The printed ``k`` is ``b / (u
mag)``.  The counts, with the line of csrc/tconv.hip each is read from:
  * ``qi = scale4(rs, ld4(q ...))`` (l. 355), ``rs = rsqrtf(H)`` (l. 349): the factor and the product, k = 2;
  * ``gi`` behind the activation (l. 370: ``vi * (keep ? keep_scale : 0) * (vr > 0 ? 1 : slope)``): two products, k = 2;
  * the logit ``s`` (l. 438-441) is the forward's code: k = ``logit_count`` = 8 + log2(H / 4) + D over rs (<|q|, |k|> + <|q|
    |We|, |ea|>); ``da`` (l. 438-442) has the same shape with ``gi`` (k = 2) for ``qi``: the same count over <|g|, |v|> +
    <|g| |We|, |ea|>;
  * ``a = __expf(s - m) * inv`` (l. 444; ``inv = 1 / stats[2 i + 1]``, l. 393): ``m`` and ``denom`` are stage inputs, no running
    maximum, no rescale: relative error ``expm1(b_s) + (2 |s - m| + C0) u`` (the subtraction and the scaling by log2 e each
    round ``|s - m|``; the instruction, the reciprocal and the product are inside C0);
  * ``ada = a * da`` (l. 445): a product; ``sada += ada`` (l. 446): deg terms on one chain;
  * ``a1, a2, p1, p2`` (l. 449-455): fma chains of deg products with an input row / feature;
  * ``pd = p1 - sada * p2`` (l. 467), ``r = a1 - sada a2`` (l. 470): a product and a sum of two;
  * ``rc = fmaf(wl, pd, rc)`` D times, ``rc *= rs`` (l. 475-476): D + 1 terms, then the factor (2);
  * ``wc = fmaf(qi, pd, gi * p2)`` (l. 495): two products, a sum of two; the rows of a workgroup added in LDS (l. 512), the
    workgroups by ``partial_sum_kernel`` (one level or two: l. 793-801) or QOT_ROLE_SUM_ROWS: N terms in any order,
    whatever the grid;
  * tile mode: the rows of RPB graphs added in LDS (l. 528-531), the groups by ``qot_rowsum_wide`` / QOT_ROLE_SUM_ROWS: the B
    nodes of a table row in any order, whatever the grid;
  * source pass: ``myds = mya * (escr[2 p + 1] - delta[myi]) * rs`` (l. 584): a sum of two, a product, the factor (2);
    ``av = fma4(a, gr, av)``, ``ak = fma4(ds, qr, ak)`` (l. 608-609): chains of out-degree products with an input row.
csrc/tconv_rows.hip (the destination pass l. 87-251 has the same lines; what differs): ``sM[t] = rs * Mtab`` (l. 87: k = 2, the
``qe`` tree is the longer operand: the forward's count over rs (|scores| + <|q| |We|, |ea|>)); ``myda`` adds the D feature
products first and the value dot last (l. 196, 214: the same terms); ``sada``, ``p1``, ``p2`` are lane partials met by
``group_sum`` (l. 229-234: any order); ``escr[2 p + 1] = a * (da - sada)`` (l. 244); the slice's destinations of a row are added
in registers and LDS (l. 166, 236, 251, 266, 272, 290), the slices on the host here: B terms in any order.  The ``grad M``
image (l. 352-371): entry (r, c) is the exact sum of its addends ``rn(ds_e 2^k)`` read back as one fp32: per addend half a
quantum ``2^-k <= 2^-(61 - cb)`` of the slice's largest ``|ds_e|`` (cb: bit length of the slice's addend count, from the case),
one rounding of the result, and the slices' sum.
csrc/edge_grad.hip: ``u = group_sum(fmaf(we, q, u)) * rs`` (l. 68, 74), ``s = fmaf(qk, rs, su)`` (l. 100) and ``da = gv + sw``
(l. 101) have the terms of the destination pass in another order: the same counts plus 2; the softmax is the kernel's own
(online, l. 104-113: ``m`` off by ``b_s``, at most one rescale per edge: relative error of ``alpha``: ``expm1(2 b) + expm1(2 b_max)
+ (2 |s - m| + 2 spread + 4 deg + 2 C0) u``); ``delta = acc * inv`` (l. 114) carries the same; ``r = fmaf(ds, u, alpha * w)``
(l. 126).

Nothing here touches the GPU; every case and host reference is built once and shared."""
import functools
import math
import types
import zlib

import numpy as np
import torch

import gnn_qot_estimation_amd as q
import tconv_fwd_cases as T
from head_cases import C0, U, check_all, compare      # noqa: F401  (re-exported)
from oracle import dropout as OD

FORMS = ("node", "table", "scores", "tile", "rows", "graph")
PER_DST_FORMS = ("node", "table", "scores", "tile")
# Beside the per-element bounds the GPU test asserts the project's global figure ``max|got - ref| <= helpers.TOL max|ref|``.  In
# the sharp family (logit spread 40 .. 60, logits up to 7e3) that figure is out of reach of ANY fp32 evaluation for what is
# built on the cancelling difference ``ds = a (da - delta)``: the logit's own rounding (k 2^-24 A_s ~ 1e-3 .. 1e-2) moves ``a``
# by that much relatively, and ``da - delta`` is small next to either term.  The same chain in fp32 on the CPU misses it there
# (0.2 for grad_k in sharp_rows_h256_d1_b9; tests/test_tconv_bwd_cases_cpu.py prints the figures), so for these tensors the
# sharp cases assert the per-element bound alone; every other tensor and every other case keeps the global figure.
CANCELLING = ("ds", "pds", "gq", "gk", "gk_table", "grad_qkvs", "grad_qkvs_rows", "gwe", "gwe_rows", "gea", "gM", "gP", "grad_b")
WEDGE_GROUP = 128          # kWedgeGroup (csrc/tconv.hip l. 695): two levels of lin_edge partials above 2 x 128 workgroups


# ------------------------------------------------------------------ case table
def _cases():
    out = {name: dict(cfg) for name, cfg in T.CASES.items() if cfg["form"] in FORMS}
    # tile mode with two full groups of RPB graphs and a ragged third (the forward cases have B = RPB + 1)
    out["tile_h64_d4_b33"] = T._c("tile", 64, 4, 12, 2 * T.rpb(64) + 1, env=T._TILE)
    # 2 kWedgeGroup + 1 = 257 workgroups of qot_tconv_bwd_dst (node mode: N / RPB; H = 256 has RPB = 4, the fewest nodes:
    # N = 1027 in 85 graphs of 12 and one of 7), so that the two-level lin_edge sum runs
    out["node_h256_d1_wedge"] = T._c("node", 256, 1, None, None, N=4 * 2 * WEDGE_GROUP + 3)
    return out


CASES = _cases()


def forms_of(name):
    return (CASES[name]["form"],)


def env_of(name):
    """The forward's switches; the backward of a per-destination form never takes the row form."""
    cfg = CASES[name]
    return dict(cfg["env"]) if cfg["form"] in ("rows", "graph") else dict(cfg["env"], QOT_NO_TCONV_ROWS="1")


def out_classes(H):
    b = T.bt(H)
    return [0, 1, b - 1, b, b + 1, 2 * b + 1]


# ------------------------------------------------------------------ re-dealing the sources
def _redeal(n, ei, H, want, gen):
    """New sources for one graph (``ei`` local, in edge order).  Self loops stay (and count as out-edges); the other slots are dealt so
    that the nodes take the out-degrees at the head of ``want`` (a rotating list of ``out_classes``: what fits this graph is
    taken and moved to the tail), the rest at random to the nodes left without a class.  Then, by exchanging the sources of
    two slots (which keeps every degree): the smallest destination of in-degree >= 2 takes all its in-edges from the node of
    the largest out-degree, and the smallest source of out-degree >= 2 sends all its out-edges to one destination."""
    src, dst = ei[0].tolist(), ei[1].tolist()
    E = len(src)
    free = [e for e in range(E) if src[e] != dst[e]]
    loops = [sum(1 for e in range(E) if src[e] == dst[e] == r) for r in range(n)]        # they count as out-edges
    room, quota = len(free), {}
    for r in range(n - 1):                     # the last node stays without a class: it takes what is left
        for _ in range(len(want)):
            k = want[0] - loops[r]
            if 0 <= k <= room:
                quota[r] = k
                room -= k
                want.append(want.pop(0))
                break
            want.append(want.pop(0))
    rest = [r for r in range(n) if r not in quota]
    pool = [r for r, k in quota.items() for _ in range(k)]
    if room:
        assert rest, "no node left for the remaining edges"
        pool += [rest[int(k)] for k in torch.randint(0, len(rest), (room,), generator=gen)]
    perm = torch.randperm(len(pool), generator=gen).tolist()
    for slot, k in zip(free, perm):
        src[slot] = pool[k]

    def gather(node, dest):
        """Exchange sources until ``dest`` hears from ``node`` alone, or ``node`` has no out-edge left elsewhere."""
        inside = [e for e in free if dst[e] == dest and src[e] != node]
        outside = [e for e in free if dst[e] != dest and src[e] == node and e not in locked]
        while inside and outside:
            e1, e2 = inside.pop(), outside.pop()
            src[e1], src[e2] = src[e2], src[e1]
    locked = set()
    indeg = [sum(1 for e in range(E) if dst[e] == r) for r in range(n)]
    freedeg = [sum(1 for e in free if dst[e] == r) for r in range(n)]
    fo = [sum(1 for e in free if src[e] == r) for r in range(n)]
    d2 = y = None
    cand = [r for r in range(n) if indeg[r] >= 2 and freedeg[r] == indeg[r] and max(fo) >= indeg[r]]
    if cand:
        d2 = min(cand, key=lambda r: indeg[r])
        y = max(range(n), key=lambda r: fo[r])
        gather(y, d2)
        locked |= {e for e in free if dst[e] == d2}
    xs = [r for r in range(n) if r != y and not loops[r] and fo[r] >= 2
          and any(d != d2 and freedeg[d] >= fo[r] for d in range(n))]
    if xs:
        x = min(xs, key=lambda r: fo[r])
        gather(x, max((d for d in range(n) if d != d2), key=lambda d: freedeg[d]))
    return torch.tensor([src, dst], dtype=torch.long).view(2, -1)


def _csc(c):
    """Host CSC over the CSR slots (stable by source): ``slot`` of every out-edge, its position in the source's row."""
    col = c.ix.col
    slot = torch.argsort(col, stable=True)
    outdeg = torch.bincount(col, minlength=c.N)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), outdeg.cumsum(0)])
    pos = torch.arange(c.E) - ptr[col[slot]]
    return types.SimpleNamespace(slot=slot, outdeg=outdeg, ptr=ptr, pos=pos)


@functools.lru_cache(maxsize=None)
def bwd_case(name, cus=T.TRIP_CUS):
    cfg = CASES[name]
    f = T.tconv_case(name, cus) if name in T.CASES else T.build_case(name, cfg, cus)
    gen = torch.Generator().manual_seed(zlib.crc32(("bwd " + name).encode()))
    c = types.SimpleNamespace(**vars(f))
    H = c.H
    sharp = c.family == "sharp"
    one_graph = sharp and c.table_mode           # the forward repeats one graph: a table row has ONE spread
    want = out_classes(H)
    graphs, first = [], None
    for g in range(f.B):
        lo, hi = int(f.batch.edge_ptr[g]), int(f.batch.edge_ptr[g + 1])
        n = int(f.batch.ptr[g + 1] - f.batch.ptr[g])
        ei = f.ei[:, lo:hi] - int(f.batch.ptr[g])
        if hi > lo:
            if one_graph and first is not None:
                ei = first.clone()
            else:
                ei = _redeal(n, ei, H, want, gen)
                first = first if first is not None else ei
        graphs.append(q.Data(edge_index=ei.clone(), edge_attr=f.edge_attr[lo:hi].clone(), node_ids=torch.arange(n), num_nodes=n))
    c.batch = q.Batch.from_data_list(graphs)
    c.ei, c.edge_attr = c.batch.edge_index, c.batch.edge_attr
    assert torch.equal(c.ei[1], f.ei[1]) and torch.equal(c.edge_attr, f.edge_attr)      # destinations, order and features stay
    c.ix = T._index(c.ei, c.N)
    c.csc = _csc(c)
    if sharp:
        # the spread 40 .. 60 of the family, again: q's rows are scaled (a positive factor per row)
        _, spread = T._logits64(c, c.qkvs)
        per_row = torch.zeros(c.V, dtype=torch.float64).scatter_reduce(0, c.rows, spread, "amax")
        target = 42.0 + 16.0 * torch.rand(c.V, generator=gen, dtype=torch.float64)
        fac = torch.where(per_row > 0, target / per_row.clamp_min(1e-30), torch.ones((), dtype=torch.float64))
        c.qkvs = c.qkvs.clone()
        c.qkvs[:, :H] = (c.qkvs[:, :H].double() * fac[:, None]).float()
    _, c.spread = T._logits64(c, c.qkvs)
    c.g = torch.randn(c.N, H, generator=gen)
    graph_form = cfg["form"] == "graph"
    fwd = T._evaluate(c, torch.float64, lookup=T.host_lookup(c, "graph") if graph_form else None)
    # host stand-ins of what the product's forward saves
    c.stats = T.stats_of(fwd).float()
    c.y = fwd["out"].float()
    if graph_form:
        c.alpha, c.aa = fwd["alpha"].float(), fwd["aa"].float()
    if c.E:
        assert not torch.equal(c.ix.eid, torch.arange(c.E)), name
        assert bool((c.ei[0] == c.ei[1]).any()), name
        assert torch.unique(c.ei, dim=1).shape[1] < c.E, name
    if sharp:
        assert float(c.spread.max()) <= 60.0 and float(c.spread[c.ix.deg >= 2].min()) >= 40.0, (name, c.spread)
    elif c.E:
        assert float(c.spread.max()) <= 16.0, (name, float(c.spread.max()))
    return c


def planted(c):
    """What the re-deal planted: the out-degrees present, the destinations (in-degree >= 2) fed by one source alone, the
    sources (out-degree >= 2) that feed one destination alone."""
    ix, N = c.ix, c.N
    lo = torch.full((N,), c.N, dtype=torch.long).scatter_reduce(0, ix.row, ix.col, "amin")
    hi = torch.full((N,), -1, dtype=torch.long).scatter_reduce(0, ix.row, ix.col, "amax")
    lo_t = torch.full((N,), c.N, dtype=torch.long).scatter_reduce(0, ix.col, ix.row, "amin")
    hi_t = torch.full((N,), -1, dtype=torch.long).scatter_reduce(0, ix.col, ix.row, "amax")
    return types.SimpleNamespace(outdeg=set(c.csc.outdeg.tolist()),
                                 one_source=torch.nonzero((ix.deg >= 2) & (lo == hi)).view(-1),
                                 one_destination=torch.nonzero((c.csc.outdeg >= 2) & (lo_t == hi_t)).view(-1))


def host_stage(c):
    st = dict(m=c.stats[:, 0], denom=c.stats[:, 1], y=c.y, g=c.g)
    if c.cfg["form"] == "graph":          # the graph form's backward reads the forward's weights and sum alpha ea, not stats
        st.update(alpha=c.alpha, aa=c.aa)
    return st


def host_scores(c):
    return T.host_lookup(c, "scores")


# ------------------------------------------------------------------ the chain, in any dtype
DEFECTS = {
    "delta_left_out": "ds = a da",
    "grad_k_unscaled": "1 / sqrt(H) left off grad_k",
    "grad_q_edge_term_unscaled": "1 / sqrt(H) left off the We term of grad_q",
    "da_edge_term_missing": "We ea_e left out of da",
    "grad_w_edge_q_term_missing": "rs q (x) pd left out of grad_w_edge",
    "grad_w_edge_g_term_missing": "g (x) p2 left out of grad_w_edge",
    "slope_from_sign_of_g": "the leaky-ReLU slope chosen from the sign of g instead of y",
    "mask_numbered_at_table_row": "the dropout index taken from the table row",
    "features_by_slot": "ea read at the CSR slot instead of eid[slot]",
    "dst_edge_at_bt_dropped": "the in-edge at CSR position BT dropped in the destination pass",
    "src_edge_at_bt_dropped": "the out-edge at CSC position BT dropped in the source pass",
    "src_reads_escr_at_csc_slot": "the source pass reads escr at its CSC slot instead of pos_t[slot]",
    "tile_last_group_dropped": "the last, ragged group of graphs dropped from the tile-mode table sum",
    "colf_is_node": "the node index instead of the table row of the source",
    "weight_off_1e-4": "one attention weight per destination multiplied by 1 + 1e-4",
}


def _segsum(x, row, N):
    return torch.zeros((N,) + tuple(x.shape[1:]), dtype=x.dtype).index_add_(0, row, x)


def _evaluate(c, dtype, stage=None, defect=None, scores=None, src_stage=None):
    """The backward chain in plain tensor operations in ``dtype`` from the stage inputs (``stage``: m, denom, y, g; default
    ``host_stage``); per CSR slot: s, a, da, ds; per node: delta, pds, pal, gq, gk, gv, gskip; ``grad_qkvs`` as autograd
    returns it ([N, 4H], or [V, 4H] summed over the graphs), ``gwe`` [H, D], ``gea`` [E, D] in edge order; row form (``scores``
    given: the dense part of the logit looked up): gM [n, n], gP [n, D], gTs, gTv [n, H], gwe_g.  ``src_stage``: the source
    pass alone from given (a, da or ds, delta, gskip)."""
    assert defect is None or defect in DEFECTS
    st = stage if stage is not None else host_stage(c)
    H, D, N, ix = c.H, c.D, c.N, c.ix
    t, we, ea = c.qkvs.to(dtype), c.w_edge.to(dtype), c.edge_attr.to(dtype)
    m, denom, g = st["m"].to(dtype), st["denom"].to(dtype), st["g"].to(dtype)
    rs = 1.0 / math.sqrt(H)
    rows = c.rows
    ri = rows[ix.row]
    rj = (ix.col % c.V) if defect == "colf_is_node" else rows[ix.col]
    e = ea[torch.arange(c.E)] if defect == "features_by_slot" else ea[ix.eid]
    tq, tk, tv = t[:, :H], t[:, H:2 * H], t[:, 2 * H:3 * H]
    keep = c.keep
    if defect == "mask_numbered_at_table_row":
        keep = OD.keep_mask(c.seed, c.step, (c.V, H), c.p)[rows]
    sign = g if defect == "slope_from_sign_of_g" else st["y"]
    one = torch.ones((), dtype=dtype)
    gi = g * (keep.to(dtype) * c.ks) * torch.where(sign > 0, one, one * T.SLOPE32)
    qe, ge = (tq @ we) * rs, gi @ we
    dense = scores.to(dtype)[ri, rj] if scores is not None else (tq[ri] * tk[rj]).sum(-1)
    s = dense * rs + (qe[ri] * e).sum(-1)
    a = st["alpha"].to(dtype) if "alpha" in st else (s - m[ix.row]).exp() / denom[ix.row]
    if defect == "weight_off_1e-4":
        a = torch.where((ix.pos == 0) & (ix.deg[ix.row] >= 2), a * (1 + 1e-4), a)
    da = (gi[ix.row] * tv[rj]).sum(-1)
    if defect != "da_edge_term_missing":
        da = da + (ge[ix.row] * e).sum(-1)
    live = (ix.pos != T.bt(H)) if defect == "dst_edge_at_bt_dropped" else torch.ones(c.E, dtype=torch.bool)
    al = a * live.to(dtype)
    ada = al * da
    delta = _segsum(ada, ix.row, N)
    p1, p2 = _segsum(ada[:, None] * e, ix.row, N), _segsum(al[:, None] * e, ix.row, N)
    a1, a2 = _segsum(ada[:, None] * tk[rj], ix.row, N), _segsum(al[:, None] * tk[rj], ix.row, N)
    dl = delta if defect != "delta_left_out" else torch.zeros_like(delta)
    p2u = st["aa"].to(dtype) if "aa" in st else p2          # the graph form reads the forward's ``aa`` here
    pd = p1 - dl[:, None] * p2u
    edge_term = pd @ we.t()
    if defect == "grad_q_edge_term_unscaled":
        edge_term = edge_term * math.sqrt(H)
    gq = ((a1 - dl[:, None] * a2) + edge_term) * rs
    ds = al * (da - dl[ix.row])
    # source pass: over the out-edges, from what the destination pass left (or from given bits)
    if src_stage is not None:
        a_s, da_s, dl_s, gi_s = (src_stage[k].to(dtype) for k in ("a", "da", "delta", "gskip"))
    else:
        a_s, da_s, dl_s, gi_s = al, da, dl, gi
    if defect == "src_reads_escr_at_csc_slot":
        wrong = torch.empty(c.E, dtype=torch.long)
        wrong[c.csc.slot] = torch.arange(c.E)                # the out-edge's own CSC index, used as a CSR slot
        a_s, da_s = a_s[wrong], da_s[wrong]
    dss = a_s * (da_s - dl_s[ix.row]) * rs
    lsrc = torch.ones(c.E, dtype=dtype)
    if defect == "src_edge_at_bt_dropped":
        lsrc[c.csc.slot[c.csc.pos == T.bt(H)]] = 0
    gk = _segsum((dss * lsrc)[:, None] * tq[ri], ix.col, N)
    if defect == "grad_k_unscaled":
        gk = gk * math.sqrt(H)
    gv = _segsum((a_s * lsrc)[:, None] * gi_s[ix.row], ix.col, N)
    gnode = torch.cat([gq, gk, gv, gi], 1)
    if c.table_mode:
        w = torch.ones(N, dtype=dtype)
        if defect == "tile_last_group_dropped" and c.B % T.rpb(H):
            w[(c.B // T.rpb(H)) * T.rpb(H) * c.n:] = 0
        grad_qkvs = _segsum(gnode * w[:, None], rows, c.V)
    else:
        grad_qkvs = gnode
    gwe_q = (tq[rows] * rs).t() @ pd
    gwe_g = gi.t() @ p2u
    gwe = (0 if defect == "grad_w_edge_q_term_missing" else gwe_q) + (0 if defect == "grad_w_edge_g_term_missing" else gwe_g)
    gea_slot = ds[:, None] * qe[ri] + al[:, None] * ge[ix.row]
    gea = torch.zeros(c.E, D, dtype=dtype).index_copy_(0, ix.eid, gea_slot)
    res = dict(s=s, a=al, da=da, ds=ds, delta=delta, pds=pd, pal=p2, gq=gq, gk=gk, gv=gv, gskip=gi, grad_qkvs=grad_qkvs,
               gwe=gwe, gea=gea)
    if scores is not None or "alpha" in st:           # the table-level sums (node r of every graph is table row r)
        n = c.n
        res["gM"] = torch.zeros(n * n, dtype=dtype).index_add_(0, ri * n + rj, ds).view(n, n)
        res["gP"] = _segsum(pd, rows, n)
        res["gTs"] = _segsum(gi, rows, n)
        res["gTv"] = _segsum(gv, rows, n)
        res["gwe_g"] = gwe_g
    return res


# ------------------------------------------------------------------ bounds: (mag, b) pairs
def _inp(x):
    x = x.double().abs()
    return x, torch.zeros_like(x)


def _mul(x, y, extra=1.0):
    mag = x[0] * y[0]
    return mag, x[1] * y[0] + x[0] * y[1] + extra * U * mag


def _scale(x, factor, extra=2.0):
    """Times a constant that is itself rounded (rsqrtf): the factor and the product."""
    return x[0] * factor, x[1] * factor + extra * U * x[0] * factor


def _seg(x, index, N, terms):
    """Sum per segment, ``terms`` addends (a tensor per segment, or a number) in any order."""
    mag = _segsum(x[0], index, N)
    n1 = (torch.as_tensor(terms, dtype=torch.float64) - 1).clamp_min(0)
    n1 = n1.view(-1, *([1] * (mag.dim() - 1))) if n1.dim() else n1
    return mag, _segsum(x[1], index, N) + n1 * U * mag


def _add(*xs):
    mag = sum(x[0] for x in xs)
    return mag, sum(x[1] for x in xs) + (len(xs) - 1) * U * mag


def _bc(x, idx=None, col=False):
    """Index / broadcast both members alike."""
    if idx is not None:
        x = (x[0][idx], x[1][idx])
    return (x[0][:, None], x[1][:, None]) if col else x


def reference(c, form, stage=None, scores=None, src_stage=None, slices=None):
    """``{quantity: dict(value, bound, k, A)}`` in fp64 for case ``c``: the chain from ``stage`` (default: the host's).  Row
    form: ``scores`` (the kernel's own, else the host's), ``slices``: the slice's addend counts for the ``grad M`` image (list of
    per-(slice, row) counts, default one slice).  ``src_stage``: the source pass alone, from the destination pass's bits."""
    assert form in FORMS
    st = stage if stage is not None else host_stage(c)
    if form == "rows" and scores is None:
        scores = host_scores(c)
    if form != "rows":
        scores = None
    r = _evaluate(c, torch.float64, st, scores=scores)
    H, D, N, ix = c.H, c.D, c.N, c.ix
    f64 = torch.float64
    rs = 1.0 / math.sqrt(H)
    rows = c.rows
    ri, rj = rows[ix.row], rows[ix.col]
    deg, outdeg = ix.deg.double(), c.csc.outdeg.double()
    t = c.qkvs.double().abs()
    tq, tk, tv = t[:, :H], t[:, H:2 * H], t[:, 2 * H:3 * H]
    we = c.w_edge.double().abs()
    e = c.edge_attr.double().abs()[ix.eid]
    qs = _scale(_inp(c.qkvs[:, :H]), rs)                                  # rs q, per table row
    gi = (r["gskip"].abs(), 2 * U * r["gskip"].abs())
    dense = scores.double().abs()[ri, rj] if scores is not None else (tq[ri] * tk[rj]).sum(-1)
    a_s = rs * (dense + ((tq @ we)[ri] * e).sum(-1))
    kl = float(T.logit_count("node", H, D))
    b_s = kl * U * a_s
    x = (r["s"] - st["m"].double()[ix.row]).abs()
    a = (r["a"], r["a"] * (torch.expm1(b_s) + (2 * x + C0) * U))
    a_da = (gi[0][ix.row] * tv[rj]).sum(-1) + ((gi[0] @ we)[ix.row] * e).sum(-1)
    da = (r["da"].abs(), kl * U * a_da)
    ada = _mul(a, da)
    delta = _seg(ada, ix.row, N, deg)
    ein, kin = _inp(c.edge_attr[ix.eid]), _inp(c.qkvs[:, H:2 * H][rj])
    p1 = _seg(_mul(_bc(ada, col=True), ein, 0.0), ix.row, N, deg + 1)     # fma: the addition rounds, once per term
    p2 = _seg(_mul(_bc(a, col=True), ein, 0.0), ix.row, N, deg + 1)
    a1 = _seg(_mul(_bc(ada, col=True), kin, 0.0), ix.row, N, deg + 1)
    a2 = _seg(_mul(_bc(a, col=True), kin, 0.0), ix.row, N, deg + 1)
    dcol = _bc(delta, col=True)
    pd = _add(p1, _mul(dcol, p2))
    rr = _add(a1, _mul(dcol, a2))
    wterm = (pd[0] @ we.t(), pd[1] @ we.t() + D * U * (pd[0] @ we.t()))       # D products with an input, on rc's chain
    gq = _scale(_add(rr, wterm), rs)
    sub = _add(da, _bc(delta, ix.row))
    ds = _mul(a, sub)
    # source pass
    if src_stage is not None:
        rsrc = _evaluate(c, f64, st, scores=scores, src_stage=src_stage)
        sa, sda, sdl, sgi = (_inp(src_stage[k]) for k in ("a", "da", "delta", "gskip"))
        dss = _scale(_mul(sa, _add(sda, _bc(sdl, ix.row))), rs)
    else:
        rsrc, sa, sgi = r, a, gi
        dss = _scale(ds, rs)
    gk = _seg(_mul(_bc(dss, col=True), _inp(c.qkvs[:, :H][ri]), 0.0), ix.col, N, outdeg + 1)
    gv = _seg(_mul(_bc(sa, col=True), _bc(sgi, ix.row), 0.0), ix.col, N, outdeg + 1)
    per_row = torch.bincount(rows, minlength=c.V).double()

    def table(xnode):
        return _seg(xnode, rows, c.V, per_row) if c.table_mode else xnode
    parts = [table(gq), table(gk), table(gv), table(gi)]
    grad_qkvs = (torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1))
    # lin_edge: per node two products and a sum of two, then N terms in any order
    qn = _bc(qs, rows)
    wq = (qn[0].t() @ pd[0], qn[1].t() @ pd[0] + qn[0].t() @ pd[1] + U * (qn[0].t() @ pd[0]))
    wg = (gi[0].t() @ p2[0], gi[1].t() @ p2[0] + gi[0].t() @ p2[1] + U * (gi[0].t() @ p2[0]))
    gwe_mag = wq[0] + wg[0]
    gwe = (gwe_mag, wq[1] + wg[1] + (N + 1) * U * gwe_mag)
    gweg = (wg[0], wg[1] + (N + 1) * U * wg[0])

    out = {}

    def put(name, value, pair):
        mag, b = pair
        k = torch.where(mag > 0, b / (U * mag.clamp_min(1e-300)), torch.zeros((), dtype=f64))
        assert bool((mag * (1 + 1e-9) + 1e-300 >= value.abs()).all()), name
        k = k if k.numel() else torch.zeros((), dtype=f64)
        out[name] = dict(value=value, bound=b, k=k, A=mag)
    put("a", r["a"], a)
    put("da", r["da"], da)
    put("delta", r["delta"], delta)
    put("pds", r["pds"], pd)
    put("pal", r["pal"], p2)
    put("gq", r["gq"], gq)
    put("gskip", r["gskip"], gi)
    put("gk", rsrc["gk"], gk)
    put("gv", rsrc["gv"], gv)
    if c.table_mode:             # tile mode leaves the source pass's rows summed over the graphs
        put("gk_table", _segsum(rsrc["gk"], rows, c.V), table(gk))
        put("gv_table", _segsum(rsrc["gv"], rows, c.V), table(gv))
    put("ds", r["ds"], ds)
    if src_stage is None:
        put("grad_qkvs", r["grad_qkvs"], grad_qkvs)
        put("gwe", r["gwe"], gwe)
        # the edge-feature gradient: csrc/edge_grad.hip, its own online softmax
        sp = c.spread[ix.row]
        bmax = torch.zeros(N, dtype=f64).scatter_reduce(0, ix.row, (kl + 2) * U * a_s, "amax")[ix.row]
        rel = torch.expm1(2 * (kl + 2) * U * a_s) + torch.expm1(2 * bmax) + (2 * x + 2 * sp + 4 * deg[ix.row] + 2 * C0) * U
        al = (r["a"], r["a"] * rel)
        dae = (r["da"].abs(), (kl + 2) * U * a_da)
        dle = _seg(_mul(al, dae), ix.row, N, 4 * deg + C0)
        dse = _mul(al, _add(dae, _bc(dle, ix.row)))
        u_ = (rs * (tq @ we), (H + 3) * U * rs * (tq @ we))
        w_ = (gi[0] @ we, (H + 3) * U * (gi[0] @ we))
        gslot = _add(_mul(_bc(dse, col=True), _bc(u_, ri), 0.0), _mul(_bc(al, col=True), _bc(w_, ix.row)))
        gea = tuple(torch.zeros(c.E, D, dtype=f64).index_copy_(0, ix.eid, z) for z in gslot)
        put("gea", r["gea"], gea)
    if form == "rows" and src_stage is None:
        n = c.n
        # grad M: per slice the exact sum of rn(ds 2^k) read back as fp32; quantum <= 2^-(61 - cb) of the slice's max |ds|
        gm_mag = torch.zeros(n * n, dtype=f64).index_add_(0, ri * n + rj, ds[0]).view(n, n)
        gm_b = torch.zeros(n * n, dtype=f64).index_add_(0, ri * n + rj, ds[1]).view(n, n)
        addends = torch.zeros(n * n, dtype=f64).index_add_(0, ri * n + rj, torch.ones(c.E, dtype=f64)).view(n, n)
        row_addends = torch.zeros(n, dtype=f64).index_add_(0, ri, torch.ones(c.E, dtype=f64))
        cb = torch.floor(torch.log2(row_addends.clamp_min(1))) + 1            # least favourable: the whole batch in one slice
        dmax = torch.zeros(n, dtype=f64).scatter_reduce(0, ri, ds[0] + ds[1], "amax")
        quantum = 2 * dmax * torch.pow(torch.tensor(2.0, dtype=f64), -(61 - cb))       # max |ds| < 2^(eb - 126) <= 2 max
        nsl = float(slices or 1)
        gm_b = gm_b + 0.5 * addends * quantum[:, None] + (1 + nsl) * U * gm_mag
        put("gM", r["gM"], (gm_mag, gm_b))
        put("gP", r["gP"], _seg(pd, rows, n, per_row[:n]))
        put("gTs", r["gTs"], _seg(gi, rows, n, per_row[:n]))
        put("gwe_g", r["gwe_g"], gweg)
        # what autograd returns in the row form: grad T_q = rs (grad M T_k + grad P We^T) (qot_gemm_nt_planes: the npad + D
        # live columns of one product, in any order), grad T_k = rs grad M^T T_q (qot_gemm_tn_planes: n addends), grad T_v and
        # grad T_skip as summed; grad_w_edge = gwe_g + rs T_q^T grad P (_small_gemm: n addends); C0 for the factors
        gP, gTs, gTv = (_seg(z, rows, n, per_row[:n]) for z in (pd, gi, gv))
        npad = (n + 31) // 32 * 32
        gq_mag = rs * (gm_mag @ tk[:n] + gP[0] @ we.t())
        gq_b = rs * (gm_b @ tk[:n] + gP[1] @ we.t()) + (npad + D + C0) * U * gq_mag
        gk_mag = rs * (gm_mag.t() @ tq[:n])
        gk_b = rs * (gm_b.t() @ tq[:n]) + (n + C0) * U * gk_mag
        put("grad_qkvs_rows", r["grad_qkvs"], (torch.cat([gq_mag, gk_mag, gTv[0], gTs[0]], 1),
                                               torch.cat([gq_b, gk_b, gTv[1], gTs[1]], 1)))
        wq_mag = rs * (tq[:n].t() @ gP[0])
        put("gwe_rows", r["gwe"], (gweg[0] + wq_mag, gweg[1] + rs * (tq[:n].t() @ gP[1]) + (n + C0) * U * wq_mag
                                   + U * (gweg[0] + wq_mag)))
    if form == "rows":
        put("gTv", rsrc["gTv"], _seg(gv, rows, c.n, per_row[:c.n]))
    out["isolated"] = ix.deg == 0
    out["no_out"] = c.csc.outdeg == 0
    return out


@functools.lru_cache(maxsize=None)
def host_reference(name, cus=T.TRIP_CUS):
    c = bwd_case(name, cus)
    return reference_graph(c) if c.cfg["form"] == "graph" else reference(c, c.cfg["form"])


def escr_of(res, second="da"):
    """``[E, 2]`` as the destination pass leaves it."""
    return torch.stack([res["a"], res[second]], 1)


# ------------------------------------------------------------------ the graph form (csrc/tconv_graph.hip, tconv_bwd_graph_kernel)
def reference_graph(c, stage=None):
    """The summed partial row of ``qot_tconv_bwd_graph`` -- gTv [n, H], gTs [n, H], gM [n, n], gP [n, D], gwe_g [H, D] (the value
    path's share) -- from its stage inputs: ``g``, ``y``, the value rows of ``t4``, ``w_edge`` and the forward's ``alpha``,
    ``ea_csr``, ``aa`` (fp32 bits; alpha is NOT recomputed).  Counts, with the lines of csrc/tconv_graph.hip:
      * ``gi`` behind the activation (l. 450): k = 2;
      * ``da`` (l. 479-481, 540): H products of ``gi`` with a value row on four chains, ``ge`` (l. 493-495) likewise with We,
        D products of ``ge`` with a feature: k = H + D + 3 over <|g|, |v|> + <|g| |We|, |ea|>;
      * ``ada = sAl[p] * da`` (l. 542), ``sada`` over the quad's lanes and two DPP steps (l. 543-548): deg terms, any order;
      * ``ds = sAl[p] * (sDa[p] - sada)`` added into the LDS image by ``atomicAdd`` (l. 550): the entry's addends of the whole
        batch in any order (the image lives across the workgroup's graphs; the partial rows are summed afterwards);
      * ``sGP += q - sada * sAa`` (l. 545-556): p1 a chain of deg products, a product, a sum of two; the B graphs in any order;
      * ``gTs`` (l. 454), ``gTv`` (l. 513-516: chains of out-degree products), ``wc = fmaf(gc, ad, wc)`` (l. 522; N terms)."""
    st = stage if stage is not None else host_stage(c)
    r = _evaluate(c, torch.float64, st)
    H, D, N, n, ix = c.H, c.D, c.N, c.n, c.ix
    f64 = torch.float64
    rows = c.rows
    ri, rj = rows[ix.row], rows[ix.col]
    deg, outdeg = ix.deg.double(), c.csc.outdeg.double()
    tv = c.qkvs.double().abs()[:, 2 * H:3 * H]
    we = c.w_edge.double().abs()
    e = c.edge_attr.double().abs()[ix.eid]
    gi = (r["gskip"].abs(), 2 * U * r["gskip"].abs())
    a_da = (gi[0][ix.row] * tv[rj]).sum(-1) + ((gi[0] @ we)[ix.row] * e).sum(-1)
    da = (r["da"].abs(), (H + D + 3) * U * a_da)
    al = _inp(st["alpha"])
    ada = _mul(al, da)
    delta = _seg(ada, ix.row, N, deg)
    ds = _mul(al, _add(da, _bc(delta, ix.row)))
    key = ri * n + rj
    gm_mag = torch.zeros(n * n, dtype=f64).index_add_(0, key, ds[0]).view(n, n)
    addends = torch.zeros(n * n, dtype=f64).index_add_(0, key, torch.ones(c.E, dtype=f64)).view(n, n)
    gm_b = torch.zeros(n * n, dtype=f64).index_add_(0, key, ds[1]).view(n, n) + (addends - 1).clamp_min(0) * U * gm_mag
    ein = _inp(c.edge_attr[ix.eid])
    p1 = _seg(_mul(_bc(ada, col=True), ein, 0.0), ix.row, N, deg + 1)
    pd = _add(p1, _mul(_bc(delta, col=True), _inp(st["aa"])))
    per_row = torch.bincount(rows, minlength=c.V).double()[:n]
    gv = _seg(_mul(_bc(al, col=True), _bc(gi, ix.row), 0.0), ix.col, N, outdeg + 1)
    aa = st["aa"].double().abs()
    wg_mag = gi[0].t() @ aa
    out = {}

    def put(name, value, pair):
        mag, b = pair
        k = torch.where(mag > 0, b / (U * mag.clamp_min(1e-300)), torch.zeros((), dtype=f64))
        assert bool((mag * (1 + 1e-9) + 1e-300 >= value.abs()).all()), name
        out[name] = dict(value=value, bound=b, k=k if k.numel() else torch.zeros((), dtype=f64), A=mag)
    put("gM", r["gM"], (gm_mag, gm_b))
    put("gP", r["gP"], _seg(pd, rows, n, per_row))
    put("gTs", r["gTs"], _seg(gi, rows, n, per_row))
    put("gTv", r["gTv"], _seg(gv, rows, n, per_row))
    gweg = (wg_mag, gi[1].t() @ aa + N * U * wg_mag)
    put("gwe_g", r["gwe_g"], gweg)
    # what the product returns behind qot_table_project_bwd_scores that does not depend on the projection weights: the
    # bias gradients (column sums of the table gradient's row [grad T_q | grad T_k | grad T_v | grad T_skip]) and
    # grad_w_edge = gwe_g + rs T_q^T gP (``project_bwd_reference`` has the counts)
    rs = 1.0 / math.sqrt(H)
    tq, tk = c.qkvs.double().abs()[:n, :H], c.qkvs.double().abs()[:n, H:2 * H]
    gP, gTs, gTv = (_seg(z, rows, n, per_row) for z in (pd, gi, gv))
    q_mag = rs * (gm_mag @ tk + gP[0] @ we.t())
    q_b = rs * (gm_b @ tk + gP[1] @ we.t()) + (n + D + 2) * U * q_mag
    k_mag = rs * (gm_mag.t() @ tq)
    k_b = rs * (gm_b.t() @ tq) + (n + D + 2) * U * k_mag
    g4 = (torch.cat([q_mag, k_mag, gTv[0], gTs[0]], 1), torch.cat([q_b, k_b, gTv[1], gTs[1]], 1))
    put("grad_b", r["grad_qkvs"][:n].sum(0), (g4[0].sum(0), g4[1].sum(0) + (n + C0) * U * g4[0].sum(0)))
    wq_mag = rs * (tq.t() @ gP[0])
    put("gwe", r["gwe"], (gweg[0] + wq_mag, gweg[1] + rs * (tq.t() @ gP[1]) + (n + 2 + C0) * U * (gweg[0] + wq_mag)))
    out["no_out_rows"] = torch.zeros(n, dtype=f64).index_add_(0, rows, outdeg) == 0
    return out


def project_bwd_reference(pc, S, t4, n_layout):
    """``qot_table_project_bwd_scores`` (csrc/tconv_graph_dev.hpp, ``table_project_bwd_scores_body``) from ITS inputs: the summed
    row ``S`` (fp32 bits, layout ``n_layout = (ldm, off_gv, off_gs, off_gm, off_gp, off_gwe)``), ``t4``, the table, the four
    weights and ``w_edge``: plain dot products.  The row of the table gradient (l. 179-193, 234-247): q column n + D terms
    and the factor, k column n terms and the factor (k = n + D + 2); ``grad_w`` / ``grad_b`` (l. 199-221): n terms;
    ``grad_table`` (l. 251-271): 4H terms; ``grad_w_edge`` (l. 296-297): n terms, the factor, one more; C0 once for the
    factors.  Every bound is built on the operands' magnitudes, so the key bias's gradient (analytically zero) needs no
    floor of its own."""
    H, D, n, V = pc.H, pc.D, pc.n, pc.V
    ldm, off_gv, off_gs, off_gm, off_gp, off_gwe = n_layout
    f64 = torch.float64
    rs = 1.0 / math.sqrt(H)
    S = S.double()
    gTv, gTs = S[off_gv:off_gv + n * H].view(n, H), S[off_gs:off_gs + n * H].view(n, H)
    gM = S[off_gm:off_gm + n * ldm].view(n, ldm)[:, :n]
    gP = S[off_gp:off_gp + n * D].view(n, D)
    gwe_g = S[off_gwe:off_gwe + H * D].view(H, D)
    t4 = t4.double()
    tq, tk = t4[:n, :H], t4[:n, H:2 * H]
    sd = {k: v.double() for k, v in pc.state.items()}
    we = sd["lin_edge.weight"]
    w4 = torch.cat([sd[f"{k}.weight"] for k in T._LINS], 0)
    tab = pc.table.double()
    g4 = torch.cat([rs * (gM @ tk + gP @ we.t()), rs * (gM.t() @ tq), gTv, gTs], 1)
    a4 = torch.cat([rs * (gM.abs() @ tk.abs() + gP.abs() @ we.abs().t()), rs * (gM.abs().t() @ tq.abs()), gTv.abs(), gTs.abs()], 1)
    k4 = torch.cat([torch.full((n, 2 * H), float(n + D + 2)), torch.zeros(n, 2 * H)], 1).double()
    b4 = k4 * U * a4
    val = dict(grad_w=g4.t() @ tab[:n], grad_b=g4.sum(0), grad_w_edge=gwe_g + rs * (tq.t() @ gP),
               grad_table=torch.cat([g4 @ w4, torch.zeros(V - n, H, dtype=f64)], 0))
    mag = dict(grad_w=a4.t() @ tab[:n].abs(), grad_b=a4.sum(0), grad_w_edge=gwe_g.abs() + rs * (tq.abs().t() @ gP.abs()),
               grad_table=torch.cat([a4 @ w4.abs(), torch.zeros(V - n, H, dtype=f64)], 0))
    b = dict(grad_w=b4.t() @ tab[:n].abs() + (n + C0) * U * mag["grad_w"], grad_b=b4.sum(0) + (n + C0) * U * mag["grad_b"],
             grad_w_edge=(n + 2 + C0) * U * mag["grad_w_edge"],
             grad_table=torch.cat([b4 @ w4.abs(), torch.zeros(V - n, H, dtype=f64)], 0) + (4 * H + C0) * U * mag["grad_table"])
    ref = {}
    for k in val:
        kk = torch.where(mag[k] > 0, b[k] / (U * mag[k].clamp_min(1e-300)), torch.zeros((), dtype=f64))
        ref[k] = dict(value=val[k], bound=b[k], k=kk, A=mag[k])
    return ref


def check(c, tag, got, ref, names, tol):
    """``check_all`` with the global figure ``tol``; in the sharp family without it for the tensors of ``CANCELLING``."""
    if c.family != "sharp":
        return check_all(tag, got, ref, names, global_tol=tol)
    firm = tuple(k for k in names if k not in CANCELLING)
    figs = check_all(tag, got, ref, firm, global_tol=tol) if firm else {}
    rest = tuple(k for k in names if k in CANCELLING)
    if rest:
        figs.update(check_all(tag + " (per element only)", got, ref, rest, global_tol=float("inf")))
    return figs
