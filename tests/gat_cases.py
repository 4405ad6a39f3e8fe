"""Cases, fp64 restatement and per-element error bounds of GATConv's kernels (tests/test_gat_cases_cpu.py,
tests/test_gpu_gat_kernels.py): everything in csrc/gat.hip that LightpathGNN runs -- ``gat_logits_kernel``, the forward walk
``gat_fwd_kernel``, the two backward walks ``gat_bwd_dst_kernel`` / ``gat_bwd_src_kernel`` and ``gat_att_grad_kernel``, in the
dense form (``functional.GatFn``: ``z`` is read) and in the thin form (``functional.GatThinFn``: ``z = x W^T`` formed in
registers from K <= 8 features).  heads = 4 throughout (the only dispatched value).

Every stage is judged on exactly the fp32 bits it reads:
  * logits: ``a_src, a_dst`` of ``qot_gat_logits`` from ``z, att_src, att_dst`` (``logits_reference``);
  * dense forward: ``out`` and ``stats = (m, denom)`` from ``z``, the logits HANDED IN (``GatFn.apply(..., a_src=, a_dst=)``),
    ``bias`` and the index;
  * thin forward: the same from ``x [N, K]``, ``W [4C, K]`` and the logits the kernels themselves used (``logits_sink``);
    those are products of ``qot_skinny_linear_fwd`` with a bound of their own (``thin_logits_reference``);
  * backward: fp64 autograd of the same chain from the same stage inputs and a fixed cotangent ``g``; the logits keep the
    value handed in and the derivative of ``<z[n, h, :], att[h, :]>`` (what the kernels do: "their gradient still returns
    through grad_z").  Dense: ``grad_z, grad_att_src, grad_att_dst, grad_bias``; thin: ``grad_lin`` in place of ``grad_z``.

Companions as in tests/head_cases.py: a magnitude ``A >= |value|`` and a count ``k``; the assertion is ``|got - ref| <=
k 2^-24 A`` per element (``head_cases.compare`` / ``check_all``).  A sum of n operands in ANY order counts
``max k_i + n - 1`` over ``sum A_i``, a product ``k_x + k_y + 1`` over ``A_x A_y``, a stage input has ``k = 0``.  The counts,
as read from csrc/gat.hip (u = 2^-24):

  * ``gat_logits_kernel``: ``group_sum<LPH>(dot4(zv, att))``: ``dot4`` rounds one product and three ``fmaf`` (4), the
    butterfly adds ``log2 LPH`` times: k = 4 + log2(LPH) over A = <|z|, |att|>, LPH = min(C / 4, TPR) lanes per head.
  * thin logits (``GatThinFn.forward``): ``v = sum_c W[h, c, :] att[h, c]`` is a C-term sum left to the library (any order:
    C), then ``qot_skinny_linear_fwd``'s K-term chain: k = C + K + C0 over A = <|x|, sum_c |W| |att|>.
  * ``z`` in the thin kernels (``thin_form``): K ``fmaf`` on one chain from 0: k_z = K over A_z = <|x|, |W|>; dense: k_z = 0,
    A_z = |z|.
  * ``raw = a_src[j] + a_dst[i]`` and ``s = raw > 0 ? raw : ns * raw`` are one correctly rounded addition and one
    multiplication of stage inputs: the host forms the same two operations in fp32 and has ``s``, hence the running
    maximum ``m``, BIT FOR BIT (``host_logit``; ``m`` is asserted with ``torch.equal``, 0 for a destination without
    in-edges).  The restatement therefore takes ``s`` as those fp32 bits: b_i = 0 in the terms below.  The library is built
    with the compiler's default contraction, under which ``s - mn`` may be formed as ``fmaf(ns, raw, -mn)``, i.e. from the
    unrounded product: that moves the exponent's argument by at most ``|s| u`` where ``raw <= 0`` and nothing else (``fmaxf``
    sees the rounded ``s`` either way): one term ``|s| u [raw <= 0]`` on the weight, none on ``m``.
  * weights (running maximum, ``__expf``), as in tests/tconv_fwd_cases.py: ``p_e = exp(s_e - m)`` carries the relative error
    ``(2 |s_e - m| + |s_e| [raw <= 0] + C0 + 3 r_i) u``: the subtraction and ``__expf``'s own scaling of the argument round
    it twice, the instruction is inside ``C0 u``, and every arrival of a new maximum after the first in CSR order (``r_i``
    of them, strictly larger: an equal logit gives the factor ``__expf(0) = 1`` exactly) multiplies by a factor with its own
    instruction error and two roundings.  Per head: ``r_i`` is ``[N, 4]``.
  * ``denom = l + 1e-16f``: ``l`` is a ``fmaf`` chain over the in-edges: the destination's worst weight error plus
    ``(deg + C0) u``.  An isolated destination has ``denom = 1e-16f`` and ``m = 0`` exactly.
  * ``out = acc / denom + bias``: ``alpha_e`` adds the denominator's error to the weight's; ``sum_e alpha_e (rel(alpha_e) +
    k_z u) A_z[j]`` plus ``(deg + 3 + C0) u A_out`` (the chain, ``1 / denom``, the product, the bias), ``A_out = sum alpha A_z
    + |bias|``.  An isolated destination: ``out = bias`` exactly.
  * destination pass: ``alpha = __expf(s - m) / denom`` from the forward's ``stats``: its error is inside the forward's
    ``rel(alpha_e)`` (no rescale; the denominator's error is the forward's).  ``dalpha_e = <g_i, z_j>`` per head is the logit
    kernel's tree over a computed operand: k_da = 4 + log2(LPH) + k_z + [k_z > 0] over ``A_da = <|g_i|, A_z[j]>``.
    ``delta_i = sum alpha dalpha`` (``fmaf`` chain, deg terms).  ``grad_a_dst = sal - delta salk`` with ``sal = sum alpha lk
    dalpha`` and ``salk = sum alpha lk``: the difference cancels, so its magnitude is ``A_sal + A_delta salk`` -- ``alpha
    (|dalpha| + |delta|) |lk|`` summed -- not ``|ds|``.  ``lk = lrelu'(raw)`` is discontinuous at 0, but the sign of ``raw``
    is exact on both sides (a correctly rounded sum of two stage inputs has the sign of the exact sum; the kernel's
    ``raw > 0`` sends 0 to ``ns``, as the restatement's ``where`` does): no margin is needed.
  * source pass: ``grad_a_src[j] = sum alpha (dalpha - delta_i) lk`` over the out-edges in any order, three roundings per
    term; ``grad_z[j] = sum alpha g_i + grad_a_src att_src + grad_a_dst att_dst``: outdeg + 2 operands.
  * ``grad_bias`` (column sums of g) and the dense ``grad_att_*`` (``sum_n ga[n, h] z[n, h, :]``) end in fp64 sums of
    per-workgroup fp32 partials: a lane group's chain over its rows, then RPB lane groups in turn.  The chain's length
    depends on the device's grid; it is taken from the least favourable one, ONE workgroup holding all N rows:
    ``ceil(N / RPB) + RPB``.  The thin form's ``grad_lin = grad_z^T x`` and ``grad_att_* = W_h (ga^T x)`` go through
    ``qot_skinny_linear_dw`` and a row sum (not this file's kernels): the plain number of addends, N (+ K).

Graph families (the row counts are planted, not drawn): ``degrees`` (one destination of every in-degree 0 .. 9 in a
shuffled order, two of 41 and 47 in-edges whose in-edges at CSR positions 2 and 3 -- the second batch's first at EB = 2 and
at EB = 3 -- come from the source with the largest logit, a duplicate edge, an input self loop given twice; isolated
destinations first, last, two side by side and between two destinations that share a source; built with
``gat_self_loops=True`` and, so that the isolated ones exist, without), ``logits`` (planted logit orders along CSR order;
dense only: the thin form computes its logits), ``empty`` (E = 0, N = 1 and N = RPB + 1, with and without self loops),
``thin K`` (K = 1, 5, 8; C = 256 at K = 6, the largest that fits) and ``walk``.  In the small families every lane group
walks ONE destination; the walk cases take ``N = 3 min(8 CUs, 2048) RPB + RPB + 1`` from the device (``gat_case(name,
cus)``; the host uses the stand-in ``TRIP_CUS``), which gives run >= 3 in the forward whatever the occupancy.  Two of them
(``holes``) carry explicit self loops and planted isolated destinations every few rows, built WITHOUT
``gat_self_loops``: an isolated destination inside a lane group's run, between two that share a source.

``DEFECTS`` are planted in ``_evaluate``; the three that concern the LDS image and the prefetch follow the kernel's own
decisions (``walk_places``) for a given run length and can only show where a lane group walks several destinations: on the
walk cases (which are small on the host).

Nothing here touches the GPU; every case and host reference is built once and shared."""
import functools
import math
import types
import zlib

import numpy as np
import torch

from head_cases import C0, MARGIN, U, check_all, compare      # noqa: F401  (re-exported: the checks are the head's)

HEADS = 4
NS = 0.2
NS32 = float(np.float32(NS))          # what the kernels receive: ``float neg_slope``
EPS32 = float(np.float32(1e-16))
WIDTHS = (4, 8, 16, 32, 64, 128, 256)
FORMS = ("dense", "thin")
TRIP_CUS = 2        # host stand-in for the device's multi_processor_count in the walk cases
HOST_RUN = 4        # destinations per lane group of a walk case when the grid is at min(8 CUs, 2048)


def tpr(C):
    """Lanes per destination (``GatCfg::TPR``, HC / 4 = C at four heads)."""
    return min(64, C)


def rpb(C):
    return 256 // tpr(C)


def nv(C):
    return C // tpr(C)


def lph(C):
    return min(C // 4, tpr(C))


def eb(C):
    """In-edges in flight per lane group (``EB``)."""
    return 2 if nv(C) >= 4 else 3


def thin_fits(C, K):
    """``gat_thin_fits``: the walk's static LDS and ``W^T`` within 64 KB."""
    if not 1 <= K <= 8:
        return False
    HC = HEADS * C
    fixed = rpb(C) * eb(C) * HC * 4 + eb(C) * nv(C) * 256 * 4
    return fixed + K * HC * 4 <= 64 * 1024


def walk_rows(C, cus):
    return 3 * min(8 * cus, 2048) * rpb(C) + rpb(C) + 1


# ------------------------------------------------------------------ case table
def _c(family, C, loops=True, K=5, forms=FORMS, **kw):
    assert C in WIDTHS
    return dict(family=family, C=C, loops=loops, K=K, forms=tuple(f for f in forms if f == "dense" or thin_fits(C, K)), **kw)


def _cases():
    out = {}
    for C in WIDTHS:
        out[f"degrees_c{C}"] = _c("degrees", C)
        out[f"degrees_noloop_c{C}"] = _c("degrees", C, loops=False)
        out[f"logits_c{C}"] = _c("logits", C, forms=("dense",))
    for C, n in ((4, rpb(4) + 1), (32, rpb(32) + 1), (256, rpb(256) + 1), (16, 1), (256, 1)):
        out[f"empty_c{C}_n{n}"] = _c("empty", C, N=n)
        out[f"empty_noloop_c{C}_n{n}"] = _c("empty", C, N=n, loops=False)
    for C, K in ((4, 1), (4, 8), (8, 8), (16, 1), (256, 6)):
        out[f"thin_c{C}_k{K}"] = _c("degrees", C, K=K, forms=("thin",))
    for C, kind in ((4, "chain"), (16, "band"), (32, "chain"), (64, "hubs"), (128, "chain"), (256, "chain")):
        out[f"walk_c{C}_{kind}"] = _c("walk", C, kind=kind)
    out["walk_c128_shuffled_chain"] = _c("walk", 128, kind="shuffled_chain")
    out["walk_c8_chain_holes"] = _c("walk", 8, kind="chain", loops=False, holes=True)
    # (EB = 2 and the self loop last: the first batches (i - 1, i + 1) of consecutive chain destinations share nothing, the
    # image is never hit at C = 256; with the explicit self loops FIRST they are (i, i - 1) and it is)
    out["walk_c256_chain_holes"] = _c("walk", 256, kind="chain", loops=False, holes=True, loops_first=True)
    return out


CASES = _cases()
WALK = tuple(n for n, cfg in CASES.items() if cfg["family"] == "walk")
ORDINARY = tuple(n for n, cfg in CASES.items() if cfg["family"] in ("degrees", "logits"))
RUNS = [(n, f) for n, cfg in CASES.items() for f in cfg["forms"]]

# ------------------------------------------------------------------ graphs
DEGS = (0, 4, 0, 0, 6, 1, 3, 2, 0, 2, 9, 5, 7, 8, 41, 2, 47, 3, 1, 0)
ISOLATED = (0, 2, 3, 8, 19)          # first, two side by side, between 7 and 9 (which share source 12), last
SHARED = (7, 8, 9, 12)               # (left, isolated, right, their common source)
STRONG = 1                           # the source at CSR positions 2 and 3 of the wide destinations 14 and 16
PATTERNS = ("increasing", "decreasing", "equal", "one_low", "straddle", "heads")
LEAVES = (7, 2)


def _degrees_graph(gen):
    """``(edge_index, N)`` of the ``degrees`` family, in an order that is not sorted by destination."""
    N = len(DEGS)
    src, dst = [], []
    for i, d in enumerate(DEGS):
        s = [int(v) if int(v) < i else int(v) + 1 for v in torch.randint(0, N - 1, (d,), generator=gen)]     # no self loop
        if i == SHARED[0]:
            s = [4, SHARED[3]]
        if i == SHARED[2]:
            s = [SHARED[3], 13]
        if i == 15:
            s = [5, 5]                       # a duplicate edge
        if i == 17:
            s = [17, 17, 6]                  # an input self loop, given twice
        if d > 40:
            s[2] = s[3] = STRONG
        src += s
        dst += [i] * d
    ei = torch.tensor([src, dst], dtype=torch.long)
    # the destinations in a shuffled order, each one's sources in its own: the CSR build is stable by destination
    shuffled = ei[1, torch.randperm(ei.shape[1], generator=gen)].tolist()
    nxt = {i: iter(ei[0, ei[1] == i].tolist()) for i in set(shuffled)}
    return torch.tensor([[next(nxt[d]) for d in shuffled], shuffled], dtype=torch.long), N


def _logits_graph():
    """Star destinations with leaf sources of their own: ``(edge_index, N, [(destination, pattern, leaves)])``."""
    edges, plan = [], []
    n = 0
    for L in LEAVES:
        for pat in PATTERNS:
            leaves = list(range(n + 1, n + 1 + L))
            edges += [(k, n, leaf) for k, leaf in enumerate(leaves)]
            plan.append((n, pat, leaves))
            n += 1 + L
    edges.sort()          # the destinations' edges interleaved, each destination's in its own order
    return torch.tensor([[e[2] for e in edges], [e[1] for e in edges]], dtype=torch.long), n, plan


def pattern_raw(pat, n, gen):
    """Planted ``raw`` values ``[n, 4]`` along CSR order (the inserted self loop is the last)."""
    k = torch.arange(n, dtype=torch.float64)[:, None]
    h = torch.arange(HEADS, dtype=torch.float64)[None, :]
    if pat == "increasing":
        return 0.3 + 0.37 * k + 0.01 * h
    if pat == "decreasing":
        return 0.3 + 0.37 * (n - 1 - k) + 0.01 * h
    if pat == "equal":
        return torch.full((n, HEADS), 0.75, dtype=torch.float64)
    if pat == "one_low":
        raw = 61.0 + 0.1 * k + 0.01 * h
        raw[1] = 1.0
        return raw
    if pat == "straddle":
        base = torch.tensor([-1.5, 0.8, -0.2, 1.3, -3.0, 0.1, -0.7, 0.4], dtype=torch.float64)[:n, None]
        return base * (1.0 + 0.05 * h)
    if pat == "heads":
        return torch.tensor([-200.0, -50.0, 10.0, 40.0], dtype=torch.float64)[None, :] + 0.3 * torch.randn(n, HEADS, generator=gen).double()
    raise ValueError(pat)


def _walk_graph(cfg, N):
    import test_gpu_gat_walk as W          # its generators, not a copy of them
    ei = W._graph(cfg["kind"], N, seed=3)
    if cfg.get("holes"):
        loops = torch.arange(N)
        ei = torch.cat([torch.stack([loops, loops]), ei] if cfg.get("loops_first") else [ei, torch.stack([loops, loops])], 1)
        ei = ei[:, ~is_hole(ei[1], N)]
    return ei


def is_hole(i, N):
    """The planted isolated destinations of a ``holes`` case: every seventh row, two side by side every 35, first, last."""
    return (i % 7 == 3) | (i % 35 == 10) | (i % 35 == 11) | (i == 0) | (i == N - 1)


def host_index(ei, N, loops):
    """Host CSR in the device build's order (csrc/graph_prep.hip): stable by destination, in-row order = edge id; with
    ``loops`` the input's self loops are dropped and one per node is inserted last (eid -1)."""
    if loops:
        keep = ei[0] != ei[1]
        ids = torch.nonzero(keep).view(-1)
        node = torch.arange(N)
        src = torch.cat([ei[0, keep], node])
        dst = torch.cat([ei[1, keep], node])
        eid_in = torch.cat([ids, torch.full((N,), -1, dtype=torch.long)])
    else:
        src, dst, eid_in = ei[0], ei[1], torch.arange(ei.shape[1])
    order = torch.argsort(dst, stable=True)
    deg = torch.bincount(dst, minlength=N)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])
    row = dst[order]
    pos = torch.arange(row.numel()) - rowptr[row]
    col = src[order]
    return types.SimpleNamespace(eid=eid_in[order], deg=deg, rowptr=rowptr, row=row, col=col, pos=pos,
                                 outdeg=torch.bincount(col, minlength=N), E=int(row.numel()))


def _row_scale(N, gen):
    """Every row on its own scale, spread over several decades (as ``head_cases._draw_rows`` does per graph)."""
    return 4.0 ** -torch.randint(0, 5, (N,), generator=gen).float()


@functools.lru_cache(maxsize=None)
def gat_case(name, cus=TRIP_CUS):
    """The inputs of case ``name`` (fp32 on the host).  ``cus`` sizes the walk cases only."""
    cfg = CASES[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))          # by name: adding a case moves no other
    C, K, fam = cfg["C"], cfg["K"], cfg["family"]
    HC = HEADS * C
    plan = None
    if fam == "degrees":
        ei, N = _degrees_graph(gen)
    elif fam == "logits":
        ei, N, plan = _logits_graph()
    elif fam == "empty":
        ei, N = torch.zeros(2, 0, dtype=torch.long), cfg["N"]
    else:
        N = walk_rows(C, cus)
        ei = _walk_graph(cfg, N)
    c = types.SimpleNamespace(name=name, cfg=cfg, C=C, K=K, HC=HC, N=N, ei=ei, loops=cfg["loops"], family=fam, plan=plan,
                              cus=cus)
    c.ix = host_index(ei, N, c.loops)
    c.E = c.ix.E
    c.z = torch.randn(N, HC, generator=gen) * _row_scale(N, gen)[:, None]
    c.x = torch.randn(N, K, generator=gen) * _row_scale(N, gen)[:, None]
    c.w = (torch.rand(HC, K, generator=gen) * 2 - 1) * math.sqrt(6.0 / (K + HC))          # glorot, as GATConv.lin
    stdv = math.sqrt(6.0 / (HEADS + C))
    c.att_src = (torch.rand(HEADS, C, generator=gen) * 2 - 1) * stdv
    c.att_dst = (torch.rand(HEADS, C, generator=gen) * 2 - 1) * stdv
    c.bias = torch.rand(HC, generator=gen) * 0.4 - 0.2
    c.g = torch.randn(N, HC, generator=gen) * _row_scale(N, gen)[:, None]
    # the logits handed to the dense form: drawn (they are inputs of the walk, whatever made them)
    c.a_src = torch.randn(N, HEADS, generator=gen) * 1.5
    c.a_dst = torch.randn(N, HEADS, generator=gen) * 1.5
    if fam == "degrees":
        c.a_src[STRONG] = c.a_src.max(0).values + 1.0
    if fam == "logits":
        c.a_dst[:] = 0.25
        c.a_src[:] = 0.5
        for d, pat, leaves in plan:
            raw = pattern_raw(pat, len(leaves) + 1, gen)
            c.a_src[leaves + [d]] = (raw - 0.25).float()
    return c


def host_logit(c, logits=None):
    """``(raw, s)`` per CSR slot and head in fp32, as the kernels form them: one addition, one multiplication."""
    a_src, a_dst = logits if logits is not None else (c.a_src, c.a_dst)
    raw = a_src.float()[c.ix.col] + a_dst.float()[c.ix.row]
    s = torch.where(raw > 0, raw, torch.tensor(NS32, dtype=torch.float32) * raw)
    return raw, s


def host_thin_logits(c):
    """The thin form's logits as the host would leave them: ``x (W_h^T att_h)`` in fp32."""
    w3 = c.w.view(HEADS, c.C, c.K)
    v_src = (w3 * c.att_src[:, :, None]).sum(1)
    v_dst = (w3 * c.att_dst[:, :, None]).sum(1)
    return c.x @ v_src.t(), c.x @ v_dst.t()


def walk_places(ix, C, run):
    """The kernel's own decisions about every in-edge of the first batch, for lane groups that walk ``run`` consecutive
    destinations: ``cached`` (served from the LDS image: its source was among the live first-batch sources of the
    previous destination of the same run), ``prefetched`` (its source is the one row requested a destination ahead) and
    ``pid [N]`` (that row, -1 when none)."""
    N, EB = ix.deg.numel(), eb(C)
    F = torch.full((N, EB), -1, dtype=torch.long)
    for e in range(EB):
        has = ix.deg > e
        F[has, e] = ix.col[ix.rowptr[:-1][has] + e]
    prev = torch.roll(F, 1, 0)
    prev[0] = -1
    inrun = (torch.arange(N) % run != 0)
    match = torch.zeros(N, EB, dtype=torch.bool)
    for e in range(EB):
        for k in range(EB):
            match[:, e] |= (F[:, e] >= 0) & (F[:, e] == prev[:, k])
    pid = torch.full((N,), -1, dtype=torch.long)
    for e in reversed(range(EB)):
        pid = torch.where((F[:, e] >= 0) & ~match[:, e], F[:, e], pid)
    prev_any = torch.roll(ix.deg, 1) > 0
    prev_any[0] = False
    pid = torch.where(inrun & prev_any, pid, torch.full_like(pid, -1))
    pref = (F == pid[:, None]) & (pid >= 0)[:, None]
    cached = match & inrun[:, None] & ~pref
    edge = lambda t: _first_batch_to_edges(t, ix, EB)
    return dict(cached=edge(cached), prefetched=edge(pref), pid=pid)


def _first_batch_to_edges(t, ix, EB):
    out = torch.zeros(ix.E, dtype=torch.bool)
    for e in range(EB):
        has = ix.deg > e
        out[ix.rowptr[:-1][has] + e] = t[has, e]
    return out


# ------------------------------------------------------------------ the chain, in any dtype
DEFECTS = {
    "cached_logit_of_head0": "a row served from the LDS image takes head 0's source logit for every head",
    "stale_row_after_empty_destination": "the destination behind an isolated one takes a row left from before it",
    "prefetch_one_destination_late": "the prefetched row is the one requested for the previous destination",
    "ragged_tail_slot_accumulated": "the clamped duplicates of a short last batch are added",
    "second_batch_first_edge_dropped": "the in-edge at CSR position EB is dropped",
    "no_rescale_on_new_max": "no rescale of the running sums when a new maximum arrives",
    "self_loop_missing": "the inserted self loop is left out",
    "slope_on_the_positive_side": "ns applied where raw > 0",
    "bias_inside_the_normalisation": "(acc + bias) / denom",
    "isolated_not_bias": "an isolated destination gets 0",
    "thin_w_untransposed": "the thin form reads W [4C, K] as if it were [K, 4C]",
    "weight_off_1e-4": "one weight per destination of degree >= 2 multiplied by 1 + 1e-4",
    "delta_not_subtracted": "ds = alpha dalpha lrelu'",
    "logit_gradient_not_returned_to_grad_z": "grad_z without the attention vectors' terms",
}
WALK_DEFECTS = ("cached_logit_of_head0", "stale_row_after_empty_destination", "prefetch_one_destination_late")
_LOGIT_DEFECTS = WALK_DEFECTS + ("slope_on_the_positive_side",)          # those that change the logits themselves


def _segsum(x, row, N):
    return torch.zeros((N,) + tuple(x.shape[1:]), dtype=x.dtype).index_add_(0, row, x)


def _segmax(x, row, N):
    return torch.full((N,), -float("inf"), dtype=x.dtype).scatter_reduce(0, row, x, "amax")


def _by_position(ix):
    """``[(nodes with deg > p, their CSR slot p)]`` for p = 0, 1, ...: a walk along CSR order, all destinations at once."""
    order = torch.argsort(ix.deg, descending=True)
    sdeg = ix.deg[order]
    out = []
    for p in range(int(sdeg[0]) if sdeg.numel() else 0):
        nodes = order[:int((sdeg > p).sum())]
        out.append((nodes, ix.rowptr[:-1][nodes] + p))
    return out


def _running_max(s, ix):
    """Per slot: the largest ``s`` of the destination up to and including it (CSR order); ``r``: arrivals of a strictly
    larger maximum after the first."""
    N = ix.deg.numel()
    run = torch.full((N,), -float("inf"), dtype=s.dtype)
    r = torch.zeros(N, dtype=torch.float64)
    out = torch.empty_like(s)
    for p, (nodes, slots) in enumerate(_by_position(ix)):
        v = s[slots]
        if p:
            r[nodes] += (v > run[nodes]).double()
        run[nodes] = torch.maximum(run[nodes], v)
        out[slots] = run[nodes]
    return out, r


def _stale_col(ix):
    """``stale_row_after_empty_destination``: the first in-edge of a destination behind an isolated one reads the first
    source of the nearest non-empty destination before the gap."""
    col = ix.col.clone()
    last_first = -1
    deg, rp = ix.deg.tolist(), ix.rowptr.tolist()
    for i in range(len(deg)):
        if deg[i] == 0:
            continue
        if i and deg[i - 1] == 0 and last_first >= 0:
            col[rp[i]] = last_first
        last_first = int(ix.col[rp[i]])
    return col


def _evaluate(c, dtype, defect=None, form="dense", logits=None, run=HOST_RUN, backward=True, ns=NS32, pin=True):
    """The chain in plain tensor operations in ``dtype``, head by head (the heads share nothing but the index), the
    gradients by autograd against the cotangent ``c.g``; ``logits``: ``(a_src, a_dst)`` fp32 as the walk reads them
    (default: the case's own for the dense form, ``host_thin_logits`` for the thin one); ``defect``: one of DEFECTS.
    ``pin=False`` (with ``ns``): logits of any dtype, taken as they are -- the comparison with the oracle."""
    assert defect is None or defect in DEFECTS
    assert form in FORMS
    N, C, K, ix = c.N, c.C, c.K, c.ix
    if logits is None:
        logits = (c.a_src, c.a_dst) if form == "dense" else host_thin_logits(c)
    a_src32, a_dst32 = (t.to(dtype) for t in logits)
    raw32, s32 = host_logit(c, logits)
    row, col = ix.row, ix.col
    if defect == "stale_row_after_empty_destination":
        col = _stale_col(ix)
    places = walk_places(ix, C, run) if defect in ("cached_logit_of_head0", "prefetch_one_destination_late") else None
    if defect == "prefetch_one_destination_late":
        late = torch.roll(places["pid"], 1)
        late[0] = -1
        swap = places["prefetched"] & (late[row] >= 0)
        col = torch.where(swap, late[row], col)
    live = torch.ones(ix.E, dtype=torch.bool)
    if defect == "second_batch_first_edge_dropped":
        live = ix.pos != eb(C)
    if defect == "self_loop_missing":
        live = ~((ix.eid < 0) if c.loops else (ix.col == ix.row))
    dup = torch.ones(ix.E, dtype=dtype)
    if defect == "ragged_tail_slot_accumulated":
        short = (eb(C) - ix.deg % eb(C)) % eb(C)
        dup = torch.where(ix.pos == ix.deg[row] - 1, 1.0 + short[row].to(dtype), dup)
    x = c.x.to(dtype)
    res = {k: [] for k in ("out", "m", "denom", "alpha", "grad_z", "grad_lin", "grad_att_src", "grad_att_dst", "grad_bias")}
    one, zero = torch.ones((), dtype=dtype), torch.zeros((), dtype=dtype)
    for h in range(HEADS):
        sl = slice(h * C, (h + 1) * C)
        att_s = c.att_src[h].to(dtype).requires_grad_(backward)
        att_d = c.att_dst[h].to(dtype).requires_grad_(backward)
        bias = c.bias[sl].to(dtype).requires_grad_(backward)
        if form == "thin":
            w = c.w[sl].to(dtype).requires_grad_(backward)
            z = x @ (c.w.to(dtype).reshape(K, c.HC)[:, sl] if defect == "thin_w_untransposed" else w.t())
            leaf = w
        else:
            z = c.z[:, sl].to(dtype).requires_grad_(backward)
            leaf = z
        zl = z.detach() if defect == "logit_gradient_not_returned_to_grad_z" else z
        # the logits: the value handed in, the derivative of <z, att>
        ps, pd = (zl * att_s).sum(-1), (zl * att_d).sum(-1)
        a_s = a_src32[:, h].to(dtype) + (ps - ps.detach())
        a_d = a_dst32[:, h].to(dtype) + (pd - pd.detach())
        a_s_e = a_s[col]
        if defect == "cached_logit_of_head0":
            a_s_e = torch.where(places["cached"], a_src32[:, 0].to(dtype)[col], a_s_e)
        raw = a_s_e + a_d[row]
        if defect == "slope_on_the_positive_side":
            s = torch.where(raw > 0, ns * raw, raw)
        else:
            s = torch.where(raw > 0, raw, ns * raw)
        if pin and defect not in _LOGIT_DEFECTS:
            s = s32[:, h].to(dtype) + (s - s.detach())          # the value: the fp32 bits the kernels have
        s_live = torch.where(live, s.detach(), -float("inf") * one)
        m = _segmax(s_live, row, N)
        has = m > -float("inf")
        m = torch.where(has, m, zero)
        p = torch.where(live, (s - m[row]).exp(), zero) * dup
        if defect == "no_rescale_on_new_max":        # every weight stays relative to the maximum of its own time
            p = (s - _running_max(s.detach(), ix)[0]).exp()
        if defect == "weight_off_1e-4":
            p = torch.where((ix.pos == 0) & (ix.deg[row] >= 2), p * (1 + 1e-4), p)
        l = _segsum(p, row, N)
        denom = l + EPS32
        alpha = p / (denom.detach() if defect == "delta_not_subtracted" else denom)[row]
        acc = _segsum(alpha[:, None] * z[col], row, N)
        if defect == "bias_inside_the_normalisation":
            out = acc + bias / denom.detach()[:, None]
        else:
            out = acc + bias
        if defect == "isolated_not_bias":
            out = out * has.to(dtype)[:, None]
        res["out"].append(out.detach())
        res["m"].append(m)
        res["denom"].append(denom.detach())
        res["alpha"].append(alpha.detach())
        if backward:
            grads = torch.autograd.grad((out * c.g[:, sl].to(dtype)).sum(), [leaf, att_s, att_d, bias], allow_unused=True)
            grads = [torch.zeros_like(t) if gr is None else gr for gr, t in zip(grads, (leaf, att_s, att_d, bias))]
            res["grad_lin" if form == "thin" else "grad_z"].append(grads[0])
            res["grad_att_src"].append(grads[1])
            res["grad_att_dst"].append(grads[2])
            res["grad_bias"].append(grads[3])
    out = dict(out=torch.cat(res["out"], 1), m=torch.stack(res["m"], 1), denom=torch.stack(res["denom"], 1),
               alpha=torch.stack(res["alpha"], 1))
    if backward:
        out.update(grad_att_src=torch.stack(res["grad_att_src"]), grad_att_dst=torch.stack(res["grad_att_dst"]),
                   grad_bias=torch.cat(res["grad_bias"]))
        if form == "thin":
            out["grad_lin"] = torch.cat(res["grad_lin"], 0)
        else:
            out["grad_z"] = torch.cat(res["grad_z"], 1)
    return out


CHECKED = {"dense": ("out", "m", "denom", "grad_z", "grad_att_src", "grad_att_dst", "grad_bias"),
           "thin": ("out", "m", "denom", "grad_lin", "grad_att_src", "grad_att_dst", "grad_bias")}


# ------------------------------------------------------------------ the bounds
def dot_count(C):
    """``group_sum<LPH>(dot4(.))`` over stage inputs."""
    return 4 + int(math.log2(lph(C)))


def _entry(value, bound, k):
    k = torch.as_tensor(k, dtype=torch.float64)
    while k.dim() and k.dim() < bound.dim():
        k = k[..., None]
    A = torch.where(k > 0, bound / (k * U).clamp_min(1e-300), value.abs().double())
    return dict(value=value, bound=bound, k=k, A=A)


def reference(c, form, logits=None):
    """``{quantity: dict(value, A, k, bound)}`` in fp64 for case ``c`` in ``form``; ``logits``: the fp32 logits the walk
    read (default as in ``_evaluate``).  ``alpha`` is per CSR slot and head; ``m``, ``denom`` are ``[N, 4]``."""
    assert form in FORMS
    f64 = torch.float64
    N, C, K, ix = c.N, c.C, c.K, c.ix
    if logits is None:
        logits = (c.a_src, c.a_dst) if form == "dense" else host_thin_logits(c)
    r = _evaluate(c, f64, form=form, logits=logits)
    raw32, s32 = host_logit(c, logits)
    row, col = ix.row, ix.col
    deg, outdeg = ix.deg.double(), ix.outdeg.double()
    kz = float(K) if form == "thin" else 0.0
    k_da = dot_count(C) + kz + (1.0 if kz else 0.0)
    chain = float(-(-N // rpb(C)) + rpb(C))            # one workgroup holding all N rows
    xa = c.x.double().abs()
    ref = {}
    parts = {k: [] for k in ("out", "denom", "alpha", "grad_z", "grad_lin", "grad_att_src", "grad_att_dst", "grad_bias", "nrec")}
    for h in range(HEADS):
        sl = slice(h * C, (h + 1) * C)
        s = s32[:, h].double()
        m = r["m"][:, h]
        alpha = r["alpha"][:, h]
        _, nrec = _running_max(s, ix)
        neg = (raw32[:, h] <= 0).double()
        relp = (2 * (s - m[row]).abs() + s.abs() * neg + C0 + 3 * nrec[row]) * U
        relmax = torch.zeros(N, dtype=f64).scatter_reduce(0, row, relp, "amax")
        rel_den = relmax + (deg + C0) * U
        rela = relp + rel_den[row]
        if form == "thin":
            wa = c.w[sl].double().abs()
            zA = xa @ wa.t()
            zv = c.x.double() @ c.w[sl].double().t()
        else:
            zA = c.z[:, sl].double().abs()
            zv = c.z[:, sl].double()
        ba = c.bias[sl].double().abs()
        a_out = _segsum(alpha[:, None] * zA[col], row, N) + ba
        b_out = _segsum((alpha * (rela + kz * U))[:, None] * zA[col], row, N) + ((deg + 3 + C0) * U)[:, None] * a_out
        parts["out"].append(b_out)
        parts["denom"].append(torch.where(ix.deg == 0, torch.zeros((), dtype=f64), r["denom"][:, h] * rel_den))
        parts["alpha"].append(alpha * rela)
        parts["nrec"].append(nrec)
        # backward
        gA = c.g[:, sl].double().abs()
        A_da = (gA[row] * zA[col]).sum(-1)
        lk = torch.where(raw32[:, h] > 0, 1.0, NS32).double()
        A_delta = _segsum(alpha * A_da, row, N)
        b_delta = _segsum(alpha * A_da * (rela + k_da * U), row, N) + (deg + C0) * U * A_delta
        salk = _segsum(alpha * lk, row, N)
        A_sal = _segsum(alpha * lk * A_da, row, N)
        b_sal = _segsum(alpha * lk * A_da * (rela + (k_da + 1) * U), row, N) + (deg + C0) * U * A_sal
        b_salk = _segsum(alpha * lk * (rela + U), row, N) + (deg + C0) * U * salk
        A_gad = A_sal + A_delta * salk
        b_gad = b_sal + b_delta * salk + A_delta * b_salk + 2 * U * A_gad
        A_t = alpha * lk * (A_da + A_delta[row])
        b_t = alpha * lk * ((rela + 3 * U) * (A_da + A_delta[row]) + k_da * U * A_da + b_delta[row])
        A_gas = _segsum(A_t, col, N)
        b_gas = _segsum(b_t, col, N) + (outdeg + C0) * U * A_gas
        ats, atd = c.att_src[h].double().abs(), c.att_dst[h].double().abs()
        A_gz = _segsum(alpha[:, None] * gA[row], col, N) + A_gas[:, None] * ats + A_gad[:, None] * atd
        b_gz = (_segsum((alpha * rela)[:, None] * gA[row], col, N) + b_gas[:, None] * ats + b_gad[:, None] * atd
                + ((outdeg + 2 + C0) * U)[:, None] * A_gz)
        parts["grad_bias"].append((chain + C0) * U * gA.sum(0))
        if form == "dense":
            parts["grad_z"].append(b_gz)
            za = zv.abs()
            parts["grad_att_src"].append(b_gas @ za + (chain + C0) * U * (A_gas @ za))
            parts["grad_att_dst"].append(b_gad @ za + (chain + C0) * U * (A_gad @ za))
        else:
            parts["grad_lin"].append(b_gz.t() @ xa + (N + C0) * U * (A_gz.t() @ xa))
            for key, A_g, b_g in (("grad_att_src", A_gas, b_gas), ("grad_att_dst", A_gad, b_gad)):
                A_dw = A_g @ xa
                b_dw = b_g @ xa + (N + C0) * U * A_dw
                parts[key].append(wa @ b_dw + (K + 1) * U * (wa @ A_dw))
    kd = deg[:, None]
    ref["out"] = _entry(r["out"], torch.cat(parts["out"], 1), deg + 3 + C0 + kz)
    ref["m"] = _entry(r["m"], torch.zeros_like(r["m"]), 0.0)
    ref["denom"] = _entry(r["denom"], torch.stack(parts["denom"], 1), (kd + C0).expand(N, HEADS))
    ref["alpha"] = _entry(r["alpha"], torch.stack(parts["alpha"], 1), (deg[row] + C0)[:, None].expand(ix.E, HEADS))
    ref["grad_bias"] = _entry(r["grad_bias"], torch.cat(parts["grad_bias"]), chain + C0)
    if form == "dense":
        ref["grad_z"] = _entry(r["grad_z"], torch.cat(parts["grad_z"], 1), outdeg + 2 + C0)
        ref["grad_att_src"] = _entry(r["grad_att_src"], torch.stack(parts["grad_att_src"]), chain + C0)
        ref["grad_att_dst"] = _entry(r["grad_att_dst"], torch.stack(parts["grad_att_dst"]), chain + C0)
    else:
        ref["grad_lin"] = _entry(r["grad_lin"], torch.cat(parts["grad_lin"], 0), float(N + C0))
        ref["grad_att_src"] = _entry(r["grad_att_src"], torch.stack(parts["grad_att_src"]), float(N + K + C0))
        ref["grad_att_dst"] = _entry(r["grad_att_dst"], torch.stack(parts["grad_att_dst"]), float(N + K + C0))
    ref["isolated"] = ix.deg == 0
    ref["nrec"] = torch.stack(parts["nrec"], 1)
    return ref


@functools.lru_cache(maxsize=None)
def host_reference(name, form, cus=TRIP_CUS):
    """``reference`` with the host's logits (cached)."""
    return reference(gat_case(name, cus), form)


def logits_reference(c):
    """``a_src, a_dst`` of ``qot_gat_logits`` from ``z`` and the attention vectors."""
    z3 = c.z.double().view(c.N, HEADS, c.C)
    k = torch.tensor(float(dot_count(c.C)), dtype=torch.float64)
    ref = {}
    for key, att in (("a_src", c.att_src), ("a_dst", c.att_dst)):
        A = (z3.abs() * att.double().abs()).sum(-1)
        ref[key] = dict(value=(z3 * att.double()).sum(-1), A=A, k=k, bound=k * U * A)
    return ref


def thin_logits_reference(c):
    """The thin form's logits ``x (W_h^T att_h)``: a C-term sum in any order, then a K-term chain."""
    w3 = c.w.double().view(HEADS, c.C, c.K)
    x = c.x.double()
    k = torch.tensor(float(c.C + c.K + C0), dtype=torch.float64)
    ref = {}
    for key, att in (("a_src", c.att_src), ("a_dst", c.att_dst)):
        v = (w3 * att.double()[:, :, None]).sum(1)
        va = (w3.abs() * att.double().abs()[:, :, None]).sum(1)
        A = x.abs() @ va.t()
        ref[key] = dict(value=x @ v.t(), A=A, k=k, bound=k * U * A)
    return ref
