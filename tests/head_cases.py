"""Cases, fp64 restatement and per-element error bounds of the read-out head (tests/test_head_cases_cpu.py,
tests/test_gpu_head.py):  pool -> Linear -> LeakyReLU -> Dropout -> Linear -> SmoothL1(mean, beta) -> backward, optionally
through the producer's ``dropout(leaky_relu(.))`` (the fold of ``functional.HeadFn``).

``head_reference(case)`` restates the chain in fp64 with plain tensor operations (no autograd) and gives every quantity two
companions:

* a magnitude ``A >= |value|``: the same formula with every operand replaced by its companion, subtraction turned into
  addition, derivative and mask factors by their absolute value;
* a count ``k``: the additions on the element's own longest chain, plus the counts of its operands (for a product: of both
  factors), plus ``C0 = 16`` once for the divisions and scale factors on the way.

The assertion is ``|got - ref| <= k * 2^-24 * A`` for every element; nothing in it is measured.  Why it is a bound: a sum
of n terms, in ANY order, each term off by at most ``k_i u A_i``, is off by at most ``(max k_i + n - 1) u sum A_i`` to
first order (u = 2^-24); a product of two such operands by ``(k_x + k_y + 1) u A_x A_y``.  The kernels add with ``fmaf``
(no rounding of the product), so a dot product of n terms and a bias counts its ``n + 1`` addends -- one more than its
roundings.  How each count was read from csrc/head.hip stands next to it in ``_companions``.  The roundings that are not
additions, on the longest path (to grad_x under fold): ``1 / cnt`` and the product with it (2), ``keep_scale * slope`` and
the product with it (2), ``out - y`` (1), ``/ beta`` (1), ``1 / (B O)`` and the product with it (2), the product with the
activation's derivative (1), ``1 / cnt`` and its product again (2), the fold's two factors (2), the fp32 rounding of an
explicitly fed ``grad_out`` (1): 14 <= C0.

The chain has three kinks (leaky_relu at pre = 0, Huber at |df| = beta, the sign of df); ``margins`` measures how far every
element is from them in units of its own bound, and the generator redraws until all are >= 4 (``MARGIN``).

Nothing here touches the GPU; every case and reference is built once and shared."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dropout as OD

U = 2.0 ** -24
C0 = 16
MARGIN = 4.0
GLOBAL_TOL = 1e-5                 # the existing head test's bar (tests/test_gpu_parity.py::test_fused_head_matches_unfused)
SLOPE = 0.01
WIDTHS = (16, 32, 64, 128)
BIG = (127, 128, 129, 300)        # around kHeadRowsCap / 4 * kHeadKeep = 128 rows kept, and far beyond
HEAD_BLOCKS = 512                 # kHeadBwdBlocks (csrc/head.hip); the GPU test asserts the trip counts it implies
HEAD_SEED = (1 << 63) + 0x1234567    # all 64 bits in use
FOLD_SEED = (1 << 62) + 0x7654321
HEAD_STEP, FOLD_STEP = 5, 11


def graphs_per_pass(H):
    """GB of head_train_batched_kernel (256 / H graphs per pass); head_train_kernel (H = 128) walks one graph at a time."""
    return 256 // H if H <= 64 else 1


# ------------------------------------------------------------------ case tables
_SETTINGS = [dict(p=p, fold=fold, in_p=in_p) for p in (0.0, 0.5) for fold, in_p in ((False, 0.0), (True, 0.0), (True, 0.5))]
_LOSSES = [(O, beta) for O in (1, 3, 8) for beta in (1.0, 0.25)]


def _name(kind, H, c):
    fold = f"fold{c['in_p']}" if c["fold"] else "nofold"
    return f"{kind}_h{H}_o{c['O']}_beta{c['beta']}_p{c['p']}_{fold}" + (f"_v{c['variant']}" if kind == "trip" else "")


def _small_cases():
    """Every width meets all six (p, fold) settings and all six (O, beta) pairs; the pairing rotates with the width."""
    out = {}
    for w, H in enumerate(WIDTHS):
        for i, s in enumerate(_SETTINGS):
            O, beta = _LOSSES[(i + w) % len(_LOSSES)]
            c = dict(s, kind="small", H=H, O=O, beta=beta, seed=1000 * H + i)
            out[_name("small", H, c)] = c
    return out


TRIP_B = {16: 24599, 32: 12299, 64: 6149, 128: 2051}      # GB * (3 * 512) + GB + r with 0 < r < GB; 2051 at GB = 1
_TRIP_SETTINGS = [dict(p=0.0, fold=False, in_p=0.0, O=3, beta=1.0), dict(p=0.5, fold=True, in_p=0.5, O=8, beta=0.25),
                  dict(p=0.5, fold=True, in_p=0.0, O=1, beta=1.0), dict(p=0.0, fold=True, in_p=0.5, O=3, beta=0.25)]


def _trip_cases():
    """Four variants per width: variant v puts BIG[(place + slot + v) % 4] into the slots of every planted place, so that
    each place sees each of the four sizes."""
    out = {}
    for H in WIDTHS:
        for v, s in enumerate(_TRIP_SETTINGS):
            c = dict(s, kind="trip", H=H, variant=v, seed=77000 + 10 * H + v)
            out[_name("trip", H, c)] = c
    return out


SMALL_CASES = _small_cases()
TRIP_CASES = _trip_cases()
CASES = {**SMALL_CASES, **TRIP_CASES}


def small_sizes(gen):
    """41 graphs: an empty one first, a 300-node graph between two empty ones, two empty ones side by side, the sizes
    around every threshold, an empty one last.  41 % GB != 0 for GB = 16, 8, 4."""
    planted = [0, 300, 0, 0, 1, 2, 63, 64, 65, 127, 128, 129]
    rest = torch.randint(1, 41, (28,), generator=gen).tolist()
    return planted + rest + [0]


def trip_places(H, B):
    """First graph of every planted place of a trip case: index 0; workgroup 0's second and last trip in the fused train
    kernels (pass ps of workgroup ps % 512 holds graphs ps * GB ...) and in head_bwd_kernel (graph b of workgroup b % 512);
    the last live slot."""
    GB = graphs_per_pass(H)
    npass = -(-B // GB)
    return [0, HEAD_BLOCKS * GB, ((npass - 1) // HEAD_BLOCKS) * HEAD_BLOCKS * GB, HEAD_BLOCKS,
            ((B - 1) // HEAD_BLOCKS) * HEAD_BLOCKS, B - 1]


def trip_sizes(H, variant, gen):
    B = TRIP_B[H]
    sizes = torch.randint(0, 4, (B,), generator=gen).tolist()
    GB = graphs_per_pass(H)
    for j, start in enumerate(trip_places(H, B)):
        for i in range(1 if start == B - 1 else min(GB, 4)):
            if start + i < B:
                sizes[start + i] = BIG[(j + i + variant) % 4]
    return sizes


def trips(B, H, blocks, train):
    """``{workgroup: trips}`` of a launch of ``blocks`` workgroups: passes of GB graphs in the fused train kernels, single
    graphs in head_bwd_kernel."""
    units = -(-B // graphs_per_pass(H)) if train else B
    return {w: len(range(w, units, blocks)) for w in range(blocks)}


# ------------------------------------------------------------------ inputs
def _slope32(s):
    return float(np.float32(s))


def _draw_rows(c, rows, gen):
    """Fresh node rows (fp32): unit normals on the row's graph scale, 3 % exact zeros (the derivative of leaky_relu at 0 is
    the slope, also behind the fold); under fold the producer's ``dropout(leaky_relu(.))`` with the restated mask."""
    z = torch.randn(len(rows), c.H, generator=gen) * c.scale[c.batch[rows]][:, None]
    zero = torch.rand(len(rows), c.H, generator=gen) < 0.03
    if c.fold:
        z = F.leaky_relu(z, _slope32(c.in_slope)) * c.in_keep[rows].float() * float(c.in_ks)
    z[zero] = 0.0
    return z


@functools.lru_cache(maxsize=None)
def head_case(name):
    """The inputs of case ``name`` (fp32 on the host), redrawn until every kink is at least MARGIN bounds away."""
    cfg = CASES[name]
    gen = torch.Generator().manual_seed(cfg["seed"])
    H, O = cfg["H"], cfg["O"]
    sizes = small_sizes(gen) if cfg["kind"] == "small" else trip_sizes(H, cfg["variant"], gen)
    cnt = torch.tensor(sizes, dtype=torch.long)
    B, N = len(sizes), int(cnt.sum())
    assert N < 100000
    c = types.SimpleNamespace(name=name, cfg=cfg, H=H, O=O, B=B, N=N, cnt=cnt, beta=cfg["beta"], slope=SLOPE, p=cfg["p"],
                              seed=HEAD_SEED + cfg["seed"], step=HEAD_STEP, fold=cfg["fold"], in_slope=SLOPE,
                              in_p=cfg["in_p"], in_seed=FOLD_SEED + cfg["seed"], in_step=FOLD_STEP)
    c.ptr = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])
    c.batch = torch.repeat_interleave(torch.arange(B), cnt)
    c.keep = OD.keep_mask(c.seed, c.step, (B, H), c.p)
    c.ks = OD.keep_scale(c.p) if c.p > 0 else np.float32(1.0)
    c.in_keep = OD.keep_mask(c.in_seed, c.in_step, (N, H), c.in_p) if c.fold else torch.ones(N, H, dtype=torch.bool)
    c.in_ks = OD.keep_scale(c.in_p) if c.fold and c.in_p > 0 else np.float32(1.0)
    c.scale = torch.tensor([0.0625, 0.25, 1.0])[torch.randint(0, 3, (B,), generator=gen)]
    c.w0 = torch.randn(H, H, generator=gen) / H ** 0.5
    c.b0 = torch.randn(H, generator=gen) * 0.5
    # a small second layer: grad_out = (out - y) / beta / (B O) is judged on the scale of 1 / (B O) by the global check, which
    # multiplies out's rounding by 1 / beta; |W3| A_h + |b3| of order one keeps that a few 1e-7 (the per-element bound follows
    # A and stays as sharp)
    c.w3 = torch.randn(O, H, generator=gen) / H
    c.b3 = torch.randn(O, generator=gen) * 0.3
    c.x = _draw_rows(c, torch.arange(N), gen)
    c.y = torch.zeros(B, O)
    c.rounds = 0
    for c.rounds in range(1, 33):
        m = margins(c, forward_only=True)
        bad = (m["pre"] < MARGIN).any(1)
        if not bool(bad.any()):
            break
        # an empty graph's pre is b0 itself (its bound is a few ulp of it): no redraw can be needed there
        assert bool((cnt[bad] > 0).all()), name
        rows = torch.nonzero(bad[c.batch]).view(-1)
        c.x[rows] = _draw_rows(c, rows, gen)
    # the target: half of the graphs in the quadratic branch (|df| in [0.1, 0.9] beta), half in the linear one ([1.2, 3]
    # beta), either sign; far from both kinks on the scale of out's bound, which the margins below confirm
    out = _evaluate(c, torch.float64)["out"]
    quad = torch.rand(B, 1, generator=gen) < 0.5
    mag = torch.where(quad, 0.1 + 0.8 * torch.rand(B, O, generator=gen), 1.2 + 1.8 * torch.rand(B, O, generator=gen))
    sign = torch.where(torch.rand(B, O, generator=gen) < 0.5, -1.0, 1.0)
    c.y = (out - (sign * mag * c.beta).double()).float()
    return c


# ------------------------------------------------------------------ the chain, in any dtype
DEFECTS = {
    "pool_skips_last_row": "the last row of the first 300-node graph is left out of the pool",
    "count_not_clamped": "cnt instead of max(cnt, 1) in the pool and in the pool backward",
    "gw0_skips_graph": "the term of graph 1 (300 nodes) is left out of gW0",
    "head_mask_shifted": "the head's mask numbered at b * H + o + 1",
    "fold_slope_at_zero": "the fold's slope applied where y >= 0 instead of y > 0",
    "inv_n_of_last_pass": "1 / (B O) taken with the live graphs of the last pass only, for that pass",
}


def _evaluate(c, dtype, defect=None):
    """The chain with plain tensor operations in ``dtype``; ``defect``: one of DEFECTS planted."""
    assert defect is None or defect in DEFECTS
    x, w0, b0, w3, b3, y = (t.to(dtype) for t in (c.x, c.w0, c.b0, c.w3, c.b3, c.y))
    B, H, O, N = c.B, c.H, c.O, c.N
    slope, in_slope = _slope32(c.slope), _slope32(c.in_slope)
    xs = x
    if defect == "pool_skips_last_row":
        g = int(torch.nonzero(c.cnt == 300)[0])
        xs = x.clone()
        xs[int(c.ptr[g + 1]) - 1] = 0
    div = (c.cnt if defect == "count_not_clamped" else c.cnt.clamp(min=1)).to(dtype)[:, None]
    pool = torch.zeros(B, H, dtype=dtype).index_add_(0, c.batch, xs) / div
    pre = pool @ w0.t() + b0
    keep = c.keep
    if defect == "head_mask_shifted":
        keep = OD.keep_mask(c.seed, c.step, (B * H + 1,), c.p)[1:].view(B, H)
    one = torch.ones((), dtype=dtype)
    d = torch.where(pre > 0, one, one * slope) * (keep.to(dtype) * float(c.ks))      # d/dpre of dropout(leaky_relu(pre))
    h = pre * d
    out = h @ w3.t() + b3
    df = out - y
    ad = df.abs()
    quad = ad < c.beta
    inv_n = torch.full((B, 1), 1.0 / (B * O), dtype=dtype)
    if defect == "inv_n_of_last_pass":
        live = B % graphs_per_pass(H) or graphs_per_pass(H)
        inv_n[B - live:] = 1.0 / (live * O)
    lelem = torch.where(quad, 0.5 * df * df / c.beta, ad - 0.5 * c.beta) * inv_n
    go = torch.where(quad, df / c.beta, torch.where(df > 0, one, -one)) * inv_n
    loss_rows = lelem.sum(1)
    gh = (go @ w3) * d
    gp = gh @ w0
    gx = (gp / div)[c.batch]
    res = dict(pool=pool, pre=pre, d=d, h=h, out=out, df=df, quad=quad, grad_out=go, loss_rows=loss_rows,
               loss=loss_rows.sum(), gh=gh, gp=gp)
    if c.fold:
        pos = (x >= 0) if defect == "fold_slope_at_zero" else (x > 0)
        fac = torch.where(pos, one, one * in_slope) * (c.in_keep.to(dtype) * float(c.in_ks))
        gx = gx * fac
        res["fac"] = fac
        res["gbias"] = gx.sum(0)
    ghw = gh
    if defect == "gw0_skips_graph":
        ghw = gh.clone()
        ghw[1] = 0
    res.update(gx=gx, gw0=ghw.t() @ pool, gb0=gh.sum(0), gw3=go.t() @ h, gb3=go.sum(0))
    return res


CHECKED = ("pool", "h", "out", "grad_out", "loss_rows", "loss", "gx", "gw0", "gb0", "gw3", "gb3", "gbias")


def _companions(c, r):
    """``{name: (A, n)}`` for ``r = _evaluate(c, float64)``; the count is ``k = n + C0``.  ``n`` is per graph wherever the
    chain length depends on the graph's node count only."""
    B, H, O, N = c.B, c.H, c.O, c.N
    f64 = torch.float64
    aw0, ab0, aw3, ab3 = (t.double().abs() for t in (c.w0, c.b0, c.w3, c.b3))
    cm = c.cnt.clamp(min=1).double()[:, None]
    ncnt = c.cnt.double()[:, None]
    inv_n = 1.0 / (B * O)
    dabs = r["d"].abs()
    quad = r["quad"]
    A, n = {}, {}
    # pool: cnt rows added (lane-group partials, then the partials: every order adds cnt - 1 times; cnt over-estimates)
    A["pool"] = torch.zeros(B, H, dtype=f64).index_add_(0, c.batch, c.x.double().abs()) / cm
    n["pool"] = ncnt
    # pre: the bias and H products on one fmaf chain (head_fwd_kernel, head_train_kernel; the batched kernel splits the
    # chain over KS lanes and adds the bias last: shorter), on top of the pool
    A["pre"] = A["pool"] @ aw0.t() + ab0
    n["pre"] = n["pool"] + (H + 1)
    # h = pre * d: no addition
    A["h"] = A["pre"] * dabs
    n["h"] = n["pre"]
    # out: the bias and H products on one chain (the batched kernel: 16 chains of H / 16 and a 4-step DPP sum: shorter)
    A["out"] = A["h"] @ aw3.t() + ab3
    n["out"] = n["h"] + (H + 1)
    A["df"] = A["out"] + c.y.double().abs()
    n["df"] = n["out"] + 1
    # grad_out: df / beta / (B O) in the quadratic branch; +-1 / (B O) in the linear one (no operand at all)
    A["grad_out"] = torch.where(quad, A["df"] / c.beta, torch.ones((), dtype=f64)) * inv_n
    n["grad_out"] = torch.where(quad, n["df"].expand(B, O), torch.zeros((), dtype=f64))
    # a graph's loss: O elements added in turn; 0.5 df df / beta is a product of df with itself (2 n_df), |df| - beta / 2
    # one more addition
    alel = torch.where(quad, 0.5 * A["df"] ** 2 / c.beta, A["df"] + 0.5 * c.beta) * inv_n
    nlel = torch.where(quad, 2 * n["df"].expand(B, O), n["df"].expand(B, O) + 1)
    A["loss_rows"] = alel.sum(1)
    n["loss_rows"] = nlel.max(1).values + O
    # the loss: B shares (QOT_ROLE_SUM_ROWS; the plain number of addends)
    A["loss"] = A["loss_rows"].sum()
    n["loss"] = n["loss_rows"].max() + B
    # gh = (W3^T go) * d: O products on one chain
    A["gh"] = (A["grad_out"] @ aw3) * dabs
    n["gh"] = n["grad_out"].max(1, keepdim=True).values + O
    # gp = W0^T gh: H products on one chain (the batched kernel: KS shorter ones)
    A["gp"] = A["gh"] @ aw0
    n["gp"] = n["gh"] + H
    # grad_x: gp / cnt on every row, times the fold's factors: no addition
    A["gx"] = (A["gp"] / cm)[c.batch]
    n["gx"] = n["gp"][c.batch]
    if c.fold:
        A["gx"] = A["gx"] * r["fac"].abs()
        # the producer's bias gradient: column sums over all N rows (per lane group, per workgroup, then over the
        # workgroups' partials: the plain number of addends)
        A["gbias"] = A["gx"].sum(0)
        n["gbias"] = n["gx"].max() + N if N else torch.zeros((), dtype=f64)
    # parameter gradients: one term per graph, added per thread over the workgroup's trips, then over the workgroups'
    # partials (head_partial_sum_kernel / QOT_ROLE_SUM_ROWS): B addends in all (the plain number), each a product of two
    # computed operands
    A["gw0"] = A["gh"].t() @ A["pool"]
    n["gw0"] = (n["gh"] + n["pool"]).max() + B
    A["gb0"] = A["gh"].sum(0)
    n["gb0"] = n["gh"].max() + B
    A["gw3"] = A["grad_out"].t() @ A["h"]
    n["gw3"] = (n["grad_out"].max(1, keepdim=True).values + n["h"]).max() + B
    A["gb3"] = A["grad_out"].sum(0)
    n["gb3"] = n["grad_out"].max() + B
    return A, n


def _reference(c):
    r = _evaluate(c, torch.float64)
    A, n = _companions(c, r)
    ref = {}
    for name in A:
        k = torch.as_tensor(n[name], dtype=torch.float64) + C0
        ref[name] = dict(value=r[name], A=A[name], k=k, bound=k * U * A[name])
        # a companion below its value is a derivation error (equal ones may differ by fp64 rounding)
        assert bool((A[name] * (1 + 1e-12) >= r[name].abs()).all()), name
    ref["quad"] = r["quad"]
    return ref


@functools.lru_cache(maxsize=None)
def _cached_reference(name):
    return _reference(head_case(name))


def head_reference(case):
    """``{quantity: dict(value, A, k, bound)}`` in fp64 for a case of ``head_case`` (cached) or any namespace of its form."""
    if getattr(case, "name", None) in CASES and head_case(case.name) is case:
        return _cached_reference(case.name)
    return _reference(case)


def margins(c, forward_only=False):
    """Distance of every element from the chain's kinks, in units of the element's bound: ``pre`` (leaky_relu at 0, |pre|
    over pre's own bound), ``huber`` (||df| - beta| over out's bound) and ``sign`` (|df| over out's bound)."""
    ref = _reference(c) if forward_only else head_reference(c)
    m = dict(pre=ref["pre"]["value"].abs() / ref["pre"]["bound"])
    if not forward_only:
        df = ref["df"]["value"].abs()
        m["huber"] = (df - c.beta).abs() / ref["out"]["bound"]
        m["sign"] = df / ref["out"]["bound"]
    return m


# ------------------------------------------------------------------ the check
def compare(got, entry):
    """``got`` against a reference entry: the worst ``error / bound`` ratio (a record), whether every element is inside its
    bound, and the global figure ``max|got - ref| / max|ref|``.  A NaN anywhere fails both."""
    ref, bound = entry["value"], entry["bound"]
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    inside = bool((err <= bound).all())
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    worst = float(err.max()) if err.numel() else 0.0
    glob = worst / scale if scale > 0 else (0.0 if worst == 0 else float("inf"))
    return dict(ratio=float(ratio.max()) if ratio.numel() else 0.0, inside=inside, glob=glob,
                nan=bool(torch.isnan(got).any()))


def check_all(tag, results, ref, names=None, global_tol=GLOBAL_TOL):
    """Print every tensor's figures, then assert: per element ``|got - ref| <= k 2^-24 A``, no NaN, and (as the existing
    head test) ``max|got - ref| <= 1e-5 max|ref|`` (``global_tol``).  Returns ``{name: ratio}``."""
    figs = {name: compare(results[name], ref[name]) for name in (names or results)}
    for name, f in figs.items():
        print(f"{tag} {name}: error/bound {f['ratio']:.3e}  global {f['glob']:.3e}  k <= {float(ref[name]['k'].max()):.0f}")
    bad = [(name, f) for name, f in figs.items()
           if f["nan"] or not f["inside"] or not f["glob"] <= global_tol]
    assert not bad, (tag, bad)
    return {name: f["ratio"] for name, f in figs.items()}
