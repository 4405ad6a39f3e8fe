"""Cases, fp64 restatement and per-element error bounds of BatchNorm (tests/test_bn_cases_cpu.py, tests/test_gpu_bn.py):
column statistics -> running statistics -> ``y = [relu](xhat w + b)`` -> backward, in the dense form (``BnFn``), the rows
form (``BnRowsFn``: only some rows carry a gradient) and folded into the next projection (``BnLinearFn``).

``bn_reference`` restates the chain in fp64 with plain tensor operations (no autograd) and gives every quantity the two
companions of tests/head_cases.py: a magnitude ``A >= |value|`` (same formula, subtraction turned into addition, every
operand replaced by its companion) and a count ``k``; the assertion is ``|got - ref| <= k 2^-24 A`` for every element
(``head_cases.compare`` / ``check_all``).  Rules: a sum of n operands counts ``max k_i + n - 1`` over ``sum A_i``, a product
``k_x + k_y + 1`` over ``A_x A_y``; ``C0 = 16`` once per statistic for divisions, square root, the shift and the rounding to
fp32.

Counts read from csrc/misc.hip (``chain(N, C)``):
  * ``bn_partial_kernel``'s row loop ``for (r = r0 + slot; r < r1e; r += RPB)``: ``ceil(chunk / RPB)`` additions per thread,
    with ``chunk = ceil(N / nblk)``, ``nblk = bn_blocks(N) = min(2048, ceil(N / 64))``, ``RPB = 256 / (C / 4)``;
  * its merge ``for (k = 1; k < RPB; ++k)``: ``RPB`` slots, of which only ``min(RPB, chunk)`` hold a row (the others add
    exact zeros);
  * ``bn_finalize_*_kernel`` add the workgroups' partials in fp64: no fp32 rounding, no count.

The statistics' contract is stated in reference terms only, never through a kernel's shift.  The ordinary data holds no
element beyond ``Z = 4`` standard deviations of its column (``max_z``; the planted outliers aside), so EVERY row ``s`` of it
is a legitimate shift: ``mean|x - s| <= (1 + Z) sigma`` and ``mean (x - s)^2 = var + (mean - s)^2 <= var (1 + Z^2)``.
  mean   A = mean|x| + (1 + Z) sigma,                       k = chain + C0
  var    bound = k u var (1 + Z^2) + bound(mean)^2,          k = chain + (2 chain + 1) + 1 + C0
         (the sum of squares, the square of the shifted mean -- a product of two sums --, their difference; the second
         term is what a mean off by its own bound adds to a centred sum of squares: the rounding of the mean, all that a
         constant column's variance may be; as a magnitude: A = var (1 + Z^2) + bound(mean)^2 / (k u))
  rstd   from the variance's bound over ``var + eps``: A = rstd (1 + A_var / (2 (var + eps))), k = k_var
Batch statistics do not depend on the order of the rows: an "outlier first" case (row 0 at 1e2 .. 1e4 sigma) is its
"typical first" twin with rows 0 and 1 swapped, and takes the twin's statistics, reference and bound.

How sharp this is: the statistics' own bounds are a few hundred times what a correct kernel shows (error / bound 1e-4 ..
0.27 on the MI355X), sharp enough for one column's rstd off by 1e-4, a row left out, or ``1 / N`` for ``1 / (N - 1)``.
Behind them the rules multiply companions: ``A_xhat = (|x| + A_mean) A_rstd`` is tens of times ``|xhat|`` in an ordinary
column and thousands in a large-offset one (where fp32 holds ``x - mean`` to 1e-5 sigma at best), and the training-mode
grad_x, which contains ``xhat`` twice, shows 1e-8 .. 3e-2 of its bound (y: 3e-5 .. 0.11; eval mode, without batch
statistics: up to 0.16 for both).  Those bounds still catch every structural defect of ``DEFECTS`` (a wrong row count,
mask, divisor or column), not a last-digit error of grad_x.

The only kink is ReLU at ``y = 0``; ``margins`` gives ``|y_ref| / bound(y)`` and the generator nudges ``x`` until every
element is at least ``MARGIN = 4`` bounds away (an exact zero behind ``w = b = 0`` -- the last column -- has no rounding
and counts as infinitely far).  Nothing here touches the GPU; every case and reference is built once and shared."""
import functools
import types

import numpy as np
import torch

from head_cases import C0, MARGIN, U, check_all, compare      # noqa: F401  (re-exported: the checks are the head's)

Z = 4.0
EPS = float(np.float32(1e-5))             # what the kernels receive: ``float eps``, ``float momentum``
MOMENTUM = float(np.float32(0.1))
LEVELS = (1e2, 1e3, 1e4)
CONSTANT = float(np.float32(0.7))         # not a dyadic number: its fp32 column sums round (DEFECTS: variance_not_clamped)
FOLD_OUT = 256                            # two heads of 128 columns for the logits epilogue


# ------------------------------------------------------------------ the kernels' chunking
def chunking(N, C):
    """``(nblk, chunk, RPB)`` of bn_partial_kernel for N rows of C columns."""
    nblk = min(2048, max(1, (N + 63) // 64))
    return nblk, -(-N // nblk), 256 // (C // 4)


def chain(N, C):
    nblk, chunk, rpb = chunking(N, C)
    return -(-chunk // rpb) + min(rpb, chunk)


# ------------------------------------------------------------------ case tables
_SHAPES = {4: (2, 65, 4099), 20: (3, 64, 129, 131073), 128: (2, 63, 65, 4099), 344: (3, 64, 129), 516: (63, 129, 4099),
           1024: (2, 3, 64, 65)}
_SETTINGS = [(True, True), (True, False), (True, True), (False, True), (True, True), (True, False), (False, False)]     # (training, relu)
_OUTLIER_SHAPES = [(65, 4), (131073, 20), (4099, 128), (129, 344), (4099, 516), (64, 1024)]


def _cases():
    out, i = {}, 0
    for C, ns in _SHAPES.items():
        for N in ns:
            training, relu = (True, True) if N == 131073 else _SETTINGS[i % len(_SETTINGS)]     # the trip case trains
            out[f"n{N}_c{C}_{'train' if training else 'eval'}_{'relu' if relu else 'lin'}"] = dict(
                N=N, C=C, training=training, relu=relu, kind="typical", seed=7000 + i)
            i += 1
    for j, (N, C) in enumerate(_OUTLIER_SHAPES):
        cfg = dict(N=N, C=C, training=True, relu=j not in (0, 4), rot=2 - j % 3, seed=9000 + j)
        out[f"twin_n{N}_c{C}"] = dict(cfg, kind="twin")
        out[f"outlier_n{N}_c{C}"] = dict(cfg, kind="outlier", twin=f"twin_n{N}_c{C}")
    return out


CASES = _cases()
FOLD_CASES = {f"fold_n{N}_c{C}": dict(N=N, C=C, training=True, relu=True, kind="fold", seed=11000 + N + C)
              for C in (32, 128) for N in (77, 4099)}
ALL_CASES = {**CASES, **FOLD_CASES}


def family(c):
    return ("ordinary", "offset", "constant", "tiny")[c % 4]


def outlier_level(cfg, c):
    return LEVELS[(c // 4 + cfg.get("rot", 0)) % 3]


def _draw_columns(cfg, cols, gen):
    """Fresh fp32 columns: unit normals clipped at 3 (so that no element ends beyond Z sigma of the column it is in)."""
    N = cfg["N"]
    z = torch.randn(N, len(cols), generator=gen, dtype=torch.float64).clamp(-3.0, 3.0)
    x = torch.empty(N, len(cols), dtype=torch.float64)
    for i, c in enumerate(cols):
        fam = family(c)
        if fam == "ordinary":
            s = (0.25, 1.0, 4.0)[(c // 4) % 3]
            x[:, i] = z[:, i] * s + s * (float(torch.rand((), generator=gen)) * 2 - 1)
            if cfg["kind"] == "twin" and N > 1:
                x[1, i] = x[1, i] + outlier_level(cfg, c) * s * (1 if (c // 4) % 2 == 0 else -1)
        elif fam == "offset":
            x[:, i] = 100.0 + 0.1 * z[:, i]
        elif fam == "constant":
            x[:, i] = CONSTANT
        else:
            x[:, i] = 0.5 + 1e-3 * z[:, i]
    return x.float()


@functools.lru_cache(maxsize=None)
def bn_case(name):
    """The inputs of case ``name`` (fp32 on the host), nudged until the ReLU kink is at least MARGIN bounds away."""
    cfg = ALL_CASES[name]
    if cfg["kind"] == "outlier":
        t = bn_case(cfg["twin"])
        c = types.SimpleNamespace(**vars(t))
        c.name, c.cfg = name, cfg
        perm = torch.arange(t.N)
        perm[0], perm[1] = 1, 0
        c.x, c.g = t.x[perm].contiguous(), t.g[perm].contiguous()
        return c
    gen = torch.Generator().manual_seed(cfg["seed"])
    N, C = cfg["N"], cfg["C"]
    c = types.SimpleNamespace(name=name, cfg=cfg, N=N, C=C, training=cfg["training"], relu=cfg["relu"], steps=2)
    sign = lambda n: torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)      # noqa: E731
    c.w = (0.75 + 1.25 * torch.rand(C, generator=gen)) * sign(C)
    c.b = (0.25 + 0.25 * torch.rand(C, generator=gen)) * sign(C)
    c.w[C - 1] = 0.0            # the dead column: y = 0 exactly, the mask ``y > 0`` is off for every row of it
    c.b[C - 1] = 0.0
    c.rm0 = torch.randn(C, generator=gen) * 0.5
    c.rv0 = 0.5 + torch.rand(C, generator=gen)
    c.x = _draw_columns(cfg, list(range(C)), gen)
    c.g = torch.randn(N, C, generator=gen) * torch.tensor([0.25, 1.0, 4.0])[torch.randint(0, 3, (N, 1), generator=gen)]
    if cfg["kind"] == "fold":
        c.lin = torch.randn(FOLD_OUT, C, generator=gen) / C ** 0.5
        c.gz = torch.randn(N, FOLD_OUT, generator=gen)
    c.rounds = 0
    for c.rounds in range(1, 33):
        if not c.relu:
            break
        ref = _reference(c, forward_only=True)
        m = _margin_of(ref)
        bad = m < MARGIN
        if not bool(bad.any()):
            break
        cols = torch.nonzero(bad.any(0)).view(-1).tolist()
        assert all(family(j) != "constant" for j in cols), (name, cols)
        if N <= 3 and c.training:           # a nudge would move the statistics as much as the element: redraw the columns
            c.x[:, cols] = _draw_columns(cfg, cols, gen)
            continue
        # move the element to 6 bounds from the kink, on the side it is on: xhat = (+-6 bound - b) / w
        y, bound = ref["ypre"]["value"], ref["ypre"]["bound"]
        target = torch.where(y >= 0, 6.0, -6.0) * bound
        xhat = (target - c.b.double()) / c.w.double()
        xn = (ref["mean"]["value"] + xhat / ref["rstd"]["value"]).float()
        c.x = torch.where(bad, xn, c.x)
    return c


def rows_index(c, n):
    """``n`` unique, unsorted rows (the rows form's ``idx``)."""
    gen = torch.Generator().manual_seed(c.cfg["seed"] * 31 + n)
    idx = torch.randperm(c.N, generator=gen)[:n]
    return idx.flip(0) if n > 1 and torch.equal(idx, idx.sort().values) else idx


def rows_counts(N):
    return sorted({0, 1, max(1, N // 10), N})


# ------------------------------------------------------------------ the chain, in any dtype
DEFECTS = {
    "chunk_last_row_skipped": "the last row of the first workgroup's chunk is left out of the statistics' sums",
    "running_var_biased": "running_var takes the biased variance",
    "rows_inv_n_consumed": "the rows-form backward divides by the consumed rows instead of all rows",
    "relu_mask_at_zero": "the ReLU mask taken at y >= 0",
    "partial_from_neighbour": "column 0 takes its statistics from column 1's partials",
    "variance_not_clamped": "the variance as E[x^2] - E[x]^2 without the clamp at 0",
}


def _evaluate(c, dtype, defect=None, rows=None):
    """The chain with plain tensor operations in ``dtype`` (statistics centred: two passes); ``defect``: one of DEFECTS
    planted; ``rows``: the rows form with that many consumed rows (the others' gradient is zero)."""
    assert defect is None or defect in DEFECTS
    x, w, b, g = (t.to(dtype) for t in (c.x, c.w, c.b, c.g))
    N, C = c.N, c.C
    res = {}
    if rows is not None:
        idx = rows_index(c, rows)
        keep = torch.zeros(N, 1, dtype=dtype)
        keep[idx] = 1
        g = g * keep
        res["idx"] = idx
    if c.training:
        xs, cnt = x, torch.ones(N, 1, dtype=dtype)
        if defect == "chunk_last_row_skipped":
            cnt = cnt.clone()
            cnt[chunking(N, C)[1] - 1] = 0
        mean = (xs * cnt).sum(0) / N
        var = (((xs - mean) ** 2) * cnt).sum(0) / N
        if defect == "variance_not_clamped":
            var = (x * x).sum(0) / N - mean * mean
        if defect == "partial_from_neighbour":
            mean, var = mean.clone(), var.clone()
            mean[0], var[0] = mean[1], var[1]
        rstd = 1.0 / torch.sqrt(var + EPS)
        unb = var if (defect == "running_var_biased" or N == 1) else var * (N / (N - 1.0))
        rm, rv = c.rm0.to(dtype), c.rv0.to(dtype)
        for _ in range(c.steps):
            rm = (1.0 - MOMENTUM) * rm + MOMENTUM * mean
            rv = (1.0 - MOMENTUM) * rv + MOMENTUM * unb
        res.update(var=var, running_mean=rm, running_var=rv)
    else:
        mean = c.rm0.to(dtype)
        rstd = 1.0 / torch.sqrt(c.rv0.to(dtype) + EPS)
    xhat = (x - mean) * rstd
    ypre = xhat * w + b
    y = torch.relu(ypre) if c.relu else ypre
    mask = ((ypre >= 0) if defect == "relu_mask_at_zero" else (ypre > 0)) if c.relu else torch.ones_like(ypre, dtype=torch.bool)
    res.update(mean=mean, rstd=rstd, xhat=xhat, ypre=ypre, y=y, mask=mask)
    if c.cfg["kind"] == "fold":
        lin, gz = c.lin.to(dtype), c.gz.to(dtype)
        res["z"] = y @ lin.t()
        res["grad_lin"] = gz.t() @ y
        g = gz @ lin
    gm = g * mask.to(dtype)
    gb = gm.sum(0)
    gw = (gm * xhat).sum(0)
    if c.training:
        inv = 1.0 / (rows if (defect == "rows_inv_n_consumed" and rows) else N)
        gx = w * rstd * (gm - gb * inv - xhat * gw * inv)
    else:
        gx = gm * w * rstd
    res.update(g=g, grad_x=gx, grad_weight=gw, grad_bias=gb)
    return res


STATS = ("mean", "rstd", "running_mean", "running_var")
CHECKED = ("mean", "rstd", "running_mean", "running_var", "y", "grad_x", "grad_weight", "grad_bias")
FOLD_CHECKED = ("mean", "rstd", "running_mean", "running_var", "z", "grad_x", "grad_weight", "grad_bias", "grad_lin")


def _add(*ops):
    return sum(a for a, _ in ops), functools.reduce(torch.maximum, [torch.as_tensor(k, dtype=torch.float64) for _, k in ops]) + (len(ops) - 1)


def _mul(x, y):
    return x[0] * y[0], torch.as_tensor(x[1], dtype=torch.float64) + y[1] + 1


def stat_companions(x64, mean, var, ks, k_merge=0, rm0=None, rv0=None, steps=0):
    """``{name: (A, k)}`` of the batch statistics of ``x64`` under the contract at the top.  ``ks``: additions on a thread's
    chain plus slots merged; ``k_merge``: further roundings per merged slot (the GATConv epilogue's Chan merges)."""
    N = x64.shape[0]
    sigma = var.sqrt()
    k1 = float(ks + k_merge)
    out = {"mean": (x64.abs().mean(0) + (1 + Z) * sigma, k1 + C0)}
    a_mean, k_mean = out["mean"]
    k_var = k1 + (2 * k1 + 1) + 1 + C0
    out["var"] = (var * (1 + Z * Z) + (k_mean * U * a_mean) ** 2 / (k_var * U), k_var)      # bound = k u var (1 + Z^2) + bound(mean)^2
    a_var = out["var"][0]
    rstd = 1.0 / torch.sqrt(var + EPS)
    out["rstd"] = (rstd * (1 + 0.5 * a_var / (var + EPS)), k_var)
    if rm0 is not None:
        a_rm, a_rv = rm0.double().abs(), rv0.double().abs()
        a_unb = a_var * (N / (N - 1.0)) if N > 1 else a_var
        for s in range(steps):      # every step: one sum of two terms, rounded to fp32
            a_rm = (1.0 - MOMENTUM) * a_rm + MOMENTUM * a_mean
            a_rv = (1.0 - MOMENTUM) * a_rv + MOMENTUM * a_unb
        out["running_mean"] = (a_rm, k_mean + steps)
        out["running_var"] = (a_rv, k_var + steps)
    return out


def _companions(c, r, rows=None):
    """``{name: (A, k)}`` for ``r = _evaluate(c, float64, rows=rows)``."""
    N, C = c.N, c.C
    x, w, b = c.x.double().abs(), c.w.double().abs(), c.b.double().abs()
    if c.training:
        q = stat_companions(c.x.double(), r["mean"], r["var"], chain(N, C), 0, c.rm0, c.rv0, c.steps)
    else:           # the running statistics as they stand; rstd = rsqrt(running_var + eps) in fp32
        q = {"mean": (c.rm0.double().abs(), 0.0), "rstd": (r["rstd"], float(C0))}
    # y = fmaf((x - mean) rstd, w, b)  (bn_apply_kernel)
    q["xhat"] = _mul(_add((x, 0.0), q["mean"]), q["rstd"])
    q["ypre"] = _add(_mul(q["xhat"], (w, 0.0)), (b, 0.0))
    q["y"] = q["ypre"]
    mask = r["mask"].double()
    if c.cfg["kind"] == "fold":
        lin, gz = c.lin.double().abs(), c.gz.double().abs()
        # the projection's operand: scale = rstd w, shift = b - mean scale (torch, fp32), relu(fmaf(x, scale, shift));
        # the same magnitude as y's, two roundings more
        a_y, k_y = q["y"]
        yf = (a_y * mask, k_y + 2)
        q["z"] = ((yf[0] @ lin.t()), yf[1].max() + C)                       # C products on the MFMA's chains, any order
        q["grad_lin"] = (gz.t() @ yf[0], yf[1].max() + 1 + N)               # N products, over split-K planes, any order
        g = (gz @ lin, float(FOLD_OUT + 1))                                 # grad_y: FOLD_OUT products
    else:
        g = (r["g"].abs(), 0.0)
    # column sums over the rows that carry a gradient: bn_partial_kernel<1> over n rows (rows form) or all N
    kc = chain(rows, C) if rows else chain(N, C)
    gm = (g[0] * mask, g[1])
    q["grad_bias"] = (gm[0].sum(0), torch.as_tensor(gm[1], dtype=torch.float64).max() + kc + C0)
    t = _mul(gm, q["xhat"])
    q["grad_weight"] = (t[0].sum(0), t[1].max() + kc + C0)
    wr = _mul((w, 0.0), q["rstd"])
    if c.training:      # w rstd (g' - gb / N - xhat gw / N)  (bn_bwd_apply_kernel)
        inner = _add(gm, (q["grad_bias"][0] / N, q["grad_bias"][1] + 2), _mul(q["xhat"], (q["grad_weight"][0] / N, q["grad_weight"][1] + 2)))
        q["grad_x"] = _mul(inner, wr)
    else:
        q["grad_x"] = _mul(gm, wr)
    return q


def _reference(c, forward_only=False, rows=None):
    r = _evaluate(c, torch.float64, rows=rows)
    q = _companions(c, r, rows)
    ref = {}
    for name, (A, k) in q.items():
        if forward_only and name not in ("mean", "rstd", "ypre", "y"):
            continue
        k = torch.as_tensor(k, dtype=torch.float64)
        ref[name] = dict(value=r[name], A=A, k=k, bound=k * U * A)
        assert bool((A * (1 + 1e-12) >= r[name].abs()).all()), name      # a companion below its value: a derivation error
    ref["mask"] = r["mask"]
    if rows is not None:
        ref["idx"] = r["idx"]
    return ref


@functools.lru_cache(maxsize=None)
def bn_reference(name, rows=None):
    """``{quantity: dict(value, A, k, bound)}`` in fp64 for case ``name`` (cached).  An outlier-first case takes its
    statistics, their values and their bounds, from its typical-first twin."""
    c = bn_case(name)
    ref = _reference(c, rows=rows)
    if c.cfg["kind"] == "outlier":
        twin = bn_reference(c.cfg["twin"])
        for s in STATS + ("var",):
            ref[s] = twin[s]
    return ref


def _margin_of(ref):
    y, bound = ref["ypre"]["value"].abs(), ref["ypre"]["bound"]
    inf = torch.full_like(y, float("inf"))
    return torch.where(bound > 0, y / bound.clamp_min(1e-300), torch.where(y == 0, inf, torch.zeros_like(y)))


def margins(name):
    """``|y_ref| / bound(y)`` per element before the ReLU (all ``inf`` without one): the distance from the only kink."""
    c = bn_case(name)
    m = _margin_of(bn_reference(name))
    return m if c.relu else torch.full_like(m, float("inf"))


def max_z(name):
    """The largest ``|x - mean| / sigma`` over the elements that are not planted outliers (0 where sigma = 0 and the column is
    constant)."""
    c = bn_case(name)
    x = c.x.double()
    mean = x.mean(0)
    sigma = ((x - mean) ** 2).mean(0).sqrt()
    dev = (x - mean).abs()
    if c.cfg["kind"] in ("twin", "outlier"):
        row = 1 if c.cfg["kind"] == "twin" else 0
        ordinary = torch.tensor([family(j) == "ordinary" for j in range(c.C)])
        dev[row, ordinary] = 0
    z = torch.where(sigma > 0, dev / sigma.clamp_min(1e-300), torch.where(dev == 0, torch.zeros_like(dev), torch.full_like(dev, float("inf"))))
    return float(z.max())


# ------------------------------------------------------------------ statistics from the GATConv epilogue's partials
GAT_WIDTHS = (16, 128, 1024)              # heads * C at heads = 4
GAT_OUTLIER = 100.0                       # every 1000th row of the ordinary columns, in units of the column's scale


def gat_lanes(HC):
    """``(TPR, RPB)`` of GatCfg<4, HC / 4> (csrc/gat.hip): threads per row, rows (lane groups) per workgroup."""
    tpr = min(HC // 4, 64)
    return tpr, 256 // tpr


def gat_chain(N, HC, nblk):
    """``(run, chain, merge)`` of gat_fwd_kernel's statistics: a lane group adds its own ``run`` rows (shifted by the first
    of them), the workgroup merges ``RPB`` groups with Chan's formula -- forming (mean, M2) takes 4 roundings per group, a
    merge 6 more (``dl``, ``fb``, ``w``, the mean's fmaf, ``dl dl w``, two additions) --, bn_finalize_chan_kernel merges the
    workgroups in fp64."""
    rpb = gat_lanes(HC)[1]
    chunk = -(-(-(-N // nblk)) // rpb) * rpb
    run = chunk // rpb
    return run, run + rpb, 10 * rpb


@functools.lru_cache(maxsize=None)
def partials_input(N, HC, family_name):
    """``z`` (fp32) for the edge-free GATConv in front of the statistics: ``ordinary`` columns only, the four families of
    the other cases (``offset``: the large-offset columns among them), or those with an outlier every 1000th row."""
    gen = torch.Generator().manual_seed(13000 + N + HC)
    cfg = dict(N=N, kind="typical")
    cols = [4 * (j % 3) for j in range(HC)] if family_name == "ordinary" else list(range(HC))     # 0, 4, 8: the three scales
    z = _draw_columns(cfg, cols, gen)
    if family_name == "outlier":
        for j in range(HC):
            if family(j) == "ordinary":
                z[999::1000, j] += GAT_OUTLIER * (0.25, 1.0, 4.0)[(j // 4) % 3]
    return z


def stats_reference(x64, ks, k_merge, rm0, rv0, steps):
    """The batch statistics of ``x64`` in fp64 with the contract's bounds (``stat_companions``)."""
    N = x64.shape[0]
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    unb = var * (N / (N - 1.0))
    rm, rv = rm0.double(), rv0.double()
    for _ in range(steps):
        rm = (1.0 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1.0 - MOMENTUM) * rv + MOMENTUM * unb
    val = dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + EPS), running_mean=rm, running_var=rv)
    ref = {}
    for name, (A, k) in stat_companions(x64, mean, var, ks, k_merge, rm0, rv0, steps).items():
        k = torch.as_tensor(k, dtype=torch.float64)
        ref[name] = dict(value=val[name], A=A, k=k, bound=k * U * A)
    return ref
