"""Every backward form at the gradient scales training has (tests/grad_scale_cases.py): the forward runs once, then
``c * g`` is back-propagated for c in {2^-30, 2^-15, 1, 2^15, 2^30} and, at c = 1, ``g`` with a NaN row and with one +inf.

  check 1  every returned gradient against fp64 on the tensor's OWN scale: max|got / c - ref| <= TOL * max|ref|
           (helpers.TOL = 1e-4; analytically zero tensors on the scale of the tensor the case table names).  The worst
           per-element figure |got / c - ref| / (|ref| + 1e-6 max|ref|) is printed, not asserted;
  check 2  against the sibling implementation: error vs fp64 <= 2x (max) and 1.5x (RMS) the sibling's at the same c, plus
           the floors 1e-7 / 1e-8 of tests/test_gpu_nnconv_split_bf16.py (relative to max|ref|, i.e. scaled by c);
  check 3  homogeneity, bit for bit: grads(c g) == c * grads(g) (c is a power of two), except the tensors summed with
           fp32 atomics, each named in the case table with the atomic's file and line;
  check 4  wherever the fp64 gradient of a poisoned ``g`` is non-finite, the kernel's is non-finite too.

Every figure is printed before anything is asserted (``pytest -s``).  The GPU results of a (case, switches) pair are
computed once and shared by the four checks."""
import math

import pytest
import torch

import grad_scale_cases as G
from helpers import TOL

pytestmark = pytest.mark.gpu

_SWITCHES = ("QOT_TCONV_ROWS_PARTS", "QOT_NO_TCONV_SCORES", "QOT_NO_TCONV_GRAPH", "QOT_NO_TCONV_ROWS", "QOT_NO_TCONV_TILE", "QOT_NO_TCONV_FWD_ROWS",
             "QOT_NNCONV_F32_MFMA", "QOT_SPLIT_NNCONV_BWD", "QOT_GAT_THIN_MIN_ROWS", "QOT_NO_GAT_THIN", "QOT_NO_LAUNCH_GROUPS",
             "QOT_NO_TABLE_GEMM", "QOT_NO_HEAD_TRAIN", "QOT_NO_BN_ROWS", "QOT_FUSE_BN_PROJECTION", "QOT_NO_FUSED_LOGITS",
             "QOT_LIBRARY_GEMM", "QOT_DISABLE_GEMM_TN", "QOT_NO_GAT_BY_GRAPH")
_RUNS = {}


def _set_env(monkeypatch, env):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _record(monkeypatch):
    from gnn_qot_estimation_amd import _lib
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def _backwards(out, params, g, bad):
    """``{tag: {name: grad on the host}}``: tags are the scales and the names of the poisoned gradients."""
    res = {}
    for tag, gg in [(c, g * c) for c in G.SCALES] + list(bad.items()):
        for p in params.values():
            p.grad = None
        out.backward(gg, retain_graph=True)
        torch.cuda.synchronize()
        res[tag] = {k: p.grad.detach().cpu().clone() for k, p in params.items()}
    return res


def _tconv_run(name, dev, monkeypatch, env):
    key = ("tconv", name, tuple(sorted(env.items())))
    if key not in _RUNS:
        import gnn_qot_estimation_amd as q
        from gnn_qot_estimation_amd import functional as QF
        from gnn_qot_estimation_amd.graph import cached_i32, graph_index_for, table_maps_for
        case = G.tconv_case(name)
        c = case["cfg"]
        _set_env(monkeypatch, env)
        conv = q.nn.TransformerConv(c["H"], c["H"], edge_dim=c["D"])
        conv.load_state_dict(case["state"], strict=True)
        conv.to(dev)
        table = case["table"].to(dev).requires_grad_(True)
        batch = case["batch"].to(dev)
        calls = _record(monkeypatch)
        graph = graph_index_for(batch, batch.num_nodes)
        maps = table_maps_for(batch, graph)
        act = (G.SLOPE, 0.0, 0, None)
        if maps is None:
            x = QF.EmbedFn.apply(table, cached_i32(batch, "node_ids"))
            out = conv(x, batch.edge_index, batch.edge_attr, graph=graph, act=act)
        else:
            plan = conv.graph_form(table, graph, maps)
            if plan is not None:
                pre = conv.prepare_graph_form(table, plan)
                out = conv.forward_table_graph(table, batch.edge_attr, graph, maps, plan, pre, act=act)
            else:
                out = conv.forward_table(table, batch.edge_attr, graph, maps, act=act)
        params = dict([("table", table)] + list(conv.named_parameters()))
        grads = _backwards(out, params, case["g"].to(dev), {k: v.to(dev) for k, v in case["bad"].items()})
        _RUNS[key] = dict(calls=list(calls), grads=grads)
    return _RUNS[key]


def _nnconv_run(kind, dev, monkeypatch, env):
    key = ("nnconv", kind, tuple(sorted(env.items())))
    if key not in _RUNS:
        from gnn_qot_estimation_amd import functional as QF
        from gnn_qot_estimation_amd.graph import build_graph_index
        case = G.nnconv_case(kind)
        _set_env(monkeypatch, env)
        t = {k: v.to(dev).clone().requires_grad_(k != "ea") for k, v in case["p"].items()}
        calls = _record(monkeypatch)
        graph = build_graph_index(case["ei"].to(dev), case["N"])
        out = QF.NNConvFn.apply(t["x"], t["ea"], t["w1"], t["b1"], t["w2"], t["b2"], t["wroot"], t["bias"], graph)
        params = {k: t[k] for k in G.NNCONV_NAMES}
        grads = _backwards(out, params, case["g"].to(dev), {k: v.to(dev) for k, v in case["bad"].items()})
        _RUNS[key] = dict(calls=list(calls), grads=grads)
    return _RUNS[key]


def _model_run(name, dev, monkeypatch, env):
    key = ("model", name, tuple(sorted(env.items())))
    if key not in _RUNS:
        import gnn_qot_estimation_amd as q
        case = G.model_case(name)
        c = case["cfg"]
        _set_env(monkeypatch, env)
        hip = (q.TopologicalGNN if c["kind"] == "topo" else q.LightpathGNN)(**G.model_kwargs(c))
        hip.load_state_dict(case["state"], strict=True)
        hip.to(dev).train()
        calls = _record(monkeypatch)
        res = hip(case["batch"].to(dev))
        out = res if c["kind"] == "topo" else res[0]
        grads = _backwards(out, dict(hip.named_parameters()), case["g"].to(dev), {})
        _RUNS[key] = dict(calls=list(calls), grads=grads, out=out.detach().cpu())
    return _RUNS[key]


def _ran(calls, kernels):
    for k in kernels:
        any_of = k if isinstance(k, tuple) else (k,)
        assert any(a in calls for a in any_of), (k, sorted(set(calls)))


# ------------------------------------------------------------------ the four checks on one (run, reference) pair
def _errors(run, ref, zero, c, name):
    got = run["grads"][c][name].double() / c
    return G.tensor_errors(got, ref[name], ref[zero[name]] if name in zero else None)


def _check_fp64(tag, run, ref, zero):
    bad = []
    for c in G.SCALES:
        for name in ref:
            e = _errors(run, ref, zero, c, name)
            print(f"{tag} c=2^{round(math.log2(c))} {name}: max {e['max']:.3e} rms {e['rms']:.3e} "
                  f"per-element {e['elem']:.3e}" + (f" (scale of {zero[name]})" if name in zero else ""))
            if not e["max"] <= TOL:
                bad.append((c, name, e["max"]))
    assert not bad, (tag, bad)


def _check_sibling(tag, run, sib, ref, zero):
    bad = []
    for c in G.SCALES:
        for name in ref:
            es, en = _errors(run, ref, zero, c, name), _errors(sib, ref, zero, c, name)
            print(f"{tag} c=2^{round(math.log2(c))} {name}: max {es['max']:.3e} (sibling {en['max']:.3e}) "
                  f"rms {es['rms']:.3e} (sibling {en['rms']:.3e})")
            if not es["max"] <= G.SIBLING_MAX * en["max"] + G.FLOOR_MAX:
                bad.append((c, name, "max", es["max"], en["max"]))
            if not es["rms"] <= G.SIBLING_RMS * en["rms"] + G.FLOOR_RMS:
                bad.append((c, name, "rms", es["rms"], en["rms"]))
    assert not bad, (tag, bad)


def _check_homogeneous(tag, run, names, excepted):
    assert set(excepted) <= set(names), (tag, set(excepted) - set(names))
    bad = []
    base = run["grads"][1.0]
    for c in G.SCALES:
        for name in names:
            same = torch.equal(run["grads"][c][name], base[name] * c)
            if not same:
                d = float((run["grads"][c][name].double() / c - base[name].double()).abs().max())
                print(f"{tag} c=2^{round(math.log2(c))} {name}: not homogeneous, max |got / c - got(1)| = {d:.3e}"
                      + (f" -- excepted: {excepted[name]}" if name in excepted else ""))
                if name not in excepted:
                    bad.append((c, name, d))
    assert not bad, (tag, bad)


def _check_nonfinite(tag, run, refs):
    bad = []
    for kind in ("nan_row", "inf_element"):
        for name, r in refs[kind].items():
            want = ~torch.isfinite(r)
            got = ~torch.isfinite(run["grads"][kind][name])
            missed = int((want & ~got).sum())
            print(f"{tag} {kind} {name}: fp64 non-finite {int(want.sum())}, kernel non-finite {int(got.sum())}, "
                  f"finite where fp64 is not: {missed}")
            if missed:
                bad.append((kind, name, missed))
    assert not bad, (tag, bad)


# ------------------------------------------------------------------ TransformerConv: four forms, operator level
def _tconv(name, dev, monkeypatch, sibling=False):
    c = G.TCONV_CASES[name]
    env = dict(c.get("env", {}))
    if sibling:
        env.update(c["sibling"])
    run = _tconv_run(name, dev, monkeypatch, env)
    if sibling:
        assert "qot_tconv_bwd_dst" in run["calls"] and not any(k in run["calls"] for k in
                                                              ("qot_tconv_bwd_dst_rows", "qot_tconv_bwd_graph")), run["calls"]
    else:
        _ran(run["calls"], G.TCONV_KERNELS[c["form"]])
        if c["form"] in ("dst_table", "node"):
            assert "qot_tconv_bwd_graph" not in run["calls"] and "qot_tconv_bwd_dst_rows" not in run["calls"]
    return run


@pytest.mark.parametrize("name", list(G.TCONV_CASES))
def test_tconv_against_fp64_on_each_tensors_own_scale(cuda_device, monkeypatch, name):
    _check_fp64(name, _tconv(name, cuda_device, monkeypatch), G.tconv_case(name)["ref"][1.0], G.ZERO_TCONV)


@pytest.mark.parametrize("name", [n for n, c in G.TCONV_CASES.items() if "sibling" in c])
def test_tconv_against_the_per_destination_kernels(cuda_device, monkeypatch, name):
    run, sib = _tconv(name, cuda_device, monkeypatch), _tconv(name, cuda_device, monkeypatch, sibling=True)
    _check_sibling(name, run, sib, G.tconv_case(name)["ref"][1.0], G.ZERO_TCONV)


@pytest.mark.parametrize("name", list(G.TCONV_CASES))
def test_tconv_backward_is_homogeneous_bit_for_bit(cuda_device, monkeypatch, name):
    _check_homogeneous(name, _tconv(name, cuda_device, monkeypatch), G.TCONV_NAMES,
                       G.TCONV_CASES[name].get("inhomogeneous", {}))


@pytest.mark.parametrize("name", list(G.TCONV_CASES))
def test_tconv_non_finite_gradients_are_not_swallowed(cuda_device, monkeypatch, name):
    _check_nonfinite(name, _tconv(name, cuda_device, monkeypatch), G.tconv_case(name)["ref"])


# ------------------------------------------------------------------ NNConv at H = 64, operator level
_NN_SPLIT, _NN_F32 = {}, {"QOT_NNCONV_F32_MFMA": "1"}


def _nnconv(kind, dev, monkeypatch, env):
    run = _nnconv_run(kind, dev, monkeypatch, env)
    _ran(run["calls"], ("qot_nnconv_adjoint_dw", "qot_nnconv_gradh_fused" if env else "qot_nnconv_gradh_split"))
    return run


@pytest.mark.parametrize("mode", ["split_bf16", "f32_mfma"])
@pytest.mark.parametrize("kind", ["hub", "ragged"])
def test_nnconv64_against_fp64_on_each_tensors_own_scale(cuda_device, monkeypatch, kind, mode):
    run = _nnconv(kind, cuda_device, monkeypatch, _NN_SPLIT if mode == "split_bf16" else _NN_F32)
    _check_fp64(f"nnconv64 {kind} {mode}", run, G.nnconv_case(kind)["ref"][1.0], {})


@pytest.mark.parametrize("kind", ["hub", "ragged"])
def test_nnconv64_split_bf16_against_the_fp32_mfma_kernels(cuda_device, monkeypatch, kind):
    run, sib = _nnconv(kind, cuda_device, monkeypatch, _NN_SPLIT), _nnconv(kind, cuda_device, monkeypatch, _NN_F32)
    _check_sibling(f"nnconv64 {kind}", run, sib, G.nnconv_case(kind)["ref"][1.0], {})


@pytest.mark.parametrize("mode", ["split_bf16", "f32_mfma"])
@pytest.mark.parametrize("kind", ["hub", "ragged"])
def test_nnconv64_backward_is_homogeneous_bit_for_bit(cuda_device, monkeypatch, kind, mode):
    run = _nnconv(kind, cuda_device, monkeypatch, _NN_SPLIT if mode == "split_bf16" else _NN_F32)
    _check_homogeneous(f"nnconv64 {kind} {mode}", run, G.NNCONV_NAMES, {})


@pytest.mark.parametrize("mode", ["split_bf16", "f32_mfma"])
@pytest.mark.parametrize("kind", ["hub", "ragged"])
def test_nnconv64_non_finite_gradients_are_not_swallowed(cuda_device, monkeypatch, kind, mode):
    run = _nnconv(kind, cuda_device, monkeypatch, _NN_SPLIT if mode == "split_bf16" else _NN_F32)
    _check_nonfinite(f"nnconv64 {kind} {mode}", run, G.nnconv_case(kind)["ref"])


# ------------------------------------------------------------------ whole models (read-out, NNConv widths, LightpathGNN)
def _model(name, dev, monkeypatch, sibling=False):
    c = G.MODEL_CASES[name]
    env = dict(c.get("env", {}))
    if sibling:
        env.update(c["sibling"])
    run = _model_run(name, dev, monkeypatch, env)
    if not sibling:
        _ran(run["calls"], c.get("kernels", ()))
    return run


def _zero(name):
    return G.ZERO_TOPO if G.MODEL_CASES[name]["kind"] == "topo" else G.ZERO_LIGHTPATH


@pytest.mark.parametrize("name", list(G.MODEL_CASES))
def test_model_against_fp64_on_each_tensors_own_scale(cuda_device, monkeypatch, name):
    run, case = _model(name, cuda_device, monkeypatch), G.model_case(name)
    err = float((run["out"].double() - case["out"]).abs().max() / case["out"].abs().max())
    print(f"{name} forward: {err:.3e}")
    assert err <= TOL
    _check_fp64(name, run, case["ref"][1.0], _zero(name))


@pytest.mark.parametrize("name", [n for n, c in G.MODEL_CASES.items() if "sibling" in c])
def test_model_against_its_sibling_implementation(cuda_device, monkeypatch, name):
    """``topo_h64_b8``: split-bf16 NNConv against QOT_NNCONV_F32_MFMA=1.  In a whole model the rows of a graph share their
    incoming gradient (pool backward), so the rounding of the grad-h kernel's ``g W_k^T`` product is shared by a graph's rows
    and does not average out in the sums over its edges: the gradients of the edge MLP's first layer measure that product.
    With all six cross products of a K step in one accumulator they came out at RMS 1.31e-06 / 1.61e-06 (weight / bias)
    from fp64 against the fp32-MFMA kernels' 7.36e-07 / 6.97e-07 -- 1.78x and 2.31x; with the small products in an
    accumulator of their own (csrc/split_bf16.hpp: mfma_split6_two) 8.94e-07 / 9.70e-07, 1.22x and 1.39x."""
    run, sib = _model(name, cuda_device, monkeypatch), _model(name, cuda_device, monkeypatch, sibling=True)
    assert run["calls"] != sib["calls"]
    _check_sibling(name, run, sib, G.model_case(name)["ref"][1.0], _zero(name))


@pytest.mark.parametrize("name", list(G.MODEL_CASES))
def test_model_backward_is_homogeneous_bit_for_bit(cuda_device, monkeypatch, name):
    run = _model(name, cuda_device, monkeypatch)
    _check_homogeneous(name, run, tuple(G.model_case(name)["ref"][1.0]), G.MODEL_CASES[name].get("inhomogeneous", {}))
