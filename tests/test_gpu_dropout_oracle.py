"""GPU: dropout-ON train steps against the fp64 oracle running the SAME dropout realisation.

The masks of the fused ``leaky_relu + dropout`` epilogues are no random stream: ``keep = hash(seed, step, flat element
index) >= p`` (include/qot_gnn.h).  ``oracle/dropout.py`` restates that on the host, so the oracle can be the checker
with dropout on, at the bar every ``p = 0`` parity test uses (``TOL = 1e-4``, the metric of ``helpers.grad_compare``).

* the mask itself: ``qot_act_fwd`` on all-ones input against ``oracle.dropout.keep_mask``, element for element, at the
  sizes, steps, seeds and probabilities where an indexing or rounding slip would show.  NOT covered: the ``idx4 >> 32``
  term of the hash, which needs an activation of more than 2^34 elements;
* one train step, forward and every parameter gradient, in every form conv1, conv2 and the read-out can take
  (``dropout_cases.CASES``; the forced kernels are asserted to have run through a spy on ``_lib.call``);
* two steps on one model: new masks, still the oracle's; a retained-graph second backward and a backward that runs after
  the counter has moved on both regenerate their own forward's draw;
* ``LightpathGNN``: its only dropout is torch's ``nn.Dropout`` in the MLP; the mask is read off a forward hook.

The step of a forward's draw: ``int(model._qot_step)`` before the forward, plus one (the counter is incremented, then
snapshotted).  Every test prints its figures before it asserts (``pytest -s``).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_cases as DC
from helpers import TOL, grad_compare, rel_err

pytestmark = pytest.mark.gpu


def _record(monkeypatch):
    """``[(name, args)]`` of the C entry points called from here on."""
    from gnn_qot_estimation_amd import _lib
    calls = []
    real = _lib.call

    def call(name, *args):
        calls.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return calls


def _head_hook(module, store):
    """torch's ``nn.Dropout`` draws from the device generator: read its realisation off the module's input and output
    (an element that comes out non-zero was kept; one that went in as zero says nothing and counts as kept)."""
    def hook(mod, inp, out):
        store.append(((out != 0) | (inp[0] == 0)).detach().cpu())
    return module.register_forward_hook(hook)


# ===================================================================== a. the mask, element for element
_SIZES = [(1,), (3,), (5,), (4 * 257 + 1,), (4 * 257 + 2,), (4 * 257 + 3,), (33, 16), (7, 48), ((1 << 20) + 3,)]
_STEPS = [0, 1, 1 << 31, 1 << 40]                                      # step * golden ratio wraps around 2^64
_SEEDS = [12345, (1 << 63) | 0x9E3779B9, (1 << 64) - 1]                # site seeds use all 64 bits
_PS = [0.1, 0.3, 0.5, 0.9, 0.99999]                                    # 0.99999: the threshold clamps at 65535


@pytest.mark.parametrize("p", _PS)
def test_mask_known_answer(cuda_device, p):
    from gnn_qot_estimation_amd import functional as QF
    from oracle import dropout as OD
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert OD.keep_scale(p) == scale
    for shape in _SIZES:
        for seed in _SEEDS:
            for step in _STEPS:
                x = torch.ones(*shape, device=cuda_device, requires_grad=True)
                y = QF.ActFn.apply(x, 0.01, p, seed, torch.tensor(step, dtype=torch.long, device=cuda_device))
                keep = OD.keep_mask(seed, step, shape, p)
                got = y.detach().cpu()
                assert torch.equal(got != 0, keep), (shape, seed, step, p, int(((got != 0) != keep).sum()))
                assert torch.equal(got[keep], torch.full((int(keep.sum()),), float(scale))), (shape, seed, step, p)
                y.backward(torch.ones_like(y))                         # the backward regenerates the same mask
                assert torch.equal(x.grad.cpu(), got), (shape, seed, step, p)
    big = OD.keep_mask(_SEEDS[1], 1 << 40, _SIZES[-1], p)
    n, q = big.numel(), OD.thr16(p) / 65536.0
    assert abs(float((~big).sum()) - n * q) <= 3.0 * (n * q * (1.0 - q)) ** 0.5 + 1.0


# ===================================================================== b. one train step against the masked oracle
def _hip_step(case, hip, dbatch, y_dev):
    """One forward of the HIP model (``forward_loss`` where the case says so); returns ``(out, backward)``."""
    if case["loss"]:
        out, loss, g = hip.forward_loss(dbatch, y_dev, beta=1.0)
        return out, (lambda **kw: out.backward(g, **kw)), loss
    out = hip(dbatch)
    loss = F.smooth_l1_loss(out, y_dev)
    return out, (lambda **kw: loss.backward(**kw)), loss


def _oracle_step(case, ref, batch64, keep):
    out = ref(batch64, keep=keep)
    loss = F.smooth_l1_loss(out, batch64.y.view(-1, 3))
    ref.zero_grad(set_to_none=True)
    loss.backward()
    return out, loss


def _setup(name, device, monkeypatch):
    case = DC.CASES[name]
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    batch = case["batch"]()
    ref, hip = DC.models(case, device)
    for k, v in case["attrs"].items():
        setattr(hip, k, v)
    hip._qot_seed = DC.SEED
    ref.double().train()
    hip.train()
    return case, batch, DC.to_double(batch), batch.to(device), ref, hip


def _check_forms(case, calls):
    names = [n for n, _ in calls]
    for n in case["called"]:
        assert n in names, (n, sorted(set(names)))
    for n in case["not_called"]:
        assert n not in names, (n, sorted(set(names)))
    if case["fold"] is not None:
        # qot_head_bwd(..., x_in, in_slope, in_p, in_seed, in_step) / qot_head_train(..., fold, in_slope, in_p, in_seed,
        # in_step): the fifth argument from the end says whether the last conv's activation backward was folded in
        folded = [bool(a[-5]) for n, a in calls if n in ("qot_head_bwd", "qot_head_train")]
        assert folded and all(f == case["fold"] for f in folded), folded


@pytest.mark.parametrize("name", list(DC.CASES))
def test_train_step_matches_the_masked_oracle(cuda_device, monkeypatch, name):
    case, batch, batch64, dbatch, ref, hip = _setup(name, cuda_device, monkeypatch)
    p = case["model"]["dropout_p"]
    hooked = []
    if case["head_hook"]:
        _head_hook(hip.mlp[2], hooked)
    if name == "padded_h48":
        assert hip._qot_hp == 64
    calls = _record(monkeypatch)
    draw = int(hip._qot_step) + 1
    y_dev = dbatch.y.view(-1, 3)
    out, backward, loss = _hip_step(case, hip, dbatch, y_dev)
    backward()
    torch.cuda.synchronize()
    assert int(hip._qot_step) == draw
    keep = DC.masks(case, batch, draw, head=not case["head_hook"])
    if case["head_hook"]:
        assert len(hooked) == 1
        keep["head"] = hooked[0]
    drop_rate = 1.0 - float(keep["conv1"].float().mean())
    out_ref, loss_ref = _oracle_step(case, ref, batch64, keep)
    e_out = rel_err(out, out_ref)
    print(f"\n[dropout step] {name}: p {p} conv1 drop rate {drop_rate:.3f} out {e_out:.2e}", end="")
    assert e_out <= TOL, e_out
    if case["loss"]:
        e_loss = abs(float(loss) - float(loss_ref)) / max(abs(float(loss_ref)), 1e-12)
        print(f" loss {e_loss:.2e}", end="")
        assert e_loss <= TOL, e_loss
    worst = grad_compare(ref, hip)
    print(f" grads {worst:.2e}")
    _check_forms(case, calls)


def test_two_steps_draw_new_masks_and_a_second_backward_reuses_its_draw(cuda_device, monkeypatch):
    case, batch, batch64, dbatch, ref, hip = _setup("head_fused_fold", cuda_device, monkeypatch)
    y_dev = dbatch.y.view(-1, 3)
    outs = []
    for step in (1, 2):
        hip.zero_grad(set_to_none=True)
        out = hip(dbatch)
        assert int(hip._qot_step) == step
        loss = F.smooth_l1_loss(out, y_dev)
        loss.backward(retain_graph=True)
        first = {k: v.grad.clone() for k, v in hip.named_parameters()}
        keep = DC.masks(case, batch, step)
        out_ref, _ = _oracle_step(case, ref, batch64, keep)
        assert rel_err(out, out_ref) <= TOL
        grad_compare(ref, hip)
        # the retained graph once more: the same draw (the counter has not moved, and would not matter if it had)
        hip.zero_grad(set_to_none=True)
        loss.backward()
        assert int(hip._qot_step) == step
        for k, v in hip.named_parameters():
            assert torch.equal(v.grad, first[k]), k
        outs.append((out.detach().clone(), keep))
    (o1, k1), (o2, k2) = outs
    for site in k1:
        assert not torch.equal(k1[site], k2[site]), site
    assert not torch.equal(o1, o2)


def test_backward_reads_the_snapshot_of_its_forward_not_the_live_counter(cuda_device, monkeypatch):
    """The counter moves on between a forward and its backward (as it does when another forward runs in between): the
    backward must regenerate the masks of the step its forward snapshotted."""
    case, batch, batch64, dbatch, ref, hip = _setup("head_fused_fold", cuda_device, monkeypatch)
    out = hip(dbatch)
    assert int(hip._qot_step) == 1
    hip._qot_step.add_(5)
    F.smooth_l1_loss(out, dbatch.y.view(-1, 3)).backward()
    torch.cuda.synchronize()
    assert int(hip._qot_step) == 6
    out_ref, _ = _oracle_step(case, ref, batch64, DC.masks(case, batch, 1))
    assert rel_err(out, out_ref) <= TOL
    grad_compare(ref, hip)


# ===================================================================== d. LightpathGNN
@pytest.mark.parametrize("thin", [False, True])
def test_lightpath_train_step_with_dropout(cuda_device, monkeypatch, thin):
    import gnn_qot_estimation_amd as q
    from gnn_qot_estimation_amd import synthetic as S
    from oracle import sparse as O
    monkeypatch.setenv("QOT_GAT_THIN_MIN_ROWS", "1" if thin else "1000000000")
    batch = S.lightpath_batch(64)
    kw = dict(in_channels=5, hidden_channels=32, output_dim=3, is_lut_index=1, dropout_p=0.5)
    torch.manual_seed(0)
    ref, hip = O.LightpathGNN(**kw), q.LightpathGNN(**kw)
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1 and p.abs().max() == 0:
                p.uniform_(-0.1, 0.1)
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip.to(cuda_device).train()
    ref.double().train()
    hooked = []
    _head_hook(hip.mlp[2], hooked)
    calls = _record(monkeypatch)
    out, lb = hip(batch.to(cuda_device))
    assert len(hooked) == 1 and 0.3 < 1.0 - float(hooked[0].float().mean()) < 0.7
    names = [n for n, _ in calls]
    assert ("qot_gat_fwd_thin" in names) == thin, sorted(set(names))
    out_ref, lb_ref = ref(DC.to_double(batch), keep={"head": hooked[0]})
    assert torch.equal(lb.cpu(), lb_ref)
    e_out = rel_err(out, out_ref)
    assert e_out <= TOL, e_out
    y = batch.y[lb_ref]
    F.smooth_l1_loss(out_ref, y.double()).backward()
    F.smooth_l1_loss(out, y.to(cuda_device)).backward()
    worst = grad_compare(ref, hip, analytic_zero=("conv1.bias",))
    print(f"\n[dropout step] lightpath thin={thin}: out {e_out:.2e} grads {worst:.2e}")
    for k in ("running_mean", "running_var"):
        assert rel_err(getattr(hip.norm1.module, k), getattr(ref.norm1.module, k)) <= TOL
