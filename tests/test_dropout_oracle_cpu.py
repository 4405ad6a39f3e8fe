"""``oracle.dropout`` (the host restatement of the kernels' counter-based dropout masks) and the oracle models / training
loop that accept such masks, pinned without a GPU:

* the masks: drop rate, independence of step and site, ``p = 0``, the threshold's rounding and clamp;
* the masked oracle against a chain written out by hand; ``keep=None`` is the old forward bit for bit;
* the loop's draw counter;
* conditioning of every dropout-on single-step case (``dropout_cases.CASES``) by the rule of
  tests/test_oracle_train_loop_cpu.py: the masked oracle in fp32 against itself in fp64 with the same masks stays within
  ``TOL / 10`` in the metric of the GPU test (the dropout-on trajectory cases are members of
  ``helpers.TRAJECTORY_CASES`` and go through ``test_trajectory_case_is_well_conditioned`` there).
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_cases as DC
import helpers as H
from helpers import TOL, grad_compare, rel_err
from oracle import dropout as OD, sparse as O, train_loop as TL


# --------------------------------------------------------------------------- the masks
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5, 0.9])
def test_drop_rate_within_three_sigma(p):
    n = 1 << 20
    q = OD.thr16(p) / 65536.0
    for seed, step in ((12345, 1), ((1 << 63) | 77, 1 << 40)):
        dropped = float((~OD.keep_mask(seed, step, (n,), p)).sum())
        assert abs(dropped - n * q) <= 3.0 * (n * q * (1.0 - q)) ** 0.5, (p, seed, step, dropped / n)


def test_threshold_rounding_and_clamp():
    assert OD.thr16(0.0) == 0 and OD.thr16(0.5) == 32768 and OD.thr16(0.1) == 6554 and OD.thr16(0.9) == 58982
    assert OD.thr16(0.99999) == 65535 and OD.thr16(1.0) == 65535          # 65536 does not fit 16 bits
    assert OD.thr16(1e-6) == 0                                            # rounds to no dropout at all
    assert OD.keep_scale(0.5) == np.float32(2.0)
    assert OD.keep_scale(0.1) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))


def test_p_zero_keeps_all_and_shapes():
    assert bool(OD.keep_mask(1, 2, (7, 5), 0.0).all())
    assert OD.keep_mask(1, 2, (7, 5), 0.5).shape == (7, 5)
    assert OD.keep_mask(1, 2, (0, 16), 0.5).shape == (0, 16)
    # row-major numbering: a [N, H] mask is the flat mask reshaped, and a prefix of rows is the mask of fewer rows
    flat = OD.keep_mask(9, 3, (12 * 16,), 0.5)
    assert torch.equal(OD.keep_mask(9, 3, (12, 16), 0.5).reshape(-1), flat)
    assert torch.equal(OD.keep_mask(9, 3, (5, 16), 0.5), flat.view(12, 16)[:5])


def test_steps_and_sites_give_different_masks():
    shape, p, base = (64, 32), 0.5, (1 << 62) + 5
    seeds = [OD.site_seed(base, s) for s in ("conv1", "conv2", "conv3", "head")]
    assert seeds[0] == (base + 0x9E3779B97F4A7C15) % (1 << 64)
    assert seeds[1] == OD.site_seed(base, 2) == (base + 2 * 0x9E3779B97F4A7C15) % (1 << 64)
    assert seeds[3] == (base + 97 * 0x9E3779B97F4A7C15) % (1 << 64)
    assert len(set(seeds)) == 4 and all(0 <= s < (1 << 64) for s in seeds)
    masks = [OD.keep_mask(s, 1, shape, p) for s in seeds] + [OD.keep_mask(seeds[0], t, shape, p) for t in (0, 2, 1 << 31)]
    for i in range(len(masks)):
        for j in range(i + 1, len(masks)):
            agree = float((masks[i] == masks[j]).float().mean())
            assert 0.4 < agree < 0.6, (i, j, agree)                       # independent fair coins agree half the time
    assert torch.equal(OD.keep_mask(seeds[0], 1, shape, p), masks[0])    # and the same key gives the same mask


def test_hash_known_values_by_python_integers():
    """The vectorised uint64 arithmetic against the same formula in Python's unbounded integers."""
    def h(seed, step, idx4):
        m32 = 0xFFFFFFFF
        k = (seed ^ (step * 0x9E3779B97F4A7C15)) & ((1 << 64) - 1)
        k0, k1 = k & m32, k >> 32
        p = ((idx4 & m32) ^ k0) * 0x9E3779B1
        a = ((p >> 32) ^ (p & m32) ^ (idx4 >> 32) ^ k1) & m32
        q = a * 0x85EBCA77
        r = ((a ^ k0 ^ 0x68E31DA4) & m32) * 0xC2B2AE3D
        return ((((r >> 32) ^ r) & m32) << 32) | (((q >> 32) ^ q) & m32)
    for seed, step in ((0, 0), (12345, 1), ((1 << 64) - 1, 1 << 40), ((1 << 63) | 99, 1 << 31)):
        for thr_p in (0.3, 0.9):
            keep = OD.keep_mask(seed, step, (41,), thr_p)
            want = [((h(seed, step, f >> 2) >> (16 * (f & 3))) & 0xFFFF) >= OD.thr16(thr_p) for f in range(41)]
            assert keep.tolist() == want, (seed, step, thr_p)


def test_padded_width_masks_are_numbered_at_the_padded_width():
    keep = OD.topological_masks(7, 3, 0.5, num_nodes=10, num_graphs=2, width=48, num_layers=3)
    assert sorted(keep) == ["conv1", "conv2", "conv3", "head"]
    assert keep["conv2"].shape == (10, 48) and keep["head"].shape == (2, 48)
    assert torch.equal(keep["conv2"], OD.keep_mask(OD.site_seed(7, 2), 3, (10, 64), 0.5)[:, :48])
    assert torch.equal(keep["head"], OD.keep_mask(OD.site_seed(7, "head"), 3, (2, 64), 0.5)[:, :48])
    assert "head" not in OD.topological_masks(7, 3, 0.5, 10, 2, 32, head=False)


# --------------------------------------------------------------------------- the oracle models
def _tiny():
    import gnn_qot_estimation_amd as q
    g = torch.Generator().manual_seed(3)
    ei = torch.tensor([[0, 1, 2, 2, 3], [1, 0, 1, 3, 2]])
    d = q.Data(edge_index=ei, edge_attr=torch.rand(5, 4, generator=g, dtype=torch.float64), node_ids=torch.arange(4),
               num_nodes=4)
    return q.Batch.from_data_list([d, d])


def test_masked_topological_oracle_equals_a_chain_written_by_hand():
    torch.manual_seed(1)
    m = O.TopologicalGNN(4, 16, 3, 4, dropout_p=0.3, num_layers=3).double().train()
    b = _tiny()
    keep = OD.topological_masks(11, 5, 0.3, b.num_nodes, b.num_graphs, 16, num_layers=3)
    x = m.node_embeddings(b.node_ids)
    x = F.leaky_relu(m.conv1(x, b.edge_index, b.edge_attr)) * keep["conv1"] / (1 - 0.3)
    x = F.leaky_relu(m.conv2(x, b.edge_index, b.edge_attr)) * keep["conv2"] / (1 - 0.3)
    x = F.leaky_relu(m.conv3(x, b.edge_index, b.edge_attr)) * keep["conv3"] / (1 - 0.3)
    x = torch.stack([x[:4].mean(0), x[4:].mean(0)])
    x = F.leaky_relu(m.mlp[0](x)) * keep["head"] / (1 - 0.3)
    want = m.mlp[3](x)
    got = m(b, keep=keep)
    assert got.dtype == torch.float64 and float((got - want).detach().abs().max()) <= 1e-14
    assert torch.equal(m(b, keep=keep), got)                         # nothing random is left
    with pytest.raises(ValueError):
        m(b, keep={"conv1": keep["head"]})


def test_keep_none_is_the_old_forward_bit_for_bit():
    b = _tiny()
    b.edge_attr = b.edge_attr.float()
    torch.manual_seed(1)
    m = O.TopologicalGNN(4, 16, 3, 4, dropout_p=0.5).train()

    def old_forward(data):                   # the forward as it stood before ``keep`` existed
        x = m.node_embeddings(data.node_ids)
        x = m.dropout(F.leaky_relu(m.conv1(x, data.edge_index, data.edge_attr)))
        x = m.dropout(F.leaky_relu(m.conv2(x, data.edge_index, data.edge_attr)))
        return m.mlp(O.global_mean_pool(x, data.batch))
    for train in (True, False):
        m.train(train)
        torch.manual_seed(7); a = m(b)
        torch.manual_seed(7); c = m(b, keep=None)
        torch.manual_seed(7); d = old_forward(b)
        assert torch.equal(a, c) and torch.equal(a, d)
    # a site without an entry still runs its nn.Dropout: eval mode with an empty dict is the plain eval forward
    m.eval()
    assert torch.equal(m(b, keep={}), m(b))
    from gnn_qot_estimation_amd import synthetic as S
    lb = S.lightpath_batch(6)
    torch.manual_seed(2)
    lp = O.LightpathGNN(5, 8, 3, 1, dropout_p=0.5).train()
    torch.manual_seed(7); a, ia = lp(lb)
    torch.manual_seed(7); c, ic = lp(lb, keep=None)
    assert torch.equal(a, c) and torch.equal(ia, ic)
    lp.eval()                                # (BatchNorm running statistics no longer move)
    rows = int((lb.x[:, 1] == 1.0).sum())
    keep = OD.keep_mask(5, 1, (rows, 8), 0.5)
    h = F.leaky_relu(lp.mlp[0](F.relu(lp.norm1(lp.conv1(lb.x, lb.edge_index)))[lb.x[:, 1] == 1.0]))
    assert torch.equal(lp(lb, keep={"head": keep})[0], lp.mlp[3](h * keep.float() / (1.0 - 0.5)))


# --------------------------------------------------------------------------- the loop's draws
def test_train_loop_counts_one_draw_per_train_forward_and_none_in_evaluation():
    case = H.TRAJECTORY_CASES["topo_h16_drop"]
    fit = dict(case["fit"], num_epochs=2)
    graphs = H.trajectory_graphs(case)[:60]                       # 42 train graphs, chunks of 21: two batches per epoch
    seen = []
    real = OD.topological_masks

    def spy(base_seed, step, *a, **kw):
        seen.append((base_seed, step))
        return real(base_seed, step, *a, **kw)
    try:
        OD.topological_masks = spy
        res = TL.train(H.trajectory_oracle_model(case), graphs, "topological", dtype=torch.float64,
                       dropout=(case["dropout_seed"], 10), **fit)
    finally:
        OD.topological_masks = real
    assert res["dropout_draws"] == 4 and seen == [(case["dropout_seed"], 10 + k) for k in (1, 2, 3, 4)]
    plain = TL.train(H.trajectory_oracle_model(dict(case, model=dict(case["model"], dropout_p=0.0))), graphs,
                     "topological", dtype=torch.float64, **fit)
    assert plain["dropout_draws"] == 0 and plain["loss"] != res["loss"]
    with pytest.raises(ValueError):
        TL.train(H.trajectory_oracle_model(H.TRAJECTORY_CASES["lp_c8_skip_mid"]), [], "lightpath", dropout=(1, 0))


# --------------------------------------------------------------------------- conditioning of the single-step cases
@pytest.mark.parametrize("name", list(DC.CASES))
def test_single_step_case_is_well_conditioned(name):
    """fp32 rounding alone moves neither the output nor any gradient by more than TOL / 10 under the step's own masks
    (a read-out whose mask comes from torch's generator on the GPU gets a restated one here: any realisation serves)."""
    case = DC.CASES[name]
    batch = case["batch"]()
    keep = DC.masks(case, batch, 1)
    r32, _ = DC.models(case)
    r64 = copy.deepcopy(r32).double()
    res = []
    for ref, b in ((r32, batch), (r64, DC.to_double(batch))):
        ref.train()
        out = ref(b, keep=keep)
        F.smooth_l1_loss(out, b.y.view(-1, 3)).backward()
        res.append(out)
    e_out = rel_err(res[0], res[1])
    worst = grad_compare(r64, r32)
    print(f"{name}: fp32-vs-fp64 out {e_out:.2e} grads {worst:.2e}")
    assert e_out <= TOL / 10 and worst <= TOL / 10, (e_out, worst)
    if case["model"]["dropout_p"] >= 0.5:                          # the step is not degenerate: something survives
        assert float(res[1].abs().max()) > 0 and all(float(k.float().mean()) > 0.02 for k in keep.values())
