"""CPU checks of the GATConv stand-in (tests/golden/gat_standin.py) on hand-built graphs in float64, of the GCN_IMGSNP
fixtures it produced, and of the model's CPU-side surface (state_dict keys, the shape limits of the GAT stack)."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from gat_standin import STATED, GATConvModule, gat_conv, gat_edges

D = torch.float64


def _layer(fin=1, f=1, w=1.0, a_s=0.0, a_d=0.0, le=0.0, ae=0.0, b=0.0):
    """Parameters of a layer with every entry equal to the given scalar (the hand computations below use F = Fin = 1)."""
    full = lambda *s, v: torch.full(s, float(v), dtype=D)          # noqa: E731
    return dict(weight=full(f, fin, v=w), att_src=full(1, 1, f, v=a_s), att_dst=full(1, 1, f, v=a_d),
                lin_edge=full(f, 1, v=le), att_edge=full(1, 1, f, v=ae), bias=full(f, v=b))


def _run(x, edges, ea, **p):
    ei = torch.tensor(edges, dtype=torch.long).t().contiguous()
    return gat_conv(torch.tensor(x, dtype=D), ei, torch.tensor(ea, dtype=D), return_alpha=True, **_layer(**p))


def test_stored_self_loop_is_dropped_and_readded():
    # 0 -> 1 (ea 2) and a stored loop 1 -> 1 (ea 5): the loop is replaced by one whose ea is the mean of the kept
    # incoming edges of node 1 (2, not 5); node 0 has no incoming edge: loop ea 0, alpha 1
    out, alpha, (src, dst) = _run([[1.0], [3.0]], [(0, 1), (1, 1)], [2.0, 5.0], a_s=1.0, le=1.0, ae=1.0)
    assert src.tolist() == [0, 0, 1] and dst.tolist() == [1, 0, 1]
    _, _, ea2 = gat_edges(torch.tensor([[0, 1], [1, 1]]), torch.tensor([2.0, 5.0], dtype=D), 2)
    assert ea2.tolist() == [2.0, 0.0, 2.0]
    z = torch.tensor([1.0 + 2.0, 3.0 + 2.0], dtype=D)               # a_s[src] + ea c for node 1's two entries
    w = torch.softmax(z, 0)
    assert torch.allclose(alpha[[0, 2]], w, rtol=1e-14, atol=0)
    assert alpha[1] == 1.0
    assert out[0, 0] == 1.0
    assert math.isclose(float(out[1, 0]), float(w[0] * 1.0 + w[1] * 3.0), rel_tol=1e-14)


def test_duplicate_edges_are_kept():
    # two copies of 0 -> 1 and the loop of 1, every logit 0: a third of the weight each
    out, alpha, (src, dst) = _run([[3.0], [6.0]], [(0, 1), (0, 1)], [1.0, 1.0], a_s=0.0)
    assert src.tolist() == [0, 0, 0, 1] and dst.tolist() == [1, 1, 0, 1]
    assert torch.allclose(alpha[[0, 1, 3]], torch.full((3,), 1 / 3, dtype=D), rtol=1e-15, atol=0)
    assert math.isclose(float(out[1, 0]), 2 / 3 * 3.0 + 1 / 3 * 6.0, rel_tol=1e-14)


def test_isolated_node_keeps_its_own_row():
    # node 2 receives nothing: its loop ea is 0 and its alpha 1, so out[2] = h[2] + bias even with an edge term
    out, alpha, (src, dst) = _run([[1.0], [2.0], [4.0]], [(0, 1), (2, 1)], [0.5, 1.5], w=2.0, a_s=0.3, a_d=-0.7,
                                  le=2.0, ae=1.5, b=0.25)
    _, _, ea2 = gat_edges(torch.tensor([[0, 2], [1, 1]]), torch.tensor([0.5, 1.5], dtype=D), 3)
    assert ea2[2 + 2] == 0.0 and ea2[2 + 1] == 1.0                   # node 2: 0; node 1: mean(0.5, 1.5)
    loop2 = [k for k in range(src.numel()) if src[k] == 2 and dst[k] == 2]
    assert len(loop2) == 1 and alpha[loop2[0]] == 1.0
    assert out[2, 0] == 2.0 * 4.0 + 0.25


def test_max_subtraction_with_logits_80_apart():
    # target 2 receives logits 80 (from node 0), 0 (from node 1) and 0 (its loop): the max subtraction keeps the
    # softmax exact (and finite in fp32 as well)
    for dt in (torch.float64, torch.float32):
        ei = torch.tensor([[0, 1], [2, 2]])
        p = {k: v.to(dt) for k, v in _layer(a_s=1.0).items()}
        out, alpha, _ = gat_conv(torch.tensor([[80.0], [0.0], [0.0]], dtype=dt), ei, torch.zeros(2, dtype=dt),
                                 return_alpha=True, **p)
        small = math.exp(-80.0) / (1 + 2 * math.exp(-80.0))
        assert torch.isfinite(alpha).all() and torch.isfinite(out).all()
        assert math.isclose(float(alpha[0]), 1 / (1 + 2 * math.exp(-80.0)), rel_tol=1e-6)
        assert math.isclose(float(alpha[1]), small, rel_tol=1e-5)
        assert math.isclose(float(out[2, 0]), 80.0 * float(alpha[0]), rel_tol=1e-6)


def test_negative_slope_and_denominator():
    # a logit of -10 through leaky_relu(0.2) is -2; the denominator carries + 1e-16
    out, alpha, _ = _run([[-10.0], [0.0]], [(0, 1)], [0.0], a_s=1.0)
    e = torch.exp(torch.tensor([-2.0, 0.0], dtype=D))
    assert torch.allclose(alpha[[0, 2]], e / (e.sum() + 1e-16), rtol=1e-15, atol=0)


def test_module_names_and_initialisation():
    torch.manual_seed(0)
    m = GATConvModule(3, 16, edge_dim=1)
    assert sorted(m.state_dict()) == ["att_dst", "att_edge", "att_src", "bias", "lin_dst.weight", "lin_edge.weight",
                                      "lin_src.weight"]
    assert m.lin_dst is m.lin_src and len(list(m.parameters())) == 6
    assert m.bias.abs().max() == 0
    assert m.lin_src.weight.abs().max() <= math.sqrt(6 / 19) and m.att_src.abs().max() <= math.sqrt(6 / 17)


@pytest.mark.parametrize("name", ["gcn_imgsnp_gcn", "gcn_imgsnp_gat"])
def test_fixtures_reload_with_their_meta(name):
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 500 * 1024
    store = load_golden(name)
    meta = str(store["meta"])
    assert "kernel/gcn_img_snp.py" in meta and "train_eval_gcn_img_snps.py" in meta
    assert (STATED in meta) == (name == "gcn_imgsnp_gat") and int(store["gat"]) == (name == "gcn_imgsnp_gat")
    assert store["lam"].tolist() == [0.0, 1.0, 0.5, 1.5e-6, 0.1, 0.0]
    for tag, (layers, hidden) in (("l2h16", (2, 16)), ("l3h10", (3, 10))):
        rois, h, l, bsz = store[f"{tag}/cfg"].tolist()[:4]
        assert (rois, h, l, bsz) == (90, hidden, layers, 32)
        for k in ("ce", "reg", "recon", "cluster", "orth"):
            assert np.isfinite(store[f"{tag}/step/term/{k}"]) and np.isfinite(store[f"{tag}/alt/term/{k}"])
        # the default lambda zeroes ce and orth (lambda_disease = 0)
        assert float(store[f"{tag}/step/term/ce"]) == 0.0 and float(store[f"{tag}/step/term/orth"]) == 0.0
        keys = store[f"{tag}/state_keys"].tolist()
        gat_keys = [k for k in keys if k.startswith("conv1.")]
        if name == "gcn_imgsnp_gat":
            assert "conv1.lin_dst.weight" in gat_keys and "conv1.att_edge" in gat_keys
        else:
            assert gat_keys == ["conv1.bias", "conv1.lin.weight"]


@pytest.mark.parametrize("gat", [False, True])
def test_model_state_dict_keys_match_the_fixture(gat):
    from igcn_amd import synth
    from igcn_amd.gcn_img_snp import GCN_IMGSNP
    store = load_golden("gcn_imgsnp_gat" if gat else "gcn_imgsnp_gcn")
    for tag in ("l2h16", "l3h10"):
        rois, hidden, layers, _, seed, _ = [int(v) for v in store[f"{tag}/cfg"]]
        go_snps, adj, pool_dim = synth.go_hierarchy(tuple(store["pool"].tolist()), seed=seed)
        a_g, a = synth.go_sparse_inputs(go_snps, adj)
        m = GCN_IMGSNP(layers, hidden, a_g, a, pool_dim, 32, "cpu", rois=rois, H_0=3, num_classes=3,
                       isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseFeat4Regr=True,
                       isImageOnly=False, isSNPsOnly=False, ifUseGAT=gat)
        assert sorted(m.state_dict()) == sorted(store[f"{tag}/state_keys"].tolist())
        if gat:
            assert m.conv1.lin_dst is m.conv1.lin_src
            names = [n for n, _ in m.named_parameters()]
            assert "conv1.lin_src.weight" in names and "conv1.lin_dst.weight" not in names


def test_model4eachregr_is_not_built():
    from igcn_amd import synth
    from igcn_amd.gcn_img_snp import GCN_IMGSNP
    go_snps, adj, pool_dim = synth.go_hierarchy((40, 20, 10, 4, 1), seed=3)
    a_g, a = synth.go_sparse_inputs(go_snps, adj)
    with pytest.raises(NotImplementedError):
        GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cpu", model4eachregr=True)


def test_gat_stack_limits_name_the_limit():
    from types import SimpleNamespace
    from igcn_amd import ops
    plan = SimpleNamespace(_stack_dims=(90, 300))
    assert ops.gat_stack_limits(plan, 90, 3, 16, 2) is None
    assert "F in" in ops.gat_stack_limits(plan, 90, 3, 64, 2)
    assert "layers" in ops.gat_stack_limits(plan, 90, 3, 16, 5)
    assert "H0" in ops.gat_stack_limits(plan, 90, 9, 16, 2)
    assert "LDS" in ops.gat_stack_limits(SimpleNamespace(_stack_dims=(1000, 4000)), 1000, 3, 32, 4)
    assert "uniform" in ops.gat_stack_limits(SimpleNamespace(_stack_dims=None), 90, 3, 16, 2)
