"""CPU checks of SGCN_GAT (kernel/sgcn.py:154-270) and of the edge-attribute gradient of the GAT stack
(igcn_gat_stack_bwd_ew): the reference fixture, the state_dict key set, the formula the kernel implements on a
hand-sized graph against the float64 stand-in's autograd, and the LDS sizes of the entry points that already shipped."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gat_standin import STATED, gat_conv

TAGS = ["l2h16", "l3h10"]
DATASET = SimpleNamespace(num_features=3, num_classes=2)


def test_fixture_reloads_and_names_the_standin(golden):
    store = golden("sgcn_gat")
    meta = str(store["meta"])
    assert STATED in meta and "SGCN_GAT" in meta
    for tag in TAGS:
        rois, hidden, layers, bsz, seed, top_k = [int(v) for v in store[f"{tag}/cfg"]]
        assert (rois, bsz, top_k) == (90, 4, 3)
        for mode in ("eval", "train"):
            for explain in (0, 1):
                assert store[f"{tag}/{mode}/explain{explain}/out/logp"].shape == (bsz, 2)
                assert store[f"{tag}/{mode}/explain{explain}/grad/data.x"].shape == (bsz * rois, 3)
        for k in ("loss", "term/ce", "term/mi", "term/prob"):
            assert np.isfinite(store[f"{tag}/step/{k}"])
        # the edge path: the masked pass alone reaches prob_bias, and only through the edge attributes
        g = store[f"{tag}/mi_only/grad/prob_bias"]
        assert g.shape == (6, 1) and np.abs(g).max() > 0
        assert f"{tag}/eval/explain0/grad/prob_bias" not in store          # the plain pass does not read the masks


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_keys_equal_the_reference(golden, tag):
    from igcn_amd.sgcn import SGCN_GAT
    store = golden("sgcn_gat")
    rois, hidden, layers = [int(v) for v in store[f"{tag}/cfg"][:3]]
    model = SGCN_GAT(DATASET, layers, hidden, rois=rois, H_0=3)
    assert sorted(model.state_dict().keys()) == sorted(store[f"{tag}/state_keys"].tolist())
    assert [n for n, _ in model.named_parameters()][:3] == ["prob", "prob_bias", "edge_prob"]
    assert model.lin1.in_features == 90 * layers * hidden and model.lin2.out_features == 2
    assert model.state_dict()["conv1.lin_dst.weight"].data_ptr() == model.conv1.lin_src.weight.data_ptr()
    assert repr(model) == "SGCN_GAT" and model.batched_passes and model._dropout_enabled


def test_lin1_keeps_the_references_literal_90():
    from igcn_amd.sgcn import SGCN_GAT
    assert SGCN_GAT(DATASET, 2, 8, rois=30, H_0=3).lin1.in_features == 90 * 2 * 8


def test_edge_attribute_gradient_formula_on_a_hand_sized_graph():
    """One layer, 3 nodes, stored edges 0->1, 2->1, 0->1 (duplicate), 1->2, 2->2 (stored self-loop), 1->0:
    d ea_k = c (dpre[k] + dpre[loop of dst_k] / cnt_dst) for kept edges, exactly 0 for the stored loop — dpre taken by
    hand through the softmax and the leaky ReLU — against the stand-in's autograd in float64."""
    g = torch.Generator().manual_seed(5)
    f, slope = 4, 0.2
    src = torch.tensor([0, 2, 0, 1, 2, 1])
    dst = torch.tensor([1, 1, 1, 2, 2, 0])
    ea = torch.rand(6, generator=g, dtype=torch.float64).requires_grad_(True)
    x = torch.randn(3, 2, generator=g, dtype=torch.float64)
    w = torch.randn(f, 2, generator=g, dtype=torch.float64)
    a_src, a_dst, l_e, a_e = (torch.randn(f, generator=g, dtype=torch.float64) for _ in range(4))
    bias = torch.randn(f, generator=g, dtype=torch.float64)
    dy = torch.randn(3, f, generator=g, dtype=torch.float64)
    out = gat_conv(x, torch.stack([src, dst]), ea, w, a_src, a_dst, l_e, a_e, bias)
    (out * dy).sum().backward()
    want = ea.grad

    h = x @ w.t()
    a_s, a_d, c = h @ a_src, h @ a_dst, float((l_e * a_e).sum())
    eav = ea.detach()
    got = torch.zeros(6, dtype=torch.float64)
    for i in range(3):
        kept = [k for k in range(6) if int(dst[k]) == i and int(src[k]) != i]
        cnt = len(kept)
        lea = sum(float(eav[k]) for k in kept) / cnt if cnt else 0.0
        pre = torch.tensor([float(a_s[src[k]] + a_d[i] + eav[k] * c) for k in kept] + [float(a_s[i] + a_d[i] + lea * c)],
                           dtype=torch.float64)
        z = torch.where(pre > 0, pre, slope * pre)
        ex = (z - z.max()).exp()
        alpha = ex / (ex.sum() + 1e-16)
        hs = torch.stack([h[src[k]] for k in kept] + [h[i]])
        dalpha = hs @ dy[i]
        dz = alpha * (dalpha - (alpha * dalpha).sum())
        dpre = torch.where(pre > 0, dz, slope * dz)
        for j, k in enumerate(kept):
            got[k] = c * (dpre[j] + dpre[-1] / cnt)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (got, want)
    assert float(want[4]) == 0.0 and float(got[4]) == 0.0          # the stored self-loop
    assert float(want.abs().min()) == 0.0 and int((want != 0).sum()) == 5


def test_lds_bytes_of_the_shipped_entry_points_are_unchanged():
    """profiles/gat_bench.json's values at the benchmark shape; the edge-gradient layout has a code of its own."""
    import os
    from igcn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):                          # (as tests/test_abi.py: host code, loads without a GPU)
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert int(lib.igcn_gat_stack_lds_bytes(90, 270, 3, 16, 2, 0)) == 29552
    assert int(lib.igcn_gat_stack_lds_bytes(90, 270, 3, 16, 2, 1)) == 48720
    assert int(lib.igcn_gat_stack_lds_bytes(90, 270, 3, 16, 2, 2)) == 48720 + 4 * 92      # + 1 / cnt per node
    assert hasattr(lib, "igcn_gat_stack_bwd_ew")


def test_limits_ask_for_the_edge_gradient_layout():
    from igcn_amd import ops
    plan = SimpleNamespace(_stack_dims=(90, 270))
    assert ops.gat_stack_limits(plan, 90, 3, 16, 2, ew_grad=True) is None
    assert "F in" in ops.gat_stack_limits(plan, 90, 3, 64, 2, ew_grad=True)
    assert "uniform" in ops.gat_stack_limits(SimpleNamespace(_stack_dims=None), 90, 3, 16, 2, ew_grad=True)
