"""CPU checks of GUIDE_IMGSNP (kernel/guide_img_snp.py): the gate's generator contract restated in numpy, the model's and
the GUIDE Gene_ontology_network's state_dict against the fixture captured from the reference
(tests/golden/make_golden_guide.py), and the constructor's / forward's refusals.  No kernel runs here."""
import numpy as np
import pytest
import torch

import guide_ref
from _weights import seeded_state
from oracle import dropout as OD

TAGS = ["h16", "h10"]


def _hierarchy(store, seed):
    from igcn_amd import synth
    go_snps, adj, pool_dim = synth.go_hierarchy(tuple(store["pool"].tolist()), seed=seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj)
    return a_g, a, pool_dim


def _model(store, tag):
    from igcn_amd.guide_img_snp import GUIDE_IMGSNP
    rois, hidden, _, seed, ncls, hl = [int(v) for v in store[f"{tag}/cfg"]]
    a_g, a, pool_dim = _hierarchy(store, seed)
    return GUIDE_IMGSNP(2, hidden, a_g, a, pool_dim, 32, "cpu", rois=rois, H_0=3, num_classes=ncls, num_regr=3,
                        hidden_linear=hl), seed


def test_gumbel_known_answers():
    # r = 0, 2^23 and 2^24 - 1: u = 2^-25, 1/2 + 2^-25 and 1 - 2^-25 (finite: u never rounds to 1)
    g = guide_ref.gumbel_from_draws([0, 2 ** 23, 2 ** 24 - 1]).astype(np.float64)
    want = [-np.log(25 * np.log(2.0)), -np.log(-np.log(0.5 + 2.0 ** -25)), -np.log(-np.log1p(-2.0 ** -25))]
    assert np.allclose(g, want, rtol=1e-5, atol=1e-5), (g, want)
    # the draws are the dropout generator's: the same 24-bit numbers at the same flat indices
    r = np.round(OD.uniforms(5, 64).astype(np.float64) * 16777216.0)
    assert np.array_equal(r, np.floor(r)) and r.min() >= 0 and r.max() < 2 ** 24
    g = guide_ref.gumbel_noise(5, 4, 8)
    assert g.shape == (4, 8, 2) and np.isfinite(g).all()
    assert np.array_equal(g.reshape(-1), guide_ref.gumbel_from_draws(r))


def test_hard_decision_is_torch_gumbel_softmax_on_the_same_noise():
    rng = np.random.default_rng(3)
    bias = torch.from_numpy(0.1 * (2 * rng.random((270, 2)) - 1)).float()
    noise = torch.from_numpy(guide_ref.gumbel_noise(11, 8, 270))
    logits = torch.log(torch.softmax(bias, 1)).repeat(8, 1)
    y_soft = ((logits + noise.reshape(logits.shape)) / 0.1).softmax(-1)
    index = y_soft.max(-1, keepdim=True)[1]
    hard = torch.zeros_like(logits).scatter_(-1, index, 1.0) - y_soft.detach() + y_soft
    s, z1 = guide_ref.soft_sample(bias, noise, 0.1)
    margin = (s[..., 1] - s[..., 0]).abs().reshape(-1)
    far = margin > 1e-6
    assert bool(far.float().mean() > 0.99)
    assert torch.equal((hard[:, 1] > 0.5)[far], (z1.reshape(-1) > 0.5)[far])


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_matches_the_reference_and_loads_strict(golden, tag):
    store = golden("guide_imgsnp")
    model, seed = _model(store, tag)
    sd = model.state_dict()
    keys = sorted(sd)
    assert keys == store[f"{tag}/state_keys"].tolist()
    assert [",".join(str(d) for d in sd[k].shape) for k in keys] == store[f"{tag}/state_shapes"].tolist()
    model.load_state_dict(seeded_state({k: v.shape for k, v in sd.items()}, seed, sd), strict=True)
    assert model.reset_parameters() is None
    for flag in ("isCrossAtten", "isSoftSimilarity", "graph_pool", "isuseFeat4Regr", "isImageOnly", "isSNPsOnly",
                 "ifUseGAT"):
        assert hasattr(model, flag), flag


def test_guide_go_network_state_dict_matches_the_reference(golden):
    from igcn_amd.guide_go_model import Gene_ontology_network
    store = golden("guide_imgsnp")
    bsz, seed, atten = [int(v) for v in store["go/cfg"]]
    a_g, a, pool_dim = _hierarchy(store, seed)
    net = Gene_ontology_network(a_g, a, 2, 2, [5, 5], pool_dim, 32, "cpu", dim_snps_atten=atten)
    sd = net.state_dict()
    keys = sorted(sd)
    assert keys == store["go/state_keys"].tolist()
    assert [",".join(str(d) for d in sd[k].shape) for k in keys] == store["go/state_shapes"].tolist()
    net.load_state_dict(seeded_state({k: v.shape for k, v in sd.items()}, seed, sd), strict=True)


def test_constructor_refusals(golden):
    from igcn_amd.guide_img_snp import GUIDE_IMGSNP
    store = golden("guide_imgsnp")
    a_g, a, pool_dim = _hierarchy(store, 71)
    with pytest.raises(ValueError, match="l_dim"):
        GUIDE_IMGSNP(2, 16, a_g, a, pool_dim, 16, "cpu", rois=90, H_0=3)
    with pytest.raises(ValueError, match="hidden_linear"):
        GUIDE_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cpu", rois=90, H_0=3, hidden_linear=128)
    with pytest.raises(ValueError, match="rois"):
        GUIDE_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cpu", rois=400, H_0=3)


def test_forward_refusals(golden):
    from igcn_amd import synth
    from igcn_amd.data import Batch
    store = golden("guide_imgsnp")
    model, _ = _model(store, "h16")
    short = synth.brain_graph_list(2, seed=1, rois=90, tsne_dim=16)
    g = short[1]
    g.x = g.x[:80].contiguous()
    keep = g.edge_index.max(0).values < 80
    g.edge_index, g.edge_attr = g.edge_index[:, keep].contiguous(), g.edge_attr[keep].contiguous()
    with pytest.raises(ValueError, match="rois"):
        model.eval()
        model(Batch.from_data_list(short), None, "cpu")
    model.train()
    with pytest.raises(ValueError, match="temperature"):
        model(Batch.from_data_list(synth.brain_graph_list(2, seed=1, rois=90, tsne_dim=16)), None, "cpu")
