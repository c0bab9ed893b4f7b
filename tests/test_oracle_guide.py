"""Pin the GUIDE_IMGSNP oracle (oracle/guide.py, float64) against tests/golden/guide_imgsnp.npz, which
tests/golden/make_golden_guide.py captured by running kernel/guide_img_snp.py and kernel/guide_go_model.py of the
reference: eval outputs; training outputs, the five loss terms, the loss, the running statistics, every gradient and the
parameters left without one; and the stand-alone GUIDE GO network (``go/``).  Bounds of tests/test_oracle_golden.py."""
import numpy as np
import pytest
import torch

from conftest import assert_matches, golden_group
from _weights import seeded_state
from igcn_amd import synth
from igcn_amd.data import Batch
from oracle import go_network as OG
from oracle import guide as OGD
from oracle import sgcn_img_snp as OS
from test_oracle_golden import grad_floor

TAGS = ["h16", "h10"]
NAMES = ["logp", "x_hat", "latent", "lin_f", "reg", "img", "decoded", "prob"]
TOL = {"eval": 1e-5, "train": 3e-4}
GTOL = 5e-3


def _scale(wg, prefix=""):
    """The GO branch's largest gradient: its LayerNorm scales take gradients far below it, and the fixture's fp32
    rounding through the attention moves them by ~1e-2 of their own size (tests/test_gpu_guide.py judges them alike)."""
    return max(float(np.abs(w).max()) for k, w in wg.items() if k.startswith(prefix) and not isinstance(w, tuple))


def _state(store, prefix, seed):
    keys, shapes = store[f"{prefix}/state_keys"].tolist(), store[f"{prefix}/state_shapes"].tolist()
    shp = {k: tuple(int(d) for d in s.split(",") if d) for k, s in zip(keys, shapes)}
    return OS.make_leaf_state(seeded_state(shp, seed), torch.float64)


def _index_sets(store, seed):
    pool = store["pool"].tolist()
    go_snps, adj, _ = synth.go_hierarchy(tuple(pool), seed=seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj)
    return OG.go_index_sets(a_g, a, pool, 2)


def _setup(store, tag):
    rois, _, bsz, seed, _, _ = [int(v) for v in store[f"{tag}/cfg"]]
    sd = _state(store, tag, seed)
    idx = _index_sets(store, seed)
    graphs = synth.brain_graph_list(bsz, seed=seed + 10, rois=rois, top_k=3, tsne_dim=16)
    data = OGD.batch_data(Batch.from_data_list(graphs))
    cfg = OGD.SimpleNamespace(rois=rois)
    return sd, idx, data, cfg


def _named(o):
    return dict(zip(NAMES, (o[0], o[1], o[2], o[4], o[5], o[6][0], o[6][1], o[7][0])))


def _running(sd, store, prefix, tol):
    for k, w in golden_group(store, prefix).items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(w), (k, int(sd[k]), int(w))
        else:
            assert_matches(sd[k], w, tol, "buffer " + k)


@pytest.mark.parametrize("tag", TAGS)
def test_guide_oracle_eval_matches_reference(golden, tag):
    store = golden("guide_imgsnp")
    sd, idx, data, cfg = _setup(store, tag)
    with torch.no_grad():
        outs = _named(OGD.model_forward(sd, cfg, idx, data, training=False))
    want = golden_group(store, f"{tag}/eval")
    for n in NAMES:
        assert_matches(outs[n], want[n], TOL["eval"], n)


@pytest.mark.parametrize("tag", TAGS)
def test_guide_oracle_train_matches_reference(golden, tag):
    store = golden("guide_imgsnp")
    sd, idx, data, cfg = _setup(store, tag)
    noise = torch.from_numpy(store[f"{tag}/noise"]).double()
    lam = store["lam"].tolist()
    loss, terms, outs = OGD.train_losses(sd, cfg, idx, data, float(store["tau"]), noise, lam)
    want = golden_group(store, f"{tag}/train")
    for n, o in _named(outs).items():
        assert_matches(o, want[n], TOL["train"], n)
    for k, v in terms.items():
        ref = float(store[f"{tag}/term/{k}"])
        assert abs(float(v.detach()) - ref) <= TOL["train"] * max(1.0, abs(ref)), (k, float(v.detach()), ref)
    ref = float(store[f"{tag}/loss"])
    assert abs(float(loss.detach()) - ref) <= TOL["train"] * max(1.0, abs(ref)), (float(loss.detach()), ref)
    _running(sd, store, f"{tag}/running", TOL["train"])
    loss.backward()
    wg = golden_group(store, f"{tag}/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), GTOL, "grad data.x")
    go_scale = _scale(wg, "go_network.")
    for k, w in wg.items():
        assert sd[k].grad is not None, k
        floor = grad_floor(wg, k, 1e-4)
        if k.startswith("go_network."):
            floor = max(floor, go_scale)
        assert_matches(sd[k].grad, w, GTOL, "grad " + k, floor=floor)
    no_grad = set(store[f"{tag}/no_grad"].tolist())
    assert no_grad and no_grad.isdisjoint(wg)
    for k in no_grad:
        assert sd[k].grad is None, "unexpected grad " + k
    for k, v in sd.items():
        if v.requires_grad and k not in no_grad:
            assert k in wg, "the reference has a gradient the fixture lacks: " + k


def test_guide_go_oracle_matches_reference(golden):
    store = golden("guide_imgsnp")
    bsz, seed, _ = [int(v) for v in store["go/cfg"]]
    sd = _state(store, "go", seed)
    idx = _index_sets(store, seed)
    snps = Batch.from_data_list(synth.brain_graph_list(bsz, seed=seed + 10, rois=90, top_k=3, tsne_dim=16)).snps_feat
    snps = snps.double()
    latent, x_d, atten_out = OGD.go_forward(sd, idx, snps, training=True)
    want = golden_group(store, "go/out")
    for n, o in (("latent", latent), ("x_d", x_d), ("atten_out", atten_out)):
        assert_matches(o, want[n], TOL["train"], n)
    _running(sd, store, "go/running", TOL["train"])
    c1, c2 = (torch.from_numpy(store[k]).double() for k in ("go/c1", "go/c2"))
    ((latent * c1).sum() + (x_d * c2).sum()).backward()
    wg = golden_group(store, "go/grad")
    scale = _scale(wg)
    for k, w in wg.items():
        assert sd[k].grad is not None, k
        assert_matches(sd[k].grad, w, GTOL, "grad " + k, floor=scale)
    no_grad = set(store["go/no_grad"].tolist())
    assert no_grad
    for k in no_grad:
        assert sd[k].grad is None, "unexpected grad " + k


def test_prelu_is_the_single_decision_point(golden, monkeypatch):
    """Every PReLU of the oracle goes through oracle.guide.prelu, with the module key of its slope."""
    store = golden("guide_imgsnp")
    sd, idx, data, cfg = _setup(store, "h10")
    seen = []
    orig = OGD.prelu

    def recorded(site, u, a):
        seen.append(site)
        return orig(site, u, a)
    monkeypatch.setattr(OGD, "prelu", recorded)
    with torch.no_grad():
        OGD.model_forward(sd, cfg, idx, data, training=False)
    slopes = sorted(k[:-7] for k, v in sd.items() if k.endswith(".weight") and tuple(v.shape) == (1,)
                    and not k.startswith("go_network.classification."))
    assert sorted(seen) == slopes, (seen, slopes)
