"""CPU checks of the genetics-only trainer (kernel/train_eval_snps.py on kernel/go_model.py's ``classification`` module)
against the fixture captured from the reference (tests/golden/snps_only.npz, written by
tests/golden/make_golden_snps.py): the restatement tests/snps_ref.py evaluated in fp32 — the reference's arithmetic — at
the bounds tests/test_clusterlabel_reference.py holds its restatement to; the BCE restatement against torch's own
BCELoss, saturated sigmoids included; the library's CPU route (``snps.losses_snps`` off the GPU takes torch's ops for
every piece) against the same fixture; and the condition the GPU tests' float64 comparisons rest on: no ReLU decision of
the head within rounding of zero for any input they use."""
import numpy as np
import pytest
import torch

import snps_ref as REF
from clusterlabel_ref import group
from conftest import assert_matches, relu_margins
from oracle import sgcn_img_snp as OS
from test_oracle_golden import grad_floor

TAGS = list(REF.CONFIGS)
# tests/test_clusterlabel_reference.py: eval 1e-5 outputs / 5e-4 gradients; training mode 1e-4 / 5e-3
TOL = {"eval": 1e-5, "train": 1e-4}
GTOL = {"eval": 5e-4, "train": 5e-3}


def _check_grads(sd_grads, store, tag, mode, tol, floor=1e-4):
    wg = group(store, f"{tag}/{mode}/grad")
    no_grad = set(store[f"{tag}/{mode}/no_grad"].tolist())
    assert no_grad == {"conc_for_attention.0.weight", "conc_for_attention.1.bias", "conc_for_attention.1.weight"}
    assert no_grad.isdisjoint(wg) and any(k.startswith("classification.") for k in wg)
    for k in no_grad:                      # atten_out feeds nothing in this trainer
        g = sd_grads.get(k)
        assert g is None or not bool(g.abs().max() > 0), k
    for k, w in wg.items():
        assert sd_grads.get(k) is not None, k
        assert_matches(sd_grads[k], w, tol, "grad " + k, floor=grad_floor(wg, k, floor))
    return wg


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_restatement_matches_reference(golden, tag, mode):
    store = golden("snps_only")
    cfg, idx, sd0 = REF.fixture_setup(store, tag)
    assert "train_eval_snps" in str(store["meta"]) and cfg.lambda0 == 1e-5
    sd = OS.make_leaf_state(sd0, torch.float32)
    data, label = REF.inputs(tag, mode)
    assert sorted(set(data.unique().tolist())) == [0.0, 1.0, 2.0] and sorted(set(label.tolist())) == [0.0, 1.0]
    loss, terms, outs = REF.losses(sd, idx, data, label, cfg.lambda0, training=(mode == "train"))
    want = group(store, f"{tag}/{mode}/out")
    for n, o in zip(("latent", "x_hat", "y_hat"), outs):
        assert_matches(o, want[n], TOL[mode], n)
    w = float(store[f"{tag}/{mode}/loss"])
    assert abs(float(loss) - w) <= 1e-5 * max(1.0, abs(w))
    assert sorted(terms) == sorted(REF.TERMS)
    for k, v in terms.items():
        w = float(store[f"{tag}/{mode}/term/{k}"])
        assert abs(float(v) - w) <= 1e-5 * max(1.0, abs(w)), k
    loss.backward()
    _check_grads({k: v.grad for k, v in sd.items()}, store, tag, mode, GTOL[mode])


@pytest.mark.parametrize("tag", TAGS)
def test_train_step_matches_reference(golden, tag):
    store = golden("snps_only")
    cfg, idx, sd0 = REF.fixture_setup(store, tag)
    sd = OS.make_leaf_state(sd0, torch.float32)
    data, label = REF.inputs(tag, "train")
    loss, _, _ = REF.train_step(sd, idx, data, label, lr=1e-3, lambda0=cfg.lambda0)
    w = float(store[f"{tag}/train/loss"])
    assert abs(float(loss) - w) <= 1e-5 * max(1.0, abs(w))
    grads = group(store, f"{tag}/train/grad")
    lr = 1e-3
    for k, w in group(store, f"{tag}/step/param_after").items():
        # (tests/test_clusterlabel_reference.py: Adam's first step is ill-conditioned where the gradient is rounding noise)
        if isinstance(w, tuple) or k not in grads or isinstance(grads[k], tuple):
            assert_matches(sd[k], w, 2.5 * lr, "param " + k, floor=1.0)
            continue
        g = torch.from_numpy(grads[k])
        solid = g.abs() > 2e-2 * g.abs().max()
        sib = grads.get(k[:-5] + ".weight") if k.endswith(".bias") else None
        if sib is not None and not isinstance(sib, tuple) and float(g.abs().max()) < 1e-2 * float(np.abs(sib).max()):
            solid = torch.zeros_like(solid)
        diff = (sd[k].detach() - torch.from_numpy(w)).abs()
        assert float(diff[solid].max() if solid.any() else 0.0) <= 2e-5, "param " + k
        assert float(diff.max()) <= 2.01 * lr, "param (noise-level grads) " + k
    for k, w in group(store, f"{tag}/step/buffers_after").items():
        assert_matches(sd[k], w, 3e-4, "buffer " + k, floor=1e-2)


def _model(cfg):
    from igcn_amd.go_model import Gene_ontology_network
    return Gene_ontology_network(cfg.a_g, cfg.a, 2, 2, [5, 5], cfg.pool_dim, cfg.l_dim, "cpu")


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_is_the_reference(golden, tag):
    store = golden("snps_only")
    cfg, _, sd0 = REF.fixture_setup(store, tag)
    model = _model(cfg)
    assert sorted(model.state_dict()) == store[f"{tag}/state_keys"].tolist()
    assert isinstance(model.classification, torch.nn.Sequential) and len(model.classification) == 8
    model.load_state_dict(sd0)                       # strict: the seeded reference state loads as it is


def test_bce_restatement_is_torchs_bceloss():
    """values and gradients with respect to the logit, fp32, saturated sigmoids included."""
    zs, ys = [-30.0, -5.0, 0.0, 5.0, 30.0], [0.0, 0.3, 1.0]
    z0 = torch.tensor([z for z in zs for _ in ys])
    y = torch.tensor([v for _ in zs for v in ys])
    z1, z2 = z0.clone().requires_grad_(True), z0.clone().requires_grad_(True)
    v1 = REF.bce(torch.sigmoid(z1), y)
    v2 = torch.nn.BCELoss(reduction="none")(torch.sigmoid(z2), y)
    v1.sum().backward()
    v2.sum().backward()
    assert torch.allclose(v1, v2, rtol=1e-6, atol=0) and torch.allclose(z1.grad, z2.grad, rtol=1e-6, atol=1e-12)
    at = lambda z, yy: zs.index(z) * len(ys) + ys.index(yy)          # noqa: E731
    assert float(v1[at(30.0, 0.0)]) == 100.0 and float(z1.grad[at(30.0, 0.0)]) == 0.0
    assert abs(float(v1[at(-30.0, 1.0)]) - 30.0) < 1e-4 and abs(float(z1.grad[at(-30.0, 1.0)]) + 0.0936) < 1e-4


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_library_cpu_route_matches_reference(golden, tag, mode):
    """``snps.losses_snps`` off the GPU: the GO network's ops need the device, so what runs here is the head, the BCE and
    the reconstruction term on the reference's latent / x_hat — the unfused route with torch's op for every piece."""
    from igcn_amd import snps
    store = golden("snps_only")
    cfg, idx, sd0 = REF.fixture_setup(store, tag)
    model = _model(cfg)
    model.load_state_dict(sd0)
    model.train(mode == "train")
    model._dropout_enabled = False
    data, label = REF.inputs(tag, mode)
    want = group(store, f"{tag}/{mode}/out")
    with torch.no_grad():
        latent = REF.G.go_forward(sd0, idx, data, mode == "train", False)[0]
    assert_matches(latent, want["latent"], TOL[mode], "latent")
    latent.requires_grad_(True)
    y_hat = snps._head_unfused(model, latent, data, None, None)
    assert_matches(y_hat, want["y_hat"], TOL[mode], "y_hat")
    cls = torch.nn.functional.binary_cross_entropy(y_hat, label, reduction="sum")
    w = float(store[f"{tag}/{mode}/term/class"])
    assert abs(float(cls) - w) <= 1e-5 * max(1.0, abs(w))
    cls.backward()
    wg = group(store, f"{tag}/{mode}/grad")
    for k, p in model.classification.named_parameters():
        assert_matches(p.grad, wg["classification." + k], GTOL[mode], "grad " + k, floor=grad_floor(wg, "classification." + k, 1e-4))
    if mode == "eval":
        got = snps.classify(model, latent.detach(), data)
        assert_matches(got, want["y_hat"], TOL[mode], "classify")
    assert snps.SNPS_LAMBDA0 == 1e-5
    with pytest.raises(ValueError, match="more than one sample"):
        model.train()
        snps.losses_snps(model, data[:1], label[:1])
    with pytest.raises(ValueError, match="weight_decay"):
        snps.train_step_snps(model, torch.optim.Adam(model.parameters(), weight_decay=0.1), data, label)


def test_host_metrics_are_the_device_contract():
    """The host route of eval_scores_snps against tests/eval_metrics_ref.py (the restatement of igcn_eval_metrics), one
    score of exactly 0.5 — class 0 — included."""
    from eval_metrics_ref import metrics
    from igcn_amd import snps
    rng = np.random.default_rng(5)
    p = rng.random(200).astype(np.float32)
    p[17] = 0.5
    truth = rng.random(200) < 0.5
    pred = p > 0.5
    assert not pred[17]
    acc, auc, f1, sens, spec = snps._host_metrics(p, truth, pred)
    want = metrics(np.stack([np.log1p(-p), np.log(p)], 1), pred, truth, np.zeros((200, 0)), np.zeros((200, 0)), 2)
    assert acc == want["accuracy"] and auc == want["auc"] and sens == want["sensitivity"] and spec == want["specificity"]
    assert f1 == pytest.approx(want["f1"], rel=1e-12)


# ---- the condition the GPU tests' float64 comparisons rest on ------------------------------------------------------
def _assert_clear(rm, sites, what):
    for s in sites:
        near = int(rm.sites[s].sum())
        assert near == 0, f"{what}: {near} ReLU pre-activation(s) of site {s} within {rm.band} of the tensor's scale"


def test_no_head_relu_decision_within_rounding_for_the_launch_cases():
    """Every input tests/test_gpu_snps.py hands the launch: in the float64 reference neither the first-layer nor the
    second-layer ReLU has a pre-activation within 1e-5 of its tensor's largest magnitude.  A seed that violates this is
    replaced (snps_ref.head_case), not masked."""
    n = 0
    for name, case, training in REF.head_cases():
        with relu_margins(band=1e-5) as rm:
            REF.head_loss_of(case, training)
        assert len(rm.sites) == 2
        _assert_clear(rm, (0, 1), name)
        n += 1
    assert n == 3 * len(REF.HEAD_SHAPES) + 2


@pytest.mark.parametrize("tag", TAGS)
def test_no_head_relu_decision_within_rounding_for_the_fixture_batches(golden, tag):
    """... and the same for the head's two ReLUs (the last two of the forward) on the batches the GPU tests run the whole
    model on: both modes of both configurations, and the dropout-on step under the masks of its stream counter."""
    import dropout_cases as DC
    store = golden("snps_only")
    cfg, idx, sd0 = REF.fixture_setup(store, tag)
    runs = [("eval", False, False), ("train", True, False)]
    if tag == REF.DROPOUT_TAG:
        runs.append(("train", True, DC.feed(REF.dropout_sites(tag), DC.COUNTER, REF.HEAD_SITES)))
    for mode, training, dropout in runs:
        sd = OS.make_leaf_state(sd0, torch.float64)
        data, label = REF.inputs(tag, mode)
        with torch.no_grad(), relu_margins(band=1e-5) as rm:
            REF.losses(sd, idx, data.double(), label.double(), cfg.lambda0, training, dropout)
        if dropout is not False:
            dropout.close()
        _assert_clear(rm, (len(rm.sites) - 2, len(rm.sites) - 1), f"{tag}/{mode}")
