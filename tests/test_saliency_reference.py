"""CPU checks of the ROI x modality saliency maps (gradient x input, integrated gradients, Grad-CAM): the float64
restatement the GPU tests compare with (tests/saliency_ref.py) on closed-form cases, its integrated gradients run against
the fp64 oracle (oracle/sgcn.py, oracle/sgcn_img_snp.py), the C ABI's new entry points, and what the models and the
cohort pass refuse before anything is launched."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import saliency_ref as S
from conftest import ROOT
from igcn_amd import _lib

NAMES = ("igcn_saliency_maps", "igcn_grad_cam")


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 3, 16])
@pytest.mark.parametrize("base_form", [None, "rois", "full"])
def test_linear_score_ig_is_gradient_x_input_and_delta_vanishes(steps, base_form):
    rng = np.random.default_rng(steps)
    b, r, h0 = 3, 7, 2
    x = rng.standard_normal((b * r, h0))
    w = rng.standard_normal((b * r, h0))
    base = None if base_form is None else rng.standard_normal((r if base_form == "rois" else b * r, h0))

    def score_and_grad(xx):
        return (w * xx).reshape(b, -1).sum(1) + 0.25, w

    attr, roi, delta, dx = S.integrated_gradients(score_and_grad, x, r, steps, base)
    want, want_roi, s = S.saliency_maps(x, w, r, base)                              # gradient x (input - baseline)
    assert dx.shape == (steps, b * r, h0)
    assert float(np.abs(attr - want).max()) <= 1e-15 * max(1.0, float(np.abs(want).max()))
    assert float(np.abs(roi - want_roi).max()) <= 1e-14
    assert float(np.abs(delta).max()) <= 1e-13, delta
    full = np.zeros_like(x) if base is None else (base if base.shape[0] == b * r else np.tile(base, (b, 1)))
    assert np.array_equal(want, ((x - full) * w).reshape(b, r, h0)) and np.allclose(s, np.abs((x - full) * w).reshape(b, r, h0))
    assert np.array_equal(want_roi, np.abs(want).sum(2))


def test_saliency_normalisation_and_the_all_zero_subject():
    rng = np.random.default_rng(2)
    b, r, h0 = 3, 5, 3
    x, dx = rng.standard_normal((b * r, h0)), rng.standard_normal((4, b * r, h0))
    dx[:, r:2 * r] = 0.0                                                            # subject 1: no gradient at all
    attr, roi, _ = S.saliency_maps(x, dx, r)
    nattr, nroi, _ = S.saliency_maps(x, dx, r, norm=True)
    assert np.array_equal(attr[1], np.zeros((r, h0))) and np.array_equal(nattr[1], attr[1]) and not np.isnan(nroi).any()
    for k in (0, 2):
        assert nroi[k].max() == 1.0
        assert np.allclose(nattr[k], attr[k] / roi[k].max(), rtol=1e-15) and np.allclose(nroi[k], roi[k] / roi[k].max())
    # M path points are averaged: one point repeated is that point
    one, _, _ = S.saliency_maps(x, np.repeat(dx[:1], 5, axis=0), r)
    assert np.allclose(one, S.saliency_maps(x, dx[0], r)[0], rtol=1e-15)


def test_grad_cam_closed_forms():
    r, k = 6, 3
    acts = np.abs(np.random.default_rng(0).standard_normal((2 * r, k))) + 0.1        # positive activations
    grads = np.ones((2 * r, k))
    grads[:r] *= -1.0                                                               # subject 0: every weight negative
    cam, alpha, s = S.grad_cam(acts, grads, r)
    assert np.array_equal(alpha, np.array([[-1.0] * k, [1.0] * k]))
    assert np.array_equal(cam[0], np.zeros(r))                                      # negative everywhere: all zeros
    assert np.allclose(cam[1], acts[r:].sum(1)) and np.allclose(s[0], acts[:r].sum(1))
    ncam = S.grad_cam(acts, grads, r, norm=True)[0]
    assert np.array_equal(ncam[0], np.zeros(r)) and not np.isnan(ncam).any()        # norm leaves it at zero
    assert ncam[1].max() == 1.0 and np.allclose(ncam[1], cam[1] / cam[1].max())


# ---- 2. the restated IG on the fp64 oracle: the quadrature gap shrinks with the steps -------------------------------------
def _target_score(logp, x, tgt):
    score = logp.gather(1, tgt.view(-1, 1)).view(-1)
    g, = torch.autograd.grad(score.sum(), x)                                        # (eval mode: subjects are independent)
    return score.detach().numpy(), g.numpy()


def _shrinks(score_and_grad, x, rois):
    d4 = S.integrated_gradients(score_and_grad, x, rois, 4)[2]
    a32, _, d32, _ = S.integrated_gradients(score_and_grad, x, rois, 32)
    print(f"sum |delta|: steps=4 {np.abs(d4).sum():.3e}, steps=32 {np.abs(d32).sum():.3e}, sum |attr| {np.abs(a32).sum():.3e}")
    assert np.abs(d32).sum() < np.abs(d4).sum()
    assert np.abs(d32).sum() <= 0.05 * np.abs(a32).sum()


@pytest.mark.parametrize("explain", [False, True])
def test_ig_delta_shrinks_on_the_sgcn_oracle(golden, explain):
    from igcn_amd.data import Batch
    from test_oracle_golden import _sgcn_setup
    OSG, rois, sd0, graphs, seed = _sgcn_setup(golden("sgcn_only"))
    sd = {k: v.double() if v.dtype.is_floating_point else v for k, v in sd0.items()}
    data = Batch.from_data_list(graphs)
    data.edge_attr = data.edge_attr.double()
    x = data.x.double().numpy()
    tgt = OSG.model_forward(sd, rois, _with_x(data, x), explain, training=False).argmax(1)

    def score_and_grad(xx):
        d = _with_x(data, xx, grad=True)
        return _target_score(OSG.model_forward(sd, rois, d, explain, training=False), d.x, tgt)
    _shrinks(score_and_grad, x, rois)


def _with_x(data, x, grad=False):
    data.x = torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(grad)
    return data


def test_ig_delta_shrinks_on_the_imaging_genetics_oracle(golden):
    from igcn_amd.data import Batch
    from oracle import sgcn_img_snp as OS
    from test_oracle_golden import _full_setup
    cfg, idx, sd0, graphs, seed = _full_setup(golden("full_tiny"))
    sd = {k: v.double() if v.dtype.is_floating_point else v for k, v in sd0.items()}
    data = Batch.from_data_list(graphs)
    data.edge_attr, data.snps_feat = data.edge_attr.double(), data.snps_feat.double()
    x = data.x.double().numpy()
    fwd = lambda d: OS.model_forward(sd, cfg, idx, d, False, training=False)[0]      # noqa: E731
    tgt = fwd(_with_x(data, x)).argmax(1)

    def score_and_grad(xx):
        d = _with_x(data, xx, grad=True)
        return _target_score(fwd(d), d.x, tgt)
    _shrinks(score_and_grad, x, cfg.rois)


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_saliency_entry_points():
    header = open(os.path.join(ROOT, "include", "igcn.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    assert "kernel/sgcn_img_snp.py:210-211" in header and "kernel/sgcn.py:16-17,72,124-126" in header
    P, I = _lib.P, _lib.I
    assert _lib.SIGNATURES["igcn_saliency_maps"] == (I, [I, I, I, I, P, P, I, P, I, P, P, P])
    assert _lib.SIGNATURES["igcn_grad_cam"] == (I, [I, I, I, P, P, I, P, P, P])


def test_entry_points_refuse_shapes_outside_their_bounds_on_the_host():
    """Refused before any launch (no GPU needed): IGCN_ERR_UNSUPPORTED = -3, never a truncated run."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for b, r, h0, m in ((1, 513, 1, 1), (1, 512, 17, 1), (1, 90, 3, 4097)):
        assert lib.igcn_saliency_maps(b, r, h0, m, None, None, 0, None, 0, None, None, None) == -3, (b, r, h0, m)
        assert b"saliency_maps" in lib.igcn_last_error()
    for b, r, k in ((1, 513, 8), (1, 90, 161)):
        assert lib.igcn_grad_cam(b, r, k, None, None, 0, None, None, None) == -3, (b, r, k)
        assert b"grad_cam" in lib.igcn_last_error()
    assert lib.igcn_saliency_maps(0, 90, 3, 1, None, None, 0, None, 0, None, None, None) == -1      # bad argument
    assert lib.igcn_grad_cam(1, 90, 0, None, None, 0, None, None, None) == -1


# ---- 4. refusals before any launch -------------------------------------------------------------------------------------
def _go_inputs():
    from igcn_amd import synth
    go_snps, adj, pool_dim = synth.go_hierarchy((60, 30, 20, 9, 1), seed=2)
    return synth.go_sparse_inputs(go_snps, adj, "cpu") + (pool_dim,)


def _batch_stub(rois=90, h0=3):
    return SimpleNamespace(x=torch.zeros(rois, h0), edge_index=torch.zeros(2, 0, dtype=torch.int64),
                           edge_attr=torch.zeros(0), snps_feat=torch.zeros(1, 54))


def test_models_refuse_what_they_cannot_map(monkeypatch):
    from calltrace import record_calls
    from igcn_amd.gcn_img_snp import GCN_IMGSNP
    from igcn_amd.sgcn import SGCN_GAT, SGCN_GCN, SGCN_Ori
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
    a_g, a, pool_dim = _go_inputs()
    image_only = [SGCN_GCN(None, 2, 8), SGCN_Ori(3, 8, 8, 8),
                  SGCN_GAT(SimpleNamespace(num_features=3, num_classes=2), 2, 8)]
    genetics = [SGCN_GCN_IMGSNP(2, 8, a_g, a, pool_dim, 32, "cpu", rois=90, H_0=3, num_classes=3),
                SGCN_GCN_CLUSTERLABEL(2, 8, a_g, a, pool_dim, 32, "cpu", H_0=3, num_features=3),
                GCN_IMGSNP(2, 8, a_g, a, pool_dim, 32, "cpu", rois=90, H_0=3, num_classes=3)]
    seen = record_calls(monkeypatch)
    for model in image_only + genetics:
        model.train()
        for call in (model.input_saliency, model.integrated_gradients):
            with pytest.raises(ValueError, match="inputs='pixels'"):
                call(_batch_stub(), inputs="pixels")
            with pytest.raises(ValueError, match="exactly rois=90 nodes"):
                call(_batch_stub(rois=91))
        if not isinstance(model, SGCN_Ori):
            with pytest.raises(ValueError, match="never fills final_conv_acts"):
                model.grad_cam(_batch_stub())
        assert model.training
    for model in image_only:
        for inputs in ("snps", "both"):
            with pytest.raises(ValueError, match="image-only model"):
                model.input_saliency(_batch_stub(), inputs=inputs)
            with pytest.raises(ValueError, match="image-only model"):
                model.integrated_gradients(_batch_stub(), inputs=inputs)
    with pytest.raises(ValueError, match="one plain pass"):
        genetics[2].input_saliency(_batch_stub(), isExplain=True)
    with pytest.raises(ValueError, match=r"steps=0"):
        image_only[0].integrated_gradients(_batch_stub(), steps=0)
    assert seen == []


def test_guide_model_has_no_saliency_methods():
    from igcn_amd.guide_img_snp import GUIDE_IMGSNP
    assert not any(hasattr(GUIDE_IMGSNP, m) for m in ("input_saliency", "integrated_gradients", "grad_cam"))


def test_saliency_maps_refuses_before_any_launch(monkeypatch):
    from calltrace import record_calls
    from igcn_amd.sgcn import SGCN_GCN
    from igcn_amd.train import saliency_maps
    model = SGCN_GCN(None, 2, 8)
    seen = record_calls(monkeypatch)
    with pytest.raises(ValueError, match="method='lime'"):
        saliency_maps(model, [], method="lime")
    with pytest.raises(ValueError, match="target='truth'"):
        saliency_maps(model, [], target="truth")
    with pytest.raises(ValueError, match="'gradcam' maps the image branch only"):
        saliency_maps(model, [], method="gradcam", inputs="both")
    with pytest.raises(ValueError, match="num_classes=0"):
        saliency_maps(model, [], num_classes=0)
    with pytest.raises(ValueError, match="the loader is empty"):
        saliency_maps(model, [])
    assert seen == []
