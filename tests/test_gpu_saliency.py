"""GPU tests of the ROI x modality saliency maps: igcn_saliency_maps / igcn_grad_cam against the float64 restatement
(tests/saliency_ref.py), the models' ``input_saliency`` / ``integrated_gradients`` / ``grad_cam`` against the eval-mode
``data.x.grad`` the suite already tests and against the fp64 oracle, that the model is left as it was, and
train.saliency_maps against the per-batch outputs summed on the host.

Bounds.  Kernels: |got - want| <= 1e-6 + 1e-4 s per element, s the sum of the absolute terms of the element's reduction
(an fp32 sum of n <= 512 terms errs by at most (n - 1) 2^-24 <= 3.1e-5 of s).  Normalisation: against the same call's
un-normalised output, one fp32 division: 2^-23 relative.  Models against the ordinary eval backward: assert_matches 1e-6.
Models against the oracle: the map is the input gradient times an exactly known factor, so the bound is the bound the
existing eval-mode ``data.x.grad`` test of that model holds the gradient to (tol * max|grad|) times |factor|, plus one
fp32 rounding of the product."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import saliency_ref as S
from conftest import assert_matches
from _weights import seeded_state

pytestmark = pytest.mark.gpu

B, ROIS = 5, 90
CROSS = dict(isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseProb4Regr=True,
             isImageOnly=False, isSNPsOnly=False)
POOL = (37, 18, 9, 3, 1)                        # the smallest synthetic GO DAG of the sibling GPU tests


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


# ---- 1. the kernels against the restatement ------------------------------------------------------------------------------
def _raw_saliency(x, dx, b, r, h0, m, base, norm):
    """igcn_saliency_maps into buffers filled with NaN beforehand: whatever the launch does not write stays NaN."""
    from igcn_amd import _lib
    attr = torch.full((b, r, h0), float("nan"), device="cuda")
    roi = torch.full((b, r), float("nan"), device="cuda")
    per_subject = int(base is not None and base.shape[0] == b * r and b > 1)
    _lib.call("igcn_saliency_maps", b, r, h0, m, _lib.ptr(x), _lib.ptr(base), per_subject, _lib.ptr(dx), norm,
              _lib.ptr(attr), _lib.ptr(roi), _lib.stream_ptr())
    return attr, roi


SAL_SHAPES = [(1, 1, 1, 1, None), (3, 90, 3, 1, "rois"), (2, 90, 1, 5, "full"), (2, 270, 1, 4, None),
              (1, 512, 3, 2, "full"), (4, 54, 1, 1, "rois")]


@pytest.mark.parametrize("b,r,h0,m,base_form", SAL_SHAPES)
def test_saliency_maps_kernel_vs_restatement(b, r, h0, m, base_form):
    rng = np.random.default_rng(b * 1000 + r + h0 + m)
    x = torch.from_numpy(rng.standard_normal((b * r, h0))).float()
    dx = torch.from_numpy(rng.standard_normal((m, b * r, h0))).float()
    if b > 1:
        dx[:, :r] = 0.0                                                              # subject 0: an all-zero map
    base = None if base_form is None else torch.from_numpy(
        rng.standard_normal((r if base_form == "rois" else b * r, h0))).float()
    xg, dxg, bg = x.cuda(), dx.cuda(), None if base is None else base.cuda()
    attr, roi = _raw_saliency(xg, dxg, b, r, h0, m, bg, 0)
    want, want_roi, s = S.saliency_maps(x, dx, r, base)
    err, err_roi = np.abs(attr.double().cpu().numpy() - want), np.abs(roi.double().cpu().numpy() - want_roi)
    print(f"attr: largest fraction of the bound {float((err / S.bound(s)).max()):.3e}; roi {float((err_roi / S.bound(s.sum(2))).max()):.3e}")
    assert not torch.isnan(attr).any() and not torch.isnan(roi).any()                # every element written
    assert (err <= S.bound(s)).all() and (err_roi <= S.bound(s.sum(2))).all()
    # two runs: the same bits
    again = _raw_saliency(xg, dxg, b, r, h0, m, bg, 0)
    assert torch.equal(again[0], attr) and torch.equal(again[1], roi)
    if base is None:                                                                 # NULL == an explicit zero baseline
        for zero in (torch.zeros(r, h0, device="cuda"), torch.zeros(b * r, h0, device="cuda")):
            z = _raw_saliency(xg, dxg, b, r, h0, m, zero, 0)
            assert torch.equal(z[0], attr) and torch.equal(z[1], roi)
    # normalisation, against this call's own un-normalised output
    nattr, nroi = _raw_saliency(xg, dxg, b, r, h0, m, bg, 1)
    assert torch.equal(_raw_saliency(xg, dxg, b, r, h0, m, bg, 1)[0], nattr)
    assert not torch.isnan(nattr).any() and not torch.isnan(nroi).any()
    a64, r64 = attr.double().cpu(), roi.double().cpu()
    mx = r64.max(1).values
    for k in range(b):
        if float(mx[k]) == 0.0:
            assert float(nattr[k].abs().max()) == 0.0 and float(nroi[k].abs().max()) == 0.0
            continue
        wa, wr = a64[k] / mx[k], r64[k] / mx[k]
        assert bool(((nattr[k].double().cpu() - wa).abs() <= 2.0 ** -23 * wa.abs()).all())
        assert bool(((nroi[k].double().cpu() - wr).abs() <= 2.0 ** -23 * wr.abs()).all())
        assert float(nroi[k].max()) == 1.0
    if b > 1:
        assert float(mx[0]) == 0.0 and float(mx[1]) > 0.0


def _raw_cam(acts, grads, b, r, k, norm):
    from igcn_amd import _lib
    cam = torch.full((b, r), float("nan"), device="cuda")
    alpha = torch.full((b, k), float("nan"), device="cuda")
    _lib.call("igcn_grad_cam", b, r, k, _lib.ptr(acts), _lib.ptr(grads), norm, _lib.ptr(cam), _lib.ptr(alpha),
              _lib.stream_ptr())
    return cam, alpha


@pytest.mark.parametrize("b,r,k", [(1, 1, 1), (3, 90, 5), (2, 90, 33), (2, 90, 160), (1, 512, 64), (2, 270, 20)])
def test_grad_cam_kernel_vs_restatement(b, r, k):
    rng = np.random.default_rng(b * 1000 + r + k)
    acts = torch.from_numpy(rng.standard_normal((b * r, k))).float()
    grads = torch.from_numpy(rng.standard_normal((b * r, k))).float()
    if b > 1:                                                   # subject 0: the weighted sum is negative everywhere
        acts[:r] = acts[:r].abs() + 0.1
        grads[:r] = -grads[:r].abs() - 0.1
    ag, gg = acts.cuda(), grads.cuda()
    cam, alpha = _raw_cam(ag, gg, b, r, k, 0)
    want, want_alpha, s = S.grad_cam(acts, grads, r)
    s_alpha = np.abs(grads.double().numpy()).reshape(b, r, k).mean(1)
    err, err_a = np.abs(cam.double().cpu().numpy() - want), np.abs(alpha.double().cpu().numpy() - want_alpha)
    print(f"cam: largest fraction of the bound {float((err / S.bound(s)).max()):.3e}; alpha {float((err_a / S.bound(s_alpha)).max()):.3e}")
    assert not torch.isnan(cam).any() and not torch.isnan(alpha).any()
    assert (err <= S.bound(s)).all() and (err_a <= S.bound(s_alpha)).all()
    assert float(cam.min()) >= 0.0
    again = _raw_cam(ag, gg, b, r, k, 0)
    assert torch.equal(again[0], cam) and torch.equal(again[1], alpha)
    ncam, nalpha = _raw_cam(ag, gg, b, r, k, 1)
    assert torch.equal(nalpha, alpha) and torch.equal(_raw_cam(ag, gg, b, r, k, 1)[0], ncam)
    assert not torch.isnan(ncam).any()
    c64 = cam.double().cpu()
    for j in range(b):
        mx = c64[j].max()
        if float(mx) == 0.0:
            assert float(ncam[j].abs().max()) == 0.0
            continue
        w = c64[j] / mx
        assert bool(((ncam[j].double().cpu() - w).abs() <= 2.0 ** -23 * w.abs()).all()) and float(ncam[j].max()) == 1.0
    if b > 1:
        assert float(c64[0].max()) == 0.0 and float(c64[1].max()) > 0.0


def test_kernels_refuse_shapes_outside_their_bounds():
    from igcn_amd import _lib, ops
    z = torch.zeros(8, device="cuda")
    for b, r, h0, m in ((1, 513, 1, 1), (1, 512, 17, 1), (1, 90, 3, 4097)):
        with pytest.raises(_lib.IgcnError, match=r"rc=-3"):                           # (refused on the host: no launch)
            _lib.call("igcn_saliency_maps", b, r, h0, m, _lib.ptr(z), None, 0, _lib.ptr(z), 0, _lib.ptr(z), _lib.ptr(z),
                      _lib.stream_ptr())
    for b, r, k in ((1, 513, 8), (1, 90, 161)):
        with pytest.raises(_lib.IgcnError, match=r"rc=-3"):
            _lib.call("igcn_grad_cam", b, r, k, _lib.ptr(z), _lib.ptr(z), 0, _lib.ptr(z), _lib.ptr(z), _lib.stream_ptr())
    with pytest.raises(ValueError, match="saliency_maps: rois=513"):
        ops.saliency_maps(torch.zeros(513, 1, device="cuda"), torch.zeros(513, 1, device="cuda"), 513)
    with pytest.raises(ValueError, match="grad_cam: rois=90, K=161"):
        ops.grad_cam(torch.zeros(90, 161, device="cuda"), torch.zeros(90, 161, device="cuda"), 90)


def test_ops_wrappers_are_the_raw_launches():
    from igcn_amd import ops
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((2 * 90, 3))).float().cuda()
    dx = torch.from_numpy(rng.standard_normal((3, 2 * 90, 3))).float().cuda()
    base = torch.from_numpy(rng.standard_normal((90, 3))).float().cuda()
    for norm in (False, True):
        got = ops.saliency_maps(x, dx, 90, base, normalize=norm)
        want = _raw_saliency(x, dx, 2, 90, 3, 3, base, int(norm))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    one = ops.saliency_maps(x, dx[0], 90)                                            # a single gradient is M = 1
    assert torch.equal(one[0], (x * dx[0]).view(2, 90, 3))                           # gradient x input, exactly
    acts, grads = x.repeat(1, 4).contiguous(), dx[1].repeat(1, 4).contiguous()
    cam, alpha = ops.grad_cam(acts, grads, 90, normalize=False, return_alpha=True)
    raw = _raw_cam(acts, grads, 2, 90, 12, 0)
    assert torch.equal(cam, raw[0]) and torch.equal(alpha, raw[1])


# ---- 2. the models -------------------------------------------------------------------------------------------------------
def _go(device="cuda"):
    from igcn_amd import synth
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=2)
    return synth.go_sparse_inputs(go_snps, adj, device) + (pool_dim,), (go_snps, adj)


def _seed(model, seed):
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, seed)
    model.load_state_dict(sd)
    return sd


def _model(kind):
    torch.manual_seed(11)
    if kind in ("imgsnp", "clusterlabel", "gcn_img_snp"):
        (a_g, a, pool_dim), _ = _go()
        if kind == "imgsnp":
            from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
            model = SGCN_GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=ROIS, H_0=3, num_classes=3, **CROSS)
        elif kind == "clusterlabel":
            from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
            model = SGCN_GCN_CLUSTERLABEL(2, 16, a_g, a, pool_dim, 32, "cuda", rois=ROIS, H_0=3, num_features=3,
                                          isCrossAtten=True)
        else:
            from igcn_amd.gcn_img_snp import GCN_IMGSNP
            model = GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=ROIS, H_0=3, num_classes=3, isCrossAtten=True,
                               num_regr=3, isImageOnly=False, isSNPsOnly=False)
    elif kind == "sgcn_gcn":
        from igcn_amd.sgcn import SGCN_GCN
        model = SGCN_GCN(None, 2, 16, rois=ROIS, H_0=3, num_features=3, num_classes=3)
    elif kind == "sgcn_gat":
        from igcn_amd.sgcn import SGCN_GAT
        model = SGCN_GAT(SimpleNamespace(num_features=3, num_classes=3), 2, 16, rois=ROIS, H_0=3)
    else:
        from igcn_amd.sgcn import SGCN_Ori
        model = SGCN_Ori(3, 32, 32, 5, class_num=3, rois=ROIS)
    model = model.cuda()
    with torch.no_grad():                                       # masks of O(1) on both sides of 1/2
        model.prob.normal_()
        model.prob_bias.normal_()
    return model


def _graphs(n=B, seed=77):
    from igcn_amd import synth
    return synth.brain_graph_list(n, seed=seed, rois=ROIS, h0=3, top_k=3, tsne_dim=16, num_classes=3)


def _batch(graphs):
    from igcn_amd.data import Batch
    return Batch.from_data_list(graphs).to("cuda")


def _forward(model, data, explain):
    if hasattr(model, "go_network"):
        if getattr(model, "single_pass", False):
            return model(data, None, "cuda")[0]
        return model(data, None, "cuda", isExplain=explain)[0]
    return model(data, isExplain=explain)


KINDS = ["imgsnp", "clusterlabel", "gcn_img_snp", "sgcn_gcn", "sgcn_gat", "sgcn_ori"]


@pytest.mark.parametrize("explain", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_input_saliency_is_the_tested_input_gradient_times_x(kind, explain):
    """``attr`` = data.x.grad * x of an ordinary eval forward + (logp * onehot).sum().backward(), for the predicted class,
    one class for everybody and the labels."""
    model, graphs = _model(kind).eval(), _graphs()
    if kind == "gcn_img_snp" and explain:
        with pytest.raises(ValueError, match="one plain pass"):
            model.input_saliency(_batch(graphs), None, "cuda", isExplain=True)
        return
    data = _batch(graphs)
    for target in (None, 1, "y"):
        ref = _batch(graphs)
        logp = _forward(model, ref, explain)
        tgt = logp.detach().argmax(1) if target is None else (
            torch.full((B,), 1, device="cuda") if target == 1 else ref.y.view(-1))
        onehot = torch.nn.functional.one_hot(tgt, 3).float()
        (logp * onehot).sum().backward()
        want = (ref.x.grad * ref.x.detach()).view(B, ROIS, 3)
        r = model.input_saliency(data, None, "cuda", target=data.y if target == "y" else target, isExplain=explain)
        assert set(r) == {"attr", "roi", "target"} and r["target"].dtype == torch.int64
        assert torch.equal(r["target"], tgt) and float(want.abs().max()) > 0
        assert_matches(r["attr"], want.cpu().numpy(), 1e-6, f"{kind} attr target={target}")
        assert_matches(r["roi"], want.abs().sum(2).cpu().numpy(), 1e-6, f"{kind} roi target={target}")
        n = model.input_saliency(data, None, "cuda", target=tgt, isExplain=explain, normalize=True)
        assert float((n["roi"].max(1).values - 1).abs().max()) == 0.0
    assert torch.equal(model.input_saliency(data, None, "cuda", target=1, isExplain=explain)["attr"],
                       model.input_saliency(data, None, "cuda", target=1, isExplain=explain)["attr"])


def test_image_only_models_and_non_ori_models_refuse():
    data = _batch(_graphs())
    model = _model("sgcn_gcn")
    for inputs in ("snps", "both"):
        with pytest.raises(ValueError, match="image-only model"):
            model.input_saliency(data, inputs=inputs)
    for kind in ("sgcn_gcn", "imgsnp"):
        with pytest.raises(ValueError, match="never fills final_conv_acts"):
            _model(kind).grad_cam(data)


def test_refuses_to_run_under_stream_capture(monkeypatch):
    model, data = _model("sgcn_gcn"), _batch(_graphs())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for call in (model.input_saliency, model.integrated_gradients):
        with pytest.raises(RuntimeError, match="eagerly only"):
            call(data)
    with pytest.raises(RuntimeError, match="eagerly only"):
        _model("sgcn_ori").grad_cam(data)


# ---- 3. against the fp64 oracle ------------------------------------------------------------------------------------------
def _assert_product(got, factor, grad_ref, tol, what):
    """got == factor * grad_ref where the gradient is held to tol * max|grad_ref| (the existing data.x.grad bound) and
    ``factor`` is known exactly; one fp32 rounding of the product on top."""
    factor, grad_ref = np.asarray(factor, dtype=np.float64), np.asarray(grad_ref, dtype=np.float64)
    want = factor * grad_ref
    bound = tol * np.abs(grad_ref).max() * np.abs(factor) + 2.0 ** -23 * np.abs(want)
    err = np.abs(got.double().cpu().numpy().reshape(want.shape) - want)
    print(f"{what}: largest fraction of the bound {float((err / np.maximum(bound, 1e-300)).max()):.3e}")
    assert (err <= bound).all(), (what, float(err.max()))
    return want


def _cpu_batch(graphs, snps=False):
    from igcn_amd.data import Batch
    d = Batch.from_data_list(graphs)
    d.x = d.x.double().requires_grad_(True)
    d.edge_attr = d.edge_attr.double()
    if snps:
        d.snps_feat = d.snps_feat.double().requires_grad_(True)
    return d


@pytest.mark.parametrize("explain", [False, True])
def test_sgcn_gcn_saliency_and_ig_vs_oracle(explain):
    """SGCN_GCN(2, 16): gradient x input at the 3e-3 of test_sgcn_only_vs_oracle_config_sizes, and integrated_gradients
    (steps = 4) against the oracle's midpoint rule: attr at the same bound (the mean over the path points of the
    per-point bounds), delta within 1e-3 sum|attr_oracle| + 1e-5 of the oracle's delta."""
    from igcn_amd.sgcn import SGCN_GCN
    from oracle import sgcn as OSG, sgcn_img_snp as OS
    model = SGCN_GCN(None, 2, 16, rois=ROIS, H_0=3, num_features=3, num_classes=3).cuda().eval()
    sd = _seed(model, 6)
    graphs = _graphs()
    data = _batch(graphs)
    sdo = OS.make_leaf_state(sd, dtype=torch.float64)
    tgt = data.y.view(-1).cpu()
    onehot = torch.nn.functional.one_hot(tgt, 3).double()

    def score_and_grad(xx):
        d = _cpu_batch(graphs)
        d.x = torch.from_numpy(np.ascontiguousarray(xx)).requires_grad_(True)
        logp = OSG.model_forward(sdo, ROIS, d, explain)
        g, = torch.autograd.grad((logp * onehot).sum(), d.x)
        return (logp.detach() * onehot).sum(1).numpy(), g.numpy()

    x64 = data.x.detach().double().cpu().numpy()
    _, g_ref = score_and_grad(x64)
    r = model.input_saliency(data, target=data.y, isExplain=explain)
    want = _assert_product(r["attr"], x64, g_ref, 3e-3, f"SGCN_GCN attr explain={explain}")
    roi_bound = (3e-3 * np.abs(g_ref).max() * np.abs(x64) + 2.0 ** -22 * np.abs(want)).reshape(B, ROIS, 3).sum(2)
    assert (np.abs(r["roi"].double().cpu().numpy() - np.abs(want).reshape(B, ROIS, 3).sum(2)) <= roi_bound).all()
    # integrated gradients, steps = 4
    ig = model.integrated_gradients(data, target=data.y, isExplain=explain, steps=4)
    assert set(ig) == {"attr", "roi", "target", "delta"} and tuple(ig["delta"].shape) == (B,)
    attr_o, roi_o, delta_o, dx_o = S.integrated_gradients(score_and_grad, x64, ROIS, 4)
    bound = 3e-3 * np.mean([np.abs(g).max() for g in dx_o]) * np.abs(x64) + 2.0 ** -22 * np.abs(attr_o).reshape(-1, 3)
    err = np.abs(ig["attr"].double().cpu().numpy() - attr_o).reshape(-1, 3)
    print(f"IG attr: largest fraction of the bound {float((err / np.maximum(bound, 1e-300)).max()):.3e}")
    assert (err <= bound).all()
    derr = np.abs(ig["delta"].double().cpu().numpy() - delta_o)
    dbound = 1e-3 * np.abs(attr_o).sum((1, 2)) + 1e-5
    print(f"IG delta: oracle {delta_o}, got {ig['delta'].cpu().numpy()}, fraction of the bound {float((derr / dbound).max()):.3e}")
    assert (derr <= dbound).all()
    # a baseline in either form: the same path as the oracle's
    base = torch.from_numpy(np.random.default_rng(1).standard_normal((ROIS, 3)) * 0.1).float()
    ig_b = model.integrated_gradients(data, target=data.y, isExplain=explain, steps=2, baseline=base.cuda())
    ig_f = model.integrated_gradients(data, target=data.y, isExplain=explain, steps=2, baseline=base.repeat(B, 1).cuda())
    assert torch.equal(ig_b["attr"], ig_f["attr"]) and torch.equal(ig_b["delta"], ig_f["delta"])
    attr_b, _, delta_b, dx_b = S.integrated_gradients(score_and_grad, x64, ROIS, 2, base.double().numpy())
    d64 = x64 - np.tile(base.double().numpy(), (B, 1))
    bound = 3e-3 * np.mean([np.abs(g).max() for g in dx_b]) * np.abs(d64) + 2.0 ** -22 * np.abs(attr_b).reshape(-1, 3) \
        + 2.0 ** -23 * np.abs(x64) * np.abs(dx_b).mean(0)                               # (x - base is rounded once in fp32)
    assert (np.abs(ig_b["attr"].double().cpu().numpy() - attr_b).reshape(-1, 3) <= bound).all()
    assert (np.abs(ig_b["delta"].double().cpu().numpy() - delta_b) <= 1e-3 * np.abs(attr_b).sum((1, 2)) + 1e-5).all()


@pytest.mark.parametrize("explain", [False, True])
def test_sgcn_ori_saliency_and_grad_cam_vs_oracle(explain):
    """SGCN_Ori(3, 32, 32, 5) at the bounds of test_both_routes_vs_fp64_in_eval_mode: data.x.grad and the tap's gradient
    1e-3, the tap 1e-4.  Grad-CAM from the oracle's taps: alpha is a mean of gradients (each within eg = 1e-3 max|grads|),
    acts lie within ea = 1e-4 max|acts|, ReLU is 1-Lipschitz, so |cam - cam_oracle| <= sum_k (|alpha_k| ea + |acts_k| eg
    + ea eg) + the kernel's own 1e-6 + 1e-4 s."""
    import sgcn_ori_ref as REF
    from igcn_amd.sgcn import SGCN_Ori
    model = SGCN_Ori(3, 32, 32, 5, class_num=3, rois=ROIS).cuda().eval()
    _seed(model, 8)
    graphs = _graphs()
    data = _batch(graphs)
    sd = {k: (v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu())
          for k, v in model.state_dict().items()}
    dcpu = _cpu_batch(graphs)
    taps = {}
    logp = REF.model_forward(sd, ROIS, dcpu, explain, training=False, taps=taps)
    onehot = torch.nn.functional.one_hot(dcpu.y.view(-1), 3).double()
    g_x, g_acts = torch.autograd.grad((logp * onehot).sum(), [dcpu.x, taps["acts"]])
    x64 = dcpu.x.detach().numpy()
    r = model.input_saliency(data, target=data.y, isExplain=explain)
    _assert_product(r["attr"], x64, g_x.numpy(), 1e-3, f"SGCN_Ori attr explain={explain}")
    cam = model.grad_cam(data, target=data.y, isExplain=explain, normalize=False)
    assert tuple(cam.shape) == (B, ROIS) and cam.dtype == torch.float32
    acts_o = taps["acts"].detach().numpy()
    want, alpha_o, s = S.grad_cam(acts_o, g_acts.numpy(), ROIS)
    ea, eg = 1e-4 * np.abs(acts_o).max(), 1e-3 * np.abs(g_acts.numpy()).max()
    bound = (np.abs(alpha_o)[:, None, :] * ea + np.abs(acts_o).reshape(B, ROIS, -1) * eg + ea * eg).sum(2) + S.bound(s)
    err = np.abs(cam.double().cpu().numpy() - want)
    print(f"grad_cam: largest fraction of the bound {float((err / bound).max()):.3e}; max cam {float(want.max()):.3e}")
    assert (err <= bound).all() and float(want.max()) > 0
    # ... and it is the kernel on the taps an ordinary eval forward + backward of the same score leaves, bit for bit
    from igcn_amd import ops
    ref = _batch(graphs)
    out = model(ref, isExplain=explain)
    (out * torch.nn.functional.one_hot(ref.y.view(-1), 3).float()).sum().backward()
    assert torch.equal(ops.grad_cam(model.final_conv_acts, model.final_conv_grads, ROIS, normalize=False), cam)
    ncam = model.grad_cam(data, target=data.y, isExplain=explain)                       # normalize=True is the default
    mx = cam.double().max(1).values
    assert bool((mx > 0).all())
    w = cam.double() / mx[:, None]
    assert bool(((ncam.double() - w).abs() <= 2.0 ** -23 * w).all())
    assert torch.equal(model.grad_cam(data, target=data.y, isExplain=explain), ncam)


@pytest.mark.parametrize("explain", [False, True])
def test_imgsnp_saliency_vs_oracle(explain):
    """SGCN_GCN_IMGSNP(2, 16) by the relu_forced procedure of test_full_model_vs_oracle_larger and its 1e-3, ``snps``
    included: the HIP path's decisions at relu(out_proj(attention)) are observed and imposed on the oracle inside a 2e-5
    band, agreement is required outside it."""
    from conftest import relu_forced
    from igcn_amd import ops, synth
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    from oracle import go_network as OG, sgcn_img_snp as OS
    (a_g, a, pool_dim), (go_snps, adj) = _go()
    model = SGCN_GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=ROIS, H_0=3, num_classes=3, **CROSS).cuda().eval()
    sd = _seed(model, 5)
    graphs = _graphs()
    data = _batch(graphs)
    seen = []
    real_ca = model._cross_attention

    def spy(query, memory, **kw):
        out = real_ca(query, memory, **kw)
        if not kw.get("defer_out_proj"):
            seen.append(out.detach().cpu() > 0)
        return out
    model._cross_attention = spy
    real_fused = ops.OutProjHeadInputs.apply

    def spy_fused(*args):
        out = real_fused(*args)
        seen.append(out[3].detach().cpu().view(args[0].shape[0], -1, args[1].shape[0]) > 0)
        return out
    ops.OutProjHeadInputs.apply = spy_fused
    try:
        r = model.input_saliency(data, None, "cuda", target=data.y, isExplain=explain, inputs="both")
    finally:
        ops.OutProjHeadInputs.apply = real_fused
        del model._cross_attention
    assert set(r) == {"attr", "roi", "target", "snps"} and tuple(r["snps"].shape) == (B, 54)
    a_g_c, a_c = synth.go_sparse_inputs(go_snps, adj)
    idx = OG.go_index_sets(a_g_c, a_c, list(POOL), 2)
    sdo = OS.make_leaf_state(sd, dtype=torch.float64)
    dcpu = _cpu_batch(graphs, snps=True)
    cfg = SimpleNamespace(num_layers=2, rois=ROIS, image_only=False, rbf_gamma=0.01)
    with relu_forced({11: seen[0]}, band=2e-5) as rf:           # (site 11 of a pass with two GCNConv layers: out_proj)
        logp = OS.model_forward(sdo, cfg, idx, dcpu, explain, training=False)[0]
    assert rf.mismatch_outside == 0 and rf.flips <= 4, (rf.mismatch_outside, rf.flips)
    onehot = torch.nn.functional.one_hot(dcpu.y.view(-1), 3).double()
    g_x, g_s = torch.autograd.grad((logp * onehot).sum(), [dcpu.x, dcpu.snps_feat])
    assert float(g_s.abs().max()) > 0
    _assert_product(r["attr"], dcpu.x.detach().numpy(), g_x.numpy(), 1e-3, f"IMGSNP attr explain={explain}")
    _assert_product(r["snps"], dcpu.snps_feat.detach().numpy(), g_s.numpy(), 1e-3, f"IMGSNP snps explain={explain}")
    only = model.input_saliency(data, None, "cuda", target=data.y, isExplain=explain, inputs="snps")
    assert torch.equal(only["snps"], r["snps"]) and torch.equal(only["attr"], r["attr"])


def test_imgsnp_integrated_gradients_over_both_modalities():
    """Completeness over image + SNPs: delta is sum attr + sum snps - (score(x, s) - score(0, 0)) of the call's own
    outputs, and it shrinks as the steps grow."""
    model, data = _model("imgsnp").eval(), _batch(_graphs())
    with torch.no_grad():
        logp = model(data, None, "cuda")[0]
        zero = _batch(_graphs())
        zero.x, zero.snps_feat = torch.zeros_like(zero.x), torch.zeros_like(zero.snps_feat)
        logp0 = model(zero, None, "cuda")[0]
    tgt = logp.argmax(1)
    gap = (logp.gather(1, tgt[:, None]) - logp0.gather(1, tgt[:, None])).view(-1).double()
    deltas = []
    for steps in (2, 16):
        r = model.integrated_gradients(data, None, "cuda", inputs="both", steps=steps)
        assert set(r) == {"attr", "roi", "target", "snps", "delta"} and torch.equal(r["target"], tgt)
        total = r["attr"].double().sum((1, 2)) + r["snps"].double().sum(1)
        assert float((r["delta"].double() - (total - gap)).abs().max()) <= 1e-5 * max(1.0, float(gap.abs().max()))
        deltas.append(float(r["delta"].abs().sum()))
    print(f"sum |delta|: steps=2 {deltas[0]:.3e}, steps=16 {deltas[1]:.3e}")
    s = model.integrated_gradients(data, None, "cuda", inputs="snps", steps=2)
    assert set(s) == {"target", "snps", "delta"}


# ---- 4. the model is left as it was --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["imgsnp", "sgcn_ori"])
def test_saliency_calls_leave_the_model_as_it_was(kind):
    from igcn_amd import train
    model, twin = _model(kind).train(), _model(kind).train()                          # (seeded alike: the same bits)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), twin.state_dict().values()))
    graphs = _graphs()
    data = _batch(graphs)
    both = kind == "imgsnp"
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
    data.x.requires_grad_(True)
    data.x.grad = torch.ones_like(data.x)
    if both:
        data.snps_feat.requires_grad_(False)
    grads = {k: (p.grad, p.grad.clone()) for k, p in model.named_parameters()}
    xg = data.x.grad
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rng, host_rng = torch.cuda.get_rng_state(), torch.get_rng_state()
    drop = getattr(getattr(model, "go_network", None), "_drop_state", None)
    counter = None if drop is None else drop.state.clone()
    acts_before = getattr(model, "final_conv_acts", None)
    inputs = "both" if both else "image"
    model.input_saliency(data, None, "cuda", inputs=inputs)
    assert train.stream_pending() == 0
    model.input_saliency(data, None, "cuda", isExplain=True, target=data.y, normalize=True)
    model.integrated_gradients(data, None, "cuda", inputs=inputs, steps=2)
    if kind == "sgcn_ori":
        model.grad_cam(data)
        model.grad_cam(data, isExplain=True, target=0)
        assert model.final_conv_acts is acts_before and model.final_conv_grads is None
    assert train.stream_pending() == 0
    assert all(m.training for m in model.modules())
    assert all(p.requires_grad for p in model.parameters())
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k                                            # (num_batches_tracked included)
    for k, p in model.named_parameters():
        assert p.grad is grads[k][0] and torch.equal(p.grad, grads[k][1]), k
    assert data.x.grad is xg and bool((xg == 1).all()) and data.x.requires_grad
    if both:
        assert not data.snps_feat.requires_grad and data.snps_feat.grad is None
    assert torch.equal(torch.cuda.get_rng_state(), rng) and torch.equal(torch.get_rng_state(), host_rng)
    assert counter is None or torch.equal(model.go_network._drop_state.state, counter)
    assert model.last_edge_prob is None
    # a train step afterwards is the train step of a model that never made the calls
    opt, opt2 = train.FlatAdam(model.parameters(), lr=1e-3), train.FlatAdam(twin.parameters(), lr=1e-3)
    data.x.grad = None
    torch.manual_seed(5)
    loss = float(train.train_step(model, opt, data))
    torch.manual_seed(5)
    loss2 = float(train.train_step(twin, opt2, _batch(graphs)))
    assert loss == loss2 and np.isfinite(loss), (loss, loss2)
    assert train.stream_pending() == 0


# ---- 5. the cohort pass --------------------------------------------------------------------------------------------------
LABELS = [0, 2, 2, 0, 2, 0, 2, 2, 0, 0, 2, 0, 2]                                      # class 1 has no subject


def _cohort_graphs():
    graphs = _graphs(13, seed=6)
    for g_, lab in zip(graphs, LABELS):
        g_.y = torch.tensor([lab])
    return graphs


@pytest.mark.parametrize("case", ["gradxinput", "gradxinput_both", "ig", "gradcam"])
def test_saliency_maps_over_a_ragged_loader(case):
    """5 + 5 + 3 subjects, 3 classes, one empty: the tables equal the per-batch method outputs summed on the host in
    fp64."""
    from igcn_amd.data import DataLoader
    from igcn_amd.train import saliency_maps
    kind = {"gradxinput_both": "imgsnp", "gradcam": "sgcn_ori"}.get(case, "sgcn_gcn")
    method = case.split("_")[0]
    model, graphs = _model(kind), _cohort_graphs()
    kw = {"inputs": "both"} if case == "gradxinput_both" else {}
    target = "label" if case == "ig" else None
    r = saliency_maps(model, DataLoader(graphs, batch_size=5), method=method, target=target, steps=2, num_classes=3,
                      top_k=5, device="cuda", **kw)
    attrs, rois, snps, deltas = [], [], [], []
    for lo, hi in ((0, 5), (5, 10), (10, 13)):
        d = _batch(graphs[lo:hi])
        if method == "gradcam":
            o = {"roi": model.grad_cam(d)}
            o["attr"] = o["roi"]
        elif method == "ig":
            o = model.integrated_gradients(d, None, "cuda", target=d.y, steps=2, normalize=True)
            deltas.append(o["delta"].double().cpu())
        else:
            o = model.input_saliency(d, None, "cuda", normalize=True, **kw)
        attrs.append(o["attr"].double().cpu())
        rois.append(o["roi"].double().cpu())
        if "snps" in o:
            snps.append(o["snps"].double().cpu())
    attrs, rois, y = torch.cat(attrs), torch.cat(rois), torch.tensor(LABELS)

    def per_class(t):
        return torch.stack([t[y == c].mean(0) if bool((y == c).any()) else torch.zeros_like(t[0]) for c in range(3)])

    want = {"mean": per_class(attrs), "overall": attrs.mean(0), "roi_mean": per_class(rois), "roi_overall": rois.mean(0)}
    keys = {"mean", "overall", "roi_mean", "roi_overall", "count", "n", "top_regions"}
    if snps:
        want["snps_mean"] = per_class(torch.cat(snps))
        keys |= {"snps_mean", "top_snps"}
    if method == "ig":
        keys |= {"mean_abs_delta"}
        assert abs(r["mean_abs_delta"] - float(torch.cat(deltas).abs().mean())) <= 1e-6 * max(1.0, r["mean_abs_delta"])
    assert set(r) == keys and r["n"] == 13 and r["count"].cpu().tolist() == [6, 0, 7]
    assert tuple(r["mean"].shape) == ((3, ROIS) if method == "gradcam" else (3, ROIS, 3))
    for k, w in want.items():
        got = r[k]
        assert got.dtype == torch.float32 and got.shape == w.shape, k
        assert torch.allclose(got.double().cpu(), w, rtol=1e-6, atol=1e-12), k
    assert float(r["mean"][1].abs().max()) == 0.0 and float(r["roi_overall"].max()) > 0
    top = r["top_regions"].cpu()
    assert tuple(top.shape) == (5,) and top.dtype == torch.int64
    vals = r["roi_overall"].cpu()[top]
    assert torch.equal(vals, torch.topk(r["roi_overall"].cpu(), 5).values)
    assert torch.allclose(vals.double(), torch.topk(want["roi_overall"], 5).values, rtol=1e-6, atol=1e-12)
    if snps:
        overall = torch.cat(snps).mean(0).abs()
        assert torch.allclose(overall[r["top_snps"].cpu()], torch.topk(overall, 5).values, rtol=1e-6, atol=1e-12)


def test_saliency_maps_empty_loader_and_bad_label():
    from igcn_amd import _lib
    from igcn_amd.data import DataLoader
    from igcn_amd.train import saliency_maps
    model = _model("sgcn_gcn")
    with pytest.raises(ValueError, match="the loader is empty"):
        saliency_maps(model, [], device="cuda")
    graphs = _graphs(4, seed=6)
    for g_, lab in zip(graphs, (0, 1, 5, 1)):
        g_.y = torch.tensor([lab])
    with pytest.raises(_lib.IgcnError, match="1 of 4 labels lie outside"):
        saliency_maps(model, DataLoader(graphs, batch_size=3), device="cuda")          # lin2: 3 classes
    with pytest.raises(_lib.IgcnError, match="1 of 4 labels lie outside"):
        saliency_maps(model, DataLoader(graphs, batch_size=3), target="label", device="cuda")
    with pytest.raises(ValueError, match="never fills final_conv_acts"):
        saliency_maps(model, DataLoader(graphs, batch_size=3), method="gradcam", device="cuda")
    # three quantities (attr, roi, snps) bump the one state word: the subject is still counted once
    with pytest.raises(_lib.IgcnError, match=r"saliency_maps: 1 of 4 labels lie outside \[0, 3\)"):
        saliency_maps(_model("imgsnp"), DataLoader(graphs, batch_size=3), inputs="both", device="cuda")
