"""Every form of the dense-block SGCN kernels (csrc/sgcn_dense.hip, ops.DenseSgcn) against the fp64 oracle of
test_gpu_dense.py (``_oracle``: cal_probability, PyG GCNConv, loss_probability), one direct op-level case per mechanism
the entry points dispatch on.  test_gpu_dense.py holds the generic form at R = 64 / 128, H0 = 3, no status words; the
whole-model tests reach R = 512 only behind the GO network, heads and losses.

Forms (``FORMS``; the comment at each case names what it is the smallest instance of):
  * pipelined walks (R = 256: every wave's walk is ONE chunk pair, only the peeled tail of ``ds_walk`` runs; R = 512: one
    trip of the steady-state loop in k_ds_deg and k_ds_mask_bwd, the benchmark's kernels), with the LDS-staged k_ds_aggT;
  * mixed (R = 768, 1024: k_ds_mask_bwd<L, true> beside the generic k_ds_deg / k_ds_agg / k_ds_aggT);
  * uneven wave ranges of k_ds_mask_bwd (R = 192: 1, 2, 1, 2 ... 16-source blocks per wave; R = 320: 2, 3, 2, 3 ...);
  * the XCD remap of ``ds_block`` / ``ds_block_of`` on (grids of 8 and 24 workgroups; with R / 64 = 3 an XCD's run of ids
    straddles graph boundaries) and off (grids of 12, 5, 4);
  * the limits of the ABI: L = 4, H0 = 1, H0 = 8, R = 1024.
ABI corners: the structure check riding in k_ds_deg's launch, the dual output, the refusals, run-to-run determinism.
Edge values: a target without incoming weight (deg = 0), saturated masks (logits to +-30), and the inf * 0 corner of
``ds_mask`` (u <= -89 against v >= 104), which is a NaN loss: the documented domain is |u|, |v| <~ 87.
The pipelined form is also held to the general kernels of csrc/sgcn.hip through the model's switch.

Bounds: the ceilings of test_gpu_dense.py — xcat 1e-4, loss 1e-5 relative, gradients 1e-3 with floor 1e-6 (the 1e-3
is there for the regulariser's eps approximation, comment at ds_reg_term_logit).  With ``reg_w = 0`` the regulariser
contributes nothing to the gradients and the pipelined / odd-R/64 forms are held to ``NOREG_BOUND``, which comes from the
GENERIC form's own error (see there), not from the cases it is applied to.

Measured on the MI355X (scale-relative, as conftest.assert_matches; the DENSE_FORMS lines every case prints are in
docs/LABLOG.md §F).  Per-tensor maximum over all cases of ``FORMS`` and ``NOREG``:
  xcat 4.33e-7   loss 1.47e-7   dx 6.30e-7   prob 6.34e-7   prob_bias 2.83e-7   snps_prob 3.34e-7
  conv1.lin.weight 2.42e-7   conv1.bias 1.68e-7   convs.0.lin.weight 2.98e-7   convs.0.bias 1.67e-7
  convs.1.lin.weight 1.76e-7   convs.1.bias 2.02e-7   convs.2.lin.weight 1.38e-7   convs.2.bias 1.66e-7
(most of them at (1024, 1, L = 4, H0 = 8); the reg_w = 0 cases: at most 2.36e-7 against NOREG_BOUND = 1.64e-6).  The
edge-value cases: at most 8.18e-7 (prob, saturated masks at R = 256); zero degree and the dual output at most 4.25e-7.
No case needed imposed ReLU decisions (conftest.relu_forced): no near-zero pre-activation moved a gradient."""
import copy

import numpy as np
import pytest
import torch

from conftest import assert_matches
from test_gpu_dense import HP, _batch, _oracle

pytestmark = pytest.mark.gpu

F = 16
REG_W = 0.37
REG_HP = (HP.lamda_x_l1, HP.lamda_x_ent, HP.lamda_e_l1, HP.lamda_e_ent, 1e-6)
GRADS = ("prob", "prob_bias", "snps_prob")

# (rois, n_graphs, layers, h0, mode)
FORMS = [
    # pipelined, tail only (rows per wave = 32 = one chunk pair: the loop of ds_walk runs zero times), grid 8: remap on,
    # every pass combination of the three template instances (NC, M0)
    (256, 2, 2, 3, "plain"),
    (256, 2, 2, 3, "masked"),
    (256, 2, 2, 3, "both"),
    # pipelined, grid 12: remap off; k_ds_mask_bwd<1, true>
    (256, 3, 1, 3, "both"),
    # pipelined with one trip of the steady-state loop (k_ds_deg: 64 rows per wave; k_ds_mask_bwd: 4 blocks per wave) and
    # k_ds_agg's 8-step chunks: the benchmark's kernels (configs[4]), grid 8
    (512, 1, 2, 3, "both"),
    # grid 24 from a graph count that is no power of two, L = 3 pipelined, single masked pass (NC = 1, M0)
    (512, 3, 3, 3, "masked"),
    # odd R / 64 = 3: grid 24 with the remap on, an XCD's run of 3 ids straddles graph boundaries; k_ds_mask_bwd's wave
    # ranges are 1, 2, 1, 2, ... blocks of 16 sources; dup holds 12 rows
    (192, 8, 2, 3, "both"),
    # wave ranges of 2, 3, 2, 3, ... blocks; grid 5
    (320, 1, 2, 3, "masked"),
    # remap on at one block per graph (grid 8), four of eight waves of k_ds_mask_bwd idle
    (64, 8, 2, 3, "both"),
    # mixed: pipelined k_ds_mask_bwd (R % 256 == 0, three chunk pairs per wave) beside generic k_ds_deg / k_ds_agg / k_ds_aggT
    (768, 1, 2, 3, "both"),
    # the upper limit of R, L and H0 together: mixed form, grid 16 (remap on), K = 64 and bop[4][4][4] in k_ds_mask_bwd<4, true>
    (1024, 1, 4, 8, "both"),
    # L = 4 on the generic k_ds_mask_bwd<4, false>, H0 = 1
    (128, 2, 4, 1, "masked"),
    # H0 = 8 generic (k_ds_prep / k_ds_h0 / k_ds_node_mid at fin = 8, k_ds_mask_nodes' 16 partial columns)
    (128, 2, 2, 8, "both"),
]
# mode "both" without the regulariser's gradient: pipelined tail-only, pipelined with a loop trip, odd R / 64
NOREG = [(256, 2, 2), (512, 1, 2), (192, 8, 2)]

# The largest scale-relative gradient error of the GENERIC form against the fp64 oracle with reg_w = 0, measured on the
# parent commit's library at test_gpu_dense.py's cases (64, 3, 2) and (128, 2, 3), all three modes, over dx and every
# parameter gradient (floor 1e-6): 4.11e-7, dx of (64, 3, 2) 'both' (docs/LABLOG.md §F).  Times 4 for seed and shape variation of
# fp32 rounding, capped at the suite's 1e-3.
PARENT_NOREG_ERR = 4.11e-7
NOREG_BOUND = min(4 * PARENT_NOREG_ERR, 1e-3)

_ORACLE = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _inputs(rois, n_graphs, layers, h0):
    """The construction of test_dense_sgcn_vs_fp64_oracle: (batch on the host, state dict, cotangent of a 'both' run)."""
    rng = np.random.default_rng(rois + layers)
    b = _batch(n_graphs, rois, seed=rois)
    if h0 != 3:                                       # synth.brain_batch makes 3 features per node
        b.x = torch.from_numpy(np.random.default_rng(7 * rois + h0).random((n_graphs * rois, h0))).float()
    t = lambda *s: torch.from_numpy(rng.standard_normal(s)).float()                        # noqa: E731
    sd = {"prob": t(rois, h0) * 0.7, "prob_bias": t(2 * h0, 1) * 0.8, "snps_prob": t(1, 54),
          "conv1.lin.weight": t(F, h0) * 0.6, "conv1.bias": t(F) * 0.2}
    for l in range(1, layers):
        sd[f"convs.{l - 1}.lin.weight"] = t(F, F) * 0.4
        sd[f"convs.{l - 1}.bias"] = t(F) * 0.2
    return b, sd, t(2 * n_graphs * rois, layers * F)


def _wb(dev, layers):
    out = []
    for l in range(layers):
        out += [dev["conv1.lin.weight"], dev["conv1.bias"]] if l == 0 else [dev[f"convs.{l - 1}.lin.weight"],
                                                                            dev[f"convs.{l - 1}.bias"]]
    return out


def _leaves(b, sd):
    """(device batch, leaf copy of x, leaf copies of the parameters); ``b`` itself stays on the host."""
    bd = copy.copy(b).to("cuda")
    return bd, bd.x.clone().requires_grad_(True), {k: v.cuda().requires_grad_(True) for k, v in sd.items()}


def _apply(ops, bd, xg, dev, layers, mode, rois, status=None):
    return ops.DenseSgcn.apply(xg, bd.edge_attr, dev["prob"], dev["prob_bias"], dev["snps_prob"], mode, rois, REG_HP,
                               status, *_wb(dev, layers))


def _grads(total, xg, dev):
    """{name: gradient or None} of ``total`` for x and every parameter."""
    names = ["x"] + list(dev)
    return dict(zip(names, torch.autograd.grad(total, [xg] + list(dev.values()), allow_unused=True)))


def _run(ops, b, sd, cot, layers, mode, rois, reg_w, status=None):
    """One forward + backward of sum(xcat * cot) + reg_w * sum(regp): (xcat, regp, gradients)."""
    bd, xg, dev = _leaves(b, sd)
    xcat, regp = _apply(ops, bd, xg, dev, layers, mode, rois, status)
    total = (xcat * cot.cuda()).sum()
    if mode != "plain":
        total = total + reg_w * regp.sum()
    return xcat, regp, _grads(total, xg, dev)


def _rel(got, want, floor=0.0):
    w = want.double()
    scale = max(float(w.abs().max()), floor, 1e-30)
    return float((got.detach().cpu().double() - w).abs().max()) / scale


def _against_oracle(ops, key, b, sd, cot, layers, mode, rois, h0, reg_w, got=None):
    """Run the op (or take ``got``), compare with the fp64 oracle at the suite's ceilings, print the DENSE_FORMS line;
    -> ({tensor: relative error}, (xcat, regp, gradients)).  The oracle of a case is computed once and left unchanged."""
    n_graphs = b.x.shape[0] // rois
    if key not in _ORACLE:
        _ORACLE[key] = _oracle(b, sd, layers, mode, cot, reg_w)
    want_xcat, want_reg, want_dx, want = _ORACLE[key]
    plan = ops.plan_for(copy.copy(b).to("cuda"))
    assert plan.dense_blocks and ops.dense_sgcn_supported(plan, rois, h0, F, layers)
    xcat, regp, grads = got if got is not None else _run(ops, b, sd, cot, layers, mode, rois, reg_w)
    errs = {"xcat": _rel(xcat, want_xcat)}
    if mode != "plain":
        errs["loss"] = abs(float(regp.detach().sum()) - float(want_reg)) / abs(float(want_reg))
    errs["dx"] = _rel(grads["x"], want_dx)
    for k, g in want.items():
        if mode == "plain" and k in GRADS:
            assert grads[k] is None
        else:
            errs["grad " + k] = _rel(grads[k], g, 1e-6)
    print(f"\nDENSE_FORMS [{key} R={rois} G={n_graphs} L={layers} H0={h0} {mode} reg_w={reg_w}] rel err "
          + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert_matches(xcat, want_xcat.numpy(), 1e-4, "xcat")
    if mode != "plain":
        assert errs["loss"] <= 1e-5, errs["loss"]
    else:
        assert regp.numel() == 0
    assert_matches(grads["x"], want_dx.numpy(), 1e-3, "dx")
    for k, g in want.items():
        if grads[k] is not None:
            assert_matches(grads[k], g.numpy(), 1e-3, "grad " + k, floor=1e-6)
    return errs, (xcat, regp, grads)


@pytest.fixture(scope="module")
def ops():
    from igcn_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------- 1. form coverage
@pytest.mark.parametrize("rois,n_graphs,layers,h0,mode", FORMS)
def test_dense_forms_vs_fp64_oracle(ops, rois, n_graphs, layers, h0, mode):
    b, sd, cot = _inputs(rois, n_graphs, layers, h0)
    if mode != "both":
        cot = cot[:n_graphs * rois]
    _against_oracle(ops, ("form", rois, n_graphs, layers, h0, mode), b, sd, cot, layers, mode, rois, h0, REG_W)


@pytest.mark.parametrize("rois,n_graphs,layers", NOREG)
def test_pipelined_and_odd_forms_without_the_regulariser_gradient(ops, rois, n_graphs, layers):
    """reg_w = 0: every gradient is the message passing's alone, so the regulariser's eps approximation (the reason for
    the 1e-3 ceiling) is out of the picture and the forms are held to the generic form's own error."""
    b, sd, cot = _inputs(rois, n_graphs, layers, 3)
    errs, _ = _against_oracle(ops, ("noreg", rois, n_graphs, layers), b, sd, cot, layers, "both", rois, 3, 0.0)
    worst = max((v, k) for k, v in errs.items() if k == "dx" or k.startswith("grad "))
    # parent, generic form: 4.11e-7 (PARENT_NOREG_ERR); bound = min(4 * 4.11e-7, 1e-3) = 1.644e-6 (NOREG_BOUND)
    assert worst[0] <= NOREG_BOUND, (worst, NOREG_BOUND)


# ------------------------------------------------------------------------------------------------- 4. forms agree
def test_pipelined_form_matches_the_general_kernels_through_the_model(ops, monkeypatch):
    """R = 256 (pipelined, tail only), 2 graphs, 2 layers: the model's train losses on the dense-block path against the
    general kernels of csrc/sgcn.hip (IGCN_NO_DENSE_BLOCKS: sorted plan, record streams) on the same weights — xcat of
    both passes, every loss term and every gradient at the 2e-4 / 2e-5 of test_model_takes_the_dense_path…: a second,
    independent implementation at an R nothing else runs."""
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    from igcn_amd.train import losses
    from _weights import seeded_state
    from calltrace import record_calls
    rois = 256
    go_snps, adj, pool_dim = synth.go_hierarchy((40, 20, 10, 4, 1), seed=3)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    model = SGCN_GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=rois, H_0=3, num_classes=3, isSoftSimilarity=True,
                            rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseProb4Regr=True, isImageOnly=False,
                            isSNPsOnly=False).cuda().train()
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, 7)
    for m in (model, model.go_network):
        m._dropout_enabled = False
    graphs = synth.brain_graph_list(2, seed=4, rois=rois, tsne_dim=8, dense=True)
    lam = [1.0, 1.0, 0.5, 1.5e-6, 0.1, 0.2]
    seen = record_calls(monkeypatch)
    xcats = []
    dense_route, stack = model._dense_route, model._stack
    monkeypatch.setattr(model, "_dense_route", lambda *a, **k: (lambda r: (xcats.append(r.xcat.detach().clone()), r)[1])(
        dense_route(*a, **k)))
    monkeypatch.setattr(model, "_stack", lambda *a, **k: (lambda r: (xcats.append(r[0].detach().clone()), r)[1])(
        stack(*a, **k)))
    res, calls = {}, {}
    for tag in ("dense", "general"):
        if tag == "general":
            monkeypatch.setenv("IGCN_NO_DENSE_BLOCKS", "1")
        seen.clear()
        model.load_state_dict(sd)
        model.zero_grad()
        model.batched_passes = True
        data = Batch.from_data_list(graphs).to("cuda")
        assert ops.plan_for(data).dense_blocks == (tag == "dense")
        loss, terms, _ = losses(model, data, lam)
        loss.backward()
        res[tag] = (float(loss), {k: float(v) for k, v in terms.items()}, data.x.grad.clone(),
                    {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        calls[tag] = [c[0] for c in seen]
    assert "igcn_dense_sgcn_fwd" in calls["dense"] and "igcn_dense_sgcn_bwd" in calls["dense"]
    assert not [c for c in calls["general"] if c.startswith("igcn_dense_sgcn")]
    assert len(xcats) == 2 and xcats[0].shape == xcats[1].shape == (2 * 2 * rois, 2 * F)
    assert_matches(xcats[0], xcats[1].cpu().numpy(), 2e-4, "xcat")
    (ld, td, gxd, gd), (lg, tg, gxg, gg) = res["dense"], res["general"]
    assert abs(ld - lg) <= 2e-5 * max(1.0, abs(lg)), (ld, lg)
    for k in tg:
        assert abs(td[k] - tg[k]) <= 2e-5 * max(1.0, abs(tg[k])), (k, td[k], tg[k])
    assert_matches(gxd, gxg.cpu().numpy(), 2e-4, "data.x.grad")
    assert set(gd) == set(gg)
    for k in gg:
        assert_matches(gd[k], gg[k].cpu().numpy(), 2e-4, "grad " + k, floor=1e-6)


# ------------------------------------------------------------------------------------------------- 5. ABI corners
def _same_bits(a, b, what):
    xa, ra, ga = a
    xb, rb, gb = b
    assert torch.equal(xa, xb), what + ": xcat"
    assert torch.equal(ra, rb), what + ": regp"
    assert set(ga) == set(gb)
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None) and (ga[k] is None or torch.equal(ga[k], gb[k])), f"{what}: grad {k}"
        assert ga[k] is None or bool(torch.isfinite(ga[k]).all()), f"{what}: grad {k} is not finite"


def test_riding_structure_check_changes_no_bit_and_poisons_a_malformed_batch(ops, monkeypatch):
    """R = 256, mode 'both': ``status=GraphPlan`` with a pending check adds workgroups to k_ds_deg's launch (the index
    pairs stream beside the weights; ds_block_of then maps ids on the DEGREE blocks alone).  Same bits as ``status=None``;
    the plan's check passes; two swapped edges turn xcat into NaN and the plan's check reports them."""
    from calltrace import record_calls
    from igcn_amd import _lib
    rois, n_graphs, layers = 256, 2, 2
    b, sd, cot = _inputs(rois, n_graphs, layers, 3)
    bd = copy.copy(b).to("cuda")
    plan = ops.plan_for(bd)
    assert plan.dense_blocks
    seen = record_calls(monkeypatch)
    plain = _run(ops, b, sd, cot, layers, "both", rois, REG_W, status=None)
    plan.rebuild(bd.edge_index)                                     # what every step does: the check is now pending
    riding = _run(ops, b, sd, cot, layers, "both", rois, REG_W, status=plan)
    fwd = [c for c in seen if c[0] == "igcn_dense_sgcn_fwd"]
    assert len(fwd) == 2 and fwd[0][-2] is None and fwd[1][-2] == "*", "the check did not ride in the second forward"
    assert plan.take_pending_check() is None                       # consumed by that forward
    _same_bits(plain, riding, "riding check")
    plan.check()
    bad = bd.edge_index.clone()
    k = rois * rois + 7                                            # two edges of graph 1 swapped
    bad[:, [k, k + 1]] = bad[:, [k + 1, k]]
    plan.rebuild(bad)
    xcat, regp, _ = _run(ops, b, sd, cot, layers, "both", rois, REG_W, status=plan)
    assert bool(torch.isnan(xcat).all())
    with pytest.raises(_lib.IgcnError, match="complete graphs"):
        plan.check()


def test_dual_output_sums_the_two_handles_gradients(ops):
    """``rois = -256``: two autograd handles of one xcat; their cotangents meet in k_ds_node_top / k_ds_node_mid
    (dxcat + dxcat2).  Equal to a single-handle run fed the fp32 sum, bit for bit, and to the fp64 oracle; a handle that
    nobody reads equals explicit zeros, bit for bit."""
    rois, n_graphs, layers = 256, 2, 2
    b, sd, cot = _inputs(rois, n_graphs, layers, 3)
    c1 = cot.cuda()
    c2 = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(cot.shape))).float().cuda()

    def dual(weigh):
        bd, xg, dev = _leaves(b, sd)
        xcat, regp, xcat2 = _apply(ops, bd, xg, dev, layers, "both", -rois)
        assert xcat2.data_ptr() == xcat.data_ptr()
        return xcat, regp, _grads(weigh(xcat, xcat2) + REG_W * regp.sum(), xg, dev)

    both = dual(lambda a, b2: (a * c1).sum() + (b2 * c2).sum())
    single = _run(ops, b, sd, (c1 + c2).cpu(), layers, "both", rois, REG_W)
    _same_bits(both, single, "dual vs the sum")
    _against_oracle(ops, ("dual", rois), b, sd, (c1 + c2).cpu(), layers, "both", rois, 3, REG_W, got=both)
    zeros = torch.zeros_like(c1)
    _same_bits(dual(lambda a, b2: (a * c1).sum()), dual(lambda a, b2: (a * c1).sum() + (b2 * zeros).sum()),
               "second handle unused")
    _same_bits(dual(lambda a, b2: (b2 * c2).sum()), dual(lambda a, b2: (a * zeros).sum() + (b2 * c2).sum()),
               "first handle unused")


@pytest.mark.parametrize("rois,layers,h0", [(1088, 2, 3), (96, 2, 3), (64, 5, 3), (64, 2, 9)])
def test_unsupported_sizes_are_refused_by_the_entry_point(ops, monkeypatch, rois, layers, h0):
    from calltrace import record_calls
    from igcn_amd._lib import IgcnError
    assert not ops._lib.load().igcn_dense_sgcn_supported(rois, h0, F, layers)
    z = lambda *s: torch.zeros(*s, device="cuda")                                            # noqa: E731
    wb = [z(F, h0), z(F)] + [t for _ in range(layers - 1) for t in (z(F, F), z(F))]
    seen = record_calls(monkeypatch)
    with pytest.raises(IgcnError, match=rf"dense_sgcn_fwd: needs 64 <= R <= 1024, R % 64 == 0, F == 16, L <= 4, H0 <= 8 "
                                        rf"\(R={rois}, H0={h0}, F=16, L={layers}\)"):
        ops.DenseSgcn.apply(z(rois, h0), z(rois * rois), z(rois, h0), z(2 * h0, 1), z(1, 54), "both", rois, REG_HP, None, *wb)
    assert [c[0] for c in seen] == ["igcn_dense_sgcn_fwd"]


def test_pipelined_form_is_deterministic(ops):
    """(256, 2, 2) 'both' twice: workgroup partials summed in a fixed order, no atomics."""
    b, sd, cot = _inputs(256, 2, 2, 3)
    _same_bits(_run(ops, b, sd, cot, 2, "both", 256, REG_W), _run(ops, b, sd, cot, 2, "both", 256, REG_W), "second run")


# ------------------------------------------------------------------------------------------------- 6. edge values
def _logit_parts(b, sd, rois):
    """fp64 (u, v) [G, R]: the logit of edge (s, d) of a graph is u[s] + v[d] (cal_probability)."""
    h0 = b.x.shape[1]
    xm = b.x.double().view(-1, rois, h0) * sd["prob"].double()
    pb = sd["prob_bias"].double().view(-1)
    return xm @ pb[:h0], xm @ pb[h0:]


@pytest.mark.parametrize("rois", [64, 256])
def test_zero_in_degree_gives_relu_bias_and_finite_gradients(ops, rois):
    """A target whose incoming weights are all zero (its self loop included: a stored loop keeps its weight) has
    deg = 0 in both passes: k_ds_deg's ``deg > 0 ? deg^-1/2 : 0`` branch, gcn_norm's inf -> 0.  Its rows of xcat are
    relu(bias) exactly.  A source row of zeros in another graph."""
    n_graphs, layers, tgt, src = 2, 2, 5, rois - 3
    b, sd, cot = _inputs(rois, n_graphs, layers, 3)
    ew = b.edge_attr.clone().view(n_graphs, rois, rois)               # [graph][source][target]
    ew[0, :, tgt] = 0.0
    ew[1, src, :] = 0.0
    b.edge_attr = ew.reshape(-1)
    _, (xcat, regp, grads) = _against_oracle(ops, ("zero_degree", rois), b, sd, cot, layers, "both", rois, 3, REG_W)
    assert bool(torch.isfinite(xcat).all()) and bool(torch.isfinite(regp).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    for row in (tgt, n_graphs * rois + tgt):                          # the plain and the masked copy
        for l, name in enumerate(["conv1.bias", "convs.0.bias"]):
            assert torch.equal(xcat[row, l * F:(l + 1) * F].cpu(), torch.relu(sd[name])), (row, name)


@pytest.mark.parametrize("rois", [64, 256])
def test_saturated_masks_stay_finite_and_match_the_oracle(ops, rois):
    """prob_bias scaled until the logits u[s] + v[d] span about +-30 with |u|, |v| <= 40: e rounds to exactly 1 or lies
    below 1e-12 on many edges (the clamps of ds_reg_term_logit and ds_logit_part, e (1 - e) = 0 in the mask gradient)."""
    n_graphs, layers = 2, 2
    b, sd, cot = _inputs(rois, n_graphs, layers, 3)
    u, v = _logit_parts(b, sd, rois)
    hi = max(float((u.max(1).values + v.max(1).values).max()), -float((u.min(1).values + v.min(1).values).min()))
    sd["prob_bias"] = sd["prob_bias"] * (30.0 / hi)
    u, v = _logit_parts(b, sd, rois)
    top, low = float((u.max(1).values + v.max(1).values).max()), float((u.min(1).values + v.min(1).values).min())
    z = u[:, :, None] + v[:, None, :]
    one, tiny = float((z >= 17.0).double().mean()), float((z <= -27.7).double().mean())   # fp32 e == 1 / e < 1e-12
    print(f"\nDENSE_FORMS saturated R={rois}: logits [{low:.1f}, {top:.1f}], max |u| {float(u.abs().max()):.1f} "
          f"max |v| {float(v.abs().max()):.1f}, e == 1 on {one:.3f} of the edges, e < 1e-12 on {tiny:.4f}")
    assert 29.9 <= max(top, -low) <= 30.1 and min(top, -low) >= 15.0
    assert float(u.abs().max()) <= 40.0 and float(v.abs().max()) <= 40.0
    assert one > 0.0
    _, (xcat, regp, grads) = _against_oracle(ops, ("saturated", rois), b, sd, cot, layers, "both", rois, 3, REG_W)
    assert bool(torch.isfinite(xcat).all()) and bool(torch.isfinite(regp).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())


@pytest.mark.parametrize("rois", [64, 256])
def test_inf_times_zero_corner_is_a_nan_loss(ops, rois):
    """Outside the documented domain (|u|, |v| <~ 87): one node's features scaled until u[s] <= -89, so
    its factor exp(-u) overflows to inf, another's until v[d] >= 104, so its factor exp(-v) is 0.  On the edge (s, d)
    ds_mask is 1 / (inf * 0 + 1) = NaN where sigmoid(u + v) is finite (the oracle's value).  Loud, not silent: the
    regulariser — hence the loss — is NaN, and so is the target's row of the masked pass; the plain pass is untouched."""
    n_graphs, layers = 2, 2
    b, sd, cot = _inputs(rois, n_graphs, layers, 3)
    u, v = _logit_parts(b, sd, rois)
    s = int(u[0].argmin())
    others = v[0].clone()
    others[s] = -float("inf")
    d = int(others.argmax())
    assert float(u[0, s]) < 0 < float(v[0, d]) and s != d
    x = b.x.clone()
    x[s] *= 95.0 / -float(u[0, s])
    x[d] *= 110.0 / float(v[0, d])
    b.x = x
    u, v = _logit_parts(b, sd, rois)
    assert float(u[0, s]) <= -89.0 and float(v[0, d]) >= 104.0
    assert bool(torch.isfinite(torch.sigmoid(u[0, s] + v[0, d])))          # the reference's mask of that edge
    bd, xg, dev = _leaves(b, sd)
    xcat, regp = _apply(ops, bd, xg, dev, layers, "both", rois)
    n = n_graphs * rois
    assert bool(torch.isnan(regp.sum()))
    assert bool(torch.isnan(xcat[n + d]).any())
    assert bool(torch.isfinite(xcat[:n]).all())
