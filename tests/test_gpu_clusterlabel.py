"""GPU checks of SGCN_GCN_CLUSTERLABEL and its launches (csrc/cluster.hip, igcn_mask_reg3_* in csrc/loss.hip):
  * igcn_cluster_head_loss_fwd + igcn_cluster_loss_final against float64 torch over batch sizes, widths, class counts,
    dropout factors and both loss forms; exact zeros without the cluster head; bit-identical repeats; refusals;
  * igcn_mask_reg3_* against float64, and bit for bit against igcn_mask_reg_* when the snps group shares its weights;
  * the model against the fixture captured from the reference (tests/golden/clusterlabel.npz): eval, training mode, one
    train step — through the fused launch and under IGCN_NO_HEAD_LOSS_FUSED=1 — and forward_pair against two forwards;
  * GraphedTrainStep against eager train_step, fit_epoch against the eager loop, eval_acc's pair;
  * dropout on: the step's loss, terms and gradients against the float64 restatement fed the step's own masks by site
    name; fresh masks per replay, nothing left queued after a step, also one that raised half way."""
import copy
import itertools

import numpy as np
import pytest
import torch

import clusterlabel_ref as REF
import dropout_cases as DC
from conftest import assert_matches
from test_gpu_model import grad_floor

pytestmark = pytest.mark.gpu

TAGS = ["h0_1", "h0_3", "nopredict"]
NAMES = ("logp", "logp_cluster", "x_hat", "out_z")
# the bounds tests/test_gpu_model.py holds the headline model's fixtures to: 1e-4 on outputs in eval mode and in training
# mode at B = 32, 1e-3 on eval-mode gradients, 2e-4 on the step's loss and terms.  Training-mode gradients: the reference
# ran in fp32, and its stored GO-network gradients are up to 2.3e-3 (probed groups: 2.7e-3) from the float64 evaluation
# of the same model (tests/test_clusterlabel_reference.py measures both); another fp32 evaluation order cannot be asked
# to sit closer to those numbers than the exact value does: 5e-3, as tests/test_oracle_golden.py's training-mode bound
TOL, GTOL = 1e-4, {"eval": 1e-3, "train": 5e-3}
# One probed group sits on a ReLU decision that fp32 cannot make: in (h0_1, training mode, plain pass) the pre-activation
# of the GO read-out of sample 19, node 67 is 9.0e-7 of its tensor's largest magnitude, and deciding it the other way
# moves d go_network.w_inc.0.weight by 2.53 on a scale of 245 (1.03e-2) and, furthest, d go_network.w_att_s.1.weight by
# 2.3e-2 — tests/test_clusterlabel_reference.py::test_the_read_out_decision_fp32_cannot_make pins these numbers in the
# float64 restatement.  The HIP path decides it unlike the reference's CPU run (its w_inc.0.weight is the fixture's plus
# exactly that shift, to 2e-3 of the shift).  As tests/test_gpu_model.py does for var_multifusion_l3h10, the GO-network
# gradients of that one group are held to the general bound plus the shift; every other tensor and group keeps GTOL.
FLIP_GROUP, FLIP_SLACK = ("h0_1", "train", False), 2.3e-2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _close(got, want, tol, what, floor=0.0):
    assert_matches(got, want.detach().float().cpu().numpy(), tol, what, floor=floor)


# ---- igcn_cluster_head_loss_fwd against float64 torch ----------------------------------------------------------------
def _head_case(b, k, c1, c2, s, keep, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g)                           # noqa: E731
    t = dict(x1=r(2 * b, k).relu(), x2=r(2 * b, k).relu(), w1=r(c1, k) * 0.3, b1=r(c1) * 0.1, w2=r(c2, k) * 0.3,
             b2=r(c2) * 0.1, x_hat=r(2 * b, s), snps=torch.rand(b, s, generator=g), prob=torch.rand(5, generator=g),
             keep1=(torch.rand(2 * b, k, generator=g) > 0.5).float() * 2.0 if keep else None,
             keep2=(torch.rand(2 * b, k, generator=g) > 0.5).float() * 2.0 if keep else None)
    t = {n: (v.cuda() if v is not None else None) for n, v in t.items()}
    t["y"] = torch.randint(0, c1, (b,), generator=g).cuda()
    t["cy"] = torch.randint(0, c2, (b,), generator=g).cuda()
    return t


def _head_launch(t, b, k, c1, c2, s, hp_ce, hp_mi, lam0, predict):
    """The raw entry points: (outputs dict) with wpart reduced by igcn_reduce_rows_final and the value by
    igcn_cluster_loss_final."""
    from igcn_amd import _lib
    from igcn_amd._lib import call, ptr, stream_ptr
    lib = _lib.load()
    nblk = int(lib.igcn_cluster_head_loss_blocks(b, k))
    assert nblk == -(-2 * b // (256 // (k // 4)))
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")           # noqa: E731
    wcols = c1 * k + c1 + c2 * k + c2
    o = dict(logp1=nan(2 * b, c1), logp2=nan(2 * b, c2), dx1=nan(2 * b, k), dx2=nan(2 * b, k), dxhat=nan(2 * b, s),
             parts=nan(nblk, 5), wpart=nan(nblk, wcols), dprob=nan(1))
    call("igcn_cluster_head_loss_fwd", b, k, c1, c2, s, ptr(t["x1"]), ptr(t["keep1"]), ptr(t["w1"]), ptr(t["b1"]),
         ptr(t["x2"]), ptr(t["keep2"]), ptr(t["w2"]), ptr(t["b2"]), ptr(t["y"]), ptr(t["cy"]), ptr(t["x_hat"]),
         ptr(t["snps"]), hp_ce, hp_mi, lam0, int(predict), ptr(o["logp1"]), ptr(o["logp2"]), ptr(o["dx1"]), ptr(o["dx2"]),
         ptr(o["dxhat"]), ptr(o["parts"]), ptr(o["wpart"]), ptr(o["dprob"]), stream_ptr())
    o["dwb"] = nan(wcols)
    call("igcn_reduce_rows_final", ptr(o["wpart"]), nblk, wcols, wcols, ptr(o["dwb"]), stream_ptr())
    wts = torch.tensor([hp_ce, hp_mi, lam0, float(b), float(predict)], device="cuda")
    o["out8"] = nan(8)
    call("igcn_cluster_loss_final", ptr(o["parts"]), nblk, ptr(t["prob"]), t["prob"].numel(), ptr(wts), ptr(o["out8"]),
         stream_ptr())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("k", [4, 64, 256])
@pytest.mark.parametrize("b", [1, 2, 3, 33, 256])
def test_cluster_head_loss_vs_fp64(b, k):
    """Every (C1, C2) in {1..4}^2, S in {1, 54}, dropout factors NULL and given, predict_cluster 0 and 1 at this (B, K):
    outputs and loss terms at 1e-4, gradients at 1e-3 (scale-relative), exact zeros for the cluster head's gradients
    without predict_cluster, and two identical calls bit for bit."""
    hp_ce, hp_mi, lam0 = 1.3, 0.8, 1.5e-3
    n = 0
    for c1 in range(1, 5):
        for c2 in range(1, 5):
            for s, keep, predict in itertools.product((1, 54), (False, True), (False, True)):
                n += 1
                t = _head_case(b, k, c1, c2, s, keep, 1000 * b + 10 * k + 4 * c1 + c2)
                o = _head_launch(t, b, k, c1, c2, s, hp_ce, hp_mi, lam0, predict)
                ref = REF.head_loss(t["x1"], t["keep1"], t["w1"], t["b1"], t["x2"], t["keep2"], t["w2"], t["b2"], t["y"],
                                    t["cy"], t["x_hat"], t["snps"], t["prob"], hp_ce, hp_mi, lam0, predict)
                what = f"(C1={c1} C2={c2} S={s} keep={keep} predict={predict})"
                _close(o["logp1"], ref["logp1"], 1e-4, "logp1 " + what)
                _close(o["logp2"], ref["logp2"], 1e-4, "logp2 " + what)
                got = o["out8"].cpu()
                assert abs(float(got[0]) - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"]))), what
                for j, name in enumerate(REF.TERMS):
                    w = float(ref[name])
                    assert abs(float(got[1 + j]) - w) <= 1e-4 * max(1.0, abs(w)), (name, what)
                assert float(got[7]) == 0.0 and float(o["dprob"]) == 1.0
                o1, o2 = c1 * k + c1, c2 * k + c2
                dwb = o["dwb"]
                _close(o["dx1"], ref["dx1"], 1e-3, "dx1 " + what, floor=1e-6)
                _close(dwb[:c1 * k].view(c1, k), ref["dW1"], 1e-3, "dW1 " + what, floor=1e-6)
                _close(dwb[c1 * k:o1], ref["db1"], 1e-3, "db1 " + what, floor=1e-6)
                _close(o["dxhat"], ref["dxhat"], 1e-3, "dxhat " + what)
                if predict:
                    _close(o["dx2"], ref["dx2"], 1e-3, "dx2 " + what, floor=1e-6)
                    _close(dwb[o1:o1 + c2 * k].view(c2, k), ref["dW2"], 1e-3, "dW2 " + what, floor=1e-6)
                    _close(dwb[o1 + c2 * k:], ref["db2"], 1e-3, "db2 " + what, floor=1e-6)
                else:
                    assert ref["dx2"] is None and ref["dW2"] is None
                    assert bool((o["dx2"] == 0).all()) and bool((dwb[o1:] == 0).all()), what
                    assert bool((o["wpart"][:, o1:] == 0).all()) and o2 == dwb[o1:].numel()
                again = _head_launch(t, b, k, c1, c2, s, hp_ce, hp_mi, lam0, predict)
                for name, v in o.items():
                    assert torch.equal(v, again[name]), (name, what)
    assert n == 128


def test_cluster_head_loss_labels_outside_the_classes_poison_their_term():
    """As igcn_head_loss_fwd: no read out of bounds, the term of the offending label is NaN and the others are not."""
    b, k, c1, c2, s = 5, 64, 3, 2, 54
    t = _head_case(b, k, c1, c2, s, False, 7)
    t["cy"][2] = 2
    o = _head_launch(t, b, k, c1, c2, s, 1.0, 1.0, 1e-5, True)
    got = o["out8"].cpu()
    assert bool(torch.isnan(got[2])) and bool(torch.isnan(got[0])) and bool(torch.isfinite(got[[1, 3, 4, 5, 6]]).all())
    assert bool(torch.isfinite(o["logp2"]).all()) and bool(torch.isfinite(o["dx2"]).all())
    t["cy"][2], t["y"][0] = 0, -1
    got = _head_launch(t, b, k, c1, c2, s, 1.0, 1.0, 1e-5, True)["out8"].cpu()
    assert bool(torch.isnan(got[1])) and bool(torch.isfinite(got[2:7]).all())


@pytest.mark.parametrize("k,c1,c2,why", [(6, 3, 2, "K % 4"), (48, 3, 2, "K / 4 no power of two"), (512, 3, 2, "K > 256"),
                                          (64, 5, 2, "C1 > 4"), (64, 3, 0, "C2 < 1"), (64, 3, 5, "C2 > 4")])
def test_cluster_head_loss_refusals_write_nothing(k, c1, c2, why):
    from igcn_amd import _lib, ops
    from igcn_amd._lib import IgcnError
    b, s = 3, 54
    assert not _lib.load().igcn_cluster_head_loss_supported(k, c1, c2), why
    t = _head_case(b, k, max(c1, 1), max(c2, 1), s, True, 3)
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")           # noqa: E731
    outs = [nan(2 * b, 4), nan(2 * b, 4), nan(2 * b, k), nan(2 * b, k), nan(2 * b, s), nan(64, 5), nan(64, 4096), nan(1)]
    with pytest.raises(IgcnError, match="cluster_head_loss_fwd"):
        _lib.call("igcn_cluster_head_loss_fwd", b, k, c1, c2, s, _lib.ptr(t["x1"]), _lib.ptr(t["keep1"]),
                  _lib.ptr(t["w1"]), _lib.ptr(t["b1"]), _lib.ptr(t["x2"]), _lib.ptr(t["keep2"]), _lib.ptr(t["w2"]),
                  _lib.ptr(t["b2"]), _lib.ptr(t["y"]), _lib.ptr(t["cy"]), _lib.ptr(t["x_hat"]), _lib.ptr(t["snps"]), 1.0,
                  1.0, 1e-5, 1, *[_lib.ptr(v) for v in outs], _lib.stream_ptr())
    torch.cuda.synchronize()
    for v in outs:
        assert bool(torch.isnan(v).all()), why
    if c2 >= 1:                                       # the autograd entry point refuses too, and says so
        f = torch.randn(2 * b, k, device="cuda")
        assert not ops.cluster_head_loss_supported(f, t["w1"], f, t["w2"], None, None)
        with pytest.raises(IgcnError):
            ops.ClusterHeadLoss.apply(f, None, t["w1"], t["b1"], f, None, t["w2"], t["b2"], t["y"], t["cy"], t["x_hat"],
                                      t["snps"], t["prob"], 1.0, 1.0, 1e-5)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("predict", [True, False])
def test_cluster_head_loss_autograd_function(predict, lazy):
    """ops.ClusterHeadLoss: the unit upstream gradient of a train step (``lazy``: the value joins the deferred flush) and
    a general one, against float64."""
    from igcn_amd import ops
    from igcn_amd.train import _unit_grad, stream_pending
    b, k, c1, c2, s = 37, 64, 3, 2, 54
    t = _head_case(b, k, c1, c2, s, True, 11)
    unit = _unit_grad(torch.zeros((), device="cuda"))
    ref = REF.head_loss(t["x1"], t["keep1"], t["w1"], t["b1"], t["x2"], t["keep2"], t["w2"], t["b2"], t["y"], t["cy"],
                        t["x_hat"], t["snps"], t["prob"], 1.3, 0.8, 1.5e-3, predict)
    for upstream in (1.0, 1.7):
        ls = [t[n].clone().requires_grad_(True) for n in ("x1", "w1", "b1", "x2", "w2", "b2", "x_hat", "prob")]
        assert ops.cluster_head_loss_supported(ls[0], ls[1], ls[3], ls[4], t["keep1"], t["keep2"])
        loss, terms, logp1, logp2 = ops.ClusterHeadLoss.apply(ls[0], t["keep1"], ls[1], ls[2], ls[3], t["keep2"], ls[4],
                                                              ls[5], t["y"], t["cy"], ls[6], t["snps"], ls[7], 1.3, 0.8,
                                                              1.5e-3, predict, lazy)
        go = unit if upstream == 1.0 else torch.full((), upstream, device="cuda")
        if lazy:
            with ops.deferred_reductions():
                grads = torch.autograd.grad(loss, ls, grad_outputs=go)
        else:
            grads = torch.autograd.grad(loss, ls, grad_outputs=go)
        torch.cuda.synchronize()
        assert stream_pending() == 0
        assert abs(float(loss) - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"])))
        assert terms.shape == (6,) and not terms.requires_grad and not logp1.requires_grad
        for j, name in enumerate(REF.TERMS):
            assert abs(float(terms[j]) - float(ref[name])) <= 1e-4 * max(1.0, abs(float(ref[name]))), name
        _close(logp1, ref["logp1"], 1e-4, "logp1")
        _close(logp2, ref["logp2"], 1e-4, "logp2")
        for g, name in zip(grads, ("dx1", "dW1", "db1", "dx2", "dW2", "db2", "dxhat", "dprob")):
            if ref[name] is None:
                assert bool((g == 0).all()), name
            else:
                _close(g, ref[name] * upstream, 1e-3, name, floor=1e-6)


# ---- igcn_mask_reg3_* against float64 ------------------------------------------------------------------------------
def _reg_launch(name3, prob, e, snps, hp, partials):
    from igcn_amd import _lib
    from igcn_amd._lib import call, ptr, stream_ptr
    scratch = torch.full((1024,), float("nan"), device="cuda")
    loss = None if partials else torch.full((1,), float("nan"), device="cuda")
    sfx = "3" if name3 else ""
    call(f"igcn_mask_reg{sfx}_fwd", prob.numel(), e.numel(), snps.numel(), ptr(prob), ptr(e), ptr(snps), *hp, ptr(loss),
         ptr(scratch), stream_ptr())
    gout = torch.tensor([1.7], device="cuda")
    dp, de, ds = (torch.full_like(t, float("nan")) for t in (prob, e, snps))
    call(f"igcn_mask_reg{sfx}_bwd", prob.numel(), e.numel(), snps.numel(), ptr(prob), ptr(e), ptr(snps), *hp, ptr(gout),
         ptr(dp), ptr(de), ptr(ds), stream_ptr())
    torch.cuda.synchronize()
    blocks = int(_lib.load().igcn_mask_reg_blocks(prob.numel() + e.numel() + snps.numel()))
    return (scratch[:blocks].clone() if partials else loss), dp, de, ds, scratch


@pytest.mark.parametrize("n_edge", [1, 257, 24300])
@pytest.mark.parametrize("n_prob", [90, 270])
@pytest.mark.parametrize("n_snps", [0, 1, 54])
def test_mask_reg3_vs_fp64(n_snps, n_prob, n_edge):
    """Three independent weight pairs, summed and partials mode, against float64; with the snps group on the x group's
    weights the same bits as igcn_mask_reg_*."""
    g = torch.Generator().manual_seed(n_snps + n_prob + n_edge)
    prob = torch.randn(n_prob, generator=g).cuda()
    e = torch.rand(n_edge, generator=g).clamp(1e-3, 1 - 1e-3).cuda()
    snps = torch.randn(n_snps, generator=g).cuda()
    l1_x, ent_x, l1_e, ent_e, l1_s, ent_s, eps = 0.3, 0.1, 0.2, 0.05, 5.4, 0.7, 1e-6
    want, wp, we, ws = REF.mask_reg3(prob, e, snps, l1_x, ent_x, l1_e, ent_e, l1_s, ent_s, eps)
    hp3 = (l1_x, ent_x, l1_e, ent_e, l1_s, ent_s, eps)
    for partials in (False, True):
        loss, dp, de, ds, scratch = _reg_launch(True, prob, e, snps, hp3, partials)
        if partials:
            assert bool(torch.isnan(scratch[loss.numel():]).all())
        got = float(loss.double().sum())
        assert abs(got - float(want)) <= 1e-4 * max(1.0, abs(float(want))), (got, float(want))
        _close(dp, wp * 1.7, 1e-3, "dprob", floor=1e-7)
        _close(de, we * 1.7, 1e-3, "de", floor=1e-7)
        if n_snps:
            _close(ds, ws * 1.7, 1e-3, "dsnps", floor=1e-7)
        old = _reg_launch(False, prob, e, snps, (l1_x, ent_x, l1_e, ent_e, eps), partials)
        same = _reg_launch(True, prob, e, snps, (l1_x, ent_x, l1_e, ent_e, l1_x, ent_x, eps), partials)
        for a, b_ in zip(old[:4], same[:4]):
            assert torch.equal(a, b_) or (a.numel() == 0 and b_.numel() == 0)


def test_mask_regulariser3_autograd_function():
    from igcn_amd import ops
    g = torch.Generator().manual_seed(5)
    prob, e, snps = (torch.randn(90, 3, generator=g).cuda().requires_grad_(True),
                     torch.rand(700, generator=g).clamp(1e-3, 1 - 1e-3).cuda().requires_grad_(True),
                     torch.randn(1, 54, generator=g).cuda().requires_grad_(True))
    want, wp, we, ws = REF.mask_reg3(prob, e, snps, 0.3, 0.1, 0.1, 0.1, 5.4, 0.1, 1e-6)
    for partials in (False, True):
        out = ops.MaskRegulariser3.apply(prob, e, snps, 0.3, 0.1, 0.1, 0.1, 5.4, 0.1, 1e-6, partials)
        assert abs(float(out.sum()) - float(want)) <= 1e-4 * max(1.0, abs(float(want)))
        gp, ge, gs = torch.autograd.grad(out.sum(), [prob, e, snps])
        _close(gp, wp, 1e-3, "dprob")
        _close(ge, we, 1e-3, "de")
        _close(gs, ws, 1e-3, "dsnps")


# ---- the model against the reference's fixture ----------------------------------------------------------------------
def _model(store, tag, dropout=False):
    from _weights import seeded_state
    from igcn_amd import synth
    from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
    cfg, _, _, graphs = REF.fixture_setup(store, tag)
    go_snps, adj, pool_dim = synth.go_hierarchy(cfg.pool, seed=cfg.seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    model = SGCN_GCN_CLUSTERLABEL(cfg.layers, cfg.hidden, a_g, a, pool_dim, cfg.l_dim, "cuda", H_0=cfg.h0,
                                  num_features=cfg.h0, isCrossAtten=True, isPredictCluster=cfg.predict).cuda()
    assert sorted(model.state_dict()) == store[f"{tag}/state_keys"].tolist()
    model.load_state_dict(seeded_state({k: v.shape for k, v in model.state_dict().items()}, cfg.seed, model.state_dict()))
    model._dropout_enabled = model.go_network._dropout_enabled = dropout
    return model, graphs, cfg


def _batch(graphs):
    from igcn_amd.data import Batch
    return Batch.from_data_list(graphs).to("cuda")


def _probe(outs, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal(tuple(o.shape))).float() for o in outs]


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("explain", [False, True])
def test_model_vs_reference_golden(golden, tag, mode, explain):
    store = golden("clusterlabel")
    model, graphs, cfg = _model(store, tag)
    model.train(mode == "train")
    data = _batch(graphs[mode])
    outs = model(data, None, "cuda", isExplain=explain)
    assert len(outs) == 4 and model.input is data.x
    grp = f"{tag}/{mode}/explain{int(explain)}"
    want = REF.group(store, grp + "/out")
    for n, o in zip(NAMES, outs):
        assert_matches(o, want[n], TOL, n)
    cot = _probe(outs, cfg.seed + 3)
    sum((o * c.cuda()).sum() for o, c in zip(outs, cot)).backward()
    wg = REF.group(store, grp + "/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), GTOL[mode], "grad data.x")
    params = dict(model.named_parameters())
    for k, w in wg.items():
        assert params[k].grad is not None, k
        slack = FLIP_SLACK if (tag, mode, explain) == FLIP_GROUP and k.startswith("go_network.") else 0.0
        assert_matches(params[k].grad, w, GTOL[mode] + slack, "grad " + k, floor=grad_floor(wg, k, 1e-4))
    for k, p in params.items():             # nothing the reference leaves without a gradient gets one here
        if k not in wg and p.grad is not None:
            assert not bool(p.grad.abs().max() > 0), "unexpected grad " + k


def _run_traced(mp, fn):
    """The entry points ``fn()`` calls (tests/calltrace.py); its result is left in ``_run_traced.result``."""
    from calltrace import record_calls
    seen = record_calls(mp)
    _run_traced.result = fn()
    return seen


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("route", ["fused", "unfused", "two_passes"])
def test_train_step_vs_reference_golden(golden, monkeypatch, tag, route):
    """One train() iteration: the fused launch, IGCN_NO_HEAD_LOSS_FUSED=1 (ops.small_linear_pair + log_softmax + nll_loss +
    the torch reconstruction sum on the same batched sweep) and two forward() calls."""
    from igcn_amd.train import FlatAdam, losses
    store = golden("clusterlabel")
    model, graphs, cfg = _model(store, tag)
    model.train(True)
    model.batched_passes = route != "two_passes"
    if route == "unfused":
        monkeypatch.setenv("IGCN_NO_HEAD_LOSS_FUSED", "1")
    data = _batch(graphs["train"])
    opt = FlatAdam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    with monkeypatch.context() as mp:
        seen = [c[0] for c in _run_traced(mp, lambda: losses(model, data, hp=REF.HP))]
    loss, terms, outs = _run_traced.result
    assert (("igcn_cluster_head_loss_fwd" in seen) == (route == "fused")), seen
    assert "igcn_mask_reg3_fwd" in seen and "igcn_mask_reg_fwd" not in seen and "igcn_head_loss_fwd" not in seen
    if route == "fused":                   # both passes as one sweep: one front launch, one heads GEMM launch
        assert seen.count("igcn_mask_reg3_fwd") == 1 and seen.count("igcn_cluster_head_loss_fwd") == 1
    assert sorted(terms) == sorted(REF.TERMS)
    ref = float(store[f"{tag}/step/loss"])
    assert abs(float(loss) - ref) <= 2e-4 * max(1.0, abs(ref)), (float(loss), ref)
    for k, v in terms.items():
        ref = float(store[f"{tag}/step/term/{k}"])
        assert abs(float(v) - ref) <= 2e-4 * max(1.0, abs(ref)), (k, float(v), ref)
    if route != "two_passes":
        want = REF.group(store, f"{tag}/train/explain0/out")
        b = len(graphs["train"])
        for n, o in zip(NAMES, outs):
            assert o.shape[0] == 2 * b
            assert_matches(o[:b], want[n], TOL, n)
    loss.backward()
    params = dict(model.named_parameters())
    wg = REF.group(store, f"{tag}/step/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), GTOL["train"], "grad data.x")
    no_grad = set(store[f"{tag}/step/no_grad"].tolist())
    for k in no_grad:                      # (lin*_cluster without isPredictCluster: None, or the fused launch's zeros)
        g = params[k].grad
        assert g is None or not bool(g.abs().max() > 0), k
    grads = {}
    for k, w in wg.items():
        assert_matches(params[k].grad, w, GTOL["train"], "grad " + k, floor=grad_floor(wg, k, 1e-5))
        grads[k] = w
    opt.step()
    lr = 1e-3
    bufs = model.state_dict()
    for k, w in REF.group(store, f"{tag}/step/buffers_after").items():      # running stats: plain pass, then masked
        assert_matches(bufs[k], w, 1e-3, "buffer " + k, floor=1e-2)
    for k, w in REF.group(store, f"{tag}/step/param_after").items():        # (tests/test_gpu_model.py's Adam check)
        p = params[k].detach().cpu()
        if isinstance(w, tuple) or k not in grads or isinstance(grads[k], tuple):
            assert_matches(p, w, 2.5 * lr, "param " + k, floor=1.0)
            continue
        g = torch.from_numpy(grads[k])
        diff = (p - torch.from_numpy(w)).abs()
        solid = g.abs() > 5e-2 * g.abs().max() if g.abs().max() > 0 else torch.zeros_like(g, dtype=torch.bool)
        sib = grads.get(k[:-5] + ".weight") if k.endswith(".bias") else None
        if sib is not None and not isinstance(sib, tuple) and float(g.abs().max()) < 1e-2 * float(np.abs(sib).max()):
            solid = torch.zeros_like(solid)
        assert float(diff[solid].max() if solid.any() else 0.0) <= 5e-5, "param " + k
        assert float(diff.max()) <= 2.01 * lr, "param (noise-level grads) " + k


@pytest.mark.parametrize("tag", DC.CLUSTER_TAGS)
@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_train_losses_with_dropout_vs_oracle_under_the_steps_own_masks(golden, monkeypatch, tag, route):
    """Dropout ON (the first 8 graphs of the fixture's training batch): the step's one mask launch — 2B rows per site —
    is recorded, equals oracle.dropout.masks(recorded sites, counter) bit for bit, and clusterlabel_ref.train_losses takes
    those factors by site name.  The two head sites, lin1_classify and lin1_cluster, have one shape and one p: only their
    POSITION in the launch tells them apart, and only the values — the loss, the six terms at 1e-4, every gradient at
    1e-3 — tell whether each head got its own.  Negative controls (values only): the oracle under the masks of
    counter + 1, and under the two head masks swapped, is dropout_cases.MARGIN away."""
    from igcn_amd.train import losses
    from oracle import dropout as OD
    from oracle import sgcn_img_snp as OS
    store = golden("clusterlabel")
    model, graphs, cfg = _model(store, tag, dropout=True)
    model.train(True)
    if route == "unfused":
        monkeypatch.setenv("IGCN_NO_HEAD_LOSS_FUSED", "1")
    b = DC.CLUSTER_B
    data = _batch(graphs["train"][:b])
    counter = int(DC.set_counter(model.go_network).state[0].item())
    with monkeypatch.context() as mp:
        drawn = DC.recorded_masks(mp)
        seen = [c[0] for c in _run_traced(mp, lambda: losses(model, data, hp=REF.HP))]
    loss, terms, _ = _run_traced.result
    loss.backward()
    assert (("igcn_cluster_head_loss_fwd" in seen) == (route == "fused")), seen
    assert len(drawn.calls) == 1 and not drawn.calls[0][2]
    sites, arrays = drawn.calls[0][0], drawn.arrays(0)
    assert sites[-2:] == [((2 * b, 64), 0.5), ((2 * b, 64), 0.5)], sites[-2:]
    DC.assert_masks_rebuilt(sites, arrays, counter, f"{tag}/{route}")
    assert int(model.go_network._drop_state.state[0].item()) == counter + 1
    names = OD.go_site_names(2, OD.CLUSTER_HEADS)
    _, idx, sd, _ = REF.fixture_setup(store, tag)

    def oracle(factors, grad):
        with torch.set_grad_enabled(grad):
            st = OS.make_leaf_state(sd, torch.float64)
            dd = DC.cpu_batch(graphs["train"][:b])
            out = REF.train_losses(st, cfg.rois, idx, dd, cfg.lambda0, cfg.predict, dropout=OD.feed_of(sites, factors, names))
        return st, dd, out
    st, dd, (ref_loss, ref_terms, _) = oracle(arrays, True)
    ref_loss.backward()
    ref = float(ref_loss)
    print(f"\n[{tag}/{route}] loss {float(loss):.6f}, oracle {ref:.6f}")
    assert abs(float(loss) - ref) <= DC.LOSS_TOL * max(1.0, abs(ref)), (float(loss), ref)
    assert sorted(terms) == sorted(REF.TERMS)
    for k, v in terms.items():
        r = float(ref_terms[k])
        assert abs(float(v) - r) <= DC.LOSS_TOL * max(1.0, abs(r)), (k, float(v), r)
    params = dict(model.named_parameters())
    wg = {k: v.grad.numpy() for k, v in st.items() if v.requires_grad and v.grad is not None}
    assert_matches(data.x.grad, dd.x.grad.numpy(), 1e-3, "grad data.x")
    for k, w in wg.items():
        g = params[k].grad
        if g is None:                        # (lin*_cluster without isPredictCluster: no gradient here, zeros there)
            assert not np.abs(w).max() > 0, k
            continue
        assert_matches(g, w, 1e-3, "grad " + k, floor=grad_floor(wg, k, 1e-5))
    own = (loss, terms)
    gap_next = DC.gap(own, oracle(OD.masks(sites, counter + 1), False)[2][:2])
    print(f"[control] HIP loss against the oracle under the masks of counter + 1: {gap_next:.5f} (margin {DC.MARGIN})")
    assert gap_next > DC.MARGIN, gap_next
    if cfg.predict:
        swapped = arrays[:-2] + [arrays[-1], arrays[-2]]
        gap_heads = DC.gap(own, oracle(swapped, False)[2][:2], "terms")
        print(f"[control] a term under swapped head masks: {gap_heads:.5f}")
        assert gap_heads > DC.MARGIN, gap_heads


@pytest.mark.parametrize("tag", ["h0_1", "h0_3"])
@pytest.mark.parametrize("training", [False, True])
def test_forward_pair_equals_two_forwards(golden, tag, training):
    store = golden("clusterlabel")
    model, graphs, _ = _model(store, tag)
    model.train(training)
    data = _batch(graphs["train"])
    twin = copy.deepcopy(model)
    with torch.no_grad():
        pair = model.forward_pair(data, None, "cuda")
        single = [twin(data, None, "cuda"), twin(data, None, "cuda", isExplain=True)]
    for p, s in zip(pair, single):
        for n, a, b in zip(NAMES, p, s):
            _close(a, b, 1e-4, n)
    for (k, a), (_, b) in zip(model.state_dict().items(), twin.state_dict().items()):
        if "running_" in k:
            _close(a, b, 1e-5, k, floor=1e-2)


def test_loss_probability_is_recomputed_for_another_batch(golden):
    """The reference's signature and value on its own (no forward before it), and after a forward of ANOTHER batch."""
    store = golden("clusterlabel")
    model, graphs, cfg = _model(store, "h0_3")
    data = _batch(graphs["train"])
    want = float(store["h0_3/step/term/prob"])
    with torch.no_grad():
        got = float(model.loss_probability(data.x, data.edge_index, data.edge_attr, REF.HP))
        model(_batch(graphs["eval"]), None, "cuda", isExplain=True)
        again = float(model.loss_probability(data.x, data.edge_index, data.edge_attr, REF.HP, 1e-6))
    assert abs(got - want) <= 1e-4 * max(1.0, abs(want)) and abs(again - want) <= 1e-4 * max(1.0, abs(want))


# ---- the captured step, the epoch functions -------------------------------------------------------------------------
def _aligned_twin(m1):
    """A deep copy of ``m1`` whose dropout generator continues where ``m1``'s stands."""
    from igcn_amd import ops
    m2 = copy.deepcopy(m1)
    src = getattr(m1.go_network, "_drop_state", None)
    if src is not None:
        st = ops.DropoutState("cuda")
        st.state.copy_(src.state)
        m2.go_network._drop_state = st
    return m2


def _params_close(m1, m2):
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        d = (p1.detach() - p2.detach()).abs()
        # (tests/test_gpu_guide.py: Adam moves an element whose gradient is rounding noise by up to lr per step)
        tol = torch.full_like(d, 2e-4) if p2.grad is None else torch.where(p2.grad.abs() > 1e-6, 2e-4, 3.5e-3)
        assert bool((d <= tol).all()), (k, float(d.max()))


@pytest.mark.parametrize("tag", ["h0_1", "nopredict"])
def test_graphed_step_equals_eager_steps(golden, tag):
    """Three replays on three batches against three eager train_steps (dropout off), at tests/test_gpu_guide.py's bound."""
    from igcn_amd.train import FlatAdam, GraphedTrainStep, train_step
    store = golden("clusterlabel")
    m1, graphs, _ = _model(store, tag)
    graphs = graphs["train"]
    m1.train()
    m2 = copy.deepcopy(m1)
    batches = [_batch(graphs[k::2] * 2) for k in range(2)] + [_batch(graphs[8:] + graphs[:8])]
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    step = GraphedTrainStep(m1, o1, _batch(graphs), warmup=2)
    for b in batches:
        step.load(b)
        l1 = float(step())
        l2 = float(train_step(m2, o2, b))
        assert abs(l1 - l2) <= 1e-4 * max(1.0, abs(l2)), (l1, l2)
    _params_close(m1, m2)


def test_fit_epoch_equals_the_eager_loop_and_eval_acc_pair(golden):
    """3 x 32 + 20 graphs: fit_epoch (every batch shape captured the second time it is met) against train_step by hand
    over two epochs, eval_loss, eval_outputs, and eval_acc's pair against a torch count."""
    from igcn_amd.train import FlatAdam, eval_acc, eval_loss, eval_outputs, fit_epoch, train_step
    store = golden("clusterlabel")
    m1, graphs, _ = _model(store, "h0_1")
    g = graphs["train"]
    m2 = copy.deepcopy(m1)
    loader = [_batch(g), _batch(g[16:] + g[:16]), _batch(g[8:] + g[:8]), _batch(g[:20])]
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    for _ in range(2):
        got = fit_epoch(m1, o1, loader, lambda_loss=2e-5)
        m2.train()
        want = sum(float(train_step(m2, o2, b, lambda_loss=2e-5)) * b.num_graphs for b in loader) / 116
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (got, want)
    tr = next(iter(o1._igcn_epoch_trainers.values()))
    assert tr.counts == {"captured": 2, "replayed": 6, "eager": 2}
    _params_close(m1, m2)
    l1, l2 = eval_loss(m1, loader, 2e-5), eval_loss(m2, loader, 2e-5)
    assert np.isfinite(l1) and abs(l1 - l2) <= 1e-3 * max(1.0, abs(l2))
    acc, acc_c = eval_acc(m1, loader)
    m1.eval()
    hit = hit_c = 0
    with torch.no_grad():
        for b in loader:
            logp, logp_c, _, _ = m1(b, None, "cuda")
            hit += int((logp.argmax(1) == b.y.view(-1)).sum())
            hit_c += int((logp_c.argmax(1) == b.clust_y.view(-1)).sum())
    assert (acc, acc_c) == (hit / 116, hit_c / 116)
    out = eval_outputs(m1, loader)
    assert out["logp"].shape == (116, 3) and out["logp_cluster"].shape == (116, 2) and out["pred_cluster"].shape == (116,)
    assert out["out_lin"].shape == (116, 90 * 32 + 32)


# ---- dropout on ------------------------------------------------------------------------------------------------------
def test_captured_steps_draw_fresh_masks_and_leave_nothing_queued(golden, monkeypatch):
    from igcn_amd import _lib
    from igcn_amd.train import FlatAdam, GraphedTrainStep, assert_nothing_pending, stream_pending, train_step
    store = golden("clusterlabel")
    model, graphs, _ = _model(store, "h0_1", dropout=True)
    model.train()
    data = _batch(graphs["train"])
    opt = FlatAdam(model.parameters(), lr=0.0)            # (the parameters stay: only the masks differ between replays)
    step = GraphedTrainStep(model, opt, data, warmup=2)
    keeps = []
    for _ in range(2):
        step()
        torch.cuda.synchronize()
        keeps.append([m.clone() for m in model.go_network.extra_masks])
        assert stream_pending() == 0
    for a, b in zip(*keeps):
        assert a.shape == (64, 64) and set(a.unique().tolist()) <= {0.0, 2.0}       # both heads: p = 0.5
        assert not torch.equal(a, b)
    assert not torch.equal(keeps[0][0], keeps[0][1])
    monkeypatch.setattr(_lib, "_DEBUG_SYNC", True)         # checked mode: assert_nothing_pending raises on leftovers
    train_step(model, opt, data)
    assert_nothing_pending("after an eager step")
    monkeypatch.setattr(_lib, "_DEBUG_SYNC", False)
    # a step that raises half way: the masks drawn ahead ride in the plan build, which never comes
    seen = {}

    def boom(*a, **k):
        seen["pending"] = int(_lib.load().igcn_stream_pending(_lib.stream_ptr()))
        raise RuntimeError("injected")
    with monkeypatch.context() as mp:
        mp.setattr(step.plan, "rebuild", boom)
        with pytest.raises(RuntimeError, match="injected"):
            step._fwd_bwd()
    assert seen["pending"] >= 1 and stream_pending() == 0
    assert model.go_network._predrawn is None
    # ... and one that dies inside the forward, behind the mask launch
    from igcn_amd import ops
    with monkeypatch.context() as mp:
        mp.setattr(ops, "linear_pair", boom)
        with pytest.raises(RuntimeError, match="injected"):
            train_step(model, opt, data)
    assert stream_pending() == 0
    monkeypatch.setattr(_lib, "_DEBUG_SYNC", True)
    loss = train_step(model, opt, data)
    assert_nothing_pending("after the next step")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
