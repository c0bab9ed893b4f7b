"""GPU checks of the genetics-only trainer (igcn_amd/snps.py) and its launches (csrc/snps_head.hip):
  * igcn_snps_head_loss_fwd / _bwd against the float64 restatement tests/snps_ref.py over the batch sizes and widths at
    which the kernel can go wrong, with and without dropout factors, both modes, two upstream gradients; a constant
    column, soft labels, lambda0 = 0, saturated sigmoids against torch's fp32 BCELoss; the running statistics;
  * refusals write nothing; one sample in training mode raises;
  * the model against the fixture captured from the reference (tests/golden/snps_only.npz): both modes, the fused launch
    and IGCN_NO_HEAD_LOSS_FUSED=1, one train step's Adam update;
  * GraphedSnpsStep against eager train_step_snps, fit_epoch_snps against the eager loop (ragged tail), the evaluation
    functions against the host metrics;
  * dropout on: the head's two sites ride in the GO network's one mask launch, and the step matches the float64
    restatement fed the step's own masks."""
import copy

import numpy as np
import pytest
import torch

import dropout_cases as DC
import snps_ref as REF
from clusterlabel_ref import group
from conftest import assert_matches
from test_gpu_model import grad_floor

pytestmark = pytest.mark.gpu

TAGS = list(REF.CONFIGS)
# the bounds tests/test_gpu_clusterlabel.py holds its model to
TOL, GTOL, STEP_TOL = 1e-4, {"eval": 1e-3, "train": 5e-3}, 2e-4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _close(got, want, tol, what, floor=0.0):
    assert_matches(got, want.detach().float().cpu().numpy(), tol, what, floor=floor)


# ---- the launches against float64 ------------------------------------------------------------------------------------
OUT_NAMES = ("y_hat", "out", "dlatent", "dxhat", "dgamma", "dbeta", "dW1", "dW2", "db2", "running_mean", "running_var")


def _launch(c, training, lambda0=REF.LAMBDA0, upstream=None, backward=True):
    """The raw entry points on a ``snps_ref.head_case`` dict (moved to the device); every output starts as NaN."""
    from igcn_amd import _lib
    from igcn_amd._lib import call, ptr, stream_ptr
    t = {k: (v.cuda() if v is not None else None) for k, v in c.items()}
    b, l = t["latent"].shape
    s, h = t["snps"].shape[1], t["w1"].shape[0]
    k1 = l + s
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")           # noqa: E731
    ws_bytes = int(_lib.load().igcn_snps_head_workspace_bytes(b, l, s, h))
    assert ws_bytes >= 4 * (2 * k1 + b * h)
    o = dict(y_hat=nan(b), out=nan(3), ws=nan((ws_bytes + 3) // 4), dlatent=nan(b, l), dxhat=nan(b, s), dgamma=nan(k1),
             dbeta=nan(k1), dW1=nan(h, k1), dW2=nan(1, h), db2=nan(1), running_mean=t["running_mean"].clone(),
             running_var=t["running_var"].clone())
    call("igcn_snps_head_loss_fwd", b, l, s, h, ptr(t["latent"]), ptr(t["snps"]), ptr(t["gamma"]), ptr(t["beta"]),
         ptr(o["running_mean"]), ptr(o["running_var"]), 0.1, 1e-5, int(training), ptr(t["keep1"]), ptr(t["keep2"]),
         ptr(t["w1"]), ptr(t["w2"]), ptr(t["b2"]), ptr(t["label"]), ptr(t["x_hat"]), lambda0, ptr(o["y_hat"]), ptr(o["out"]),
         ptr(o["ws"]), stream_ptr())
    if backward:
        up = None if upstream is None else torch.tensor([upstream], device="cuda")
        call("igcn_snps_head_loss_bwd", b, l, s, h, int(training), ptr(t["latent"]), ptr(t["snps"]), ptr(t["gamma"]),
             ptr(t["beta"]), ptr(t["keep1"]), ptr(t["keep2"]), ptr(t["w1"]), ptr(t["w2"]), ptr(t["label"]), ptr(o["y_hat"]),
             ptr(t["x_hat"]), lambda0, ptr(up), ptr(o["ws"]), ptr(o["dlatent"]), ptr(o["dxhat"]), ptr(o["dgamma"]),
             ptr(o["dbeta"]), ptr(o["dW1"]), ptr(o["dW2"]), ptr(o["db2"]), stream_ptr())
    torch.cuda.synchronize()
    return o


def _check_case(name, c, training, lambda0=1.5e-3):
    """y_hat, the loss and each term at 1e-4, the gradients at 1e-3 (scale-relative, test_cluster_head_loss_vs_fp64's
    floors), the running statistics at 1e-5, for the upstream gradients 1 (NULL) and 1.7; two calls agree bit for bit."""
    for upstream in (None, 1.7):
        o = _launch(c, training, lambda0, upstream)
        ref = REF.head_loss_of(c, training, lambda0=lambda0, upstream=1.0 if upstream is None else upstream)
        what = f"{name} upstream={upstream}"
        _close(o["y_hat"], ref["y_hat"], 1e-4, "y_hat " + what)
        got = o["out"].cpu()
        for j, k in enumerate(("loss", "class", "recon")):
            w = float(ref[k])
            print(f"[{what}] {k}: {float(got[j]):.7g} vs {w:.7g}")
            assert abs(float(got[j]) - w) <= 1e-4 * max(1.0, abs(w)), (k, what)
        for k in ("dlatent", "dxhat", "dgamma", "dbeta", "dW1", "dW2", "db2"):
            assert bool(torch.isfinite(o[k]).all()), (k, what)
            _close(o[k], ref[k].reshape(o[k].shape), 1e-3, f"{k} {what}", floor=0.0 if k == "dxhat" else 1e-6)
        for k in ("running_mean", "running_var"):
            _close(o[k], ref[k], 1e-5, f"{k} {what}")
            if not training:
                assert torch.equal(o[k].cpu(), c[k]), k
        again = _launch(c, training, lambda0, upstream)
        for k in OUT_NAMES:
            assert torch.equal(o[k], again[k]), (k, what)


@pytest.mark.parametrize("b,l", REF.HEAD_SHAPES)
def test_snps_head_loss_vs_fp64(b, l):
    """(B, L): B = 2 is the smallest legal training batch (unbiased factor 2), 3 an odd one, 30 / 32 the fixtures', 257 one
    row past four 64-row passes (and past 256); K1 = 59 and 86 are no multiples of four and put the seam between the two
    input buffers at columns 5 and 32.  Eval mode, training mode, training mode with dropout factors."""
    names = {n: (c, tr) for n, c, tr in REF.head_cases()}
    for sfx in ("eval", "train", "train+masks"):
        c, training = names[f"B{b}L{l}/{sfx}"]
        _check_case(f"B{b}L{l}/{sfx}", c, training)


def test_snps_head_loss_constant_column_and_soft_labels():
    names = {n: (c, tr) for n, c, tr in REF.head_cases()}
    c, training = names["const_col"]
    assert float(c["snps"][:, 7].var()) == 0.0
    _check_case("const_col", c, training)
    c, training = names["soft"]
    assert 0.0 < float(c["label"].min()) and float(c["label"].max()) < 1.0
    _check_case("soft", c, training)


def test_snps_head_loss_lambda0_zero_is_exact():
    c = REF.head_case(30, 5, masks=True)
    c["x_hat"][3, 4] = float("inf")                       # (0 * inf would be NaN: the term is switched off, not scaled)
    o = _launch(c, True, lambda0=0.0, upstream=1.7)
    out = o["out"].cpu()
    assert float(out[2]) == 0.0 and float(out[0]) == float(out[1]) and np.isfinite(float(out[0]))
    assert bool((o["dxhat"] == 0).all())


def test_snps_head_loss_saturated_sigmoid_is_torchs_bceloss():
    """W2 = 0, b2 = +-30: y_hat = sigmoid(+-30) in fp32, where BCELoss on the probability and the logits form part ways.
    Values against torch's fp32 BCELoss to 1e-5 relative; z = +30, y = 0: the value 100 and a gradient of exactly zero."""
    for z in (30.0, -30.0):
        c = REF.head_case(30, 5)
        c["w2"] = torch.zeros_like(c["w2"])
        c["b2"] = torch.tensor([z])
        c["label"] = torch.tensor([0.0, 1.0, 0.3] * 10)
        o = _launch(c, True, lambda0=0.0)
        p = torch.sigmoid(torch.full((30,), z, device="cuda").requires_grad_(True))
        zz = torch.full((30,), z, device="cuda", requires_grad=True)
        want = torch.nn.BCELoss(reduction="none")(torch.sigmoid(zz), c["label"].cuda())
        want.sum().backward()
        assert torch.allclose(o["y_hat"], p.detach(), rtol=1e-6, atol=0)
        got, w = float(o["out"][1]), float(want.sum())
        assert abs(got - w) <= 1e-5 * abs(w), (z, got, w)
        # db2 = sum of d loss / d z over the rows; W2 = 0: nothing reaches the layers in front
        assert abs(float(o["db2"]) - float(zz.grad.sum())) <= 1e-5 * max(abs(float(zz.grad.sum())), 1e-30), z
        assert bool((o["dW1"] == 0).all()) and bool((o["dlatent"] == 0).all())
        if z > 0:
            c["label"] = torch.zeros(30)
            o = _launch(c, True, lambda0=0.0)
            assert float(o["out"][1]) == 3000.0 and float(o["db2"]) == 0.0 and bool((o["dW2"] == 0).all())


def test_snps_head_running_statistics_are_batchnorm1ds():
    for b, l in ((2, 5), (257, 32)):
        c = REF.head_case(b, l)
        o = _launch(c, True, backward=False)
        bn = torch.nn.BatchNorm1d(l + 54).cuda().train()
        with torch.no_grad():
            bn.running_mean.copy_(c["running_mean"])
            bn.running_var.copy_(c["running_var"])
            bn(torch.cat((c["latent"], c["snps"]), 1).cuda())
        _close(o["running_mean"], bn.running_mean, 1e-5, "running_mean")
        _close(o["running_var"], bn.running_var, 1e-5, "running_var")


def test_snps_head_predict_is_the_eval_forward_on_a_grid():
    """y_hat alone (no labels): any batch size, here 1 and 1500 (beyond the one-workgroup launches' 1024)."""
    from igcn_amd import ops
    for b in (1, 1500):
        c = REF.head_case(b, 32)
        bn = torch.nn.BatchNorm1d(86).cuda().eval()
        with torch.no_grad():
            bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"])                     # noqa: E702
            bn.running_mean.copy_(c["running_mean"]); bn.running_var.copy_(c["running_var"])      # noqa: E702
        got = ops.snps_head_predict(c["latent"].cuda(), c["snps"].cuda(), bn, c["w1"].cuda(), c["w2"].cuda(), c["b2"].cuda())
        ref = REF.head_loss_of(c, False)
        _close(got, ref["y_hat"], 1e-4, f"y_hat B={b}")


# ---- refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,l,s,h,why", [(1025, 32, 54, 16, "B > 1024"), (30, 50, 54, 16, "L + S > 96"),
                                         (30, 5, 54, 8, "H != 16"), (30, 5, 54, 32, "H != 16"), (30, 0, 54, 16, "L < 1")])
def test_snps_head_loss_refusals_write_nothing(b, l, s, h, why):
    from igcn_amd import _lib
    from igcn_amd._lib import IgcnError, call, ptr, stream_ptr
    assert not _lib.load().igcn_snps_head_supported(b, l, s, h), why
    k1 = l + s
    r = lambda *sh: torch.randn(*sh, device="cuda")                          # noqa: E731
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")           # noqa: E731
    t = dict(latent=r(b, max(l, 1)), snps=r(b, s), gamma=r(k1), beta=r(k1), w1=r(h, k1), w2=r(1, h), b2=r(1),
             label=torch.rand(b, device="cuda"), x_hat=r(b, s))
    rm, rv = torch.zeros(k1, device="cuda"), torch.ones(k1, device="cuda")
    outs = dict(y_hat=nan(b), out=nan(3), ws=nan(2 * k1 + 4 + b * h), dlatent=nan(b, max(l, 1)), dxhat=nan(b, s),
                dgamma=nan(k1), dbeta=nan(k1), dW1=nan(h, k1), dW2=nan(h), db2=nan(1))
    with pytest.raises(IgcnError, match="snps_head_loss_fwd") as e:
        call("igcn_snps_head_loss_fwd", b, l, s, h, ptr(t["latent"]), ptr(t["snps"]), ptr(t["gamma"]), ptr(t["beta"]), ptr(rm),
             ptr(rv), 0.1, 1e-5, 1, None, None, ptr(t["w1"]), ptr(t["w2"]), ptr(t["b2"]), ptr(t["label"]), ptr(t["x_hat"]),
             1e-5, ptr(outs["y_hat"]), ptr(outs["out"]), ptr(outs["ws"]), stream_ptr())
    assert "rc=-3" in str(e.value)                   # IGCN_ERR_UNSUPPORTED
    with pytest.raises(IgcnError, match="snps_head_loss_bwd") as e:
        call("igcn_snps_head_loss_bwd", b, l, s, h, 1, ptr(t["latent"]), ptr(t["snps"]), ptr(t["gamma"]), ptr(t["beta"]), None,
             None, ptr(t["w1"]), ptr(t["w2"]), ptr(t["label"]), ptr(t["label"]), ptr(t["x_hat"]), 1e-5, None, ptr(outs["ws"]),
             ptr(outs["dlatent"]), ptr(outs["dxhat"]), ptr(outs["dgamma"]), ptr(outs["dbeta"]), ptr(outs["dW1"]),
             ptr(outs["dW2"]), ptr(outs["db2"]), stream_ptr())
    assert "rc=-3" in str(e.value)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool(torch.isnan(v).all()), (k, why)
    assert bool((rm == 0).all()) and bool((rv == 1).all())


def test_one_sample_in_training_mode_raises(golden):
    from igcn_amd import _lib, ops, snps
    c = {k: (v.cuda() if v is not None else None) for k, v in REF.head_case(2, 5).items()}
    one = lambda k: c[k][:1].contiguous()                                     # noqa: E731
    with pytest.raises(ValueError, match="more than one sample"):
        ops.SnpsHeadLoss.apply(one("latent"), one("snps"), one("x_hat"), one("label"), c["gamma"], c["beta"],
                               c["running_mean"], c["running_var"], 0.1, 1e-5, True, None, None, c["w1"], c["w2"], c["b2"],
                               1e-5)
    with pytest.raises(_lib.IgcnError, match="more than one row"):          # (the entry point itself: a bad argument)
        _launch({k: (v[:1] if k in ("latent", "snps", "x_hat", "label") else v) for k, v in REF.head_case(2, 5).items()},
                True, backward=False)
    model, cfg = _model(golden("snps_only"), "main20")
    data, label = (t.cuda() for t in REF.inputs("main20"))
    model.train()
    with pytest.raises(ValueError, match="more than one sample"):
        snps.losses_snps(model, data[:1], label[:1])
    model.eval()                                       # eval mode takes one sample
    loss, _, (_, _, y_hat) = snps.losses_snps(model, data[:1], label[:1])
    assert y_hat.shape == (1,) and bool(torch.isfinite(loss))


def test_snps_head_loss_autograd_function():
    """ops.SnpsHeadLoss: the cached unit upstream gradient of a train step (passed on as "one") and a general one."""
    from igcn_amd import ops
    from igcn_amd.train import _unit_grad
    c = REF.head_case(32, 32, masks=True)
    t = {k: (v.cuda() if v is not None else None) for k, v in c.items()}
    unit = _unit_grad(torch.zeros((), device="cuda"))
    for upstream, lazy in ((1.0, True), (1.7, False)):
        ref = REF.head_loss_of(c, True, upstream=upstream)
        names = ("latent", "x_hat", "gamma", "beta", "w1", "w2", "b2")
        ls = [t[n].clone().requires_grad_(True) for n in names]
        rm, rv = t["running_mean"].clone(), t["running_var"].clone()
        assert ops.snps_head_supported(ls[0], t["snps"], ls[4])
        loss, terms, y_hat = ops.SnpsHeadLoss.apply(ls[0], t["snps"], ls[1], t["label"], ls[2], ls[3], rm, rv, 0.1, 1e-5, True,
                                                    t["keep1"], t["keep2"], ls[4], ls[5], ls[6], REF.LAMBDA0, lazy)
        go = unit if upstream == 1.0 else torch.full((), upstream, device="cuda")
        grads = torch.autograd.grad(loss, ls, grad_outputs=go)
        assert terms.shape == (2,) and not terms.requires_grad and not y_hat.requires_grad
        assert abs(float(loss) - float(ref["loss"])) <= 1e-4 * max(1.0, abs(float(ref["loss"])))
        _close(y_hat, ref["y_hat"], 1e-4, "y_hat")
        _close(rm, ref["running_mean"], 1e-5, "running_mean")
        for g, n in zip(grads, ("dlatent", "dxhat", "dgamma", "dbeta", "dW1", "dW2", "db2")):
            _close(g, ref[n].reshape(g.shape), 1e-3, n, floor=0.0 if n == "dxhat" else 1e-6)


# ---- the model against the reference's fixture ----------------------------------------------------------------------
def _model(store, tag, dropout=False):
    from igcn_amd import synth
    from igcn_amd.go_model import Gene_ontology_network
    cfg, _, sd = REF.fixture_setup(store, tag)
    go_snps, adj, pool_dim = REF.hierarchy(tag)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    model = Gene_ontology_network(a_g, a, 2, 2, [5, 5], pool_dim, cfg.l_dim, "cuda").cuda()
    assert sorted(model.state_dict()) == store[f"{tag}/state_keys"].tolist()
    model.load_state_dict(sd)
    model._dropout_enabled = dropout
    return model, cfg


def _traced(mp, fn):
    from calltrace import record_calls
    seen = record_calls(mp)
    return fn(), [c[0] for c in seen]


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_model_vs_reference_golden(golden, monkeypatch, tag, mode, route):
    """Outputs at 1e-4, the loss and both terms at 2e-4, gradients at 1e-3 (eval mode) / 5e-3 (training mode); in training
    mode also the parameters after one Adam step (train_step_snps) and the BatchNorm buffers.  Every parameter the
    reference's loss reaches receives a gradient, ``classification.*`` included."""
    from igcn_amd import snps
    from igcn_amd.train import FlatAdam
    store = golden("snps_only")
    model, cfg = _model(store, tag)
    model.train(mode == "train")
    if route == "unfused":
        monkeypatch.setenv("IGCN_NO_HEAD_LOSS_FUSED", "1")
    data, label = (t.cuda() for t in REF.inputs(tag, mode))
    with monkeypatch.context() as mp:
        (loss, terms, outs), seen = _traced(mp, lambda: snps.losses_snps(model, data, label, cfg.lambda0))
    assert ("igcn_snps_head_loss_fwd" in seen) == (route == "fused"), seen
    assert ("igcn_small_linear_fwd" in seen) == (route == "unfused"), seen
    want = group(store, f"{tag}/{mode}/out")
    for n, o in zip(("latent", "x_hat", "y_hat"), outs):
        assert_matches(o, want[n], TOL, n)
    w = float(store[f"{tag}/{mode}/loss"])
    print(f"\n[{tag}/{mode}/{route}] loss {float(loss):.6f}, reference {w:.6f}")
    assert abs(float(loss) - w) <= STEP_TOL * max(1.0, abs(w)), (float(loss), w)
    assert sorted(terms) == sorted(REF.TERMS)
    for k, v in terms.items():
        w = float(store[f"{tag}/{mode}/term/{k}"])
        assert abs(float(v) - w) <= STEP_TOL * max(1.0, abs(w)), (k, float(v), w)
    loss.backward()
    params = dict(model.named_parameters())
    wg = group(store, f"{tag}/{mode}/grad")
    assert any(k.startswith("classification.") for k in wg)
    for k in store[f"{tag}/{mode}/no_grad"].tolist():
        g = params[k].grad
        assert g is None or not bool(g.abs().max() > 0), k
    for k, w in wg.items():
        assert params[k].grad is not None, k
        assert_matches(params[k].grad, w, GTOL[mode], "grad " + k, floor=grad_floor(wg, k, 1e-5))
    if mode != "train":
        return
    # one train() iteration on a fresh model: the golden's Adam step (tests/test_gpu_clusterlabel.py's check)
    model, cfg = _model(store, tag)
    model.train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    got = snps.train_step_snps(model, opt, data, label, cfg.lambda0)
    w = float(store[f"{tag}/train/loss"])
    assert abs(float(got) - w) <= STEP_TOL * max(1.0, abs(w))
    params, bufs, lr = dict(model.named_parameters()), model.state_dict(), 1e-3
    for k, w in group(store, f"{tag}/step/buffers_after").items():
        assert_matches(bufs[k], w, 1e-3, "buffer " + k, floor=1e-2)
    assert int(bufs["classification.0.num_batches_tracked"]) == 1 and int(bufs["latent.1.num_batches_tracked"]) == 1
    for k, w in group(store, f"{tag}/step/param_after").items():
        p = params[k].detach().cpu()
        if isinstance(w, tuple) or k not in wg or isinstance(wg[k], tuple):
            assert_matches(p, w, 2.5 * lr, "param " + k, floor=1.0)
            continue
        g = torch.from_numpy(wg[k])
        diff = (p - torch.from_numpy(w)).abs()
        solid = g.abs() > 5e-2 * g.abs().max() if g.abs().max() > 0 else torch.zeros_like(g, dtype=torch.bool)
        sib = wg.get(k[:-5] + ".weight") if k.endswith(".bias") else None
        if sib is not None and not isinstance(sib, tuple) and float(g.abs().max()) < 1e-2 * float(np.abs(sib).max()):
            solid = torch.zeros_like(solid)
        assert float(diff[solid].max() if solid.any() else 0.0) <= 5e-5, "param " + k
        assert float(diff.max()) <= 2.01 * lr, "param (noise-level grads) " + k


# ---- the captured step, the epoch, the evaluation -------------------------------------------------------------------
def _params_close(m1, m2):
    """tests/test_gpu_model.py::test_graphed_train_step_matches_eager's bound."""
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        d = (p1.detach() - p2.detach()).abs()
        tol = torch.full_like(d, 2e-4) if p2.grad is None else torch.where(p2.grad.abs() > 1e-6, 2e-4, 3.5e-3)
        assert bool((d <= tol).all()), (k, float(d.max()))


def _samples(n, seed):
    rng = np.random.default_rng(seed)
    data = torch.from_numpy(rng.integers(0, 3, (n, 54)).astype(np.float32)).cuda()
    label = torch.from_numpy((rng.random(n) < 0.5).astype(np.float32)).cuda()
    return data, label


def test_graphed_step_equals_eager_steps(golden):
    """Four replays on changing batches against four eager train_step_snps calls; the constructor's warm-up steps leave no
    trace; a batch of another shape is refused."""
    from igcn_amd import snps
    from igcn_amd.train import FlatAdam
    m1, _ = _model(golden("snps_only"), "b32")
    m1.train()
    m2 = copy.deepcopy(m1)
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    snap = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    step = snps.GraphedSnpsStep(m1, o1, *_samples(32, 300), warmup=2)
    for k, v in m1.state_dict().items():
        assert torch.equal(v, snap[k]), k
    assert int(o1.step_count.item()) == 0 and not bool(o1.exp_avg.any())
    for i in range(4):
        data, label = _samples(32, 301 + i)
        step.load(data, label)
        l1 = float(step.step())
        l2 = float(snps.train_step_snps(m2, o2, data, label))
        assert abs(l1 - l2) <= 1e-4 * max(1.0, abs(l2)), (i, l1, l2)
    _params_close(m1, m2)
    assert int(o1.step_count.item()) == 4
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        if "running_" in k or "num_batches" in k:
            _close(a.float(), b.float(), 1e-4, k, floor=1e-2)
    with pytest.raises(ValueError, match="fixed shapes"):
        step.load(*_samples(6, 1))


def test_graphed_step_construction_leaves_no_trace_with_dropout_on(golden):
    """The 32-sample shape with every dropout ON, after one eager step (non-zero Adam moments, a live mask generator on
    the GO network, which here is the model itself): the constructor's two warm-up steps are rolled back — parameters,
    both moments, the step count, every buffer, the generator's counter and ``_has_state`` bit for bit, before any
    replay."""
    from igcn_amd import snps
    from igcn_amd.train import FlatAdam
    from rollback_state import assert_rolled_back, rollback_state
    model, _ = _model(golden("snps_only"), "b32", dropout=True)
    model.train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    snps.train_step_snps(model, opt, *_samples(32, 299))
    before = rollback_state(model, opt)
    assert "generator _drop_state" in before[0] and bool(before[0]["exp_avg"].any()) and any(before[1])
    snps.GraphedSnpsStep(model, opt, *_samples(32, 300), warmup=2)
    assert_rolled_back(model, opt, before)


def test_fit_epoch_equals_the_eager_loop(golden):
    """70 samples at batch 32 — two full batches and a ragged tail of 6 — over two epochs: the three returned sums and the
    final parameters against train_step_snps by hand (each shape is captured the second time it is met)."""
    from igcn_amd import snps
    from igcn_amd.train import FlatAdam
    m1, _ = _model(golden("snps_only"), "b32")
    m2 = copy.deepcopy(m1)
    data, label = _samples(70, 400)
    loader = [(data[i:i + 32], label[i:i + 32]) for i in range(0, 70, 32)]
    assert [int(d.shape[0]) for d, _ in loader] == [32, 32, 6]
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    for _ in range(2):
        got = snps.fit_epoch_snps(m1, o1, loader, lambda0=2e-5)
        m2.train()
        want = np.zeros(3)
        for d, y in loader:
            vec = snps._fwd_bwd(m2, o2, d, y, 2e-5)
            o2.step()
            want += vec.double().cpu().numpy()
        want /= 70
        assert len(got) == 3
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-4 * max(1.0, abs(w)), (got, want)
        assert abs(got[0] - (got[1] + got[2])) <= 1e-5 * max(1.0, abs(got[0]))
    tr = next(iter(o1._igcn_snps_trainers.values()))
    assert tr.counts == {"captured": 2, "replayed": 4, "eager": 2}, tr.counts
    _params_close(m1, m2)


def test_evaluation_against_host_metrics(golden):
    """eval_loss_snps / eval_acc_snps / eval_scores_snps on 200 samples (batches of 64 and a tail) against the host
    restatement of igcn_eval_metrics on the same scores; one score is exactly 0.5 and counts as class 0."""
    from eval_metrics_ref import metrics
    from igcn_amd import snps
    model, cfg = _model(golden("snps_only"), "b32")
    data, label = _samples(200, 500)
    loader = [(data[i:i + 64], label[i:i + 64]) for i in range(0, 200, 64)]
    model.eval()
    with torch.no_grad():
        latent = model(data, None, "cuda")[0]
        z = None
        # move the last layer's bias until sample 17 scores exactly 0.5 (its logit within 6e-8 of zero): y_hat is monotone
        # in the bias, so a bisection over fp32 values finds it
        del z
        bias = model.classification[6].bias
        lo, hi = float(bias) - 8.0, float(bias) + 8.0
        for _ in range(80):
            bias.fill_(0.5 * (lo + hi))
            y17 = float(snps.classify(model, latent[17:18], data[17:18]))
            if y17 == 0.5:
                break
            lo, hi = (lo, float(bias)) if y17 > 0.5 else (float(bias), hi)
        y_hat = snps.classify(model, latent, data)
    assert float(y_hat[17]) == 0.5
    true_label, pred_label, acc, auc, f1, sens, spec = snps.eval_scores_snps(model, loader, "cuda", None, None, None, cfg.lambda0)
    p = y_hat.cpu().numpy()
    assert true_label.dtype == bool and pred_label.dtype == bool and not pred_label[17]
    assert np.array_equal(pred_label, p > 0.5) and np.array_equal(true_label, label.cpu().numpy() > 0.5)
    want = metrics(np.stack([np.log1p(-p), np.log(p)], 1), pred_label, true_label, np.zeros((200, 0)), np.zeros((200, 0)), 2)
    assert acc == want["accuracy"] == float((pred_label == true_label).sum()) / 200
    for g, k in ((auc, "auc"), (sens, "sensitivity"), (spec, "specificity")):
        assert np.array_equal(g, want[k], equal_nan=True), (k, g, want[k])
    assert f1 == pytest.approx(want["f1"], rel=1e-12)
    assert 0.0 <= auc <= 1.0
    assert snps.eval_acc_snps(model, loader, "cuda", None, None, None, cfg.lambda0) == acc
    # the loss: the three sums over the loader divided by the number of samples, against the one-batch evaluation
    ll = snps.eval_loss_snps(model, loader, "cuda", None, None, None, cfg.lambda0)
    with torch.no_grad():
        loss, t, _ = snps.losses_snps(model, data, label, cfg.lambda0)
    for g, w in zip(ll, (float(loss) / 200, float(t["class"]) / 200, float(t["recon"]) / 200)):
        assert abs(g - w) <= 1e-5 * max(1.0, abs(w)), (ll, w)


# ---- dropout on ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_train_losses_with_dropout_vs_oracle_under_the_steps_own_masks(golden, monkeypatch, route):
    """Dropout ON: the head's two sites ([B, l_dim + 54] at p = 0.5, [B, 16] at p = 0.3) come out of the GO network's ONE
    mask launch — no launch is added — and are handed over in ``extra_masks``; the recorded factors equal
    oracle.dropout.masks(sites, counter) bit for bit; snps_ref.losses fed those factors by site name gives the step's loss
    and terms at 2e-4 and its gradients at the training-mode bound (tests/test_gpu_model.py's dropout-on scheme)."""
    from igcn_amd import snps
    from oracle import dropout as OD
    from oracle import sgcn_img_snp as OS
    tag = REF.DROPOUT_TAG
    store = golden("snps_only")
    model, cfg = _model(store, tag, dropout=True)
    model.train()
    if route == "unfused":
        monkeypatch.setenv("IGCN_NO_HEAD_LOSS_FUSED", "1")
    data, label = (t.cuda() for t in REF.inputs(tag))
    counter = int(DC.set_counter(model).state[0].item())
    with monkeypatch.context() as mp:
        drawn = DC.recorded_masks(mp)
        (loss, terms, _), seen = _traced(mp, lambda: snps.losses_snps(model, data, label, cfg.lambda0))
    loss.backward()
    assert ("igcn_snps_head_loss_fwd" in seen) == (route == "fused"), seen
    assert seen.count("igcn_dropout_masks") == 1 and len(drawn.calls) == 1
    sites, arrays = drawn.calls[0][0], drawn.arrays(0)
    assert sites == REF.dropout_sites(tag) and sites[-2:] == [((32, 86), 0.5), ((32, 16), 0.3)]
    assert [tuple(m.shape) for m in model.extra_masks] == [(32, 86), (32, 16)]
    assert np.array_equal(model.extra_masks[0].cpu().numpy(), arrays[-2])
    DC.assert_masks_rebuilt(sites, arrays, counter, f"{tag}/{route}")
    names = OD.go_site_names(2, REF.HEAD_SITES)
    _, idx, sd = REF.fixture_setup(store, tag)

    def oracle(factors, grad):
        with torch.set_grad_enabled(grad):
            st = OS.make_leaf_state(sd, torch.float64)
            feed = OD.feed_of(sites, factors, names)
            out = REF.losses(st, idx, data.cpu().double(), label.cpu().double(), cfg.lambda0, True, feed)
            feed.close()
        return st, out
    st, (ref_loss, ref_terms, _) = oracle(arrays, True)
    ref_loss.backward()
    ref = float(ref_loss)
    print(f"\n[{tag}/{route}] loss {float(loss):.6f}, oracle {ref:.6f}")
    assert abs(float(loss) - ref) <= STEP_TOL * max(1.0, abs(ref)), (float(loss), ref)
    for k, v in terms.items():
        r = float(ref_terms[k])
        assert abs(float(v) - r) <= STEP_TOL * max(1.0, abs(r)), (k, float(v), r)
    params = dict(model.named_parameters())
    wg = {k: v.grad.numpy() for k, v in st.items() if v.requires_grad and v.grad is not None}
    for k, w in wg.items():
        g = params[k].grad
        if g is None:
            assert not np.abs(w).max() > 0, k
            continue
        assert_matches(g, w, GTOL["train"], "grad " + k, floor=grad_floor(wg, k, 1e-5))
