"""CPU checks of SGCN_GCN_CLUSTERLABEL (kernel/sgcn_img_snp_clusterlabel.py:13-231, trained by
kernel/train_eval_sgcn_clusterlabel.py:365-447) against the fixture captured from the reference
(tests/golden/clusterlabel.npz, written by tests/golden/make_golden_clusterlabel.py): the float64 restatement
tests/clusterlabel_ref.py at the bounds tests/test_oracle_golden.py holds the headline restatement to, the drop-in's
constructor / state_dict surface, the configurations it refuses, and that the fixture tells this model's regulariser
from the headline's."""
import inspect

import numpy as np
import pytest
import torch

from conftest import assert_matches
from igcn_amd.data import Batch
from oracle import sgcn_img_snp as OS
from test_oracle_golden import grad_floor

import clusterlabel_ref as REF

TAGS = ["h0_1", "h0_3", "nopredict"]
NAMES = ("logp", "logp_cluster", "x_hat", "out_z")
# tests/test_oracle_golden.py's bounds: eval 1e-5 outputs / 5e-4 gradients; training mode 1e-4 on outputs (its bound at
# B = 32, where BatchNorm no longer amplifies rounding) and its general training-mode 5e-3 on gradients.  The tighter 1e-3
# it keeps for its own B = 32 fixtures is below the fp32 noise of THIS fixture's probed gradients: the reference ran in
# fp32, and this very restatement evaluated in fp32 — the reference's arithmetic — already sits 1.3e-3 .. 2.3e-3 from the
# stored go_network.conc / w_att_in gradients (sums over 32 x 2944 probed columns), as far as the float64 evaluation does
# (up to 2.7e-3); both are rounding of the reference's side, and a bound below it would test nothing.
TOL = {"eval": 1e-5, "train": 1e-4}
GTOL = {"eval": 5e-4, "train": 5e-3}


def _probe(outs, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal(tuple(o.shape))).float() for o in outs]


def _data64(graphs):
    data = Batch.from_data_list(graphs)
    data.x = data.x.double().requires_grad_(True)
    data.edge_attr = data.edge_attr.double()
    data.snps_feat = data.snps_feat.double()
    return data


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_has_every_label(golden, tag):
    store = golden("clusterlabel")
    cfg, _, _, graphs = REF.fixture_setup(store, tag)
    big = Batch.from_data_list(graphs["train"])
    assert sorted(set(big.clust_y.view(-1).tolist())) == [0, 1] and sorted(set(big.y.view(-1).tolist())) == [0, 1, 2]
    assert "sgcn_img_snp_clusterlabel" in str(store["meta"]) and cfg.lambda0 == 1e-5
    assert (cfg.h0, cfg.predict) == {"h0_1": (1, True), "h0_3": (3, True), "nopredict": (1, False)}[tag]


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("explain", [False, True])
def test_restatement_matches_reference(golden, tag, mode, explain):
    store = golden("clusterlabel")
    cfg, idx, sd0, graphs = REF.fixture_setup(store, tag)
    sd = OS.make_leaf_state(sd0, torch.float64)
    data = _data64(graphs[mode])
    outs = REF.model_forward(sd, cfg.rois, idx, data, explain, training=(mode == "train"), predict=cfg.predict)
    grp = f"{tag}/{mode}/explain{int(explain)}"
    want = REF.group(store, grp + "/out")
    for n, o in zip(NAMES, outs):
        assert_matches(o, want[n], TOL[mode], n)
    cot = _probe(outs, cfg.seed + 3)
    sum((o * c.double()).sum() for o, c in zip(outs, cot)).backward()
    wg = REF.group(store, grp + "/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), GTOL[mode], "grad data.x")
    for k, w in wg.items():
        assert sd[k].grad is not None, k
        assert_matches(sd[k].grad, w, GTOL[mode], "grad " + k, floor=grad_floor(wg, k, 1e-4))
    for k, v in sd.items():            # and nothing the reference leaves without a gradient gets one here
        if v.requires_grad and v.grad is not None and k not in wg:
            assert not bool(v.grad.abs().max() > 0), "unexpected grad " + k


@pytest.mark.parametrize("tag", TAGS)
def test_train_step_matches_reference(golden, tag):
    store = golden("clusterlabel")
    cfg, idx, sd0, graphs = REF.fixture_setup(store, tag)
    sd = OS.make_leaf_state(sd0, torch.float64)
    data = _data64(graphs["train"])
    loss, terms, _ = REF.train_step(sd, cfg.rois, idx, data, lr=1e-3, lambda0=cfg.lambda0, predict=cfg.predict)
    want = float(store[f"{tag}/step/loss"])
    assert abs(float(loss) - want) <= 1e-5 * max(1.0, abs(want))
    assert sorted(terms) == sorted(REF.TERMS)
    for k, v in terms.items():
        w = float(store[f"{tag}/step/term/{k}"])
        assert abs(float(v) - w) <= 1e-5 * max(1.0, abs(w)), k
    wg = REF.group(store, f"{tag}/step/grad")
    no_grad = set(store[f"{tag}/step/no_grad"].tolist())
    assert no_grad.isdisjoint(wg)
    assert ("lin2_cluster.weight" in no_grad) == (not cfg.predict)
    assert_matches(data.x.grad, wg.pop("data.x"), 5e-3, "grad data.x")
    grads = {}
    for k in no_grad:                  # what the reference's loss does not reach gets nothing here either
        assert sd[k].grad is None or not bool(sd[k].grad.abs().max() > 0), k
    for k, w in wg.items():
        assert_matches(sd[k].grad, w, 1e-2, "grad " + k, floor=grad_floor(wg, k, 1e-5))
        grads[k] = w
    lr = 1e-3
    for k, w in REF.group(store, f"{tag}/step/param_after").items():
        # (tests/test_oracle_golden.py: Adam's first step is ill-conditioned where the gradient is rounding noise)
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
    for k, w in REF.group(store, f"{tag}/step/buffers_after").items():
        assert_matches(sd[k], w, 3e-4, "buffer " + k, floor=1e-2)


def test_the_read_out_decision_fp32_cannot_make(golden):
    """(h0_1, training mode, plain pass): the GO read-out pre-activation of sample 19, node 67 — the ninth ``torch.relu``
    of the restatement's forward — lies within 1e-6 of zero on its tensor's scale, and the other decision moves
    d go_network.w_inc.0.weight by 1.03e-2 of its scale and d go_network.w_att_s.1.weight, the furthest, by 2.3e-2.
    tests/test_gpu_clusterlabel.py gives the GO-network gradients of that group this slack: an fp32 evaluation in
    another order may take either side."""
    from conftest import relu_forced
    store = golden("clusterlabel")
    site, where, key = 8, (19, 67), "go_network.w_inc.0.weight"

    def grads(forced):
        cfg, idx, sd0, graphs = REF.fixture_setup(store, "h0_1")
        sd = OS.make_leaf_state(sd0, torch.float64)
        data = _data64(graphs["train"])
        seen = []
        orig = torch.relu

        def spy(t):
            seen.append(t.detach())
            return orig(t)
        if forced is None:
            torch.relu = torch.nn.functional.relu = spy
            try:
                outs = REF.model_forward(sd, cfg.rois, idx, data, False, training=True, predict=cfg.predict)
            finally:
                torch.relu = torch.nn.functional.relu = orig
        else:
            with relu_forced(forced, band=1e-5) as rf:
                outs = REF.model_forward(sd, cfg.rois, idx, data, False, training=True, predict=cfg.predict)
            assert rf.flips == 1
        cot = _probe(outs, cfg.seed + 3)
        sum((o * c.double()).sum() for o, c in zip(outs, cot)).backward()
        return sd, seen
    sd, seen = grads(None)
    t = seen[site]
    assert t.shape == (32, 500) and float(t[where].abs() / t.abs().max()) < 1e-6
    other = t > 0
    other[where] = ~other[where]
    sd2, _ = grads({site: other})
    g, g2 = sd[key].grad, sd2[key].grad
    shift = float((g2 - g).abs().max() / g.abs().max())
    assert 1.0e-2 <= shift <= 1.06e-2, shift
    # ... and the GO-network gradient that moves furthest, in the measure the fixture holds it to (conftest.
    # assert_matches: largest difference over largest magnitude, or the summary of a tensor stored as one)
    from _weights import summarise
    wg = REF.group(store, "h0_1/train/explain0/grad")
    shifts = {}
    for k, w in wg.items():
        if not k.startswith("go_network.") or sd[k].grad is None:
            continue
        a, b = sd[k].grad, sd2[k].grad
        if isinstance(w, tuple):
            moved = float((np.abs(summarise(b) - summarise(a)) / max(abs(summarise(a)[1]), 1e-30)).max())
        else:
            moved = float((b - a).abs().max() / max(float(a.abs().max()), 1e-4))
        shifts[k] = moved
    top = max(shifts, key=shifts.get)
    print({k: round(v, 5) for k, v in shifts.items() if v > 1e-3})
    assert top == "go_network.w_att_s.1.weight" and 2.2e-2 <= shifts[top] <= 2.4e-2, (top, shifts[top])


def test_h0_3_tells_the_two_regularisers_apart(golden):
    """Only with H_0 = 3 does ``f_sum_loss = sum / rows`` differ from the headline model's mean; the fixture's ``prob``
    term is this model's and is far from the headline formula's value."""
    store = golden("clusterlabel")
    cfg, _, sd0, graphs = REF.fixture_setup(store, "h0_3")
    sd = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd0.items()}
    data = _data64(graphs["train"])
    with torch.no_grad():
        own = float(REF.loss_probability(sd, data.x, data.edge_index, data.edge_attr, cfg.rois))
        headline = float(OS.loss_probability(sd, data.x, data.edge_index, data.edge_attr, cfg.rois))
    want = float(store["h0_3/step/term/prob"])
    assert abs(own - want) <= 1e-5 * max(1.0, abs(want))
    assert abs(headline - want) > 1e-2 * abs(want)


# ---- the drop-in's surface ---------------------------------------------------------------------------------------
def _model(cfg, **kw):
    from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
    args = dict(H_0=cfg.h0, num_features=cfg.h0, isCrossAtten=True, isPredictCluster=cfg.predict)
    args.update(kw)
    return SGCN_GCN_CLUSTERLABEL(cfg.layers, cfg.hidden, cfg.a_g, cfg.a, cfg.pool_dim, cfg.l_dim, "cpu", **args)


def test_constructor_signature_is_the_reference():
    from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
    p = inspect.signature(SGCN_GCN_CLUSTERLABEL.__init__).parameters
    assert list(p)[:8] == ["self", "num_layers", "hidden", "A_g", "A", "pool_dim", "l_dim", "device"]
    defaults = {k: v.default for k, v in p.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert defaults == dict(hidden_linear=64, rois=90, H_0=1, num_features=1, num_classes=3, num_cluster=2,
                            isCrossAtten=False, isPredictCluster=True)
    f = inspect.signature(SGCN_GCN_CLUSTERLABEL.forward).parameters
    assert list(f) == ["self", "data", "temperature", "device", "isExplain"] and f["isExplain"].default is False
    lp = inspect.signature(SGCN_GCN_CLUSTERLABEL.loss_probability).parameters
    assert list(lp)[:6] == ["self", "x", "edge_index", "edge_weight", "hp", "eps"] and lp["eps"].default == 1e-6
    assert callable(SGCN_GCN_CLUSTERLABEL.consist_loss) and SGCN_GCN_CLUSTERLABEL.clusterlabel is True


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_is_the_reference(golden, tag):
    store = golden("clusterlabel")
    cfg, _, sd0, _ = REF.fixture_setup(store, tag)
    model = _model(cfg)
    sd = model.state_dict()
    keys = store[f"{tag}/state_keys"].tolist()
    assert sorted(sd) == keys
    shapes = [",".join(str(d) for d in sd[k].shape) for k in keys]
    assert shapes == store[f"{tag}/state_shapes"].tolist()
    assert {"batch_norm.weight", "edge_prob", "lin1_classify.weight", "lin1_cluster.weight"} <= set(keys)
    assert not any(k.startswith(("lin1.", "lin2.", "lin1_regr", "lin2_regr", "batch_norm_1d")) for k in keys)
    model.load_state_dict(sd0)                       # strict: the seeded reference state loads as it is
    # the literal 90 of the head widths, whatever ``rois`` says (kernel/sgcn_img_snp_clusterlabel.py:46,50)
    other = _model(cfg, rois=45)
    assert other.lin1_classify.weight.shape[1] == 90 * cfg.layers * cfg.hidden + cfg.l_dim
    assert other.lin1_cluster.weight.shape == other.lin1_classify.weight.shape and other.prob.shape == (45, cfg.h0)


def test_configurations_the_reference_cannot_run_are_refused(golden):
    store = golden("clusterlabel")
    cfg, _, _, graphs = REF.fixture_setup(store, "h0_1")
    data = Batch.from_data_list(graphs["eval"])
    with pytest.raises(ValueError, match="isCrossAtten=False"):
        _model(cfg, isCrossAtten=False)(data, None, "cpu")
    with pytest.raises(ValueError, match="rois must be 90"):
        _model(cfg, rois=45)(data, None, "cpu")
    with pytest.raises(ValueError, match="isCrossAtten=False"):
        _model(cfg, isCrossAtten=False).forward_pair(data, None, "cpu")
    with pytest.raises(ValueError, match="num_features == H_0"):
        _model(cfg, num_features=3)(data, None, "cpu", isExplain=True)


def test_trainer_entry_points_refuse_or_accept_the_model(golden):
    from igcn_amd import train
    store = golden("clusterlabel")
    cfg, _, _, _ = REF.fixture_setup(store, "h0_1")
    model = _model(cfg)
    for fn in (lambda: train.Evaluator(model), lambda: train.evaluate(model, []),
               lambda: train.eval_scores(model, [], None, train.DEFAULT_LAMBDA, None, False, "cpu")):
        with pytest.raises(ValueError, match="SGCN_GCN_CLUSTERLABEL"):
            fn()
    assert train._cluster_lambda0(train.DEFAULT_LAMBDA) == train._cluster_lambda0(None) == 1e-5
    assert train._cluster_lambda0(2e-5) == 2e-5
    assert train._batched(model) and train._single_use_parameters(model)
    assert inspect.signature(train.losses_clusterlabel).parameters["lambda0"].default == 1e-5
