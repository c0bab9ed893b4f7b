"""tests/head_loss_ref.py (the float64 reference the GPU tests hold ops.HeadLoss / ops.LossHead to) against the oracle's
train_losses on the oracle's own outputs, and its gradients against finite differences.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import head_loss_ref as R
from _weights import seeded_state
from oracle import go_network as OG
from oracle import sgcn_img_snp as OS

L_TEST = [0.7, 1.0, 0.5, 1.5e-3, 0.1, 0.2]
L_MAIN = [0, 1, 0.5, 1.5e-6, 0.1, 0]
L_TRAINER = [1, 1, 1, 2.5e-6, 0.2, 0.2]
POOL, ROIS, BSZ = (20, 10, 6, 3, 1), 12, 5


@pytest.fixture(scope="module", params=[(2, 4), (3, 3)], ids=["C2_NR4", "C3_NR3"])
def oracle_pass(request):
    """(heads, state, batch, o1, o2) of a tiny SGCN_GCN_IMGSNP in training mode, dropout off, float64: computed once."""
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    c, nr = request.param
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=4)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cpu")
    model = SGCN_GCN_IMGSNP(2, 4, a_g, a, pool_dim, 32, "cpu", rois=ROIS, H_0=3, num_classes=c, isSoftSimilarity=True,
                            rbf_gamma=0.01, isCrossAtten=True, num_regr=nr, isuseProb4Regr=True, isImageOnly=False,
                            isSNPsOnly=False)
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, 6)
    assert tuple(sd["lin2.weight"].shape)[0] == c and tuple(sd["lin2_regr.weight"].shape)[0] == nr
    sd = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    idx = OG.go_index_sets(a_g, a, list(POOL), 2)
    cfg = SimpleNamespace(num_layers=2, rois=ROIS, image_only=False, rbf_gamma=0.01)
    d = Batch.from_data_list(synth.brain_graph_list(BSZ, seed=9, rois=ROIS, tsne_dim=16, num_classes=c, num_regr=nr))
    for k in ("x", "edge_attr", "snps_feat", "clini_score", "tsne_fdim"):
        setattr(d, k, getattr(d, k).double())
    with torch.no_grad():
        _, _, (o1, o2) = OS.train_losses(sd, cfg, idx, d, L_TEST, dropout=False)
    return (c, nr), sd, cfg, idx, d, o1, o2


@pytest.mark.parametrize("lam", [L_TEST, L_MAIN, L_TRAINER], ids=["L_TEST", "L_MAIN", "L_TRAINER"])
def test_terms_equal_the_oracles_on_the_oracles_own_outputs(oracle_pass, lam):
    """The seven terms and the loss of head_loss_ref.loss_head, fed (o1, o2) of oracle.sgcn_img_snp.train_losses, equal
    train_losses' own to 1e-12 — the Gram terms and the regulariser passed both reduced ([2, 2], scalar) and as partial
    rows — and head_loss_ref.head_loss, fed the features in front of the output layers, gives the same again."""
    (c, nr), sd, cfg, idx, d, o1, o2 = oracle_pass
    with torch.no_grad():
        want_loss, want, _ = OS.train_losses(sd, cfg, idx, d, lam, dropout=False)
    logp, reg, x_hat = torch.cat([o1[0], o2[0]]), torch.cat([o1[5], o2[5]]), torch.cat([o1[1], o2[1]])
    assert logp.shape == (2 * BSZ, c) and reg.shape == (2 * BSZ, nr)
    gram = torch.stack([torch.stack([OS.consist_loss(o[2], d.tsne_fdim, cfg.rbf_gamma), OS.orthogonal_constraint(o[2])])
                        for o in (o1, o2)])
    prob = OS.loss_probability(sd, d.x, d.edge_index, d.edge_attr, cfg.rois)
    y, clin = d.y.view(-1), d.clini_score.view(-1)
    rng = np.random.default_rng(0)
    # partial rows: any split whose column sums are (consist_1, orth_1, consist_2, orth_2) / whose sum is the regulariser
    w = torch.from_numpy(rng.random((7, 1)))
    gram_rows = (w / w.sum()) * gram.reshape(1, 4)
    p = torch.from_numpy(rng.random(11))
    prob_rows = p / p.sum() * prob

    def check(got):
        assert abs(float(got["loss"]) - float(want_loss)) <= 1e-12 * max(1.0, abs(float(want_loss)))
        for j, k in enumerate(R.TERMS):
            assert abs(float(got["terms"][j]) - float(want[k])) <= 1e-12 * max(1.0, abs(float(want[k]))), k
        if lam[0] == 0:
            assert float(got["terms"][0]) == 0.0 and float(got["terms"][1]) == 0.0

    for g_, p_ in ((gram, prob), (gram_rows, prob_rows)):
        got = R.loss_head(logp, y, reg, clin, x_hat, d.snps_feat, g_, p_, lam, OS.HP.lamda_ce, OS.HP.lamda_mi,
                          from_logits=False)
        check(got)
        assert (got["grads"]["scores"] is None) == (lam[0] == 0)
    # from the features in front of lin2 / lin2_regr: lin_f is the oracle's fifth output (dropout off: h = lin_f); the
    # regression features are rebuilt as model_forward :147-153 builds them
    hf = torch.cat([o1[4], o2[4]])
    from oracle.pyg_ops import to_dense_batch
    xd, _ = to_dense_batch(d.x, d.batch, float(d.x.min()) - 1)
    img = (xd * sd["prob"]).reshape(BSZ, -1)
    hr = torch.cat([torch.relu(torch.cat([o[3], img], dim=-1) @ sd["lin1_regr.weight"].t() + sd["lin1_regr.bias"])
                    for o in (o1, o2)])
    got = R.head_loss(hf, None, sd["lin2.weight"], sd["lin2.bias"], hr, None, sd["lin2_regr.weight"], sd["lin2_regr.bias"],
                      y, clin, x_hat, d.snps_feat, gram_rows, prob_rows, lam, OS.HP.lamda_ce, OS.HP.lamda_mi)
    check(got)
    assert float((got["logp"] - logp).abs().max()) <= 1e-12 and float((got["reg"] - reg).abs().max()) <= 1e-12


def _case(rng, b, k, c, nr, s, keep, bias):
    mk = lambda *sh: torch.from_numpy(rng.standard_normal(sh))                     # noqa: E731
    kp = lambda p: torch.from_numpy((rng.random((2 * b, k)) > p) / (1 - p)) if keep else None      # noqa: E731
    return dict(hf=mk(2 * b, k), keep1=kp(0.5), w2=mk(c, k) * 0.3, b2=mk(c) * 0.1 if bias else None, hr=mk(2 * b, k),
                keep2=kp(0.3), w2r=mk(nr, k) * 0.3, b2r=mk(nr) * 0.1, y=torch.from_numpy(rng.integers(0, c, b)),
                clin=torch.from_numpy(rng.random(b * nr)), x_hat=mk(2 * b, s), snps=torch.from_numpy(rng.random((b, s))),
                gram=torch.from_numpy(rng.random((4, 4))), prob=torch.from_numpy(rng.random(3)))


@pytest.mark.parametrize("lam,keep,bias", [(L_TEST, True, True), (L_MAIN, False, True), (L_TRAINER, True, False)],
                         ids=["L_TEST", "L_MAIN", "L_TRAINER"])
def test_gradients_equal_finite_differences(lam, keep, bias):
    """Every gradient head_loss_ref returns, element by element, against central differences of its own loss in float64
    on a 3-sample case (h = 1e-6: truncation ~1e-12, rounding ~1e-10 of the loss's scale; bound 1e-7), with an upstream
    gradient of 1.7, dropout factors and a missing lin2.bias; and loss_head's against the same from the scores on."""
    rng = np.random.default_rng(11)
    hp_ce, hp_mi, up, h = 1.3, 0.8, 1.7, 1e-6
    case = _case(rng, 3, 4, 2, 2, 5, keep, bias)
    order = ("hf", "keep1", "w2", "b2", "hr", "keep2", "w2r", "b2r", "y", "clin", "x_hat", "snps", "gram", "prob")

    def run(c):
        return R.head_loss(*(c[k] for k in order), lam, hp_ce, hp_mi, up)

    def fd(f, case_, name):
        base = case_[name]
        out = torch.zeros_like(base)
        for i in range(base.numel()):
            vals = []
            for sgn in (1.0, -1.0):
                moved = base.clone()
                moved.view(-1)[i] += sgn * h
                vals.append(float(f({**case_, name: moved})["loss"]))
            out.view(-1)[i] = up * (vals[0] - vals[1]) / (2 * h)
        return out

    got = run(case)
    for name, g in got["grads"].items():
        if case[name] is None:
            assert g is None
            continue
        want = fd(run, case, name)
        if g is None:                                   # the loss does not depend on the input: lam[0] == 0
            assert lam[0] == 0 and name in ("hf", "w2", "b2") and float(want.abs().max()) == 0.0, name
            continue
        assert float((g - want).abs().max()) <= 1e-7 * max(1.0, float(want.abs().max())), name
    # the second entry point, on the scores and regression outputs the first one produced
    scores = (case["hf"] * case["keep1"] if keep else case["hf"]) @ case["w2"].t() + (case["b2"] if bias else 0.0)
    lcase = dict(scores=scores, reg=got["reg"], x_hat=case["x_hat"], gram=case["gram"], prob=case["prob"])

    def run_l(c, from_logits=True):
        return R.loss_head(c["scores"], case["y"], c["reg"], case["clin"], c["x_hat"], case["snps"], c["gram"], c["prob"],
                           lam, hp_ce, hp_mi, up, from_logits)
    got_l = run_l(lcase)
    assert abs(float(got_l["loss"]) - float(got["loss"])) <= 1e-12 * max(1.0, abs(float(got["loss"])))
    for name, g in got_l["grads"].items():
        want = fd(run_l, lcase, name)
        if g is None:
            assert lam[0] == 0 and name == "scores" and float(want.abs().max()) == 0.0
            continue
        assert float((g - want).abs().max()) <= 1e-7 * max(1.0, float(want.abs().max())), name
    # log-probabilities taken as given: d nll / d logp is -weight / B at the label and nothing else
    pcase = {**lcase, "scores": got["logp"]}
    got_p = run_l(pcase, False)
    if lam[0] != 0:
        want = fd(lambda c: run_l(c, False), pcase, "scores")
        assert float((got_p["grads"]["scores"] - want).abs().max()) <= 1e-7 * max(1.0, float(want.abs().max()))
