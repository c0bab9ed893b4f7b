"""evaluate / eval_scores / Evaluator (kernel/train_eval_sgcn_img_snps.py:551-671 in one sweep per batch, metrics on the
device): against the eager eval functions and the fp64 oracle, graphed against eager, the device metrics against the
numpy restatement (tests/eval_metrics_ref.py), no trace on training, and the epoch buffers' capacity."""
import copy
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import assert_matches
from eval_metrics_ref import metrics as ref_metrics

pytestmark = pytest.mark.gpu

LAM = [1.0, 1.0, 0.5, 1.5e-6, 0.1, 0.2]
POOL = (60, 30, 20, 9, 1)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _model(num_classes=3, num_regr=3, seed=8):
    """test_eval_passes_vs_oracle's configuration."""
    from _weights import seeded_state
    from igcn_amd import synth
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=2)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    model = SGCN_GCN_IMGSNP(2, 8, a_g, a, pool_dim, 32, "cuda", rois=90, H_0=3, num_classes=num_classes,
                            isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=num_regr,
                            isuseProb4Regr=True, isImageOnly=False, isSNPsOnly=False).cuda()
    model.load_state_dict(seeded_state({k: v.shape for k, v in model.state_dict().items()}, seed))
    for mod in (model, model.go_network):
        mod._dropout_enabled = False
    return model, (go_snps, adj)


def _graphs(n=20, seed=5, num_classes=3, num_regr=3):
    from igcn_amd import synth
    return synth.brain_graph_list(n, seed=seed, rois=90, tsne_dim=16, num_classes=num_classes, num_regr=num_regr)


def _loader(graphs, bsz=8):
    from igcn_amd.data import DataLoader
    return DataLoader(graphs, batch_size=bsz)


ROWS = ("logp", "pred", "y", "reg", "clini_score", "out_lin", "linear_outf", "sbjID")


@pytest.mark.parametrize("classes,regr", [(3, 3), (2, 4)])
def test_evaluate_matches_the_eager_eval_functions_and_the_oracle(classes, regr):
    """20 graphs at batch 8: two full batches and a ragged tail (two batch shapes, the full one captured) — with three
    classes and three regression targets, and with the trainer's heads (two classes, four targets)."""
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from igcn_amd.train import eval_acc, eval_loss, eval_outputs, evaluate
    from oracle import go_network as OG, sgcn_img_snp as OS
    model, (go_snps, adj) = _model(classes, regr)
    graphs = _graphs(num_classes=classes, num_regr=regr)
    loader = _loader(graphs)
    got = evaluate(model, loader, LAM, device="cuda", num_classes=classes, num_regr=regr)
    assert got["logp"].shape == (20, classes) and got["reg"].shape == (20, regr)
    loss = eval_loss(model, loader, LAM, device="cuda")
    acc = eval_acc(model, loader, device="cuda")
    outs = eval_outputs(model, loader, device="cuda")
    assert got["n"] == 20
    assert got["loss"] == pytest.approx(loss, rel=1e-6)
    top2 = outs["logp"].topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-5
    assert torch.equal(got["pred"][clear], outs["pred"][clear])
    if bool(clear.all()):
        assert got["accuracy"] == acc
    for k, want in (("logp", "logp"), ("reg", "reg"), ("out_lin", "out_lin"), ("linear_outf", "linear_outf")):
        assert_matches(got[k], outs[want].cpu().numpy(), 1e-5, k)
    assert torch.equal(got["y"].cpu(), torch.cat([g.y.view(-1) for g in graphs]))
    assert torch.equal(got["sbjID"].cpu(), torch.arange(20))
    assert torch.equal(got["clini_score"].cpu(), torch.cat([g.clini_score.view(1, -1) for g in graphs]))
    # the fp64 oracle, as test_eval_passes_vs_oracle checks the eager functions
    from _weights import seeded_state
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, 8)
    sd = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    a_gc, a_c = synth.go_sparse_inputs(go_snps, adj)
    idx = OG.go_index_sets(a_gc, a_c, list(POOL), 2)
    cfg = SimpleNamespace(num_layers=2, rois=90, image_only=False, rbf_gamma=0.01)
    import torch.nn.functional as F
    want, logps = 0.0, []
    with torch.no_grad():
        for lo, hi in ((0, 8), (8, 16), (16, 20)):
            d = Batch.from_data_list(graphs[lo:hi])
            for k in ("x", "edge_attr", "snps_feat", "clini_score", "tsne_fdim"):
                setattr(d, k, getattr(d, k).double())
            o1 = OS.model_forward(sd, cfg, idx, d, False, training=False)
            o2 = OS.model_forward(sd, cfg, idx, d, True, training=False)
            y, clin = d.y.view(-1), d.clini_score.view(-1)
            b = LAM[0] * F.nll_loss(o1[0], y) + LAM[0] * F.nll_loss(o2[0], y) \
                + LAM[1] * (F.mse_loss(o1[5].view(-1), clin) + F.mse_loss(o2[5].view(-1), clin)) / 2 \
                + LAM[2] * OS.loss_probability(sd, d.x, d.edge_index, d.edge_attr, 90) \
                + LAM[3] * (((o1[1] - d.snps_feat) ** 2).sum() + ((o2[1] - d.snps_feat) ** 2).sum()) / 2 \
                + LAM[4] * (OS.consist_loss(o1[2], d.tsne_fdim, 0.01) + OS.consist_loss(o2[2], d.tsne_fdim, 0.01)) / 2 \
                + LAM[5] * OS.orthogonal_constraint(o1[2])
            want += float(b) * (hi - lo)
            logps.append(o1[0])
    assert abs(got["loss"] - want / 20) <= 1e-4 * max(1.0, abs(want / 20)), (got["loss"], want / 20)
    assert_matches(got["logp"], torch.cat(logps).numpy(), 1e-4, "logp vs oracle")


def test_graphed_evaluation_equals_the_eager_one():
    """The second and third evaluate replay captured graphs; rows and metrics are bitwise those of the first call."""
    from igcn_amd.train import _EVALUATORS, evaluate
    model, _ = _model(2, 4)
    loader = _loader(_graphs(num_classes=2, num_regr=4))
    runs = [evaluate(model, loader, LAM, device="cuda", num_classes=2, num_regr=4) for _ in range(3)]
    ev = next(iter(_EVALUATORS[model].values()))
    # call 1: eager, capture + replay, eager tail; call 2: replay, replay, capture + replay; call 3: replays
    assert ev.counts == {"eager": 2, "captured": 2, "replayed": 7}, ev.counts
    for r in runs[1:]:
        for k in ROWS:
            assert torch.equal(r[k], runs[0][k]), k
        for k in ("loss", "accuracy", "auc", "f1", "sensitivity", "specificity", "corr", "r2", "rmse"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(runs[0][k]), equal_nan=True), k
        assert np.array_equal(r["confusion"], runs[0]["confusion"])


@pytest.mark.parametrize("classes,regr,nan_target", [(2, 4, None), (3, 3, None), (2, 4, 2)])
def test_device_metrics_match_the_restatement(classes, regr, nan_target):
    from igcn_amd.train import eval_scores, evaluate
    model, _ = _model(classes, regr)
    if nan_target is not None:
        with torch.no_grad():
            model.lin2_regr.bias[nan_target] = float("nan")
    loader = _loader(_graphs(num_classes=classes, num_regr=regr))
    got = evaluate(model, loader, LAM, device="cuda", num_classes=classes, num_regr=regr)
    want = ref_metrics(*(got[k].cpu().numpy() for k in ("logp", "pred", "y", "reg", "clini_score")), classes)
    assert got["accuracy"] == want["accuracy"]
    assert np.array_equal(got["confusion"], want["confusion"])
    for k in ("auc", "sensitivity", "specificity"):
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, got[k], want[k])
    assert got["f1"] == pytest.approx(want["f1"], rel=1e-12)
    if classes == 2:
        assert 0.0 <= got["auc"] <= 1.0
    else:
        assert got["auc"] == got["sensitivity"] == got["specificity"] == 0.0
    for k in ("corr", "r2", "rmse"):
        for j, (g, w) in enumerate(zip(got[k], want[k])):
            assert (math.isnan(g) and math.isnan(w)) or g == pytest.approx(w, rel=1e-9, abs=1e-12), (k, j, g, w)
    if nan_target is not None:
        assert bool(torch.isnan(got["reg"][:, nan_target]).all())
        t = got["clini_score"][:, nan_target].double().cpu().numpy()
        assert math.isnan(got["corr"][nan_target])
        assert got["rmse"][nan_target] == pytest.approx(math.sqrt((t * t).mean()), rel=1e-9)
        assert got["r2"][nan_target] == pytest.approx(1 - (t * t).sum() / ((t - t.mean()) ** 2).sum(), rel=1e-9)
    # the reference's 11-tuple
    out = eval_scores(model, loader, None, LAM, None, True, "cuda", classes, regr)
    assert len(out) == 11
    assert np.array_equal(out[0], got["y"].cpu().numpy()) and np.array_equal(out[1], got["pred"].cpu().numpy())
    assert out[2] == got["accuracy"] and np.array_equal(out[3], got["auc"], equal_nan=True)
    assert torch.equal(out[7], got["out_lin"].cpu()) and torch.equal(out[8], got["sbjID"].cpu())
    assert torch.equal(out[9], got["linear_outf"].cpu())
    true_clin, pred_clin, corr, r2, rmse = out[10]
    assert np.array_equal(np.asarray(true_clin, np.float32), got["clini_score"].cpu().numpy())
    assert not np.isnan(np.asarray(pred_clin)).any() and np.array_equal(corr, got["corr"], equal_nan=True)


def test_evaluation_leaves_no_trace_on_training():
    """Three epochs of fit_epoch with evaluate in between = three epochs without it, bit for bit."""
    from igcn_amd import train
    from igcn_amd.train import FlatAdam, evaluate, fit_epoch
    m1, _ = _model()
    m2 = copy.deepcopy(m1)
    m1.train()
    m2.train()
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    train_loader = _loader(_graphs(20, seed=11))
    eval_loader = _loader(_graphs(20, seed=12))
    for epoch in range(3):
        l1 = fit_epoch(m1, o1, train_loader, None, LAM, device="cuda")
        l2 = fit_epoch(m2, o2, train_loader, None, LAM, device="cuda")
        assert l1 == l2, (epoch, l1, l2)
        rng, table = torch.cuda.get_rng_state(), o1.table.clone()
        evaluate(m1, eval_loader, LAM, device="cuda")
        assert torch.equal(torch.cuda.get_rng_state(), rng) and torch.equal(o1.table, table)
        assert m1.training and m1._handoff.reg is None
        assert train.stream_pending() == 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1, p2), k
    for (k, b1), (_, b2) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(b1, b2), k
    for a, b in ((o1.exp_avg, o2.exp_avg), (o1.exp_avg_sq, o2.exp_avg_sq), (o1.step_count, o2.step_count)):
        assert torch.equal(a, b)


def test_buffers_regrow_and_overflow_raises():
    from igcn_amd import _lib
    from igcn_amd.train import HP, Evaluator, eval_loss
    model, _ = _model()
    ev = Evaluator(model, LAM, HP)
    small, large = _loader(_graphs(20)), _loader(_graphs(28, seed=6))
    ev.evaluate(small, "cuda")
    ev.evaluate(small, "cuda")
    assert ev.capacity == 20 and ev.counts["captured"] == 2
    got = ev.evaluate(large, "cuda")                        # 28 rows: the buffers grow, the graphs are captured anew
    assert ev.capacity == 28 and got["n"] == 28
    assert torch.equal(got["sbjID"].cpu(), torch.arange(28))
    assert got["loss"] == pytest.approx(eval_loss(model, large, LAM, device="cuda"), rel=1e-6)
    fixed = Evaluator(model, LAM, HP, capacity=12)
    with pytest.raises(_lib.IgcnError, match="do not fit"):
        fixed.evaluate(small, "cuda")                       # rows 0..7 fit, the second batch of 8 does not
    state = fixed.state.cpu().tolist()
    assert state[0] == 8 and state[1] == 1
    assert fixed.rows["logp"].shape == (12, 3)
    for k in ROWS:
        assert not bool(fixed.rows[k][8:].ne(0).any()), k  # the tail batch of 4 (it would fit) wrote nothing either


def test_graphs_are_recaptured_when_the_model_storage_moves():
    """evaluate captures its graphs on the model's storage; FlatAdam then re-binds every parameter into its flat buffer.
    The next evaluate must not replay graphs that read the old storage: it matches the eager functions on the trained
    weights."""
    from igcn_amd.train import _EVALUATORS, FlatAdam, eval_loss, eval_outputs, evaluate, fit_epoch
    model, _ = _model()
    loader = _loader(_graphs())
    before = [evaluate(model, loader, LAM, device="cuda") for _ in range(2)]
    ev = next(iter(_EVALUATORS[model].values()))
    assert ev.counts["captured"] == 2
    opt = FlatAdam(model.parameters(), lr=1e-2)
    model.train()
    fit_epoch(model, opt, _loader(_graphs(20, seed=11)), None, LAM, device="cuda")
    got = evaluate(model, loader, LAM, device="cuda")
    # the old graphs are dropped: each shape is met afresh (eager, then captured at its second sighting: the second
    # full batch of this very call)
    assert ev.counts["captured"] == 3
    assert got["loss"] != before[0]["loss"]
    assert got["loss"] == pytest.approx(eval_loss(model, loader, LAM, device="cuda"), rel=1e-6)
    outs = eval_outputs(model, loader, device="cuda")
    for k in ("logp", "reg", "out_lin", "linear_outf"):
        assert_matches(got[k], outs[k].cpu().numpy(), 1e-5, k)
    again = evaluate(model, loader, LAM, device="cuda")     # replays, and the tail's capture, on the new storage
    assert ev.counts["captured"] == 4
    for k in ROWS:
        assert torch.equal(again[k], got[k]), k


@pytest.mark.parametrize("n,C,case", [(1000, 2, "ties"), (700, 2, "absent"), (257, 2, "nan_score"), (1000, 3, "ties"),
                                      (513, 3, "plain")])
def test_metrics_kernel_on_many_rows(n, C, case):
    """igcn_eval_metrics alone on synthetic device rows: several AUC workgroups and LDS tiles, the partials summed over
    workgroups, the strided fp64 sums past 256 rows; tied scores, an absent class, a NaN score."""
    from igcn_amd._lib import call, ptr, stream_ptr
    from test_eval_metrics import _case
    NR = 3
    logp, pred, y, reg, clin = _case(n, n, C, NR, ties=(case == "ties"), absent=(1 if case == "absent" else None),
                                     constant=(1,), nan_pred=(2,))
    if case == "nan_score":
        logp[n // 2, 1] = np.nan
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()           # noqa: E731
    t = {k: dev(v) for k, v in (("logp", logp), ("pred", pred), ("y", y), ("reg", reg), ("clin", clin))}
    correct = int((pred == y).sum())
    state = torch.tensor([n, 0, correct], dtype=torch.int64, device="cuda")
    loss_sum = torch.tensor([1.25 * n], dtype=torch.float64, device="cuda")
    parts = torch.full((2 * ((n + 255) // 256),), -1, dtype=torch.int64, device="cuda")

    def run():
        out = torch.full((8 + 3 * NR + C * C,), -7.0, dtype=torch.float64, device="cuda")
        call("igcn_eval_metrics", n, C, NR, ptr(t["logp"]), ptr(t["pred"]), ptr(t["y"]), ptr(t["reg"]), ptr(t["clin"]),
             ptr(state), ptr(loss_sum), ptr(parts), ptr(out), stream_ptr())
        return out.cpu().numpy()
    v = run()
    assert np.array_equal(v, run(), equal_nan=True)                            # bitwise reproducible
    want = ref_metrics(logp, pred, y, reg, clin, C)
    assert v[0] == n and v[1] == 0 and v[2] == 1.25 and v[3] == want["accuracy"]
    assert np.array_equal(v[8 + 3 * NR:].reshape(C, C).astype(np.int64), want["confusion"])
    for j, k in ((4, "auc"), (6, "sensitivity"), (7, "specificity")):
        assert np.array_equal(v[j], want[k], equal_nan=True), (k, v[j], want[k])
    if C == 2:
        assert {"ties": lambda a: 0 < a < 1, "absent": math.isnan, "nan_score": lambda a: a == 0.0}[case](v[4]), v[4]
    assert v[5] == pytest.approx(want["f1"], rel=1e-12)
    for j, k in enumerate(("corr", "r2", "rmse")):
        for i in range(NR):
            g, w = v[8 + j * NR + i], want[k][i]
            assert (math.isnan(g) and math.isnan(w)) or g == pytest.approx(w, rel=1e-9, abs=1e-12), (k, i, g, w)
