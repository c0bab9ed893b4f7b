"""The numpy restatement of igcn_eval_metrics (tests/eval_metrics_ref.py) against the sklearn / scipy calls of the
reference's eval_scores (kernel/train_eval_sgcn_img_snps.py:633-667), on cases with ties, an absent class, constant
targets, NaN predictions and 2 or 3 classes."""
import math
import warnings

import numpy as np
import pytest

from eval_metrics_ref import metrics


def _reference(logp, pred, y, reg, clin, num_classes):
    """eval_scores :633-667, with root_mean_squared_error for mean_squared_error(squared=False)."""
    sk = pytest.importorskip("sklearn.metrics")
    stats = pytest.importorskip("scipy.stats")
    rmse_fn = getattr(sk, "root_mean_squared_error", None) or (lambda a, b: sk.mean_squared_error(a, b, squared=False))
    out = {"auc": 0.0, "sensitivity": 0.0, "specificity": 0.0}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if num_classes < 3:
            try:
                fpr, tpr, _ = sk.roc_curve(y, logp[:, 1], pos_label=1)
                out["auc"] = sk.auc(fpr, tpr)
            except Exception:      # noqa: BLE001 — the reference's bare except
                out["auc"] = 0
            tn, fp, fn, tp = sk.confusion_matrix(y, pred, labels=[0, 1]).ravel()
            out["sensitivity"] = tp / (tp + fn) if tp + fn else float("nan")
            out["specificity"] = tn / (tn + fp) if tn + fp else float("nan")
        out["f1"] = sk.f1_score(y, pred, average="weighted")
        # (the reference hands scipy float32 arrays, which it reduces in float32; the definition is checked in fp64)
        pred_reg = reg.astype(np.float64)
        pred_reg[np.isnan(pred_reg)] = 0
        clin = clin.astype(np.float64)
        out["corr"] = [stats.pearsonr(clin[:, k], pred_reg[:, k])[0] for k in range(clin.shape[1])]
        out["r2"] = [sk.r2_score(clin[:, k], pred_reg[:, k]) for k in range(clin.shape[1])]
        out["rmse"] = [rmse_fn(clin[:, k], pred_reg[:, k]) for k in range(clin.shape[1])]
    out["accuracy"] = float((pred == y).mean())
    out["confusion"] = sk.confusion_matrix(y, pred, labels=list(range(num_classes)))
    return out


def _same(a, b, rel):
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= rel * max(1.0, abs(b))


def _case(seed, n, C, NR, ties=False, absent=None, constant=(), nan_pred=()):
    rng = np.random.default_rng(seed)
    logits = rng.normal(size=(n, C)).astype(np.float32)
    if ties:
        logits = np.round(logits * 2) / 2                          # few distinct scores: many tied pairs
    logp = (logits - np.log(np.exp(logits).sum(1, keepdims=True))).astype(np.float32)
    pred = logp.argmax(1).astype(np.int64)
    y = rng.integers(C, size=n).astype(np.int64)
    if absent is not None:
        y[y == absent] = (absent + 1) % C
    clin = rng.normal(size=(n, NR)).astype(np.float32)
    reg = (0.5 * clin + rng.normal(size=(n, NR))).astype(np.float32)
    for k in constant:
        clin[:, k] = 2.5                                           # exactly representable: sklearn's SS_tot is 0 too
    for k in nan_pred:
        reg[rng.integers(n, size=3), k] = np.nan
    return logp, pred, y, reg, clin


CASES = [dict(seed=1, n=40, C=2, NR=4), dict(seed=2, n=57, C=2, NR=4, ties=True), dict(seed=3, n=30, C=2, NR=2, absent=1),
         dict(seed=4, n=30, C=2, NR=2, absent=0), dict(seed=5, n=64, C=3, NR=3), dict(seed=6, n=50, C=3, NR=3, ties=True),
         dict(seed=7, n=33, C=2, NR=4, constant=(1,), nan_pred=(2,)), dict(seed=8, n=25, C=3, NR=3, absent=2,
                                                                           constant=(0,), nan_pred=(0, 1))]


@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_restatement_matches_sklearn_and_scipy(case):
    logp, pred, y, reg, clin = _case(**case)
    got = metrics(logp, pred, y, reg, clin, case["C"])
    want = _reference(logp, pred, y, reg, clin, case["C"])
    assert got["accuracy"] == want["accuracy"]
    assert np.array_equal(got["confusion"], want["confusion"])
    for k in ("auc", "f1", "sensitivity", "specificity"):
        assert _same(got[k], want[k], 1e-12), (k, got[k], want[k])
    for k in ("corr", "r2", "rmse"):
        for j, (g, w) in enumerate(zip(got[k], want[k])):
            assert _same(g, w, 1e-9), (k, j, g, w)


def test_constant_and_nan_rules():
    """The edge rules the device follows: constant target -> corr NaN, r2 1.0 / 0.0; all-NaN predictions -> zeros."""
    logp, pred, y, reg, clin = _case(9, 20, 2, 3)
    clin[:, 0] = 1.0
    reg[:, 0] = 1.0                                                # perfect constant prediction: SS_res = 0
    reg[:, 1] = np.nan                                             # -> all zero: constant prediction
    got = metrics(logp, pred, y, reg, clin, 2)
    assert math.isnan(got["corr"][0]) and got["r2"][0] == 1.0 and got["rmse"][0] == 0.0
    t = clin[:, 1].astype(np.float64)
    assert math.isnan(got["corr"][1])
    assert got["rmse"][1] == pytest.approx(math.sqrt((t * t).mean()), rel=1e-12)
    assert got["r2"][1] == pytest.approx(1 - (t * t).sum() / ((t - t.mean()) ** 2).sum(), rel=1e-12)
    clin[:, 2] = 3.0
    assert metrics(logp, pred, y, reg, clin, 2)["r2"][2] == 0.0     # constant target, imperfect prediction
