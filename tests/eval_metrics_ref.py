"""numpy fp64 restatement of igcn_eval_metrics (include/igcn.h): the metrics eval_scores computes with sklearn / scipy
(kernel/train_eval_sgcn_img_snps.py:633-667), as the device defines them.  tests/test_eval_metrics.py checks it against
sklearn / scipy; tests/test_gpu_eval.py checks the device against it."""
import numpy as np


def metrics(logp, pred, y, reg, clin, num_classes):
    """dict of accuracy, auc, f1, sensitivity, specificity, confusion [C, C], corr / r2 / rmse (lists, one per target)."""
    logp = np.asarray(logp, np.float32).reshape(len(y), -1)
    pred, y = np.asarray(pred, np.int64), np.asarray(y, np.int64)
    reg = np.asarray(reg, np.float32).reshape(len(y), -1)
    clin = np.asarray(clin, np.float32).reshape(len(y), -1)
    n, C = len(y), int(num_classes)
    cm = np.zeros((C, C), np.int64)
    for t, p in zip(y, pred):
        if 0 <= t < C and 0 <= p < C:
            cm[t, p] += 1
    out = {"accuracy": float((pred == y).sum()) / n, "confusion": cm, "auc": 0.0, "sensitivity": 0.0,
           "specificity": 0.0}
    if C == 2:
        # roc_curve + auc (:633-638) = the Mann-Whitney statistic, ties counted 1/2; NaN scores: sklearn raises, the
        # reference's except gives 0
        s = logp[:, 1]
        pos, neg = s[y == 1], s[y != 1]
        if np.isnan(s).any():
            out["auc"] = 0.0
        elif len(pos) == 0 or len(neg) == 0:
            out["auc"] = float("nan")
        else:
            cnt = 2 * int((pos[:, None] > neg[None, :]).sum()) + int((pos[:, None] == neg[None, :]).sum())
            out["auc"] = cnt / (2.0 * len(pos) * len(neg))
        tn, fp, fn, tp = (float(v) for v in cm.ravel())
        out["sensitivity"] = tp / (tp + fn) if tp + fn else float("nan")
        out["specificity"] = tn / (tn + fp) if tn + fp else float("nan")
    # f1_score(average='weighted') (:662): labels = union of true and predicted, 0 where precision or recall is 0 / 0
    f1, wsum = 0.0, 0.0
    for lab in range(C):
        sup, prd, tp = int(cm[lab].sum()), int(cm[:, lab].sum()), float(cm[lab, lab])
        if sup + prd == 0:
            continue
        f1 += (2.0 * tp / (sup + prd) if tp else 0.0) * sup
        wsum += sup
    out["f1"] = f1 / wsum if wsum else 0.0
    # :646-655 — predictions' NaN -> 0; pearsonr, r2_score (force_finite), RMSE
    corr, r2, rmse = [], [], []
    for k in range(clin.shape[1]):
        t = clin[:, k].astype(np.float64)
        p = np.where(np.isnan(reg[:, k]), np.float32(0), reg[:, k]).astype(np.float64)
        const_t, const_p = bool((t == t[0]).all()), bool((p == p[0]).all())
        a, b = t - t.sum() / n, p - p.sum() / n
        sxx, syy, sxy, ssr = (a * a).sum(), (b * b).sum(), (a * b).sum(), ((t - p) ** 2).sum()
        corr.append(float("nan") if (n < 2 or const_t or const_p) else float(np.clip(sxy / np.sqrt(sxx * syy), -1, 1)))
        sstot = 0.0 if const_t else sxx
        r2.append((1.0 if ssr == 0 else 0.0) if sstot == 0 else float(1.0 - ssr / sstot))
        rmse.append(float(np.sqrt(ssr / n)))
    out.update(corr=corr, r2=r2, rmse=rmse)
    return out
