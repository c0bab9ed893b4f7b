"""Wall time of one epoch of the reference's loop (kernel/train_eval_sgcn_img_snps.py:123-132) at B = 32, with the
evaluation done two ways:

  (a) eager  fit_epoch, eval_loss(val), eval_loss(test), eval_acc(test), eval_outputs(test), and the sklearn / scipy
             metrics of eval_scores (:633-667) when sklearn is importable;
  (b) graphed  fit_epoch, evaluate(val), evaluate(test), eval_scores_of(test): the loop of INTEGRATION.md §2, one
             captured sweep per batch, metrics on the device, the eval_scores tuple built from the test sweep.

Data: 874 seeded synthetic subjects (synth.brain_graph_list), split 60/20/20; model: bench.py's ``full`` configuration.
Both forms train their own copy of the same model; they alternate epoch by epoch after warm-up epochs, and each epoch is
timed on the host around work that ends in a device synchronise.  Prints one JSON line: median and spread (min, max) of
the epoch time of each form and of its evaluation part.

Usage: python tools/eval_epoch_bench.py [--epochs 5] [--warmup 2] [--subjects 874] [--batch 32]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import igcn_amd  # noqa: E402,F401
from igcn_amd import synth  # noqa: E402
from igcn_amd.data import DataLoader  # noqa: E402
from igcn_amd.train import (DEFAULT_LAMBDA, FlatAdam, eval_acc, eval_loss, eval_outputs, eval_scores_of,  # noqa: E402
                            evaluate, fit_epoch)


def _sklearn_metrics(outs, loader, num_regr):
    """The host part of eval_scores (:633-667) on eval_outputs' tensors; None when sklearn / scipy are missing."""
    try:
        import numpy as np
        from scipy.stats import pearsonr
        from sklearn import metrics
    except ImportError:
        return None
    y = torch.cat([d.y.view(-1) for d in loader]).numpy()
    clin = torch.cat([d.clini_score.view(-1, num_regr) for d in loader]).numpy()
    logp, pred, reg = outs["logp"].cpu().numpy(), outs["pred"].cpu().numpy(), outs["reg"].cpu().numpy()
    reg[np.isnan(reg)] = 0
    try:
        fpr, tpr, _ = metrics.roc_curve(y, logp[:, 1], pos_label=1)
        metrics.auc(fpr, tpr)
    except Exception:             # noqa: BLE001 — the reference's bare except
        pass
    for k in range(num_regr):
        pearsonr(clin[:, k], reg[:, k])
        metrics.r2_score(clin[:, k], reg[:, k])
        np.sqrt(metrics.mean_squared_error(clin[:, k], reg[:, k]))
    metrics.f1_score(y, pred, average="weighted")
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5, help="timed epochs per form")
    ap.add_argument("--warmup", type=int, default=2, help="untimed epochs per form first")
    ap.add_argument("--subjects", type=int, default=874)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_epoch_bench: needs a GPU")
    sys.path.insert(0, ROOT)
    import bench
    dev = torch.device("cuda", 0)
    graphs = synth.brain_graph_list(args.subjects, seed=1000, rois=bench.ROIS, tsne_dim=90)
    n_tr, n_va = int(0.6 * len(graphs)), int(0.2 * len(graphs))
    train_l = DataLoader(graphs[:n_tr], args.batch, shuffle=False)
    val_l = DataLoader(graphs[n_tr:n_tr + n_va], args.batch)
    test_l = DataLoader(graphs[n_tr + n_va:], args.batch)
    base, _ = bench.build_model(dev)
    models = {"eager": base, "graphed": copy.deepcopy(base)}
    opts = {k: FlatAdam(m.parameters(), lr=1e-3) for k, m in models.items()}
    nr = base.lin2_regr.weight.shape[0]
    sk = [None]

    def epoch(form):
        m, o = models[form], opts[form]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit_epoch(m, o, train_l, None, DEFAULT_LAMBDA, device=dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if form == "eager":
            eval_loss(m, val_l, DEFAULT_LAMBDA, device=dev)
            eval_loss(m, test_l, DEFAULT_LAMBDA, device=dev)
            eval_acc(m, test_l, device=dev)
            outs = eval_outputs(m, test_l, device=dev)
            sk[0] = _sklearn_metrics(outs, test_l, nr)
        else:
            evaluate(m, val_l, DEFAULT_LAMBDA, device=dev)
            eval_scores_of(evaluate(m, test_l, DEFAULT_LAMBDA, device=dev))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3

    for _ in range(args.warmup):
        for form in models:
            epoch(form)
    times = {form: [] for form in models}
    for _ in range(args.epochs):
        for form in models:
            times[form].append(epoch(form))

    def stats(v):
        return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    out = {"metric": "eval_epoch_ms", "subjects": len(graphs), "batch": args.batch,
           "split": [len(train_l.dataset), len(val_l.dataset), len(test_l.dataset)], "epochs": args.epochs,
           "warmup": args.warmup, "sklearn_metrics": bool(sk[0])}
    for form, v in times.items():
        out[form] = {"epoch_ms": stats([a for a, _ in v]), "eval_ms": stats([b for _, b in v])}
    out["eval_speedup"] = round(out["eager"]["eval_ms"]["median"] / out["graphed"]["eval_ms"]["median"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
