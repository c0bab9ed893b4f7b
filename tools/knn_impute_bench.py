#!/usr/bin/env python3
"""Cost of one fold's preparation of the clinical scores (util/tool.py:22-73 ``KNNImputationVal``) on the device:
``impute.impute_store`` on a device-resident ``UniformGraphStore`` — the column statistics of the training rows and one
transform per split, written into the store's ``clini_score`` in place.

Workload: one fold of an 874-subject cohort (5 folds: 175 test / 175 validation / 524 training subjects), F = 9
demographics, k = 3, about 15 % of the entries missing, columns [5, 7, 8] selected behind a MinMaxScaler-shaped affine.
Per block, device events around ``--steps`` hot calls and the wall clock around the same calls including the final
synchronisation (``impute_store`` itself reads the per-column counts back once per call: the fit's refusal of an
unobserved column); median, minimum and maximum of ``--blocks`` blocks after a warm-up.  Beside it, in the same process,
the wall time of the reference-signature wrapper ``impute.KNNImputationVal`` on lists of ``Data`` and — where sklearn
imports, ``null`` otherwise — of sklearn's ``KNNImputer`` + the scaler + the selection on the host (the numpy part of
the reference's function, without its Python loops over ``Data`` objects).  Nothing here is a pass / fail threshold.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run under a time limit, e.g.
    timeout -k 10 300 python tools/knn_impute_bench.py --out profiles/knn_impute_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBJECTS, FOLDS, F, K, MISSING = 874, 5, 9, 3, 0.15
SELECT = (5, 7, 8)


def _spread(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "blocks": [round(x, digits) for x in v]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks: at least five timed blocks")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import igcn_amd  # noqa: F401  (import shim: the package directory is ``ig-gcn_amd/``)
    from igcn_amd import _lib, impute
    from igcn_amd.data import Data
    from igcn_amd.loader import UniformGraphStore
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("knn_impute_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    demo = rng.random((SUBJECTS, F)) * np.linspace(0.5, 30.0, F)
    demo[rng.random((SUBJECTS, F)) < MISSING] = np.nan
    demo = demo.astype(np.float32)
    perm = rng.permutation(SUBJECTS)
    n_test = SUBJECTS // FOLDS + 1                              # 175
    test_idx, val_idx, train_idx = perm[:n_test], perm[n_test:2 * n_test], np.sort(perm[2 * n_test:])
    scaler = SimpleNamespace(scale_=1.0 / np.nanmax(demo, axis=0).astype(np.float64), min_=np.zeros(F))
    graphs = [Data(x=torch.zeros(2, 1), edge_index=torch.zeros(2, 1, dtype=torch.long),
                   demographics=torch.from_numpy(demo[i]), clini_score=torch.zeros(len(SELECT))) for i in range(SUBJECTS)]
    store = UniformGraphStore(graphs, device=dev)
    scale, shift = impute.affine_of(scaler, dev)
    ti, vi, si = (torch.from_numpy(i).to(dev) for i in (train_idx, val_idx, test_idx))

    def on_store():
        return impute.impute_store(store, ti, vi, si, scale, shift, SELECT, K)

    for _ in range(3):                                         # warm-up: code objects, allocator
        fb = on_store()
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(args.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.steps):
            on_store()
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1) / args.steps)
        wall_ms.append((time.perf_counter() - t0) * 1e3 / args.steps)

    lists = [[graphs[i] for i in idx] for idx in (train_idx, val_idx, test_idx)]
    ns = SimpleNamespace(clinical_score_index=-1)
    impute.KNNImputationVal(ns, lists[0], lists[1], lists[2], scaler, k=K)
    wrap_ms = []
    for _ in range(args.blocks):
        t0 = time.perf_counter()
        impute.KNNImputationVal(ns, lists[0], lists[1], lists[2], scaler, k=K)
        wrap_ms.append((time.perf_counter() - t0) * 1e3)
    got = torch.stack([g.clini_score for g in lists[2]])
    same = bool(torch.equal(got, store.cols["clini_score"][si].cpu()))

    sk_ms, sk_err = None, None
    try:
        from sklearn.impute import KNNImputer
    except ImportError:
        KNNImputer = None
    if KNNImputer is not None:
        def on_host():
            imp = KNNImputer(n_neighbors=K)
            parts = [imp.fit_transform(demo[train_idx]), imp.transform(demo[val_idx]), imp.transform(demo[test_idx])]
            return [(p * scaler.scale_ + scaler.min_)[:, list(SELECT)] for p in parts]
        on_host()
        sk = []
        for _ in range(args.blocks):
            t0 = time.perf_counter()
            host = on_host()
            sk.append((time.perf_counter() - t0) * 1e3)
        sk_ms = _spread(sk, 3)
        sk_err = float(np.abs(host[2] - store.cols["clini_score"][si].cpu().double().numpy()).max())

    res = {"workload": dict(subjects=SUBJECTS, folds=FOLDS, train=len(train_idx), val=len(val_idx), test=len(test_idx),
                            columns=F, k=K, missing_fraction=round(float(np.isnan(demo).mean()), 4), select=list(SELECT)),
           "impute_store_device_ms": _spread(dev_ms),
           "impute_store_wall_ms": _spread(wall_ms),
           "fallbacks_train_val_test": [int(t) for t in fb],
           "KNNImputationVal_lists_wall_ms": _spread(wrap_ms, 3),
           "lists_equal_store_bits": same,
           "sklearn_host_wall_ms": sk_ms,
           "max_abs_difference_from_sklearn_test_split": sk_err,
           "device": torch.cuda.get_device_name(0),
           "timing": (f"eager calls; device events and wall clock (with the closing synchronisation) around {args.steps} hot "
                      f"calls per block, 3 warm-up calls, median / min / max of {args.blocks} blocks; the list wrapper and "
                      "sklearn: wall clock of one call per block")}
    d, wl = res["impute_store_device_ms"], res["impute_store_wall_ms"]
    print(f"impute_store: {d['median']:.4f} ms on the device ({d['min']:.4f} .. {d['max']:.4f}), {wl['median']:.4f} ms wall",
          flush=True)
    print(f"KNNImputationVal on lists: {res['KNNImputationVal_lists_wall_ms']['median']:.3f} ms wall; sklearn on the host: "
          f"{sk_ms['median'] if sk_ms else None} ms wall", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
