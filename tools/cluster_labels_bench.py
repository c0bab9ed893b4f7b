#!/usr/bin/env python3
"""Cost of the cluster-label pipeline (util/image_cluster.py:148-282 ``run_cluster_ADNI874``) on the device:
``cluster_labels.TSNE.fit_transform`` — captured blocks of 50 iterations, and the same launches eagerly — and
``cluster_labels.KMeans.fit`` on the embedding.

Workload: S = 874 subjects, D = 270 synthetic features (two loose groups, standardised columns), perplexity 40, the full
1000 iterations, k = 2 with k-means++ from random_state 1000.  Per block one whole call, wall clock including its
synchronisations (a fit reads its status record every 50 iterations; KMeans reads three numbers per iteration); median,
minimum and maximum of ``--blocks`` blocks after one warm-up call.  Beside it, in the same process and where sklearn
imports (``null`` otherwise), the wall time of sklearn's two calls on the host, ``--sklearn-blocks`` times.  The final KL
divergences are recorded side by side; the descents are chaotic and need not agree.  Nothing here is a pass / fail
threshold.

Prints one line per number and, with ``--out FILE``, writes them as JSON.  Run under a time limit, e.g.
    timeout -k 10 600 python tools/cluster_labels_bench.py --out profiles/cluster_labels_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBJECTS, D, PERPLEXITY, K, SEED = 874, 270, 40.0, 2, 1000


def _spread(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "blocks": [round(x, digits) for x in v]}


def _timed(fn, blocks, sync):
    out = []
    for _ in range(blocks):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="write the numbers as JSON to this file")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--sklearn-blocks", type=int, default=5, help="0: leave sklearn out")
    args = ap.parse_args()
    if args.blocks < 5:
        ap.error("--blocks: at least five timed blocks")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import igcn_amd  # noqa: F401  (import shim: the package directory is ``ig-gcn_amd/``)
    from igcn_amd import _lib, cluster_labels as CL
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_labels_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    x = rng.normal(size=(SUBJECTS, D)) + 0.6 * rng.normal(size=(2, D))[rng.integers(2, size=SUBJECTS)]
    x = ((x - x.mean(0)) / x.std(0)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    sync = torch.cuda.synchronize

    runs = {}

    def fit(captured):
        t = CL.TSNE(perplexity=PERPLEXITY, captured=captured)
        runs[captured] = (t, t.fit_transform(xd))

    fit(True)                                                  # warm-up: code objects, allocator
    cap_ms = _timed(lambda: fit(True), args.blocks, sync)
    fit(False)
    eager_ms = _timed(lambda: fit(False), args.blocks, sync)
    tsne, emb = runs[True]
    same = bool(torch.equal(emb, runs[False][1]))
    km = CL.KMeans(n_clusters=K, random_state=SEED).fit(emb)
    km_ms = _timed(lambda: CL.KMeans(n_clusters=K, random_state=SEED).fit(emb), args.blocks, sync)

    sk_tsne, sk_km, sk_kl, sk_iter, agree = None, None, None, None, None
    try:
        from sklearn.cluster import KMeans
        from sklearn.manifold import TSNE
    except ImportError:
        TSNE = None
    if TSNE is not None and args.sklearn_blocks > 0:
        host = {}

        def sk_fit():
            t = TSNE(n_components=2, perplexity=PERPLEXITY, init="pca", learning_rate="auto", method="exact",
                     random_state=SEED)
            host["emb"], host["tsne"] = t.fit_transform(x), t

        def sk_kmeans():
            host["km"] = KMeans(n_clusters=K, init="k-means++", random_state=SEED).fit(host["emb"])

        sk_tsne = _spread(_timed(sk_fit, args.sklearn_blocks, lambda: None), 1)
        sk_km = _spread(_timed(sk_kmeans, args.sklearn_blocks, lambda: None), 3)
        sk_kl, sk_iter = float(host["tsne"].kl_divergence_), int(host["tsne"].n_iter_)
        ours, theirs = km.labels_.cpu().numpy(), host["km"].labels_
        agree = float(max((ours == theirs).mean(), (ours != theirs).mean()))          # up to the naming of two clusters

    res = {"workload": dict(subjects=SUBJECTS, features=D, perplexity=PERPLEXITY, max_iter=1000, clusters=K,
                            random_state=SEED),
           "tsne_fit_transform_captured_wall_ms": _spread(cap_ms),
           "tsne_fit_transform_eager_wall_ms": _spread(eager_ms),
           "captured_equals_eager_bits": same,
           "kmeans_fit_wall_ms": _spread(km_ms),
           "device_kl_divergence": tsne.kl_divergence_, "device_n_iter": tsne.n_iter_,
           "device_kmeans": dict(n_iter=km.n_iter_, inertia=km.inertia_,
                                 sizes=torch.bincount(km.labels_, minlength=K).tolist()),
           "sklearn_tsne_host_wall_ms": sk_tsne, "sklearn_kmeans_host_wall_ms": sk_km,
           "sklearn_kl_divergence": sk_kl, "sklearn_n_iter": sk_iter,
           "labels_agreeing_with_sklearn": agree,
           "host_threads": os.cpu_count() if "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"]),
           "device": torch.cuda.get_device_name(0),
           "timing": (f"wall clock of one whole call per block, synchronisations included, one warm-up call, median / min "
                      f"/ max of {args.blocks} blocks (sklearn: {args.sklearn_blocks})")}
    c, e, k = (res[n] for n in ("tsne_fit_transform_captured_wall_ms", "tsne_fit_transform_eager_wall_ms",
                                "kmeans_fit_wall_ms"))
    print(f"TSNE.fit_transform: captured {c['median']:.1f} ms ({c['min']:.1f} .. {c['max']:.1f}), eager {e['median']:.1f} ms "
          f"({e['min']:.1f} .. {e['max']:.1f}); KMeans.fit {k['median']:.3f} ms ({k['min']:.3f} .. {k['max']:.3f})", flush=True)
    print(f"sklearn on the host: TSNE {sk_tsne['median'] if sk_tsne else None} ms, KMeans "
          f"{sk_km['median'] if sk_km else None} ms; KL device {tsne.kl_divergence_:.4f} / sklearn {sk_kl}", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
