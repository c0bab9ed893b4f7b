"""Writes tests/golden/cluster_labels.npz: what the installed sklearn computes for the cases of
tests/cluster_labels_ref.py — _joint_probabilities, _kl_divergence, KMeans from a given init, kmeans_plusplus — so that the
restatements are held to sklearn where it is not installed too.  Run from the repository root:
    python tests/golden/make_cluster_labels_golden.py"""
import os
import sys

import numpy as np
import sklearn
from scipy.spatial.distance import squareform
from sklearn.cluster import KMeans, kmeans_plusplus
from sklearn.manifold import _t_sne

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cluster_labels_ref as R  # noqa: E402

GOLDEN_P = [(7, 3), (64, 5), (65, 12)]             # (the condensed P of the larger shapes would not fit a small file)
KPP_CASES = [((96, 2, 3), 3), ((300, 7, 5), 5), ((300, 7, 5), 16), ((65, 270, 2), 2)]
KPP_SEEDS = (0, 1, 2, 1000)


def sklearn_schedule(shape):
    """The embedding after R.SCHEDULE_ITERS iterations of sklearn's schedule from the case's start, with the exploration
    phase cut to R.SCHEDULE_EXPLORATION iterations (the descent doubles a rounding difference about every iteration, so
    only a short run can be compared): _gradient_descent on _kl_divergence with the exaggerated P and momentum 0.5, then
    again with momentum 0.8 — the two calls of TSNE._tsne, with the stopping rules switched off."""
    s, _ = shape
    case = R.tsne_case(shape)
    pc = squareform(case["P"], checks=False)
    kw = dict(n_iter_check=50, n_iter_without_progress=10 ** 6, min_grad_norm=0.0, learning_rate=case["lr"], verbose=0,
              kwargs={"skip_num_points": 0})
    p0 = case["states"][0][0].ravel().copy()
    p1, _, it = _t_sne._gradient_descent(_t_sne._kl_divergence, p0, it=0, max_iter=R.SCHEDULE_EXPLORATION, momentum=0.5,
                                         args=[12.0 * pc, 1.0, s, 2], **kw)
    p2, _, it = _t_sne._gradient_descent(_t_sne._kl_divergence, p1, it=it + 1, max_iter=R.SCHEDULE_ITERS, momentum=0.8,
                                         args=[pc, 1.0, s, 2], **kw)
    assert it == R.SCHEDULE_ITERS - 1
    return p2.reshape(s, 2)


def main():
    store = {"sklearn_version": np.array(sklearn.__version__)}
    for shape in R.TSNE_SHAPES:
        s, d = shape
        case = R.tsne_case(shape)
        dist = R.f32(R.sqdist_ref(case["x"]))
        for perp in R.perplexities(s) if shape in GOLDEN_P else ():
            store[f"P/{s}x{d}/{perp}"] = _t_sne._joint_probabilities(dist, perp, 0)
        pc = squareform(case["P"], checks=False)
        for it, (y, _, _) in case["states"].items():
            for e in (12.0, 1.0):
                kl, grad = _t_sne._kl_divergence(y.ravel(), e * pc, 1.0, s, 2)
                store[f"grad/{s}x{d}/{it}/{e}"] = grad.reshape(s, 2)
                store[f"kl/{s}x{d}/{it}/{e}"] = np.array(kl)
    for shape in R.SCHEDULE_SHAPES:                 # sklearn's own two _gradient_descent calls, as TSNE._tsne makes them
        store[f"run/{shape[0]}x{shape[1]}"] = sklearn_schedule(shape)
    for n, d, k in R.KMEANS_SHAPES:
        x, init = R.kmeans_case(n, d, k)
        km = KMeans(n_clusters=k, init=init.astype(np.float32), n_init=1).fit(x.astype(np.float32))
        name = f"kmeans/{n}x{d}x{k}"
        store[name + "/labels"], store[name + "/centers"] = km.labels_, km.cluster_centers_
        store[name + "/inertia"], store[name + "/n_iter"] = np.array(km.inertia_), np.array(km.n_iter_)
    for shape, k in KPP_CASES:
        x, _ = R.kmeans_case(*shape)
        for seed in KPP_SEEDS:
            _, idx = kmeans_plusplus(x.astype(np.float32), k, random_state=seed)
            store[f"kpp/{'x'.join(map(str, shape))}/{k}/{seed}"] = idx
    np.savez_compressed(os.path.join(HERE, "cluster_labels.npz"), **store)
    print(f"wrote {len(store)} arrays with sklearn {sklearn.__version__}")


if __name__ == "__main__":
    main()
