"""numpy fp64 restatement of the KNN imputation the library computes (igcn_knn_impute): sklearn's
``KNNImputer(n_neighbors=k, weights="uniform", metric="nan_euclidean")`` plus the library's tie rule.

For a receiver row q and a training row t with F columns, P = the columns observed in both:
``dist(q, t) = sqrt(sum_{c in P} (q_c - t_c)^2 / |P| * F)``, undefined (NaN) when P is empty.  A missing entry (q, c)
takes the plain mean of column c over the min(k, #candidates) nearest candidates — training rows that observe c and have
a defined distance to q — ordered by (distance, training row index), or with no candidate the mean of column c over all
training rows that observe it.  A column that no training row observes is refused (ValueError).
"""
import numpy as np


def knn_impute_ref(fit, q, k):
    """Returns a dict: ``out`` [n_q, F] fp64, ``donors`` [n_q, F, k] (training row indices in selection order, -1 for
    unused slots and observed entries), ``fallbacks`` (entries filled by the column mean), ``means`` [F], and two
    measures of how far the input is from a decision fp32 rounding could take the other way, over all (receiver,
    column) pairs: ``min_gap`` = the smallest relative gap (d_{k+1} - d_k) / d_{k+1} between the last chosen and the
    first rejected candidate, ``order_gap`` = the same between consecutive chosen candidates (inf when there is no
    such pair)."""
    fit = np.asarray(fit, np.float64)
    q = np.asarray(q, np.float64)
    n, f = fit.shape
    mf, mq = np.isnan(fit), np.isnan(q)
    cnt = (~mf).sum(0)
    if not (cnt > 0).all():
        raise ValueError(f"no training row observes column(s) {np.nonzero(cnt == 0)[0].tolist()}")
    means = np.where(mf, 0.0, fit).sum(0) / cnt
    out = q.copy()
    donors = -np.ones(q.shape + (k,), np.int64)
    min_gap, order_gap, fallbacks = np.inf, np.inf, 0

    def rel(a, b):
        return (b - a) / b if b > 0 else 0.0

    for i in range(q.shape[0]):
        if not mq[i].any():
            continue
        both = (~mq[i])[None, :] & ~mf
        nb = both.sum(1)
        d2 = (np.where(both, q[i][None, :] - fit, 0.0) ** 2).sum(1)
        with np.errstate(all="ignore"):
            dist = np.sqrt(np.where(nb > 0, d2 / np.maximum(nb, 1) * f, np.nan))
        for c in np.nonzero(mq[i])[0]:
            cand = np.nonzero(~mf[:, c] & ~np.isnan(dist))[0]
            if cand.size == 0:
                out[i, c] = means[c]
                fallbacks += 1
                continue
            order = cand[np.lexsort((cand, dist[cand]))]        # by distance, then by training row index
            kk = min(k, order.size)
            sel = order[:kk]
            donors[i, c, :kk] = sel
            out[i, c] = fit[sel, c].sum() / kk
            if order.size > kk:
                min_gap = min(min_gap, rel(dist[order[kk - 1]], dist[order[kk]]))
            for j in range(kk - 1):
                order_gap = min(order_gap, rel(dist[sel[j]], dist[sel[j + 1]]))
    return {"out": out, "donors": donors, "fallbacks": fallbacks, "means": means, "min_gap": min_gap,
            "order_gap": order_gap}


def value_bound(fit, q, res, k, scale=None, shift=None):
    """Per element of the imputed [n_q, F] matrix, the fp32 error bound of the library against this restatement:
    ``2^-23 (k + 2) (|scale_c| max_j |v_j| + |shift_c|)`` — k roundings of the ordered fp32 mean and two of the affine —
    with v_j the donors' values, for an observed entry the value itself, for a fallback the column's largest observed
    magnitude.  Without an affine scale = 1, shift = 0."""
    fit = np.asarray(fit, np.float64)
    q = np.asarray(q, np.float64)
    f = fit.shape[1]
    scale = np.ones(f) if scale is None else np.asarray(scale, np.float64)
    shift = np.zeros(f) if shift is None else np.asarray(shift, np.float64)
    colmax = np.nanmax(np.abs(fit), axis=0)
    mag = np.abs(q)
    for i, c in zip(*np.nonzero(np.isnan(q))):
        d = res["donors"][i, c]
        d = d[d >= 0]
        mag[i, c] = np.abs(fit[d, c]).max() if d.size else colmax[c]
    return 2.0 ** -23 * (k + 2) * (np.abs(scale)[None, :] * mag + np.abs(shift)[None, :])


def draw(rng, n, f, p):
    """Continuous columns of different scales with a fraction p missing, rounded to fp32 (returned as fp64)."""
    x = rng.random((n, f)) * np.linspace(0.5, 30.0, f)[None, :]
    x[rng.random((n, f)) < p] = np.nan
    return x.astype(np.float32).astype(np.float64)


def cpu_cases():
    """The named (fit, q, k) cases of tests/test_knn_impute_reference.py and tests/golden/knn_impute.npz."""
    rng = np.random.default_rng(20240)
    cases = {}
    fit, q = draw(rng, 37, 9, 0.25), draw(rng, 11, 9, 0.25)
    cases["random"] = (fit, q, 3)
    cases["self"] = (fit, fit, 3)                          # fit_transform of the training set on itself
    # a receiver whose only observed column is unobserved in half the donors: fewer than k defined distances for ...
    fit2 = draw(rng, 6, 9, 0.2)
    fit2[:, 1] = [np.nan, np.nan, np.nan, np.nan, 2.5, 7.25]
    q2 = np.full((2, 9), np.nan)
    q2[0, 1] = 3.0
    q2[1, 1], q2[1, 4] = 6.0, 1.5
    cases["few_distances"] = (fit2, q2, 3)
    cases["one_column"] = (draw(rng, 12, 1, 0.3), np.array([[np.nan], [2.0], [np.nan]]), 2)   # every fill is the mean
    cases["two_rows"] = (np.array([[1.0, 2.0, np.nan, 4.5], [0.5, np.nan, 3.0, 2.25]]), draw(rng, 5, 4, 0.4), 3)
    full = draw(rng, 4, 9, 0.3)
    full[2] = rng.random(9) + 1.0                          # a row with nothing missing
    cases["complete_row"] = (draw(rng, 20, 9, 0.2), full, 3)
    for name, (a, _, _) in cases.items():
        assert not np.isnan(a).all(0).any(), name
    return cases


def gpu_case(n, nq, f, seed, p=0.25):
    """(fit, q) of tests/test_gpu_knn_impute.py: continuous columns; receiver 0 observes nothing (every entry is a
    column-mean fallback), receiver 1 only column 1, which half the training rows miss (fewer defined distances),
    receiver 2 everything."""
    rng = np.random.default_rng(seed)
    fit, q = draw(rng, n, f, p), draw(rng, nq, f, p)
    q[0] = np.nan
    if f > 1:
        keep = q[1, 1] if not np.isnan(q[1, 1]) else 3.0
        q[1] = np.nan
        q[1, 1] = keep
        fit[: n // 2, 1] = np.nan
    full = (rng.random(f) + 0.5).astype(np.float32).astype(np.float64)
    q[2] = full
    return fit, q
