"""fp64 numpy restatement of the max-F permutation test (igcn_amd.stats.permutation_anova, igcn_perm_maxf), for the tests.

For labels [P, S] with codes 0..K-1 and the K - 1 accumulated groups, subjects in order,
    G_g[p, e] = sum_s (labels[p, s] == g) z[s, e],        A_g[p, e] = sum_s (labels[p, s] == g) |z[s, e]|,
the last group's sum is DEFINED as minus the sum of the others (as in the kernel: the column sum of the fp32 z is zero
only to rounding) and  B = sum_{g<K-1} w_g G_g^2 + w_{K-1} (sum_{g<K-1} G_g)^2,  F = (B / (K-1)) / ((S - B) / (S - K)).

The condition on |B_gpu - B_ref| (a condition, not a measurement): with the any-order fp32 summation bound of
tests/perm_test_ref.py for every accumulated sum, beta_g = 2 (S + 8) 2^-24 A_g, the last group's sum inherits the others'
bounds plus the K - 2 fp32 additions that form it, beta_{K-1} = sum_g beta_g + (K - 2) 2^-23 |sum_g G_g|; a square moves by
at most 2 |G| beta + beta^2, and the K products, K squares and K - 1 additions of the fp32 epilogue by (K + 4) 2^-23 B:
    bound_B = sum_g w_g (2 |G_g| beta_g + beta_g^2) + (K + 4) 2^-23 B.
"""
import numpy as np

import perm_test_ref as R


def f_of_b(b, s, k):
    """The one-way ANOVA F of a column standardised over S subjects whose between-groups sum of squares is b."""
    b = np.asarray(b, dtype=np.float64)
    return (b / (k - 1)) / ((s - b) / (s - k))


def _sums(z, labels, k):
    """(G, A) [P, K-1, E] of the accumulated groups, subjects in order (the same order for every row: a relabelling
    equal to the observed one must tie exactly)."""
    p, s = labels.shape
    g, a = np.zeros((p, k - 1, z.shape[1])), np.zeros((p, k - 1, z.shape[1]))
    ind = [(labels == c).astype(np.float64) for c in range(k - 1)]
    for i in range(s):
        zi, ai = z[i], np.abs(z[i])
        for c in range(k - 1):
            g[:, c] += ind[c][:, i:i + 1] * zi
            a[:, c] += ind[c][:, i:i + 1] * ai
    return g, a


def statistic(g, a, weights, s):
    """(B, bound_B) [P, E] from the accumulated sums G, A [P, K-1, E]: g ascending, the last group's term last."""
    w = np.asarray(weights, dtype=np.float64)
    k = w.size
    b = np.zeros(g.shape[::2])
    tot = np.zeros(g.shape[::2])
    for c in range(k - 1):
        b += w[c] * g[:, c] * g[:, c]
        tot += g[:, c]
    b += w[k - 1] * tot * tot
    beta = R.bound(a, s)                                               # [P, K-1, E]
    beta_last = beta.sum(1) + (k - 2) * 2.0 ** -23 * np.abs(tot)
    bound = w[k - 1] * (2 * np.abs(tot) * beta_last + beta_last ** 2) + (k + 4) * 2.0 ** -23 * b
    for c in range(k - 1):
        bound += w[c] * (2 * np.abs(g[:, c]) * beta[:, c] + beta[:, c] ** 2)
    return b, bound


def restate(z, labels, observed, weights):
    """z [S, E], labels [P, S] and observed [S] codes 0..K-1, weights [K].  Returns a dict: G, A [P, K-1, E]; B, bound
    [P, E]; g_obs [K-1, E]; b_obs, bound_obs [E]; maxstat [P]; exceed, fwe [E] (the two counts); p_unc, p_fwe, f [E]
    (f for a standardised z and weights 1 / n_g)."""
    z = np.asarray(z, dtype=np.float64)
    labels, observed = np.asarray(labels), np.asarray(observed)
    p, s = labels.shape
    k = len(weights)
    g, a = _sums(z, labels, k)
    b, bound = statistic(g, a, weights, s)
    g_o, a_o = _sums(z, observed[None, :], k)
    b_o, bound_o = statistic(g_o, a_o, weights, s)
    b_obs = b_o[0]
    maxstat = b.max(1)
    exceed = (b >= b_obs[None, :]).sum(0)
    fwe = (maxstat[:, None] >= b_obs[None, :]).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = f_of_b(b_obs, s, k)
    return {"G": g, "A": a, "B": b, "bound": bound, "g_obs": g_o[0], "b_obs": b_obs, "bound_obs": bound_o[0],
            "maxstat": maxstat, "exceed": exceed, "fwe": fwe, "p_unc": (1 + exceed) / (1.0 + p),
            "p_fwe": (1 + fwe) / (1.0 + p), "f": f}


def near_counts(ref):
    """(near [E], near_fwe [E]): the relabellings whose restated B[p, e] (max_e B[p, e]) lies within the two bounds — its
    own and the threshold's — of the threshold b_obs[e]: the comparisons an fp32 result inside its bound may decide the
    other way."""
    thr, b_thr = ref["b_obs"], ref["bound_obs"]
    near = (np.abs(ref["B"] - thr[None, :]) <= ref["bound"] + b_thr[None, :]).sum(0)
    b_max = ref["bound"].max(1)                                        # |max_gpu - max_ref| <= max_e bound[p, e]
    near_fwe = (np.abs(ref["maxstat"][:, None] - thr[None, :]) <= b_max[:, None] + b_thr[None, :]).sum(0)
    return near, near_fwe


def cohort_k(s, e, sizes, seed, extra=3, shift=0.8, every=7):
    """The float-statistics data for K = len(sizes) groups: (x [s + extra, e] fp32, y [s + extra] int64).  As
    ``perm_test_ref.cohort``, but the kept rows get the codes 0..K-1 ``sizes`` times in a drawn order and the ``extra``
    left-out rows the label K; every ``every``-th column is shifted by ``shift`` sd in group 0 and by ``-shift / 2`` in
    the last group."""
    k = len(sizes)
    assert sum(sizes) == s
    rng = np.random.default_rng(seed)
    n = s + extra
    y = np.full(n, k, dtype=np.int64)
    kept = np.sort(rng.permutation(n)[:s])
    y[kept] = np.repeat(np.arange(k), sizes)[rng.permutation(s)]
    scale = rng.uniform(0.5, 2.0, e)
    offset = rng.uniform(1.0, 5.0, e) * rng.choice([-1.0, 1.0], e)
    x = rng.standard_normal((n, e))
    x[:, ::every] += shift * (y == 0)[:, None] - shift / 2 * (y == k - 1)[:, None]
    return (x * scale + offset).astype(np.float32), y


def draw_labels(p, lab, seed):
    """uint8 [p, S]: p rearrangements of the codes ``lab`` (numpy's generator)."""
    rng = np.random.default_rng(seed)
    lab = np.asarray(lab, dtype=np.uint8)
    return np.stack([lab[rng.permutation(lab.size)] for _ in range(p)])


# (S, E, P, sizes, cohort seed); the label rows are drawn with seed + 100
FLOAT_SHAPES = [(66, 270, 512, (20, 25, 21), 11), (131, 513, 320, (40, 50, 41), 12), (70, 130, 256, (15, 20, 17, 18), 13),
                (70, 130, 256, (12, 15, 13, 14, 16), 14), (33, 65, 129, (16, 17), 15)]
