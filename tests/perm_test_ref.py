"""fp64 numpy restatement of the max-T permutation test (igcn_amd.stats, csrc/perm_test.hip), for the tests.

G[p, e] = sum_s member[p, s] z[s, e] in fp64, with the sum of absolute terms A[p, e] = sum_s member[p, s] |z[s, e]| that
the any-order fp32 summation bound needs:  |fl32(sum) - sum| <= (S + 8) 2^-24 A  for every order of the additions (the
classical (n - 1) u bound with u = 2^-24, first order, with room for the second-order term at S <= 4096), doubled by
``bound`` because the rounding of the matrix unit's internal adder is not documented.
"""
import numpy as np


def standardize(x):
    """(z, mean, sd, constant) of the columns of x [S, E]: fp64, population sd, z = 0 for a constant column."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(0)
    sd = x.std(0)
    constant = x.max(0) == x.min(0)
    z = np.where(constant[None, :], 0.0, (x - mean) / np.where(constant, 1.0, sd))
    return z, mean, sd, constant


def student_t(g, n_a, n_b):
    """The pooled-variance Student t of a column standardised over S = n_a + n_b subjects whose group-A sum is g."""
    g = np.asarray(g, dtype=np.float64)
    s = n_a + n_b
    r = g / np.sqrt(float(n_a * n_b))
    return r * np.sqrt((s - 2) / (1.0 - r * r))


def bound(a, s):
    """2 (S + 8) 2^-24 A: the condition on |G_gpu - G_ref| (a condition, not a measurement)."""
    return 2.0 * (s + 8) * 2.0 ** -24 * np.asarray(a, dtype=np.float64)


def restate(z, member, observed):
    """z [S, E], member [P, S] 0/1, observed [S] 0/1 (group A of the true labelling).  Returns a dict: G, A [P, E];
    g_obs, a_obs [E]; maxabs [P]; exceed, fwe [E] (the two counts); p_unc, p_fwe [E]; t [E] (for a standardised z)."""
    z = np.asarray(z, dtype=np.float64)
    m = np.asarray(member, dtype=np.float64)
    o = np.asarray(observed, dtype=np.float64)
    p, s = m.shape
    n_a = int(round(o.sum()))
    # subjects in order, the same order for every row and for the observed labelling (a BLAS product may sum a row of a
    # matrix and the same row as a vector in different orders: a relabelling equal to the observed one must tie exactly)
    g, a = np.zeros((p, z.shape[1])), np.zeros((p, z.shape[1]))
    g_obs, a_obs = np.zeros(z.shape[1]), np.zeros(z.shape[1])
    for i in range(s):
        g += m[:, i:i + 1] * z[i]
        a += m[:, i:i + 1] * np.abs(z[i])
        g_obs += o[i] * z[i]
        a_obs += o[i] * np.abs(z[i])
    maxabs = np.abs(g).max(1)
    thr = np.abs(g_obs)
    exceed = (np.abs(g) >= thr[None, :]).sum(0)
    fwe = (maxabs[:, None] >= thr[None, :]).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = student_t(g_obs, n_a, s - n_a)
    return {"G": g, "A": a, "g_obs": g_obs, "a_obs": a_obs, "maxabs": maxabs, "exceed": exceed, "fwe": fwe,
            "p_unc": (1 + exceed) / (1.0 + p), "p_fwe": (1 + fwe) / (1.0 + p), "t": t}


def near_counts(ref, s):
    """(near [E], near_fwe [E]): the relabellings whose restated |G[p, e]| (max_e |G[p, e]|) lies within the two bounds —
    its own and the threshold's — of the threshold |g_obs[e]|: the comparisons an fp32 result inside its bound may
    decide the other way."""
    b, b_obs = bound(ref["A"], s), bound(ref["a_obs"], s)
    thr = np.abs(ref["g_obs"])
    near = (np.abs(np.abs(ref["G"]) - thr[None, :]) <= b + b_obs[None, :]).sum(0)
    b_max = b.max(1)                                           # |max_gpu - max_ref| <= max_e bound[p, e]
    near_fwe = (np.abs(ref["maxabs"][:, None] - thr[None, :]) <= b_max[:, None] + b_obs[None, :]).sum(0)
    return near, near_fwe


def cohort(s, e, n_a, seed, extra=3, shift=0.8, every=7):
    """The float-statistics data: (x [s + extra, e] fp32, y [s + extra] int64 with n_a zeros, s - n_a ones and ``extra``
    twos spread through the rows).  Gaussian columns with a scale and an offset per column; every ``every``-th column is
    shifted by ``shift`` sd in group 0."""
    rng = np.random.default_rng(seed)
    n = s + extra
    y = np.full(n, 2, dtype=np.int64)
    kept = np.sort(rng.permutation(n)[:s])
    lab = np.ones(s, dtype=np.int64)
    lab[rng.permutation(s)[:n_a]] = 0
    y[kept] = lab
    scale = rng.uniform(0.5, 2.0, e)
    offset = rng.uniform(1.0, 5.0, e) * rng.choice([-1.0, 1.0], e)
    x = rng.standard_normal((n, e))
    x[:, ::every] += shift * (y == 0)[:, None]
    return (x * scale + offset).astype(np.float32), y


def draw(p, s, n_a, seed):
    """uint8 [p, s]: p random relabellings with n_a ones each (numpy's generator)."""
    rng = np.random.default_rng(seed)
    m = np.zeros((p, s), dtype=np.uint8)
    for i in range(p):
        m[i, rng.permutation(s)[:n_a]] = 1
    return m
