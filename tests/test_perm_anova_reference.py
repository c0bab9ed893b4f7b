"""CPU checks of the max-F permutation test's fp64 restatement (tests/perm_anova_ref.py) — the side the GPU tests compare
against — and of ``stats.draw_labels`` on the CPU generator."""
import functools
import itertools

import numpy as np
import pytest
import torch

import perm_anova_ref as A
import perm_test_ref as R


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The restatement on the fp64 standardisation rounded to fp32 (what the device's planes hold, to an ulp)."""
    s, e, p, sizes, seed = shape
    x, y = A.cohort_k(s, e, sizes, seed)
    k = len(sizes)
    kept = y != k
    z = R.standardize(x[kept])[0].astype(np.float32)
    labels = A.draw_labels(p, y[kept], seed + 100)
    ref = A.restate(z, labels, y[kept], [1.0 / n for n in sizes])
    return x[kept], y[kept], ref


def test_f_equals_scipy_f_oneway():
    scipy_stats = pytest.importorskip("scipy.stats")
    for shape in A.FLOAT_SHAPES[1:]:
        s, e, p, sizes, seed = shape
        x, lab, _ = _case(shape)
        z = R.standardize(x)[0]                                     # fp64 z: sum z = 0 and sum z^2 = S to rounding
        ref = A.restate(z, lab[None, :].astype(np.uint8), lab, [1.0 / n for n in sizes])
        want = scipy_stats.f_oneway(*[x[lab == c].astype(np.float64) for c in range(len(sizes))]).statistic
        np.testing.assert_allclose(ref["f"], want, rtol=1e-10)
        np.testing.assert_allclose(ref["B"][0], ref["b_obs"], rtol=0, atol=0)      # the observed row ties exactly


def test_sorting_b_sorts_f():
    s, e, p, sizes, _ = A.FLOAT_SHAPES[2]
    b = _case(A.FLOAT_SHAPES[2])[2]["B"].reshape(-1)
    order = np.argsort(b, kind="stable")
    f = A.f_of_b(b, s, len(sizes))
    assert np.all(np.diff(f[order]) >= 0) and np.all(np.diff(b[order]) >= 0)
    assert np.all(f > 0) and f.max() > 10 * np.median(f)


def test_p_unc_equals_the_exact_enumeration_on_a_toy():
    """S = 7 in groups of (3, 2, 2): all 210 label rows; the count from B is the count from F computed the long way.
    Small integers with column sum 0 and the weights 6 / n_g keep the restatement exact, so that the relabellings that
    only rename the two groups of 2 tie with the observed one exactly, as they do in exact arithmetic."""
    sizes, s = (3, 2, 2), 7
    rng = np.random.default_rng(3)
    x = rng.integers(-9, 10, (s, 5)).astype(np.float64)
    x[:3, 0] += 12
    x[-1] -= x.sum(0)
    assert not np.any(x.sum(0))
    lab = np.repeat(np.arange(3), sizes)
    rows = np.array(sorted(set(itertools.permutations(lab.tolist()))), dtype=np.uint8)
    assert rows.shape == (210, s)
    ref = A.restate(x, rows, lab, [6.0 / n for n in sizes])

    def f_long(col, codes):
        groups = [col[codes == c] for c in range(3)]
        between = sum(len(g) * (g.mean() - col.mean()) ** 2 for g in groups) / 2
        within = sum(((g - g.mean()) ** 2).sum() for g in groups) / (s - 3)
        return between / within
    for e in range(x.shape[1]):
        f_obs = f_long(x[:, e], lab)
        fs = np.array([f_long(x[:, e], r) for r in rows])
        b, total = ref["b_obs"][e] / 6, (x[:, e] ** 2).sum()
        np.testing.assert_allclose((b / 2) / ((total - b) / (s - 3)), f_obs, rtol=1e-10)
        count = int((fs >= f_obs * (1 - 1e-9)).sum())
        assert ref["exceed"][e] == count and ref["p_unc"][e] == (1 + count) / 211.0
    assert ref["exceed"].min() >= 2                                 # renaming the two groups of 2 ties
    assert ref["p_unc"][0] < ref["p_unc"][1:].min()


def test_draw_labels_on_the_cpu_generator():
    from igcn_amd import stats
    observed = torch.tensor([0, 2, 1, 1, 0, 2, 2, 0, 1, 2, 3], dtype=torch.uint8)
    a = stats.draw_labels(observed, 64, seed=5, device="cpu")
    assert a.dtype == torch.uint8 and tuple(a.shape) == (64, 11) and a.stride(0) % 16 == 0 and a.data_ptr() % 16 == 0
    for c in range(4):
        assert bool(((a == c).sum(1) == int((observed == c).sum())).all())
    assert torch.equal(a, stats.draw_labels(observed, 64, seed=5, device="cpu"))
    assert not torch.equal(a, stats.draw_labels(observed, 64, seed=6, device="cpu"))
    assert len({tuple(r.tolist()) for r in a}) > 32                 # the rows differ among themselves


@pytest.mark.parametrize("shape", A.FLOAT_SHAPES)
def test_near_condition_of_the_float_shapes(shape):
    """The share of comparisons an fp32 result inside its bound could decide the other way stays below 1e-3, so the GPU
    test's count checks have teeth; planted columns are found."""
    s, e, p, sizes, _ = shape
    ref = _case(shape)[2]
    near, near_fwe = A.near_counts(ref)
    hits = np.nonzero(ref["p_fwe"] <= 0.05)[0]
    print(f"{shape[:4]}: near share {near.sum() / (p * e):.2e}, max-F near share {near_fwe.sum() / (p * e):.2e}, "
          f"{hits.size} columns at p_fwe <= 0.05")
    assert near.sum() <= 1e-3 * p * e and near_fwe.sum() <= 1e-3 * p * e
    assert hits.size > 0 and np.all(hits % 7 == 0)
