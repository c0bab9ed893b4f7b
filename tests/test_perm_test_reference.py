"""CPU checks of the max-T permutation test's restatement (tests/perm_test_ref.py), which the GPU tests hold the
kernels to: its t is scipy's pooled-variance t, |G| orders the relabellings as |t| does, its p-value is the exact
enumeration p-value on a toy, and the float-statistics data meets the condition the GPU test asserts.  Also
``stats.draw_members`` on the CPU generator."""
import itertools

import numpy as np
import pytest
import torch

import perm_test_ref as R


def _toy(s=8, e=5, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((s, e)) * rng.uniform(0.5, 3.0, e) + rng.uniform(-4.0, 4.0, e)


def test_t_is_scipys_pooled_variance_t():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(1)
    x = _toy(23, 9, seed=2)
    observed = np.zeros(23)
    observed[rng.permutation(23)[:9]] = 1
    z, _, _, _ = R.standardize(x)
    ref = R.restate(z, observed[None, :], observed)
    want = stats.ttest_ind(x[observed == 1], x[observed == 0], equal_var=True).statistic
    np.testing.assert_allclose(ref["t"], want, rtol=1e-10)
    # the standardisation takes nothing away: diff in original units from g_obs, sd, n_a, n_b
    _, _, sd, _ = R.standardize(x)
    diff = sd * ref["g_obs"] * 23 / (9 * 14)
    np.testing.assert_allclose(diff, x[observed == 1].mean(0) - x[observed == 0].mean(0), rtol=1e-10)


def test_abs_g_orders_relabellings_as_abs_t_does():
    """One increasing function for all columns and relabellings: sorting all |G[p, e]| sorts all |t[p, e]|."""
    stats = pytest.importorskip("scipy.stats")
    x = _toy(12, 4, seed=3)
    z, _, _, _ = R.standardize(x)
    member = R.draw(40, 12, 5, seed=4)
    g = member.astype(np.float64) @ z
    t = np.stack([stats.ttest_ind(x[m == 1], x[m == 0], equal_var=True).statistic for m in member])
    np.testing.assert_allclose(R.student_t(g, 5, 7), t, rtol=1e-9)
    order = np.argsort(np.abs(g).ravel(), kind="stable")
    assert np.all(np.diff(np.abs(t).ravel()[order]) >= -1e-9)


def test_p_unc_is_the_exact_enumeration_p_value():
    """members = all C(8, 3) = 56 subsets: (1 + #{|t_p| >= |t_obs|}) / 57 with t from scipy, column by column."""
    stats = pytest.importorskip("scipy.stats")
    x = _toy(8, 5, seed=5)
    subsets = list(itertools.combinations(range(8), 3))
    member = np.zeros((56, 8), dtype=np.uint8)
    for i, c in enumerate(subsets):
        member[i, list(c)] = 1
    observed = member[17]
    z, _, _, _ = R.standardize(x)
    ref = R.restate(z, member, observed)
    t = np.stack([stats.ttest_ind(x[m == 1], x[m == 0], equal_var=True).statistic for m in member])
    t_obs = t[17]
    # (the observed labelling is one of the 56: compared with itself it is a tie, counted on both sides)
    want = (1 + (np.abs(t) >= np.abs(t_obs)[None, :] * (1 - 1e-12)).sum(0)) / 57.0
    np.testing.assert_array_equal(ref["p_unc"], want)
    assert ref["exceed"].min() >= 1 and np.all(ref["fwe"] >= ref["exceed"])
    assert np.all(ref["p_fwe"] >= ref["p_unc"])


@pytest.mark.parametrize("shape", [(64, 270, 512, 29, 11), (130, 513, 320, 40, 12)])
def test_float_statistics_data_meets_the_near_condition(shape):
    """The condition the GPU test asserts, on the restatement alone (fp64 standardisation in place of the device's):
    the comparisons an fp32 result inside its bound could decide the other way are at most 1e-3 of all."""
    s, e, p, n_a, seed = shape
    x, y = R.cohort(s, e, n_a, seed)
    keep = y != 2
    z, _, _, _ = R.standardize(x[keep])
    ref = R.restate(z.astype(np.float32), R.draw(p, s, n_a, seed + 100), y[keep] == 0)
    near, near_fwe = R.near_counts(ref, s)
    print(f"near share {near.sum() / (p * e):.3e}, max-T near share {near_fwe.sum() / (p * e):.3e}")
    assert near.sum() <= 1e-3 * p * e and near_fwe.sum() <= 1e-3 * p * e
    hits = np.nonzero(ref["p_fwe"] <= 0.05)[0]
    assert np.any(hits % 7 == 0)


def test_draw_members_marks_n_a_of_n_and_repeats_under_a_seed():
    from igcn_amd import stats
    a = stats.draw_members(37, 11, 50, seed=3, device="cpu")
    b = stats.draw_members(37, 11, 50, seed=3, device="cpu")
    c = stats.draw_members(37, 11, 50, seed=4, device="cpu")
    assert a.dtype == torch.uint8 and tuple(a.shape) == (50, 37)
    assert bool((a.sum(1) == 11).all()) and int(a.max()) == 1
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert len({tuple(r.tolist()) for r in a}) > 40             # relabellings, not one row repeated
    with pytest.raises(ValueError):
        stats.draw_members(5, 5, 3, device="cpu")
