"""CPU checks of the KNN imputation's restatement (tests/knn_impute_ref.py) — the reference the GPU kernel is held to in
tests/test_gpu_knn_impute.py — against sklearn.impute.KNNImputer, live where sklearn imports and through
tests/golden/knn_impute.npz (captured with sklearn by tests/golden/make_knn_impute_golden.py) everywhere; and of the
host-only helpers of igcn_amd.impute (affine_of, fold_indices)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from igcn_amd import impute
from knn_impute_ref import cpu_cases, knn_impute_ref

CASES = cpu_cases()


def _tol(fit, k):
    # the same donors: the mean of k fp64 values added in another order differs by at most k roundings
    return (k + 1) * 2.0 ** -52 * np.nanmax(np.abs(fit))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_sklearn(name):
    sk = pytest.importorskip("sklearn.impute")
    fit, q, k = CASES[name]
    imp = sk.KNNImputer(n_neighbors=k)
    want = imp.fit_transform(fit) if name == "self" else imp.fit(fit).transform(q)
    got = knn_impute_ref(fit, q, k)
    assert got["min_gap"] > 0 and got["order_gap"] > 0         # no exact tie: sklearn's choice is defined
    assert want.shape == got["out"].shape
    assert np.abs(want - got["out"]).max() <= _tol(fit, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_golden(name):
    g = load_golden("knn_impute")
    fit, q, k = CASES[name]
    np.testing.assert_array_equal(g[name + "/fit"], fit)       # the golden's inputs are the cases' inputs
    np.testing.assert_array_equal(g[name + "/q"], q)
    assert int(g[name + "/k"]) == k
    got = knn_impute_ref(fit, q, k)
    assert np.abs(g[name + "/out"] - got["out"]).max() <= _tol(fit, k)
    obs = ~np.isnan(q)
    np.testing.assert_array_equal(got["out"][obs], q[obs])     # observed entries pass through
    assert not np.isnan(got["out"]).any()


def test_cases_cover_what_they_name():
    r = {n: knn_impute_ref(*c) for n, c in CASES.items()}
    d = r["few_distances"]["donors"]
    assert sorted(d[0, 0][d[0, 0] >= 0].tolist()) == [4, 5]    # two defined distances, k = 3
    assert (d[0, 1] == -1).all()                               # observed entry
    one = r["one_column"]
    assert one["fallbacks"] == 2 and (one["donors"] == -1).all()
    np.testing.assert_array_equal(one["out"][[0, 2], 0], one["means"][[0, 0]])
    two = r["two_rows"]["donors"]
    assert (two[..., 2] == -1).all() and two.max() <= 1        # never more than the two donors there are
    full = r["complete_row"]
    assert (full["donors"][2] == -1).all()
    np.testing.assert_array_equal(full["out"][2], CASES["complete_row"][1][2])
    own = r["self"]["donors"]                                  # a row is never its own donor
    rows = np.arange(own.shape[0])[:, None, None]
    assert not (own == rows).any()


def test_tie_rule_of_the_restatement():
    fit = np.array([[1.0, 10.0], [1.0, 20.0], [1.0, 40.0], [5.0, 80.0]])
    q = np.array([[1.0, np.nan]])
    for k, want in ((1, 10.0), (2, 15.0), (3, 70.0 / 3)):
        r = knn_impute_ref(fit, q, k)
        assert r["donors"][0, 1, :k].tolist() == list(range(k)) and r["out"][0, 1] == want
        assert r["min_gap"] == 0.0 if k < 3 else r["min_gap"] > 0


def test_unobserved_column_is_refused():
    fit = np.array([[1.0, np.nan], [2.0, np.nan]])
    with pytest.raises(ValueError):
        knn_impute_ref(fit, np.array([[np.nan, 1.0]]), 3)


def test_affine_of_matches_the_scalers():
    pre = pytest.importorskip("sklearn.preprocessing")
    rng = np.random.default_rng(5)
    x = rng.normal(size=(40, 9)) * np.linspace(0.5, 30.0, 9) + np.linspace(-3, 50, 9)
    for scaler in (pre.MinMaxScaler().fit(x), pre.StandardScaler().fit(x)):
        scale, shift = impute.affine_of(scaler)
        assert scale.dtype == torch.float32 and shift.dtype == torch.float32 and scale.shape == (9,)
        got = (torch.from_numpy(x).float() * scale + shift).double().numpy()
        bound = 2.0 ** -22 * (np.abs(x) * np.abs(scale.double().numpy()) + np.abs(shift.double().numpy()))
        assert (np.abs(got - scaler.transform(x)) <= bound).all()


def test_affine_of_is_duck_typed():
    scale, shift = impute.affine_of(SimpleNamespace(scale_=np.array([0.5, 2.0]), min_=np.array([1.0, -1.0])))
    assert scale.tolist() == [0.5, 2.0] and shift.tolist() == [1.0, -1.0]
    scale, shift = impute.affine_of(SimpleNamespace(mean_=np.array([4.0]), scale_=np.array([2.0])))
    assert scale.tolist() == [0.5] and shift.tolist() == [-2.0]
    with pytest.raises(TypeError):
        impute.affine_of(SimpleNamespace(scale_=np.ones(2)))


def test_fold_indices_on_a_hand_written_split():
    # three folds of seven subjects: validation = the previous fold's test subjects, training = the rest, ascending
    test = [torch.tensor([5, 0]), torch.tensor([3, 6, 1]), torch.tensor([2, 4])]
    train, test_out, val = impute.fold_indices(test, 7)
    assert [t.tolist() for t in test_out] == [[5, 0], [3, 6, 1], [2, 4]]
    assert [t.tolist() for t in val] == [[2, 4], [5, 0], [3, 6, 1]]
    assert [t.tolist() for t in train] == [[1, 3, 6], [2, 4], [0, 5]]
    assert all(t.dtype == torch.int64 for t in train + val)
