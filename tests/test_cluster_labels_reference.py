"""CPU checks of the cluster-label restatements (tests/cluster_labels_ref.py) — the reference the kernels are held to in
tests/test_gpu_cluster_labels.py — against sklearn 1.7: live where sklearn imports, and everywhere through
tests/golden/cluster_labels.npz (captured with sklearn by tests/golden/make_cluster_labels_golden.py); of the conditions
the GPU tests' seeds were fixed to meet; and of the host-only helpers and refusals of igcn_amd.cluster_labels."""
import numpy as np
import pytest
import torch

import cluster_labels_ref as R
from conftest import load_golden
from igcn_amd import cluster_labels as CL

GOLDEN_P = [(7, 3), (64, 5), (65, 12)]      # gradient and KL are in the golden for every shape, the condensed P for these
KPP_CASES = [((96, 2, 3), 3), ((300, 7, 5), 5), ((300, 7, 5), 16), ((65, 270, 2), 2)]
KPP_SEEDS = (0, 1, 2, 1000)
STATES = (0, 100, 400)


def _condensed(p):
    return p[np.triu_indices(p.shape[0], 1)]                  # scipy's squareform of a symmetric matrix


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---- the restatements against sklearn, live ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.TSNE_SHAPES, ids=_ids)
def test_joint_p_matches_sklearn(shape):
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    s, d = shape
    dist = R.f32(R.sqdist_ref(R.features_case(s, d)))
    for perp in R.perplexities(s):
        want = tsne._joint_probabilities(dist, perp, 0)
        got = _condensed(R.joint_p_ref(dist, perp)["P"])
        assert np.abs(got - want).max() <= 1e-12 * want.max() and (np.abs(got - want) <= 1e-12 * want + 1e-300).all()


@pytest.mark.parametrize("shape", R.TSNE_SHAPES, ids=_ids)
def test_gradient_and_kl_match_sklearn(shape):
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    s, _ = shape
    case = R.tsne_case(shape)
    pc = _condensed(case["P"])
    for it in STATES:
        y = case["states"][it][0]
        for e in (12.0, 1.0):
            kl, grad = tsne._kl_divergence(y.ravel(), e * pc, 1.0, s, 2)
            ref = R.tsne_grad_ref(case["P"], y, e)
            assert np.abs(ref["grad"] - grad.reshape(s, 2)).max() <= 1e-10 * max(np.abs(grad).max(), 1e-300)
            assert abs(ref["kl"] - kl) <= 1e-10 * max(abs(kl), 1.0)


@pytest.mark.parametrize("shape", R.KMEANS_SHAPES, ids=_ids)
def test_kmeans_matches_sklearn(shape):
    cluster = pytest.importorskip("sklearn.cluster")
    n, d, k = shape
    x, init = R.kmeans_case(n, d, k)
    # sklearn computes in float32 on float32 input (that is the 1e-4); float64 input would hide nothing but take its
    # other code path
    km = cluster.KMeans(n_clusters=k, init=init.astype(np.float32), n_init=1).fit(x.astype(np.float32))
    _check_kmeans(R.kmeans_ref(x, init), km.labels_, km.cluster_centers_, km.inertia_, km.n_iter_, x)


def _check_kmeans(ref, labels, centers, inertia, n_iter, x):
    np.testing.assert_array_equal(ref["labels"], labels)
    assert ref["n_iter"] == int(n_iter)
    assert np.abs(ref["centers"] - centers).max() <= 1e-4 * np.abs(x).max()
    assert abs(ref["inertia"] - float(inertia)) <= 1e-4 * float(inertia)


@pytest.mark.parametrize("case", KPP_CASES, ids=lambda c: _ids(c[0]) + f"-k{c[1]}")
def test_kmeanspp_matches_sklearn(case):
    cluster = pytest.importorskip("sklearn.cluster")
    shape, k = case
    x, _ = R.kmeans_case(*shape)
    for seed in KPP_SEEDS:
        _, idx = cluster.kmeans_plusplus(x.astype(np.float32), k, random_state=seed)
        np.testing.assert_array_equal(R.kmeanspp_ref(x, k, seed)["indices"], idx)


# ---- and through the golden file -----------------------------------------------------------------------------------------
def test_golden_tsne():
    g = load_golden("cluster_labels")
    for shape in R.TSNE_SHAPES:
        s, d = shape
        case = R.tsne_case(shape)
        dist = R.f32(R.sqdist_ref(case["x"]))
        for perp in R.perplexities(s) if shape in GOLDEN_P else ():
            want = g[f"P/{s}x{d}/{perp}"]
            got = _condensed(R.joint_p_ref(dist, perp)["P"])
            assert (np.abs(got - want) <= 1e-12 * want + 1e-300).all()
        for it in STATES:
            for e in (12.0, 1.0):
                ref = R.tsne_grad_ref(case["P"], case["states"][it][0], e)
                grad, kl = g[f"grad/{s}x{d}/{it}/{e}"], float(g[f"kl/{s}x{d}/{it}/{e}"])
                assert np.abs(ref["grad"] - grad).max() <= 1e-10 * max(np.abs(grad).max(), 1e-300)
                assert abs(ref["kl"] - kl) <= 1e-10 * max(abs(kl), 1.0)


# ---- the schedule: iterations under exaggeration, then update and gains start afresh ----------------------------------------
# Both sides are fp64 and differ in summation order only (1e-16), but the descent is chaotic: measured against sklearn, a
# difference doubles about every iteration (1e-11 after 20 iterations, 1e-6 after 40, everything after 80).  So the switch
# is pinned on a schedule cut to 12 + 12 iterations, where 2^24 1e-16 = 2e-9 leaves 1e-6 a wide margin.
SCHEDULE_TOL = 1e-6          # relative to the embedding's extent


def _schedule_ref(shape):
    case = R.tsne_case(shape)
    return R.tsne_run_ref(case["P"], case["states"][0][0], R.SCHEDULE_ITERS, case["lr"],
                          exploration=R.SCHEDULE_EXPLORATION)[0]


@pytest.mark.parametrize("shape", R.SCHEDULE_SHAPES, ids=_ids)
def test_schedule_matches_sklearn(shape):
    """tsne_run_ref against sklearn's own two _gradient_descent calls (the golden's maker spells them): the switch to
    momentum 0.8 starts from update = 0 and gains = 1."""
    pytest.importorskip("sklearn.manifold._t_sne")
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_cluster_labels_golden", os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "golden", "make_cluster_labels_golden.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    want = maker.sklearn_schedule(shape)
    assert np.abs(_schedule_ref(shape) - want).max() <= SCHEDULE_TOL * np.abs(want).max()


def test_golden_schedule():
    g = load_golden("cluster_labels")
    for shape in R.SCHEDULE_SHAPES:
        want = g[f"run/{shape[0]}x{shape[1]}"]
        assert np.abs(_schedule_ref(shape) - want).max() <= SCHEDULE_TOL * np.abs(want).max()
        # and a descent that carried update and gains across the switch would not pass
        case = R.tsne_case(shape)
        y, update, gains = (a.copy() for a in case["states"][0])
        for i in range(R.SCHEDULE_ITERS):
            phase = (12.0, 0.5) if i < R.SCHEDULE_EXPLORATION else (1.0, 0.8)
            y, update, gains, _, _ = R.tsne_step_ref(case["P"], y, update, gains, *phase, case["lr"])
        assert np.abs(y - want).max() > 1e3 * SCHEDULE_TOL * np.abs(want).max()


def test_golden_kmeans():
    g = load_golden("cluster_labels")
    for n, d, k in R.KMEANS_SHAPES:
        x, init = R.kmeans_case(n, d, k)
        name = f"kmeans/{n}x{d}x{k}"
        _check_kmeans(R.kmeans_ref(x, init), g[name + "/labels"], g[name + "/centers"], float(g[name + "/inertia"]),
                      int(g[name + "/n_iter"]), x)
    for shape, k in KPP_CASES:
        x, _ = R.kmeans_case(*shape)
        for seed in KPP_SEEDS:
            np.testing.assert_array_equal(R.kmeanspp_ref(x, k, seed)["indices"], g[f"kpp/{_ids(shape)}/{k}/{seed}"])


# ---- the conditions the GPU tests assert, checked here where the seeds were fixed ----------------------------------------
def test_kmeans_cases_meet_the_gap_condition_and_cover_relocation():
    for n, d, k in R.KMEANS_SHAPES:
        x, init = R.kmeans_case(n, d, k)
        ref = R.kmeans_ref(x, init)
        assert ref["min_gap"] >= 1e-4, (n, d, k, ref["min_gap"])
        assert (ref["relocated"] > 0) == ((n, d, k) == (9, 2, 4))
        assert 1 < ref["n_iter"] < 300


def test_kmeanspp_seeds_meet_the_gap_condition():
    for shape, k in KPP_CASES:
        x, _ = R.kmeans_case(*shape)
        for seed in KPP_SEEDS:
            ref = R.kmeanspp_ref(x, k, seed)
            assert ref["draw_gap"] >= 1e-6 and ref["pot_gap"] >= 1e-6, (shape, k, seed, ref["draw_gap"], ref["pot_gap"])


@pytest.mark.parametrize("shape", R.TSNE_SHAPES, ids=_ids)
def test_few_elements_sit_on_the_gain_branch(shape):
    """The update test leaves out the elements whose gradient is smaller than its own bound (their gain branch is not
    decided by the restatement): at most 1 % of them."""
    s, _ = shape
    case = R.tsne_case(shape)
    for it in STATES:
        y, update, _ = case["states"][it]
        ref = R.tsne_grad_ref(case["P"], y, R.phase_of(it)[0])
        undecided = (update != 0) & (np.abs(ref["grad"]) <= R.grad_bound(ref, s))
        assert undecided.mean() <= 0.01, (shape, it, undecided.mean())


# ---- host-only helpers and refusals of the package ------------------------------------------------------------------------
def test_pca_sign_rule():
    comps = torch.tensor([[0.1, -0.9, 0.3], [0.5, 0.2, -0.1], [-0.7, 0.7, 0.0]], dtype=torch.float64)
    got = CL.pca_sign_fix(comps)
    assert got.tolist() == [[-0.1, 0.9, -0.3], [0.5, 0.2, -0.1], [0.7, -0.7, -0.0]]        # first of equal magnitudes decides
    assert torch.equal(CL.pca_sign_fix(got), got)


def test_auto_learning_rate():
    assert CL.auto_learning_rate(874, 12.0) == 50.0
    assert CL.auto_learning_rate(4096, 12.0) == 4096 / 12.0 / 4.0
    assert CL.auto_learning_rate(4096, 4.0) == 256.0


def test_kmeanspp_draws_are_sklearns_calls():
    first, draws = CL._kmeanspp_draws(50, 5, 1000)
    rs = np.random.RandomState(1000)
    w = np.ones(50, dtype=np.float32)
    assert first == rs.choice(50, p=w / w.sum())
    assert draws.shape == (4, 3)
    np.testing.assert_array_equal(draws, np.stack([rs.uniform(size=3) for _ in range(4)]))


def test_refusals():
    with pytest.raises(ValueError):
        CL.TSNE(n_components=3)
    with pytest.raises(ValueError):
        CL.TSNE(perplexity=2.0).fit_transform(torch.zeros(3, 5))          # S < 4
    with pytest.raises(ValueError, match="perplexity"):
        CL.TSNE(perplexity=30.0).fit_transform(torch.zeros(30, 5))        # perplexity >= S, as sklearn
    with pytest.raises(ValueError):
        CL.TSNE(perplexity=5.0).fit_transform(torch.zeros(4097, 2))
    with pytest.raises(ValueError):
        CL.TSNE(perplexity=5.0).fit_transform(torch.zeros(40, 1025))
    with pytest.raises(ValueError):
        CL.KMeans(n_clusters=17)
    with pytest.raises(ValueError):
        CL.KMeans(n_clusters=0)
    with pytest.raises(ValueError):
        CL.KMeans(n_clusters=3).fit(torch.zeros(2, 2))                    # fewer points than clusters
    with pytest.raises(ValueError):
        CL.KMeans(n_clusters=2).fit(torch.zeros(8, 1025))
    with pytest.raises(ValueError, match="GPU"):
        CL.KMeans(n_clusters=2).fit(torch.zeros(8, 2))                    # no host path
    with pytest.raises(ValueError, match="GPU"):
        CL.TSNE(perplexity=2.0).fit_transform(torch.zeros(8, 2))
