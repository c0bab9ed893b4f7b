"""GPU checks of the cluster-label kernels (csrc/tsne.hip, csrc/kmeans.hip, igcn_amd.cluster_labels) against the fp64
restatements of tests/cluster_labels_ref.py.  Inputs are rounded to fp32 before the restatement sees them.

Distances: per element ``|d - ref| <= (D + 2) 2^-24 ref`` (two roundings of the difference squared, D of the fma chain),
the diagonal exactly 0, d_ij and d_ji the same bits.

P and beta: the restatement is given the DEVICE's distance matrix (sklearn rounds its distances to fp32 before the search
too; the matrix itself is held to fp64 by the test above), so both sides bisect the same numbers in fp64: beta within
1e-9, P within ``2^-23 P + 1e-30`` — no beta can move, and the bound needs no widening.

Gradient, Z, KL: ``grad_bound`` / ``z_bound`` / ``kl_bound`` of the restatement — roundings counted from the kernels
(cluster_labels_ref's docstring), times the restatement's absolute-term sums.  The update step is compared on
the elements whose gain branch the restatement decides (|grad| above its own bound, or update == 0), at most 1 % are left
out (tests/test_cluster_labels_reference.py checks that on the CPU), with the bound propagated through the step.

KMeans: condition, asserted on the restatement: every point's relative centre gap >= 1e-4 at every assignment (the fp32
distance carries (ceil(d / 64) + 8) 2^-24 <= 8e-7 relative).  Then labels and n_iter_ are equal, centres lie within
``B = 2^-23 (log2 N + d + 2) max|x|`` and the inertia within ``sum_n (4 B |x_n - c|_1 + 4 d B^2 + (ceil(d / 64) + 8) 2^-24
d2_n)``.  k-means++: for seeds whose draws keep 1e-6 (relative to the potential) from the scan values the chosen indices
equal the restatement's, and through the golden file sklearn's.

The largest use of every bound is printed; DESIGN §4 records them.
"""
import math

import numpy as np
import pytest
import torch

import cluster_labels_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

KPP_CASES = [((96, 2, 3), 3), ((300, 7, 5), 5), ((300, 7, 5), 16), ((65, 270, 2), 2)]
KPP_SEEDS = (0, 1, 2, 1000)
STATES = (0, 100, 400)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _np(t):
    return t.detach().cpu().double().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                                                    b.contiguous().view(torch.int32))


def _use(err, bound):
    m = bound > 0
    return float((err[m] / bound[m]).max()) if m.any() else 0.0


# ---- distances, P, beta -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.TSNE_SHAPES, ids=_ids)
def test_sqdist_and_joint_p(shape):
    from igcn_amd import ops
    s, d = shape
    x = R.tsne_case(shape)["x"]
    dist = ops.tsne_sqdist(_dev(x))
    got, want = _np(dist), R.sqdist_ref(x)
    bound = (d + 2) * R.U * want
    assert (np.abs(got - want) <= bound).all()
    assert (np.diag(got) == 0).all() and _same_bits(dist, dist.T.contiguous())
    print(f"{shape}: distances use {_use(np.abs(got - want), bound):.3f} of (D + 2) 2^-24")
    for perp in R.perplexities(s):
        p, betas, pstats = ops.tsne_joint_p(dist, perp)
        ref = R.joint_p_ref(got, perp)
        assert p.dtype == torch.float32 and betas.dtype == torch.float64
        assert (np.abs(_np(betas) - ref["betas"]) <= 1e-9 * ref["betas"]).all()
        err, pb = np.abs(_np(p) - ref["P"]), 2.0 ** -23 * ref["P"] + 1e-30
        assert (err <= pb).all() and (np.diag(_np(p)) == 0).all()
        # the constants are those of the STORED (fp32) P
        pf = _np(p)
        off = pf > 0
        assert abs(float(pstats[0]) - (pf[off] * np.log(pf[off])).sum()) <= 1e-12 * np.abs(pf[off] * np.log(pf[off])).sum()
        assert abs(float(pstats[1]) - pf.sum()) <= 1e-12
        print(f"{shape} perplexity {perp}: P uses {_use(err, pb):.3f} of 2^-23 P, beta "
              f"{float((np.abs(_np(betas) - ref['betas']) / ref['betas']).max()):.1e} relative")


# ---- gradient, Z, KL and one update step ------------------------------------------------------------------------------------
def _state(case, it):
    from igcn_amd import ops
    y, update, gains = case["states"][it]
    p = case["P"]
    off = p > 0
    pstats = torch.tensor([(p[off] * np.log(p[off])).sum(), p.sum()], dtype=torch.float64, device="cuda")
    st = ops.TsneState(_dev(p), pstats, _dev(y))
    st.update.copy_(_dev(update))
    st.gains.copy_(_dev(gains))
    return st


@pytest.mark.parametrize("shape", R.TSNE_SHAPES, ids=_ids)
def test_gradient_z_kl_and_update(shape):
    from igcn_amd import ops
    s, _ = shape
    case = R.tsne_case(shape)
    lr = case["lr"]
    uses = {"grad": 0.0, "Z": 0.0, "KL": 0.0, "step": 0.0}
    left_out = 0.0
    for it in STATES:
        y, update, gains = case["states"][it]
        for e in (12.0, 1.0):
            momentum = R.phase_of(it)[1]
            st = _state(case, it)
            ops.tsne_grad(st, want_kl=True)
            ops.tsne_update(st, e, momentum, lr, check=True)
            ref = R.tsne_grad_ref(case["P"], y, e)
            gb, zb, kb = R.grad_bound(ref, s), R.z_bound(ref, s), R.kl_bound(ref, s)
            gerr = np.abs(_np(st.grad) - ref["grad"])
            kl, _, z, n = (float(v) for v in st.status.cpu())
            assert (gerr <= gb).all(), (it, e, _use(gerr, gb))
            assert abs(z - ref["Z"]) <= zb and abs(kl - ref["kl"]) <= kb and n == 1.0, (it, e, z, ref["Z"], kl, ref["kl"])
            uses["grad"] = max(uses["grad"], _use(gerr, gb))
            uses["Z"], uses["KL"] = max(uses["Z"], abs(z - ref["Z"]) / zb), max(uses["KL"], abs(kl - ref["kl"]) / kb)
            # the step, on the elements whose gain branch the restatement decides
            y1, u1, g1, _, gg = R.tsne_step_ref(case["P"], y, update, gains, e, momentum, lr)
            decided = (update == 0) | (np.abs(ref["grad"]) > gb)
            left_out = max(left_out, 1.0 - decided.mean())
            assert decided.mean() >= 0.99
            assert (np.abs(_np(st.gains) - g1)[decided] <= 2 * R.U * g1[decided]).all()
            ub = 1.001 * lr * g1 * gb + 6 * R.U * (np.abs(momentum * update) + np.abs(lr * gg))
            yb = ub + 2 * R.U * np.abs(y1)
            uerr, yerr = np.abs(_np(st.update) - u1), np.abs(_np(st.y) - y1)
            assert (uerr[decided] <= ub[decided]).all() and (yerr[decided] <= yb[decided]).all()
            uses["step"] = max(uses["step"], _use(yerr[decided], yb[decided]))
            want_norm = math.sqrt((gg[decided] ** 2).sum())
            if decided.all():
                assert abs(float(st.status[1]) - want_norm) <= 1.001 * math.sqrt(((g1 * gb) ** 2).sum()) + 1e-6 * want_norm
    print(f"{shape}: largest use of the bounds: " + ", ".join(f"{k} {v:.3f}" for k, v in uses.items())
          + f"; left out of the step {left_out:.4f}")


# ---- KMeans -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.KMEANS_SHAPES, ids=_ids)
def test_kmeans_from_a_given_init(shape):
    from igcn_amd.cluster_labels import KMeans
    n, d, k = shape
    x, init = R.kmeans_case(n, d, k)
    ref = R.kmeans_ref(x, init)
    assert ref["min_gap"] >= 1e-4
    km = KMeans(n_clusters=k, init=_dev(init)).fit(_dev(x))
    np.testing.assert_array_equal(km.labels_.cpu().numpy(), ref["labels"])
    assert km.labels_.dtype == torch.int64 and km.n_iter_ == ref["n_iter"]
    b = 2.0 ** -23 * (math.log2(n) + d + 2) * np.abs(x).max()
    cerr = np.abs(_np(km.cluster_centers_) - ref["centers"])
    assert (cerr <= b).all()
    resid = x - ref["centers"][ref["labels"]]
    ib = (4 * b * np.abs(resid).sum(1) + 4 * d * b * b + (R.cdiv(d, 64) + 8) * R.U * (resid ** 2).sum(1)).sum()
    assert abs(km.inertia_ - ref["inertia"]) <= ib
    # held-out points
    rng = np.random.default_rng(5)
    held = R.f32(x[rng.integers(n, size=40)] + 0.3 * rng.normal(size=(40, d)))
    d2 = ((held[:, None, :] - ref["centers"][None]) ** 2).sum(-1)
    part = np.sort(d2, axis=1)
    clear = (part[:, 1] - part[:, 0]) / part[:, 1] >= 1e-4 if k > 1 else np.ones(40, dtype=bool)
    assert clear.mean() >= 0.9
    np.testing.assert_array_equal(km.predict(_dev(held)).cpu().numpy()[clear], d2.argmin(1)[clear])
    print(f"{shape}: {km.n_iter_} iterations, relocated {ref['relocated']}, centres use {float(cerr.max() / b):.3f}, "
          f"inertia {abs(km.inertia_ - ref['inertia']) / ib:.3f}, smallest centre gap {ref['min_gap']:.2e}")


def test_kmeans_ties_go_to_the_lower_centre():
    from igcn_amd import ops
    x = _dev(np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 5.0]]))
    centers = _dev(np.array([[1.0, 1.0], [1.0, -1.0], [1.0, 1.0]]))
    labels, mind, counts, sums, stats = ops.kmeans_assign(x, centers)
    assert labels.tolist() == [0, 0, 0] and mind.tolist() == [2.0, 2.0, 16.0] and counts.tolist() == [3, 0, 0]
    assert sums[0].tolist() == [3.0, 5.0] and float(stats[0]) == 20.0 and float(stats[1]) == 3.0
    again = ops.kmeans_assign(x, centers, labels)
    assert float(again[4][1]) == 0.0
    # two clusters came empty: 1 takes the farthest point (2), 2 the next — points 0 and 1 tie at 2.0, the lower goes
    ops.kmeans_update(x, centers, labels, mind, counts, sums, stats)
    assert centers.tolist() == [[2.0, 0.0], [1.0, 5.0], [0.0, 0.0]]
    assert float(stats[3]) == 1.0 and float(stats[2]) == 2.0 + 36.0 + 2.0
    ops.kmeans_update(x, centers.clone(), labels, mind, again[2], again[3], again[4])
    assert float(again[4][3]) == 0.0


@pytest.mark.parametrize("case", KPP_CASES, ids=lambda c: _ids(c[0]) + f"-k{c[1]}")
def test_kmeans_plusplus_indices(case):
    from igcn_amd.cluster_labels import kmeans_plusplus
    shape, k = case
    x, _ = R.kmeans_case(*shape)
    g = load_golden("cluster_labels")
    xd = _dev(x)
    for seed in KPP_SEEDS:
        ref = R.kmeanspp_ref(x, k, seed)
        assert ref["draw_gap"] >= 1e-6 and ref["pot_gap"] >= 1e-6
        centers, idx = kmeans_plusplus(xd, k, seed)
        np.testing.assert_array_equal(idx.cpu().numpy(), ref["indices"])
        np.testing.assert_array_equal(idx.cpu().numpy(), g[f"kpp/{_ids(shape)}/{k}/{seed}"])
        assert _same_bits(centers, xd[idx])


# ---- end to end ---------------------------------------------------------------------------------------------------------------
BLOBS = [(3, 32, 12, 10.0, 0), (3, 32, 12, 10.0, 1), (3, 32, 12, 10.0, 2), (2, 48, 8, 15.0, 0), (3, 37, 5, 8.0, 0)]


@pytest.mark.parametrize("blob", BLOBS, ids=_ids)
def test_cluster_labels_recover_blobs(blob):
    from igcn_amd import ops
    from igcn_amd.cluster_labels import cluster_labels
    groups, per, d, perp, seed = blob
    x, truth = R.blobs_case(groups, per, d, seed)
    xd = _dev(x)
    labels, emb, info = cluster_labels(xd, n_clusters=groups, perplexity=perp, random_state=1000, y=_dev(truth, torch.int64))
    table = np.array(info["class_counts"])
    assert labels.dtype == torch.int64 and emb.shape == (groups * per, 2) and info["n_iter"] == 999
    assert sorted(table.max(0).tolist()) == [per] * groups and sorted(table.max(1).tolist()) == [per] * groups, table
    assert info["sizes"] == [per] * groups
    # kl_divergence_ is the divergence of the embedding handed back
    p, _, _ = ops.tsne_joint_p(ops.tsne_sqdist(xd), perp)
    ref = R.tsne_grad_ref(_np(p), _np(emb), 1.0)
    assert abs(info["kl"] - ref["kl"]) <= R.kl_bound(ref, groups * per), (info["kl"], ref["kl"])
    assert info["kl"] < info["kl_exploration"]
    print(f"{blob}: KL {info['kl']:.4f} (after the exaggeration phase {info['kl_exploration']:.3f}), KMeans "
          f"{info['kmeans_n_iter']} iterations, inertia {info['inertia']:.1f}")


# ---- behaviour ----------------------------------------------------------------------------------------------------------------
def test_captured_eager_and_repeated_runs_give_the_same_bits():
    from igcn_amd.cluster_labels import TSNE
    x = _dev(R.blobs_case(3, 32, 12, 0)[0])
    runs = [TSNE(perplexity=10.0, max_iter=300, captured=c) for c in (True, False, True)]
    embs = [t.fit_transform(x).clone() for t in runs]
    assert _same_bits(embs[0], embs[1]) and _same_bits(embs[0], embs[2])
    assert runs[0].kl_divergence_ == runs[1].kl_divergence_ and runs[0].n_iter_ == runs[1].n_iter_ == 299
    assert runs[0].learning_rate_ == 50.0 and runs[0].betas_.shape == (96,)
    odd = TSNE(perplexity=10.0, max_iter=275)                   # no multiple of 50: the eager launches
    odd.fit_transform(x)
    assert odd.n_iter_ == 274 and math.isfinite(odd.kl_divergence_)
    given = TSNE(perplexity=10.0, max_iter=250, init=embs[0])
    assert given.fit_transform(x).shape == (96, 2)


def test_every_descent_call_starts_from_zero_update_and_unit_gains():
    """sklearn's _gradient_descent begins with update = 0 and gains = 1, and TSNE._fit calls it twice: what the
    exaggeration phase left in update and gains must not reach the second phase (the schedule itself is held to sklearn's
    two calls on the CPU, tests/test_cluster_labels_reference.py)."""
    from igcn_amd import ops
    from igcn_amd.cluster_labels import TSNE
    case = R.tsne_case((64, 5))
    y, update, gains = case["states"][100]
    t = TSNE(perplexity=30.0, captured=False)
    t.learning_rate_ = case["lr"]
    fresh, used = _state(case, 100), _state(case, 100)
    fresh.update.zero_()
    fresh.gains.fill_(1.0)
    assert float(used.update.abs().max()) > 0 and float((used.gains - 1).abs().max()) > 0
    for st in (fresh, used):
        t._descend(st, 250, 251, 1.0, 0.8, 300)
    assert _same_bits(fresh.y, used.y) and _same_bits(fresh.update, used.update) and _same_bits(fresh.gains, used.gains)
    y1, u1, g1, _, _ = R.tsne_step_ref(case["P"], y, np.zeros_like(y), np.ones_like(y), 1.0, 0.8, case["lr"])
    assert np.abs(_np(used.gains) - g1).max() <= 2 * R.U * g1.max()
    assert not np.allclose(_np(used.y), R.tsne_step_ref(case["P"], y, update, gains, 1.0, 0.8, case["lr"])[0], rtol=1e-4)
    ref = R.tsne_grad_ref(case["P"], y, 1.0)
    ub = 1.001 * case["lr"] * g1 * R.grad_bound(ref, 64) + 6 * R.U * np.abs(u1)
    assert (np.abs(_np(used.update) - u1) <= ub).all()


def test_wss_curve_decreases():
    from igcn_amd.cluster_labels import wss_curve
    x, _ = R.blobs_case(3, 32, 2, 4)
    wss = wss_curve(_dev(x), kmax=5, random_state=1000)
    assert len(wss) == 5 and all(a > b for a, b in zip(wss, wss[1:]))
    assert abs(wss[0] - ((x - x.mean(0)) ** 2).sum()) <= 1e-5 * wss[0]
    assert wss[2] < 0.25 * wss[0]                               # the elbow of three blobs


def test_label_store_batch_and_train_step():
    from igcn_amd import synth
    from igcn_amd.cluster_labels import label_store
    from igcn_amd.loader import UniformGraphStore
    from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
    from igcn_amd.train import FlatAdam, train_step
    dev = torch.device("cuda", 0)
    from igcn_amd.data import Data
    graphs = synth.brain_graph_list(24, seed=5, rois=90, tsne_dim=16)
    graphs = [Data(**{k: v for k, v in g.__dict__.items() if k != "A"}) for g in graphs]
    host = UniformGraphStore(graphs)
    with pytest.raises(ValueError):
        label_store(host)
    store = UniformGraphStore(graphs, device=dev)
    before = {k: v.clone() for k, v in store.cols.items()}
    info = label_store(store, perplexity=5.0, max_iter=250)
    assert sum(info["sizes"]) == 24 and info["n_iter"] == 249
    for k, v in before.items():
        if k not in ("clust_y", "tsne_fdim"):
            assert torch.equal(store.cols[k], v), k           # every other column keeps its bits
    cy, fd = store.cols["clust_y"], store.cols["tsne_fdim"]
    assert cy.dtype == torch.int64 and cy.shape == (24, 1) and fd.dtype == torch.float32 and fd.shape == (24, 1, 2)
    assert set(cy.view(-1).tolist()) <= {0, 1}
    idx = torch.tensor([3, 0, 17, 9, 22, 5, 11, 8], device=dev)
    batch = store.batch(idx)
    assert torch.equal(batch.clust_y.view(-1), cy[idx].view(-1)) and _same_bits(batch.tsne_fdim.view(8, 2), fd[idx].view(8, 2))
    flat = before["x"].reshape(24, -1)
    label_store(store, similarity="features", perplexity=5.0, max_iter=250)
    assert _same_bits(store.cols["tsne_fdim"].view(24, -1), flat) and torch.equal(store.cols["clust_y"], cy)
    assert store.cols["tsne_fdim"].data_ptr() != store.cols["x"].data_ptr()      # a copy: writing one leaves the other
    store.cols["tsne_fdim"].zero_()
    assert torch.equal(store.cols["x"], before["x"])
    pool = (40, 20, 10, 4, 1)
    go_snps, adj, pool_dim = synth.go_hierarchy(pool, seed=3)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, dev)
    torch.manual_seed(0)
    model = SGCN_GCN_CLUSTERLABEL(2, 16, a_g, a, pool_dim, 32, dev, H_0=3, num_features=3, isCrossAtten=True).to(dev)
    model.train()
    loss = train_step(model, FlatAdam(model.parameters(), lr=1e-3), batch)
    assert torch.isfinite(loss).all()
