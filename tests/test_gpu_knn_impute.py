"""GPU checks of the KNN imputation (csrc/knn_impute.hip, igcn_amd.impute) against the fp64 restatement of
tests/knn_impute_ref.py.  Inputs are rounded to fp32 before the restatement sees them.

Condition on the inputs, asserted on the RESTATEMENT, never on the kernel: ``min_gap >= 1e-5`` (the relative distance
gap between the last chosen and the first rejected candidate) — four times the fp32 bound (F + 4) 2^-24 on a
direct-difference distance at F = 32, so fp32 rounding cannot move a candidate across the cut — and, because the donors
are compared IN ORDER, the same for ``order_gap`` (the gap between consecutive chosen candidates).  The seeds below were
fixed on the CPU with the restatement to meet both.

Values: per element ``|out - ref| <= 2^-23 (k + 2) (|scale_c| max_j |v_j| + |shift_c|)`` (knn_impute_ref.value_bound:
k roundings of the ordered fp32 mean, two of the affine).  The largest use of the bound over the shapes below is
recorded in DESIGN §4.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from knn_impute_ref import gpu_case, knn_impute_ref, value_bound

pytestmark = pytest.mark.gpu

# (n_fit, n_q, F, k): sizes off every multiple of 64, two LDS tiles of training rows (300 > 256), F at both ends of its
# range, fewer donors than k
SHAPES = [(37, 11, 9, 3), (130, 23, 9, 3), (300, 17, 9, 1), (70, 9, 32, 5), (40, 6, 1, 2), (5, 7, 9, 3), (2, 5, 9, 3)]
SEED = 0
MIN_GAP = 1e-5
_REF = {}


def _case(shape):
    """(fit, q, restatement) of a shape, computed once and shared."""
    if shape not in _REF:
        n, nq, f, k = shape
        fit, q = gpu_case(n, nq, f, SEED)
        _REF[shape] = (fit, q, knn_impute_ref(fit, q, k))
    return _REF[shape]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dtype).cuda()


def _stacked(fit, q):
    """One [n_fit + n_q, F] device matrix and the two row lists."""
    x = _dev(np.concatenate([fit, q]))
    rows = torch.arange(x.shape[0], dtype=torch.int64, device=x.device)
    return x, rows[:fit.shape[0]].contiguous(), rows[fit.shape[0]:].contiguous()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_the_restatement(shape):
    from igcn_amd import ops
    n, nq, f, k = shape
    fit, q, ref = _case(shape)
    print(f"{shape}: min_gap {ref['min_gap']:.3e} order_gap {ref['order_gap']:.3e} fallbacks {ref['fallbacks']}")
    assert ref["min_gap"] >= MIN_GAP and ref["order_gap"] >= MIN_GAP
    x, rows_fit, rows_q = _stacked(fit, q)
    rng = np.random.default_rng(7)
    scale = (rng.random(f) + 0.1).astype(np.float32)
    shift = (rng.random(f) - 0.5).astype(np.float32)
    sel = np.array(sorted({0, f // 2, f - 1}), dtype=np.int32)
    counts, means = ops.knn_impute_stats(x, rows_fit)
    full, picked, donors, status = ops.knn_impute(x, means, k, rows_fit, rows_q, _dev(scale), _dev(shift),
                                                   _dev(sel, torch.int32), want_donors=True)
    np.testing.assert_array_equal(counts.cpu().numpy(), (~np.isnan(fit)).sum(0))
    got_means = means.cpu().double().numpy()
    assert (np.abs(got_means - ref["means"]) <= 2.0 ** -23 * np.nanmax(np.abs(fit), axis=0)).all()
    np.testing.assert_array_equal(donors.cpu().numpy(), ref["donors"])
    assert int(status) == ref["fallbacks"]
    out = full.cpu().double().numpy()
    bound = value_bound(fit, q, ref, k)
    err = np.abs(out - ref["out"])
    use = float((err / bound)[bound > 0].max()) if (bound > 0).any() else 0.0
    print(f"{shape}: largest use of the value bound {use:.3f} (full), ", end="")
    assert (err <= bound).all()
    obs = ~np.isnan(q)
    assert _same_bits(full[torch.from_numpy(obs).cuda()], x[rows_q][torch.from_numpy(obs).cuda()])
    # the selected, rescaled columns against the restatement under the same affine (in fp64)
    s64, h64 = scale.astype(np.float64), shift.astype(np.float64)
    want = ref["out"][:, sel] * s64[sel] + h64[sel]
    bsel = value_bound(fit, q, ref, k, s64, h64)[:, sel]
    esel = np.abs(picked.cpu().double().numpy() - want)
    print(f"{float((esel / bsel).max()):.3f} (selected)")
    assert (esel <= bsel).all()


def test_no_affine_selects_the_same_bits():
    from igcn_amd import ops
    fit, q, _ = _case(SHAPES[0])
    x, rows_fit, rows_q = _stacked(fit, q)
    _, means = ops.knn_impute_stats(x, rows_fit)
    sel = torch.tensor([5, 7, 8], dtype=torch.int32, device=x.device)
    full, picked, _, _ = ops.knn_impute(x, means, 3, rows_fit, rows_q, None, None, sel)
    assert _same_bits(picked, full[:, [5, 7, 8]].contiguous())


def test_ties_go_to_the_lower_training_row():
    from igcn_amd import ops
    # training rows 1, 2, 4, 5 are bitwise duplicates on the receiver's observed columns (0 and 1) and differ in the
    # missing column 2; rows 0 and 3 are farther away
    fit = np.array([[9.0, 9.0, 100.0], [1.5, 2.5, 10.0], [1.5, 2.5, 20.0], [7.0, 0.5, 200.0], [1.5, 2.5, 40.0],
                    [1.5, 2.5, 80.0]])
    q = np.array([[1.25, 2.0, np.nan]])
    x, rows_fit, rows_q = _stacked(fit, q)
    _, means = ops.knn_impute_stats(x, rows_fit)
    for k, want_donors, want in ((1, [1], 10.0), (2, [1, 2], 15.0)):
        ref = knn_impute_ref(fit, q, k)
        assert ref["min_gap"] == 0.0 and ref["donors"][0, 2].tolist() == want_donors
        full, _, donors, status = ops.knn_impute(x, means, k, rows_fit, rows_q, want_donors=True)
        assert donors[0, 2].tolist() == want_donors and float(full[0, 2]) == want and int(status) == 0


def test_index_route_gives_the_bits_of_the_dense_call():
    from igcn_amd import ops
    n, nq, f, k = SHAPES[1]
    fit, q, ref = _case(SHAPES[1])
    dense, rows_fit, rows_q = _stacked(fit, q)
    _, means_d = ops.knn_impute_stats(dense, rows_fit)
    sel = torch.tensor([5, 7, 8], dtype=torch.int32, device=dense.device)
    scale, shift = _dev(np.linspace(0.5, 2.0, f)), _dev(np.linspace(-1.0, 1.0, f))
    full_d, sel_d, don_d, st_d = ops.knn_impute(dense, means_d, k, rows_fit, rows_q, scale, shift, sel, want_donors=True)
    # the same rows scattered over a larger [S, F] matrix whose other rows hold values that must not be read as donors
    s = n + nq + 13
    perm = torch.randperm(s, generator=torch.Generator().manual_seed(3)).cuda()
    pf, pq = perm[:n].contiguous(), perm[n:n + nq].contiguous()
    big = torch.full((s, f), 1.0e6, dtype=torch.float32, device=dense.device)
    big[pf], big[pq] = dense[rows_fit], dense[rows_q]
    counts, means = ops.knn_impute_stats(big, pf)
    assert _same_bits(means, means_d)
    sentinel = torch.full((s, 3), -123.25, dtype=torch.float32, device=dense.device)
    dest = sentinel.clone()
    full, into, don, st = ops.knn_impute(big, means, k, pf, pq, scale, shift, sel, into=dest, want_donors=True)
    assert into is dest
    assert _same_bits(full, full_d) and torch.equal(don, don_d) and int(st) == int(st_d) == ref["fallbacks"]
    assert _same_bits(dest[pq], sel_d)
    rest = torch.ones(s, dtype=torch.bool, device=dense.device)
    rest[pq] = False
    assert _same_bits(dest[rest], sentinel[rest])             # rows outside rows_q keep their bits


def test_two_runs_give_identical_bits():
    from igcn_amd import ops
    n, nq, f, k = SHAPES[3]
    fit, q, _ = _case(SHAPES[3])
    x, rows_fit, rows_q = _stacked(fit, q)
    sel = torch.tensor([0, 31], dtype=torch.int32, device=x.device)
    scale, shift = _dev(np.linspace(0.5, 2.0, f)), _dev(np.linspace(-1.0, 1.0, f))
    runs = []
    for _ in range(2):
        _, means = ops.knn_impute_stats(x, rows_fit)
        runs.append(ops.knn_impute(x, means, k, rows_fit, rows_q, scale, shift, sel, want_donors=True))
    (f0, s0, d0, t0), (f1, s1, d1, t1) = runs
    assert _same_bits(f0, f1) and _same_bits(s0, s1) and torch.equal(d0, d1) and int(t0) == int(t1)


def test_knn_imputer_class():
    from igcn_amd.impute import KNNImputer
    n, nq, f, k = SHAPES[0]
    fit, q, ref = _case(SHAPES[0])
    imp = KNNImputer(n_neighbors=k)
    xf, xq = _dev(fit), _dev(q)
    before = xq.clone()
    out = imp.fit(xf).transform(xq)
    assert _same_bits(xq.nan_to_num(7.0), before.nan_to_num(7.0)) and out.data_ptr() != xq.data_ptr()   # a new tensor
    assert (np.abs(out.cpu().double().numpy() - ref["out"]) <= value_bound(fit, q, ref, k)).all()
    assert int(imp.last_fallbacks) == ref["fallbacks"]
    own = knn_impute_ref(fit, fit, k)
    assert own["min_gap"] >= MIN_GAP
    both = KNNImputer(n_neighbors=k).fit_transform(xf)
    assert (np.abs(both.cpu().double().numpy() - own["out"]) <= value_bound(fit, fit, own, k)).all()
    assert not torch.isnan(both).any()


def test_refusals():
    from igcn_amd import ops
    from igcn_amd._lib import IgcnError
    from igcn_amd.impute import KNNImputer, impute_fold
    x = torch.rand(6, 4, device="cuda")
    x[:, 2] = float("nan")                                    # a column no training row observes
    with pytest.raises(ValueError):
        KNNImputer().fit(x)
    idx = torch.arange(3, device="cuda")
    with pytest.raises(ValueError):
        impute_fold(x, torch.zeros(6, 1, device="cuda"), idx, None, idx + 3, None, None, select_index=(2,))
    ok = torch.rand(6, 4, device="cuda")
    with pytest.raises(ValueError):                           # clini_score width is not len(select_index)
        impute_fold(ok, torch.zeros(6, 3, device="cuda"), idx, None, idx + 3, None, None, select_index=(1,))
    wide = torch.rand(5, 33, device="cuda")
    with pytest.raises(IgcnError):
        ops.knn_impute_stats(wide)
    with pytest.raises(IgcnError):
        ops.knn_impute(wide, torch.zeros(33, device="cuda"), 3)
    _, means = ops.knn_impute_stats(ok)
    with pytest.raises(IgcnError):
        ops.knn_impute(ok, means, 0)
    with pytest.raises(IgcnError):
        ops.knn_impute(ok, means, 33)


def test_row_index_outside_the_matrix_is_reported_and_never_read():
    from igcn_amd import ops
    from igcn_amd.impute import impute_fold
    fit, q, _ = _case(SHAPES[0])
    x, rows_fit, rows_q = _stacked(fit, q)
    s = x.shape[0]
    _, means = ops.knn_impute_stats(x, rows_fit)
    sel = torch.tensor([5, 7, 8], dtype=torch.int32, device=x.device)
    good = rows_q[:3].contiguous()
    bad = torch.stack([rows_q[0], torch.tensor(s, device=x.device), rows_q[1], torch.tensor(-1, device=x.device),
                       rows_q[2]]).contiguous()
    want_full, want_sel, _, _ = ops.knn_impute(x, means, 3, rows_fit, good, None, None, sel)
    sentinel = torch.full((s, 3), -123.25, dtype=torch.float32, device=x.device)
    dest = sentinel.clone()
    full, _, _, status = ops.knn_impute(x, means, 3, rows_fit, bad, None, None, sel, into=dest)
    assert int(status) == -2                                   # two receivers outside the matrix
    assert _same_bits(full[[0, 2, 4]].contiguous(), want_full) and _same_bits(dest[good], want_sel)
    assert _same_bits(full[1], means) and _same_bits(full[3], means)      # all-missing rows: the column means
    rest = torch.ones(s, dtype=torch.bool, device=x.device)
    rest[good] = False
    assert _same_bits(dest[rest], sentinel[rest])
    off = rows_fit.clone()
    off[4] = s + 5
    counts, _ = ops.knn_impute_stats(x, off)
    assert (counts == -1).all()
    with pytest.raises(ValueError):
        impute_fold(x, dest, off, None, good, None, None)


# ---- end to end: the reference-signature wrapper, the store route, a batch and a train step -----------------------
E2E_SEED = 11


def e2e_inputs():
    """48 synthetic subjects with NaNs written into ``demographics``, a MinMaxScaler-shaped object and a split."""
    from igcn_amd import synth
    from igcn_amd.data import Data
    graphs = synth.brain_graph_list(48, seed=5, rois=90, tsne_dim=16)
    graphs = [Data(**{k: v for k, v in g.__dict__.items() if k != "A"}) for g in graphs]
    rng = np.random.default_rng(E2E_SEED)
    for g in graphs:
        g.demographics = g.demographics * torch.linspace(0.5, 30.0, 9)
        g.demographics[torch.from_numpy(rng.random(9) < 0.2)] = float("nan")
    demo = torch.stack([g.demographics for g in graphs]).double().numpy()
    scaler = SimpleNamespace(scale_=1.0 / np.linspace(0.6, 31.0, 9), min_=-np.linspace(0.0, 0.4, 9))
    perm = rng.permutation(48)
    test_idx, val_idx, train_idx = perm[:10], perm[10:20], np.sort(perm[20:])
    return graphs, demo, scaler, train_idx, val_idx, test_idx


def test_end_to_end_lists_store_batch_and_step():
    from igcn_amd import synth
    from igcn_amd.impute import KNNImputationVal, affine_of, impute_store
    from igcn_amd.loader import UniformGraphStore
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    from igcn_amd.train import FlatAdam, train_step
    graphs, demo, scaler, train_idx, val_idx, test_idx = e2e_inputs()
    dev = torch.device("cuda", 0)
    store = UniformGraphStore(graphs, device=dev)             # (before the lists' clini_score is overwritten)
    sel = [5, 7, 8]
    lists = [[graphs[i] for i in idx] for idx in (train_idx, val_idx, test_idx)]
    args = SimpleNamespace(clinical_score_index=-1)
    train, test, val = KNNImputationVal(args, lists[0], lists[1], lists[2], scaler, k=3)
    assert train is lists[0] and val is lists[1] and test is lists[2]
    s64 = affine_of(scaler)[0].double().numpy(), affine_of(scaler)[1].double().numpy()
    for idx, ds in zip((train_idx, val_idx, test_idx), lists):
        ref = knn_impute_ref(demo[train_idx], demo[idx], 3)
        assert ref["min_gap"] >= MIN_GAP
        want = ref["out"][:, sel] * s64[0][sel] + s64[1][sel]
        bound = value_bound(demo[train_idx], demo[idx], ref, 3, s64[0], s64[1])[:, sel]
        got = torch.stack([d.clini_score for d in ds])
        assert got.dtype == torch.float32 and not got.is_cuda and got.shape == (len(idx), 3)
        assert (np.abs(got.double().numpy() - want) <= bound).all()
    # a single column
    one = [[graphs[i] for i in idx] for idx in (train_idx, test_idx)]
    keep = [torch.stack([d.clini_score for d in ds]) for ds in lists]
    from igcn_amd.impute import KNNImputation
    KNNImputation(SimpleNamespace(clinical_score_index=7), one[0], one[1], scaler, k=3)
    assert _same_bits(torch.stack([d.clini_score for d in one[0]]), keep[0][:, 1:2].contiguous())
    assert _same_bits(torch.stack([d.clini_score for d in one[1]]), keep[2][:, 1:2].contiguous())
    # the store route: the same subjects in the same order give the same bits, in place
    scale, shift = affine_of(scaler, dev)
    ti, vi, si = (torch.from_numpy(i).to(dev) for i in (train_idx, val_idx, test_idx))
    fb = impute_store(store, ti, vi, si, scale, shift)
    assert all(int(t) >= 0 for t in fb)
    col = store.cols["clini_score"]
    for idx, k3 in zip((ti, vi, si), keep):
        assert _same_bits(col[idx].cpu(), k3)
    assert not torch.isnan(col).any()
    batch = store.batch(si[:8].contiguous())
    assert _same_bits(batch.clini_score.cpu().view(8, 3), keep[2][:8].contiguous())
    pool = (40, 20, 10, 4, 1)
    go_snps, adj, pool_dim = synth.go_hierarchy(pool, seed=3)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, dev)
    torch.manual_seed(0)
    model = SGCN_GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, dev, rois=90, H_0=3, num_classes=3, isSoftSimilarity=True,
                            rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseProb4Regr=True, isImageOnly=False,
                            isSNPsOnly=False).to(dev)
    model.train()
    loss = train_step(model, FlatAdam(model.parameters(), lr=1e-3), batch)
    assert torch.isfinite(loss).all()
