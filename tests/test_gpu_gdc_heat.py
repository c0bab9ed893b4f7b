"""igcn_gdc_diffuse on the GPU: the heat kernel (batched fp64 matrix exponential in LDS) and the eps threshold against the
reference's own util_gdc.py outputs (tests/golden/gdc_heat.npz) and the fp64 restatement (tests/gdc_heat_ref.py).
Edge indices and counts are exact, weights are held to rtol 3e-7 — the bound of tests/test_gdc.py: an fp64 value correct
to << 2^-24, rounded once to fp32."""
import numpy as np
import pytest
import torch

import gdc_heat_ref as HR
from gdc_cases import (COLS, HEAT, KEYS, PPR, RTOL, THRESHOLD, TOPK, adjacencies, assert_edges, assert_written,
                       batch_of_drawn, need_gpu, raw, same_batch)  # noqa: F401  (need_gpu: the module's autouse fixture)
from gdc_cases import subjects as drawn_subjects
from gdc_heat_ref import MARGIN, threshold_cases, topk_cases

pytestmark = pytest.mark.gpu


def test_heat_topk_vs_reference_golden(golden):
    from igcn_amd.gdc import diffusion
    for c, rois, k, t, a, ei, ew in topk_cases(golden("gdc_heat")):
        got = diffusion(torch.from_numpy(a).cuda()[None], kernel="heat", t=t, top_k=k)
        assert_edges(got, (ei, ew, [0, ei.shape[1]]), f"case {c}")


def test_threshold_vs_reference_golden(golden):
    """Both kernels; the last case has columns that keep nothing."""
    from igcn_amd.gdc import diffusion
    seen_empty = 0
    for c, kernel, param, eps, empty, a, ei, ew in threshold_cases(golden("gdc_heat")):
        got = diffusion(torch.from_numpy(a).cuda()[None], kernel=kernel, alpha=param, t=param, top_k=1, eps=eps)
        assert_edges(got, (ei, ew, [0, ei.shape[1]]), f"case {c} ({kernel})")
        seen_empty += empty
    assert seen_empty >= 1


@pytest.mark.parametrize("bsz,rois,k", [(7, 40, 5), (64, 90, 3)])
def test_heat_batch_vs_restatement(bsz, rois, k):
    from igcn_amd import ops
    from igcn_amd.gdc import batch_from_dense
    adjs = adjacencies(bsz, rois, seed=bsz)
    assert min(HR.margins(HR.heat_matrix(a, 5.0), k=k)[0] for a in adjs) >= MARGIN
    want_ei, want_ew, want_ptr = HR.diffusion_batch(adjs, "heat", 5.0, top_k=k)
    adj = torch.from_numpy(np.stack(adjs)).cuda()
    batch = batch_from_dense(adj, torch.rand(bsz * rois, 3, device="cuda"), top_k=k, kernel="heat", t=5.0,
                             snps_feat=torch.rand(bsz, 54, device="cuda"), clini_score=torch.rand(bsz, 3, device="cuda"))
    assert_edges((batch.edge_index, batch.edge_attr, batch.edge_ptr), (want_ei, want_ew, want_ptr))
    assert batch.num_graphs == bsz and batch._max_edges == rois * k
    plan = ops.plan_for(batch)
    assert plan.segmented
    plan.check()
    assert np.array_equal(plan.tgt_perm.cpu().numpy(), np.argsort(want_ei[1], kind="stable").astype(np.int32))


@pytest.mark.parametrize("kernel,param,eps", [("heat", 5.0, 0.02), ("ppr", 0.05, 0.03), ("heat", 5.0, 0.05)])
def test_threshold_batch_vs_restatement(kernel, param, eps):
    """A batch in threshold mode: graphs of different edge counts, squeezed; at eps = 0.05 some columns keep nothing."""
    from igcn_amd.gdc import batch_from_dense
    adjs = adjacencies(5, 40, seed=11)
    assert min(HR.margins(HR.diffusion_matrix(a, kernel, param), eps=eps)[1] for a in adjs) >= MARGIN
    want_ei, want_ew, want_ptr = HR.diffusion_batch(adjs, kernel, param, eps=eps)
    if eps == 0.05:
        assert 0 < len(np.unique(want_ei[1])) < 5 * 40                                 # empty columns are in the case
    adj = torch.from_numpy(np.stack(adjs)).cuda()
    batch = batch_from_dense(adj, torch.rand(5 * 40, 3, device="cuda"), kernel=kernel, alpha=param, t=param, eps=eps)
    assert_edges((batch.edge_index, batch.edge_attr, batch.edge_ptr), (want_ei, want_ew, want_ptr))
    assert batch._max_edges == int(np.diff(want_ptr).max())


def test_subject_list_with_an_index_outside_the_dataset():
    adjs = adjacencies(6, 40, seed=2)
    adj = torch.from_numpy(np.stack(adjs)).cuda()
    subject = torch.tensor([4, 6, 0, -1, 4], device="cuda")
    for sparsify, k, eps, cap in ((TOPK, 3, 0.0, 3), (THRESHOLD, 1, 0.02, 40)):
        ei, ew, counts = raw("resident", adj, HEAT, 5.0, sparsify, k, eps, subject=subject, n_subjects=6, bsz=5)
        ei, ew = ei.view(2, 5, 40 * cap), ew.view(5, 40 * cap)
        assert counts.tolist()[1] == 0 and counts.tolist()[3] == 0
        for g in (1, 3):
            assert bool((ei[:, g] == -1).all()) and float(ew[g].abs().max()) == 0.0
        for g, s in ((0, 4), (2, 0), (4, 4)):
            want_ei, want_ew = HR.diffusion(adjs[s], "heat", 5.0, top_k=k, eps=eps if sparsify else None)
            n = int(counts[g])
            assert n == want_ei.shape[1]
            assert np.array_equal(ei[:, g, :n].cpu().numpy(), want_ei + g * 40)
            np.testing.assert_allclose(ew[g, :n].cpu().numpy(), want_ew, rtol=RTOL, atol=0)
            assert bool((ei[:, g, n:] == -1).all()) and not bool(ew[g, n:].any())


def test_largest_supported_graph_and_one_beyond():
    from igcn_amd import _lib
    from igcn_amd.gdc import diffusion
    lib = _lib.load()
    rmax = lib.igcn_gdc_max_rois(HEAT)
    assert rmax >= 96 and lib.igcn_gdc_max_rois(PPR) == lib.igcn_gdc_topk_max_rois()
    a = adjacencies(1, rmax, seed=9, knn=9)[0]
    assert HR.margins(HR.heat_matrix(a, 5.0), k=3)[0] >= MARGIN
    want_ei, want_ew = HR.diffusion(a, "heat", 5.0, top_k=3)
    assert_edges(diffusion(torch.from_numpy(a).cuda()[None], kernel="heat", t=5.0, top_k=3),
                  (want_ei, want_ew, [0, want_ei.shape[1]]))
    with pytest.raises(_lib.IgcnError, match=f"max R = {rmax}"):
        diffusion(torch.rand(1, rmax + 1, rmax + 1, device="cuda"), kernel="heat", top_k=3)


@pytest.mark.parametrize("t", [0.0, 65.0])
def test_t_outside_the_interface_is_refused(t):
    from igcn_amd import _lib
    from igcn_amd.gdc import diffusion
    with pytest.raises(_lib.IgcnError, match=r"outside \(0,64\]"):
        diffusion(torch.rand(1, 12, 12, device="cuda"), kernel="heat", t=t)


def test_diffuse_ppr_topk_is_gdc_topk_bit_for_bit(golden):
    from igcn_amd._lib import call, ptr, stream_ptr
    store = golden("gdc")
    c = 0
    while f"case{c}/A" in store:
        rois, k, _ = [int(v) for v in store[f"case{c}/cfg"]]
        alpha = float(store[f"case{c}/alpha"])
        adj = torch.from_numpy(store[f"case{c}/A"]).cuda()[None].contiguous()
        ei = torch.full((2, rois * k), 7, dtype=torch.int64, device="cuda")
        ew = torch.full((rois * k,), 7.0, device="cuda")
        counts = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        call("igcn_gdc_topk", 1, rois, k, alpha, ptr(adj), ptr(ei), ptr(ew), ptr(counts), stream_ptr())
        got_ei, got_ew, got_counts = raw("resident", adj, PPR, alpha, TOPK, k, 0.0)
        assert torch.equal(got_ei, ei) and torch.equal(got_counts, counts), c
        assert torch.equal(got_ew.view(torch.int32), ew.view(torch.int32)), c
        c += 1
    assert c == 5


def test_two_runs_give_the_same_bits():
    adj = torch.from_numpy(np.stack(adjacencies(16, 90, seed=4))).cuda()
    for sparsify, k, eps in ((TOPK, 3, 0.0), (THRESHOLD, 1, 0.01)):
        one = raw("resident", adj, HEAT, 5.0, sparsify, k, eps)
        two = raw("resident", adj, HEAT, 5.0, sparsify, k, eps)
        for a, b in zip(one, two):
            assert torch.equal(a, b)
        assert torch.equal(one[1].view(torch.int32), two[1].view(torch.int32))


@pytest.mark.parametrize("sparsify,k,eps", [(TOPK, 3, 0.0), (THRESHOLD, 1, 0.02)])
def test_under_fenced_poisoned_allocations(sparsify, k, eps):
    """Every slot, padding included, has a writer, and nothing is written outside the three outputs."""
    from fenced import fenced, unwritten
    adjs = adjacencies(3, 33, seed=6)
    adj = torch.from_numpy(np.stack(adjs)).cuda()
    with fenced() as f:
        ei, ew, counts = raw("resident", adj, HEAT, 5.0, sparsify, k, eps)
        torch.cuda.synchronize()
        f.check()
        assert unwritten(ew) == 0
        assert_written(ei, ew, counts)
    want_ei, want_ew, want_ptr = HR.diffusion_batch(adjs, "heat", 5.0, top_k=k, eps=eps if sparsify else None)
    assert counts.tolist() == np.diff(want_ptr).tolist()
    valid = ei[0] >= 0
    assert np.array_equal(ei[:, valid].cpu().numpy(), want_ei)
    np.testing.assert_allclose(ew[valid].cpu().numpy(), want_ew, rtol=RTOL, atol=0)
    assert bool((ei[1][~valid] == -1).all()) and not bool(ew[~valid].any())


@pytest.fixture(scope="module")
def subjects():
    return drawn_subjects(20, rois=90)


def _heat_batch(adj, cols, idx):
    return batch_of_drawn(adj, cols, idx, top_k=3, kernel="heat", t=5.0)


def test_heat_feeder_equals_batch_from_dense(subjects):
    from igcn_amd.loader import DeviceGdcFeeder, EpochIndex, UniformGraphStore
    graphs, slim = subjects
    adj = torch.stack([g.A for g in graphs]).cuda()
    store = UniformGraphStore(slim, "cuda")
    cols = {k: store.cols[k] for k in COLS}
    feeder = DeviceGdcFeeder(adj, cols, 6, steps=4, top_k=3, seed=3, kernel="heat", t=5.0)
    order = EpochIndex(20, 6, seed=3, device="cuda")
    for batch in feeder:
        torch.cuda.current_stream().wait_event(batch.ready)
        want = _heat_batch(adj, cols, order.next())
        same_batch(batch, want, KEYS)
        batch.release()


def test_train_step_on_a_heat_batch(subjects):
    from igcn_amd import synth
    from igcn_amd.loader import UniformGraphStore
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    from igcn_amd.train import FlatAdam, train_step
    graphs, slim = subjects
    dev = torch.device("cuda")
    adj = torch.stack([g.A for g in graphs]).cuda()
    store = UniformGraphStore(slim, "cuda")
    batch = _heat_batch(adj, {k: store.cols[k] for k in COLS}, torch.arange(8, device="cuda"))
    assert batch.num_graphs == 8 and batch.edge_index.shape[1] == 8 * 90 * 3
    go_snps, go_adj, pool_dim = synth.go_hierarchy((40, 20, 10, 4, 1), seed=3)
    a_g, a = synth.go_sparse_inputs(go_snps, go_adj, dev)
    torch.manual_seed(0)
    model = SGCN_GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, dev, rois=90, H_0=3, num_classes=3, isSoftSimilarity=True,
                            rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseProb4Regr=True, isImageOnly=False,
                            isSNPsOnly=False).to(dev)
    model.train()
    loss = train_step(model, FlatAdam(model.parameters(), lr=1e-3), batch)
    assert torch.isfinite(loss).all()


def test_preprocess_diffusion_imgs_snps_on_one_subject(golden):
    """The reference's entry point for one Data: heat at its default t = 5, field list kept."""
    from igcn_amd.data import Data
    from igcn_amd.gdc import preprocess_diffusion_imgs_snps
    store = golden("gdc_heat")
    a, ei, ew = store["topk1/A"], store["topk1/edge_index"], store["topk1/edge_attr"]       # (90, k = 5, t = 5)
    data = Data(x=torch.rand(90, 3), A=torch.from_numpy(a).cuda(), y=torch.tensor([1]), snps_feat=torch.rand(1, 54),
                clust_y=torch.tensor([0]), sbjID=torch.tensor([7]), tsne_fdim=torch.rand(1, 2),
                clini_score=torch.rand(3), demographics=torch.rand(2))
    out = preprocess_diffusion_imgs_snps(data, isPPr=False, isTopK=True, top_k=5)
    assert np.array_equal(out.edge_index.cpu().numpy(), ei)
    np.testing.assert_allclose(out.edge_attr.cpu().numpy(), ew, rtol=RTOL, atol=0)
    assert sorted(out.keys) == sorted(["x", "edge_index", "edge_attr", "y", "A", "snps_feat", "clust_y", "sbjID",
                                       "tsne_fdim", "clini_score", "demographics"])
    assert out.x is data.x and out.A is data.A
