"""igcn_gdc_diffuse_tiled on the GPU (csrc/gdc_tiled.hip): the GDC pre-transform for graphs beyond the LDS limit, fp64
products on the matrix cores over a global-memory workspace.  Held to the reference's own util_gdc.py outputs
(tests/golden/gdc_heat.npz) and to the fp64 restatement (tests/gdc_heat_ref.py: numpy's inverse, scipy's expm) with the
bounds of tests/test_gpu_gdc_heat.py: edge_ptr and edge_index exact, weights rtol 3e-7 — an fp64 value correct to
<< 2^-24 (tests/test_gdc_tiled_reference.py: the recurrences err below 1e-12), rounded once to fp32.  Every test first
asserts that no decision on its inputs is within MARGIN of flipping."""
import numpy as np
import pytest
import torch

import gdc_heat_ref as HR
import gdc_tiled_ref as TR
from gdc_cases import (COLS, EPS, HEAT, KERNEL_ID, KEYS, PARAM, RTOL, THRESHOLD, TOPK, adjacencies, assert_edges,
                       assert_written, batch_of_drawn, matrices, need_gpu, poisoned, poisoned_workspace, raw, same_batch,
                       want, ws_need)  # noqa: F401  (need_gpu: the module's autouse fixture)
from gdc_cases import subjects as drawn_subjects
from gdc_heat_ref import MARGIN, threshold_cases, topk_cases

pytestmark = pytest.mark.gpu

# an eps at which about half of the columns keep nothing (the median of the column maxima, found on the CPU)
EMPTY_EPS = {(33, "heat"): 0.052, (33, "ppr"): 0.084, (129, "heat"): 0.036, (129, "ppr"): 0.066}


# ---- the reference's own outputs through the new route ---------------------------------------------------------------
def test_heat_topk_vs_reference_golden(golden):
    from igcn_amd.gdc import diffusion_routed
    for c, rois, k, t, a, ei, ew in topk_cases(golden("gdc_heat")):
        assert HR.margins(HR.heat_matrix(a, t), k=k)[0] >= MARGIN
        got = diffusion_routed(torch.from_numpy(a).cuda()[None], kernel="heat", t=t, top_k=k, route="tiled")
        assert_edges(got, (ei, ew, [0, ei.shape[1]]), f"case {c}")


def test_threshold_vs_reference_golden(golden):
    """Both kernels; the last case has columns that keep nothing."""
    from igcn_amd.gdc import diffusion_routed
    seen_empty = 0
    for c, kernel, param, eps, empty, a, ei, ew in threshold_cases(golden("gdc_heat")):
        assert HR.margins(HR.diffusion_matrix(a, kernel, param), eps=eps)[1] >= MARGIN
        got = diffusion_routed(torch.from_numpy(a).cuda()[None], kernel=kernel, alpha=param, t=param, top_k=1, eps=eps,
                               route="tiled")
        assert_edges(got, (ei, ew, [0, ei.shape[1]]), f"case {c} ({kernel})")
        seen_empty += empty
    assert seen_empty >= 1


def test_ppr_topk_vs_reference_golden(golden):
    """tests/golden/gdc.npz: the reference's get_ppr_matrix + get_top_k_matrix outputs."""
    from igcn_amd.gdc import diffusion_topk
    store, c = golden("gdc"), 0
    while f"case{c}/A" in store:
        rois, k, _ = [int(v) for v in store[f"case{c}/cfg"]]
        alpha, a = float(store[f"case{c}/alpha"]), store[f"case{c}/A"]
        assert HR.margins(HR.OG.ppr_matrix(a.astype(np.float64), alpha), k=k)[0] >= MARGIN
        want_ei, want_ew = HR.OG.diffusion_topk(a, k, alpha)
        got = diffusion_topk(torch.from_numpy(a).cuda()[None], top_k=k, alpha=alpha, route="tiled")
        assert_edges(got, (want_ei, want_ew, [0, want_ei.shape[1]]), f"case {c}")
        c += 1
    assert c == 5


# ---- tile seams ----------------------------------------------------------------------------------------------------------
# 15 / 16 / 17: around one MFMA tile; 33: the case size of the resident tests; 97 / 129: the first sizes past the
# resident heat / PPR limits (129: the first with three 64-tiles a side); 264: not a multiple of 16, five tiles a side
@pytest.mark.parametrize("kernel", ["heat", "ppr"])
@pytest.mark.parametrize("rois", [15, 16, 17, 33, 97, 129, 264])
def test_tile_seams_vs_restatement(rois, kernel):
    from igcn_amd.gdc import diffusion_routed
    param = PARAM[kernel]
    adjs = adjacencies(3, rois, seed=rois)
    mats = matrices(("seam", rois), adjs, kernel, param)
    for bsz in (1, 3):
        adj = torch.from_numpy(np.stack(adjs[:bsz])).cuda()
        cases = [dict(top_k=1), dict(top_k=3), dict(top_k=rois), dict(eps=EPS[kernel])]
        if (rois, kernel) in EMPTY_EPS:
            cases.append(dict(eps=EMPTY_EPS[(rois, kernel)]))
        for case in cases:
            k, eps = case.get("top_k"), case.get("eps")
            exp = want(mats[:bsz], k=k, eps=eps)
            if eps is not None and (rois, kernel) in EMPTY_EPS and eps == EMPTY_EPS[(rois, kernel)]:
                assert 0 < len(np.unique(exp[0][1])) < bsz * rois                     # columns that keep nothing
            got = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, top_k=k or 1, eps=eps, route="tiled")
            assert_edges(got, exp, f"R={rois} B={bsz} {kernel} {case}")


@pytest.mark.parametrize("kernel", ["heat", "ppr"])
def test_512_regions(kernel):
    """The full-size products, once per kernel: eight tiles a side."""
    from igcn_amd.gdc import diffusion_routed
    param = PARAM[kernel]
    adjs = [adjacencies(1, 512, seed=9, knn=9)[0], adjacencies(1, 512, seed=512, knn=5)[0]]
    mats = matrices(("512",), adjs, kernel, param)
    adj = torch.from_numpy(np.stack(adjs)).cuda()
    for case in (dict(top_k=3), dict(eps=EPS[kernel])):
        k, eps = case.get("top_k"), case.get("eps")
        got = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, top_k=k or 1, eps=eps, route="tiled")
        assert_edges(got, want(mats, k=k, eps=eps), f"R=512 B=2 {kernel} {case}")


@pytest.mark.parametrize("kernel,param", [("heat", 5.0), ("ppr", 0.05)])
def test_aal_116(kernel, param):
    from igcn_amd.gdc import diffusion_routed
    adjs = adjacencies(1, 116, seed=116)
    mats = matrices(("aal",), adjs, kernel, param)
    got = diffusion_routed(torch.from_numpy(adjs[0]).cuda()[None], kernel=kernel, alpha=param, t=param, top_k=3,
                           route="tiled")
    assert_edges(got, want(mats, k=3), f"R=116 {kernel}")


# ---- one batch, different scaling exponents ----------------------------------------------------------------------------
def _knn_and_hub(rois=97):
    rng = np.random.default_rng(7)
    knn, hub = HR.synthetic_adjacency(rng, rois, 5), HR.synthetic_adjacency(rng, rois, 5)
    w = rng.random(rois) * 0.5 + 0.5                      # a hub node joined to every other
    hub[0, :] = w
    hub[:, 0] = w
    hub[0, 0] = 0.0
    return [knn.astype(np.float32), hub.astype(np.float32)]


@pytest.mark.parametrize("t", [1.0, 5.0, 10.0])
def test_mixed_scaling_exponents_in_one_batch(t):
    from igcn_amd.gdc import diffusion_routed
    adjs = _knn_and_hub()
    s = [TR.heat_exponent(a, t) for a in adjs]
    norms = [TR.heat_norm(a, t) for a in adjs]
    print(f"t={t}: |tH|_1 = {norms[0]:.4g}, {norms[1]:.4g} -> s = {s}")
    assert s[0] < s[1] <= TR.heat_max_squarings(t, 97)
    for n, e in zip(norms, s):                            # the exponent is not a rounding away from another one
        assert n / 2.0 ** e <= 0.5 * (1 - 1e-9) and (e == 0 or n / 2.0 ** (e - 1) >= 0.5 * (1 + 1e-9))
    mats = matrices(("hub",), adjs, "heat", t)
    for order in ((0, 1), (1, 0, 0)):
        adj = torch.from_numpy(np.stack([adjs[g] for g in order])).cuda()
        got = diffusion_routed(adj, kernel="heat", t=t, top_k=3, route="tiled")
        assert_edges(got, want([mats[g] for g in order], k=3), f"t={t} graphs {order}")


# ---- subject list ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["heat", "ppr"])
def test_subject_list_with_repeats_and_an_index_outside_the_dataset(kernel):
    rois, param = 97, PARAM[kernel]
    adjs = adjacencies(3, rois, seed=rois)
    mats = matrices(("seam", rois), adjs, kernel, param)
    adj = torch.from_numpy(np.stack(adjs)).cuda()
    subject = torch.tensor([2, 3, 0, -1, 2], device="cuda")
    for sparsify, k, eps, cap in ((TOPK, 3, 0.0, 3), (THRESHOLD, 1, EPS[kernel], rois)):
        ei, ew, counts = raw("tiled", adj, KERNEL_ID[kernel], param, sparsify, k, eps, subject=subject, n_subjects=3, bsz=5)
        ei, ew = ei.view(2, 5, rois * cap), ew.view(5, rois * cap)
        assert counts.tolist()[1] == 0 and counts.tolist()[3] == 0
        for g in (1, 3):
            assert bool((ei[:, g] == -1).all()) and float(ew[g].abs().max()) == 0.0
        for g, s in ((0, 2), (2, 0), (4, 2)):
            want_ei, want_ew, _ = want([mats[s]], k=k if sparsify == TOPK else None, eps=eps if sparsify else None)
            n = int(counts[g])
            assert n == want_ei.shape[1]
            assert np.array_equal(ei[:, g, :n].cpu().numpy(), want_ei + g * rois)
            np.testing.assert_allclose(ew[g, :n].cpu().numpy(), want_ew, rtol=RTOL, atol=0)
            assert bool((ei[:, g, n:] == -1).all()) and not bool(ew[g, n:].any())


# ---- hygiene -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["heat", "ppr"])
def test_every_slot_is_written_and_two_runs_give_the_same_bits(kernel):
    """Outputs full of NaN / -7, workspace full of NaN, everything inside fenced allocations."""
    from fenced import fenced
    rois, param = 33, PARAM[kernel]
    adjs = adjacencies(3, rois, seed=rois)
    mats = matrices(("seam", rois), adjs, kernel, param)
    adj = torch.from_numpy(np.stack(adjs)).cuda()
    for sparsify, k, eps in ((TOPK, 3, 0.0), (THRESHOLD, 1, EMPTY_EPS[(rois, kernel)])):
        with fenced() as f:
            one = raw("tiled", adj, KERNEL_ID[kernel], param, sparsify, k, eps)
            two = raw("tiled", adj, KERNEL_ID[kernel], param, sparsify, k, eps)
            torch.cuda.synchronize()
            f.check()
        ei, ew, counts = one
        assert_written(ei, ew, counts)
        for a, b in zip(one, two):
            assert torch.equal(a, b)
        assert torch.equal(one[1].view(torch.int32), two[1].view(torch.int32))
        want_ei, want_ew, want_ptr = want(mats, k=k if sparsify == TOPK else None, eps=eps if sparsify else None)
        assert counts.tolist() == np.diff(want_ptr).tolist()
        valid = ei[0] >= 0
        assert np.array_equal(ei[:, valid].cpu().numpy(), want_ei)
        np.testing.assert_allclose(ew[valid].cpu().numpy(), want_ew, rtol=RTOL, atol=0)
        assert bool((ei[1][~valid] == -1).all()) and not bool(ew[~valid].any())
        # padding only behind the edges of a graph
        cap = k if sparsify == TOPK else rois
        for g in range(3):
            n = int(counts[g])
            assert bool(valid[g * rois * cap: g * rois * cap + n].all()) and not bool(valid[g * rois * cap + n: (g + 1) * rois * cap].any())


@pytest.mark.parametrize("kernel", ["heat", "ppr"])
def test_chunked_run_equals_one_chunk_bit_for_bit(kernel):
    from igcn_amd.gdc import diffusion_routed
    rois, param = 129, PARAM[kernel]
    adj = torch.from_numpy(np.stack(adjacencies(3, rois, seed=rois))).cuda()
    one = ws_need(1, rois, KERNEL_ID[kernel])
    assert ws_need(3, rois, KERNEL_ID[kernel]) == 3 * one == TR.workspace_bytes(3, rois, kernel)
    for case in (dict(top_k=3), dict(top_k=1, eps=EPS[kernel])):
        whole = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, route="tiled", **case)
        for cap in (one, 2 * one + one // 2):                                   # three chunks of one; two chunks, 2 + 1
            parts = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, route="tiled", workspace_bytes=cap, **case)
            for a, b in zip(whole, parts):
                assert a.dtype == b.dtype and a.shape == b.shape
                assert torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))


@pytest.mark.parametrize("kernel", ["heat", "ppr"])
def test_python_surface_inside_fences(kernel):
    """The buffers the Python layer itself allocates for the tiled route — outputs, workspace, the per-chunk index buffer,
    the feeder's workspace — between fences: nothing is written outside them, and the result is that of a plain run."""
    from fenced import fenced
    from igcn_amd.gdc import diffusion_routed
    from igcn_amd.loader import DeviceGdcFeeder
    rois, param = 97, PARAM[kernel]
    adj = torch.from_numpy(np.stack(adjacencies(3, rois, seed=rois))).cuda()
    one = ws_need(1, rois, KERNEL_ID[kernel])
    plain = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, top_k=3, route="tiled")
    with fenced() as f:
        whole = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, top_k=3, route="tiled")
        parts = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, top_k=3, route="tiled", workspace_bytes=one)
        thr = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, eps=EPS[kernel], route="tiled",
                               workspace_bytes=2 * one)
        feeder = DeviceGdcFeeder(adj, {"x": torch.rand(3, rois, 3, device="cuda")}, 2, steps=1, top_k=3, kernel=kernel,
                                 alpha=param, t=param, route="tiled")
        for batch in feeder:
            torch.cuda.current_stream().wait_event(batch.ready)
            batch.release()
        torch.cuda.synchronize()
        f.check()
        assert f.passed["other"] == 0, f.other_sites
        assert {s.split(":")[0] for s in f.sites} >= {"ig-gcn_amd/gdc.py"}
    for got in (whole, parts):
        for a, b in zip(plain, got):
            assert torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))
    assert_edges(thr, want(matrices(("seam", rois), adjacencies(3, rois, seed=rois), kernel, param), eps=EPS[kernel]),
                  f"fenced threshold {kernel}")


# ---- the routes agree ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["heat", "ppr"])
@pytest.mark.parametrize("rois", [90, 96])
def test_resident_and_tiled_agree(rois, kernel):
    from igcn_amd.gdc import diffusion_routed
    param = PARAM[kernel]
    adjs = adjacencies(3, rois, seed=rois)
    mats = matrices(("seam", rois), adjs, kernel, param)
    adj = torch.from_numpy(np.stack(adjs)).cuda()
    for case in (dict(top_k=3), dict(top_k=1, eps=EPS[kernel])):
        exp = want(mats, k=None if "eps" in case else 3, eps=case.get("eps"))
        res = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, route="resident", **case)
        til = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, route="tiled", **case)
        assert torch.equal(res[0], til[0]) and torch.equal(res[2], til[2])
        assert_edges(res, exp, f"R={rois} {kernel} resident {case}")
        assert_edges(til, exp, f"R={rois} {kernel} tiled {case}")
        if rois == 90:
            auto = diffusion_routed(adj, kernel=kernel, alpha=param, t=param, route="auto", **case)
            for a, b in zip(auto, res):
                assert torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))


def test_one_past_the_resident_limit():
    from igcn_amd import _lib
    from igcn_amd.gdc import batch_from_dense, diffusion, diffusion_routed
    lib = _lib.load()
    rois = lib.igcn_gdc_max_rois(HEAT) + 1
    assert rois == 97 and lib.igcn_gdc_tiled_max_rois() == 512
    adjs = adjacencies(3, rois, seed=rois)
    exp = want(matrices(("seam", rois), adjs, "heat", 5.0), k=3)
    adj = torch.from_numpy(np.stack(adjs)).cuda()
    with pytest.raises(_lib.IgcnError, match=f"max R = {rois - 1}"):
        diffusion(adj, kernel="heat", t=5.0, top_k=3)
    with pytest.raises(_lib.IgcnError, match=f"max R = {rois - 1}"):
        batch_from_dense(adj, torch.rand(3 * rois, 3, device="cuda"), kernel="heat", t=5.0)
    for route in ("auto", "tiled"):
        assert_edges(diffusion_routed(adj, kernel="heat", t=5.0, top_k=3, route=route), exp, f"R={rois} {route}")


def test_preprocess_takes_a_graph_beyond_the_resident_limit():
    from igcn_amd.data import Data
    from igcn_amd.gdc import preprocess_diffusion_imgs_snps
    a = adjacencies(3, 129, seed=129)[0]
    for is_ppr, kernel in ((True, "ppr"), (False, "heat")):
        want_ei, want_ew, _ = want([matrices(("seam", 129), adjacencies(3, 129, seed=129), kernel, PARAM[kernel])[0]], k=5)
        data = Data(x=torch.rand(129, 3), A=torch.from_numpy(a).cuda(), y=torch.tensor([1]), snps_feat=torch.rand(1, 54),
                    clust_y=torch.tensor([0]), sbjID=torch.tensor([7]), tsne_fdim=torch.rand(1, 2),
                    clini_score=torch.rand(3), demographics=torch.rand(2))
        out = preprocess_diffusion_imgs_snps(data, isPPr=is_ppr, isTopK=True, top_k=5)
        assert np.array_equal(out.edge_index.cpu().numpy(), want_ei)
        np.testing.assert_allclose(out.edge_attr.cpu().numpy(), want_ew, rtol=RTOL, atol=0)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_513_regions_are_refused():
    from igcn_amd import _lib
    from igcn_amd.gdc import diffusion_routed
    with pytest.raises(_lib.IgcnError, match=r"exceeds the kernel's limit \(max R = 512\)"):
        diffusion_routed(torch.rand(1, 513, 513, device="cuda"), kernel="heat", route="tiled")
    with pytest.raises(_lib.IgcnError, match=r"exceeds the kernel's limit \(max R = 512\)"):
        diffusion_routed(torch.rand(1, 513, 513, device="cuda"), kernel="ppr", route="auto")


@pytest.mark.parametrize("kernel", ["heat", "ppr"])
def test_a_workspace_one_byte_short_is_refused(kernel):
    from igcn_amd import _lib
    from igcn_amd.gdc import diffusion_routed
    need = ws_need(2, 40, KERNEL_ID[kernel])
    assert need == TR.workspace_bytes(2, 40, kernel)
    adj = torch.from_numpy(np.stack(adjacencies(2, 40, seed=2))).cuda()
    with pytest.raises(_lib.IgcnError, match=f"needs {need} bytes"):
        raw("tiled", adj, KERNEL_ID[kernel], PARAM[kernel], TOPK, 3, 0.0, ws_bytes=need - 1)
    with pytest.raises(_lib.IgcnError, match=f"needs {need // 2} bytes"):               # the Python cap, below one graph
        diffusion_routed(adj, kernel=kernel, route="tiled", workspace_bytes=need // 2 - 1)


@pytest.mark.parametrize("t", [0.0, 65.0])
def test_t_outside_the_interface_is_refused(t):
    from igcn_amd import _lib
    from igcn_amd.gdc import diffusion_routed
    with pytest.raises(_lib.IgcnError, match=r"outside \(0,64\]"):
        diffusion_routed(torch.rand(1, 12, 12, device="cuda"), kernel="heat", t=t, route="tiled")


def test_alpha_below_the_minimum_is_refused():
    from igcn_amd import _lib
    from igcn_amd.gdc import diffusion_routed
    adj = torch.from_numpy(adjacencies(1, 17, seed=17)[0]).cuda()[None]
    for alpha in (TR.ALPHA_MIN * 0.99, 0.0, 1.5):
        with pytest.raises(_lib.IgcnError, match=r"outside \[0\.001,1\]"):
            diffusion_routed(adj, kernel="ppr", alpha=alpha, top_k=3, route="tiled")
    # both ends of the interval are inside it
    a = adjacencies(1, 17, seed=17)
    for alpha in (TR.ALPHA_MIN, 1.0):
        s = [HR.OG.ppr_matrix(a[0].astype(np.float64), alpha)]
        if alpha == 1.0:                                  # P = I: one edge per node, nothing to decide
            ei, ew, ptr = diffusion_routed(adj, kernel="ppr", alpha=alpha, top_k=1, route="tiled")
            assert ei.cpu().tolist() == [list(range(17)), list(range(17))] and ew.cpu().tolist() == [1.0] * 17
        else:
            assert_edges(diffusion_routed(adj, kernel="ppr", alpha=alpha, top_k=3, route="tiled"), want(s, k=3),
                          f"alpha={alpha}")


# ---- feeder --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def subjects():
    return drawn_subjects(6, rois=130)


@pytest.mark.parametrize("kernel", ["ppr", "heat"])
def test_tiled_feeder_equals_batch_from_dense(subjects, kernel):
    from igcn_amd import ops
    from igcn_amd.loader import DeviceGdcFeeder, EpochIndex, UniformGraphStore
    graphs, slim = subjects
    adj = torch.stack([g.A for g in graphs]).cuda()
    param = PARAM[kernel]
    assert min(HR.margins(HR.diffusion_matrix(a.cpu().numpy(), kernel, param), k=3)[0] for a in adj) >= MARGIN
    store = UniformGraphStore(slim, "cuda")
    cols = {k: store.cols[k] for k in COLS}
    feeder = DeviceGdcFeeder(adj, cols, 2, steps=2, top_k=3, seed=3, kernel=kernel, alpha=param, t=param, route="tiled")
    assert feeder.route == "tiled" and feeder._ws.numel() == ws_need(2, 130, KERNEL_ID[kernel])
    order = EpochIndex(6, 2, seed=3, device="cuda")
    for batch in feeder:
        torch.cuda.current_stream().wait_event(batch.ready)
        same_batch(batch, batch_of_drawn(adj, cols, order.next(), top_k=3, kernel=kernel, alpha=param, t=param,
                                         route="tiled"), KEYS)
        ops.plan_for(batch).check()
        batch.release()


# ---- the Python surface: one launcher, one body ----------------------------------------------------------------------------
@pytest.mark.parametrize("sparsify", [TOPK, THRESHOLD])
@pytest.mark.parametrize("kernel", ["ppr", "heat"])
@pytest.mark.parametrize("route", ["resident", "tiled"])
def test_launch_into_is_the_entry_point_and_nothing_more(route, kernel, sparsify):
    """gdc.launch_into against the C entry point called by hand (gdc_cases.raw), both into poisoned buffers: five graphs
    drawn from six matrices of 33 regions by a subject list with a repeat, an index past the end and a negative one."""
    from igcn_amd import gdc
    rois, k, param = 33, 3, PARAM[kernel]
    eps = EPS[kernel] if sparsify == THRESHOLD else 0.0
    adj = torch.from_numpy(np.stack(adjacencies(6, rois, seed=rois))).cuda()
    subject = torch.tensor([4, 6, 0, -1, 4], device="cuda")
    by_hand = raw(route, adj, KERNEL_ID[kernel], param, sparsify, k, eps, subject=subject, n_subjects=6, bsz=5)
    ei, ew, counts = poisoned(5, rois, k if sparsify == TOPK else rois)
    nbytes = ws_need(5, rois, KERNEL_ID[kernel]) if route == "tiled" else 0
    ws = poisoned_workspace(nbytes) if route == "tiled" else None
    gdc.launch_into(route, kernel, param, sparsify, k, eps, adj, 6, subject, 5, ei, ew, counts, ws, nbytes)
    assert_written(ei, ew, counts)
    assert torch.equal(ei, by_hand[0]) and torch.equal(counts, by_hand[2])
    assert torch.equal(ew.view(torch.int32), by_hand[1].view(torch.int32))
    got = counts.tolist()
    assert got[1] == 0 and got[3] == 0 and got[0] == got[4] > 0 and got[2] > 0          # the list was followed


@pytest.mark.parametrize("route", ["resident", "tiled"])
def test_the_three_python_surfaces_are_one_body(route):
    from igcn_amd.gdc import diffusion, diffusion_routed, diffusion_topk
    adj = torch.from_numpy(np.stack(adjacencies(6, 33, seed=33))).cuda()
    one = diffusion_topk(adj, 3, route=route)
    others = [diffusion_routed(adj, "ppr", top_k=3, route=route)]
    if route == "resident":
        others.append(diffusion(adj, "ppr", top_k=3))
    assert int(one[2][-1]) > 0
    for got in others:
        for a, b in zip(one, got):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))
