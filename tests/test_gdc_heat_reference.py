"""The heat-kernel / threshold restatement (tests/gdc_heat_ref.py) against the reference's own util_gdc.py outputs
(tests/golden/gdc_heat.npz), the distance of every golden case from a flipped decision, and the argument errors of the
Python surface.  CPU only."""
import numpy as np
import pytest
import torch

import gdc_heat_ref as HR
from gdc_heat_ref import MARGIN, N_THRESHOLD, N_TOPK, threshold_cases, topk_cases


def test_fixture_holds_the_cases_of_the_issue(golden):
    store = golden("gdc_heat")
    got = [(r, k, t) for _, r, k, t, *_ in topk_cases(store)]
    assert got == [(90, 3, 5.0), (90, 5, 5.0), (12, 3, 5.0), (33, 2, 1.0), (96, 4, 5.0), (90, 3, 10.0)]
    a3 = store["topk3/A"]
    assert not np.array_equal(a3, a3.T) and np.count_nonzero(a3) == a3.size          # dense, NOT symmetric
    thr = [(kern, p, e, src.shape[0]) for _, kern, p, e, _, src, _, _ in threshold_cases(store)]
    assert thr[0] == ("heat", 5.0, 0.01, 90) and thr[1] == ("heat", 1.0, 0.01, 33) and thr[2] == ("ppr", 0.05, 1e-4, 90)
    assert max(empty for _, _, _, _, empty, *_ in threshold_cases(store)) >= 1       # a column that keeps nothing
    assert f"topk{N_TOPK}/A" not in store and f"thr{N_THRESHOLD}/cfg" not in store
    for v in store.values():
        assert v.dtype.kind in "fi"                                                  # arrays only


def test_restatement_reproduces_the_reference_topk(golden):
    for c, rois, k, t, a, ei, ew in topk_cases(golden("gdc_heat")):
        got_ei, got_ew = HR.diffusion(a, "heat", t, top_k=k)
        assert np.array_equal(got_ei, ei), c
        assert np.array_equal(got_ew, ew), c                      # same float64 arithmetic -> identical float32
        assert ei.shape[1] == rois * k


def test_restatement_reproduces_the_reference_threshold(golden):
    for c, kernel, param, eps, empty, a, ei, ew in threshold_cases(golden("gdc_heat")):
        got_ei, got_ew = HR.diffusion(a, kernel, param, eps=eps)
        assert np.array_equal(got_ei, ei), c
        assert np.array_equal(got_ew, ew), c
        assert a.shape[0] - len(np.unique(ei[1])) == empty, c


def test_every_case_is_far_from_a_flipped_decision(golden):
    store = golden("gdc_heat")
    for c, rois, k, t, a, *_ in topk_cases(store):
        gap = HR.margins(HR.heat_matrix(a, t), k=k)[0]
        print(f"top-k case {c}: margin {gap:.3g}")
        assert gap >= MARGIN, (c, gap)
    for c, kernel, param, eps, _, a, *_ in threshold_cases(store):
        gap = HR.margins(HR.diffusion_matrix(a, kernel, param), eps=eps)[1]
        print(f"threshold case {c}: margin {gap:.3g}")
        assert gap >= MARGIN, (c, gap)


def test_margins_on_a_known_matrix():
    s = np.array([[4.0, 1.0], [2.0, 3.0]])
    gap_k, gap_e = HR.margins(s, k=1, eps=2.5)
    assert gap_k == pytest.approx(0.5) and gap_e == pytest.approx(0.2)
    assert HR.margins(s, k=2) == (np.inf, np.inf)


def test_heat_matrix_is_the_scaled_exponential():
    """expm(-t (I - H)) = e^-t expm(t H): the form the device kernel computes."""
    from scipy.linalg import expm
    a = HR.synthetic_adjacency(np.random.default_rng(1), 20, 4)
    d = 1 / np.sqrt(a.sum(1))
    s = HR.heat_matrix(a, 3.0)
    assert np.allclose(s, np.exp(-3.0) * expm(3.0 * d[:, None] * a * d[None, :]), rtol=1e-12, atol=0)
    root = np.sqrt(a.sum(1))                   # H D^1/2 1 = D^1/2 1: the stationary direction is left alone
    assert np.allclose(s @ root, root, rtol=1e-12, atol=0)


def _data(rois=6):
    from igcn_amd.data import Data
    return Data(x=torch.rand(rois, 3), A=torch.rand(rois, rois), y=torch.tensor([1]), snps_feat=torch.rand(1, 54),
                clust_y=torch.tensor([0]), sbjID=torch.tensor([7]), tsne_fdim=torch.rand(1, 2),
                clini_score=torch.rand(3), demographics=torch.rand(2))


def test_threshold_without_the_host_read_is_refused():
    from igcn_amd import gdc
    with pytest.raises(ValueError, match="check=True"):
        gdc.diffusion(torch.rand(1, 6, 6), kernel="heat", eps=0.01, check=False)
    with pytest.raises(ValueError, match="check=True"):
        gdc.batch_from_dense(torch.rand(1, 6, 6), torch.rand(6, 3), eps=0.01, check=False)


def test_unknown_kernel_is_refused():
    from igcn_amd import gdc
    with pytest.raises(ValueError, match="'ppr' or 'heat'"):
        gdc.diffusion(torch.rand(1, 6, 6), kernel="cosine")


def test_feeder_refuses_the_threshold():
    from igcn_amd.loader import DeviceGdcFeeder
    with pytest.raises(ValueError, match="fixed edge count"):
        DeviceGdcFeeder(torch.rand(4, 6, 6), {"x": torch.rand(4, 6, 3)}, 2, steps=1, kernel="heat", eps=0.01)
    with pytest.raises(ValueError, match="'ppr' or 'heat'"):
        DeviceGdcFeeder(torch.rand(4, 6, 6), {"x": torch.rand(4, 6, 3)}, 2, steps=1, kernel="cosine")


def test_preprocess_refuses_the_branch_that_is_not_reproduced():
    from igcn_amd import gdc
    with pytest.raises(ValueError, match=r"util_gdc\.py:82"):
        gdc.preprocess_diffusion_imgs_snps(_data(), isPPr=False, isTopK=False)


def test_preprocess_has_the_signature_of_the_reference():
    import inspect
    from igcn_amd import gdc
    sig = inspect.signature(gdc.preprocess_diffusion_imgs_snps)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("data", inspect.Parameter.empty), ("isPPr", True), ("isTopK", True), ("top_k", 5), ("alpha", 0.05)]
    sig = inspect.signature(gdc.diffusion)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("adj", inspect.Parameter.empty), ("kernel", "ppr"), ("alpha", 0.05), ("t", 5.0), ("top_k", 3), ("eps", None),
        ("check", True)]
