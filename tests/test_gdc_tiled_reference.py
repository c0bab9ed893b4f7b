"""The product-only recurrences of the tiled GDC route (tests/gdc_tiled_ref.py) against the inverse and the matrix
exponential they replace (oracle/gdc.ppr_matrix: numpy's inv; tests/gdc_heat_ref.heat_matrix: scipy's expm), the inputs
of tests/test_gpu_gdc_tiled.py against a flipped decision, and the argument errors of the Python surface.  CPU only.

Bound: 1e-12 relative per element.  Measured here 0.7e-15 .. 3.1e-15 (PPR) and 1.4e-15 .. 3.2e-14 (heat); the bound
leaves room for another BLAS summation order."""
import os
import re

import numpy as np
import pytest
import torch

import gdc_heat_ref as HR
import gdc_tiled_ref as TR
from gdc_heat_ref import MARGIN
from oracle import gdc as OG

RTOL = 1e-12
# (R, seed, knn) of the GPU tests' inputs
INPUTS = [(17, 17, 5), (130, 1, 5), (264, 264, 5), (512, 9, 9)]


def _adj(rois, seed, knn):
    return HR.synthetic_adjacency(np.random.default_rng(seed), rois, knn)


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize("rois,seed,knn", INPUTS)
@pytest.mark.parametrize("alpha", [0.05, 0.15])
def test_ppr_recurrence_vs_the_inverse(rois, seed, knn, alpha):
    a = _adj(rois, seed, knn)
    err = _rel(TR.ppr_matrix(a, alpha), OG.ppr_matrix(a, alpha))
    print(f"R={rois} alpha={alpha}: J={TR.ppr_terms(alpha)}, largest relative element error {err:.3g}")
    assert err <= RTOL


@pytest.mark.parametrize("rois,seed,knn", INPUTS)
@pytest.mark.parametrize("t", [1.0, 5.0, 10.0])
def test_heat_recurrence_vs_expm(rois, seed, knn, t):
    a = _adj(rois, seed, knn)
    err = _rel(TR.heat_matrix(a, t), HR.heat_matrix(a, t))
    print(f"R={rois} t={t}: s={TR.heat_exponent(a, t)}, largest relative element error {err:.3g}")
    assert err <= RTOL


def test_number_of_terms_and_squarings():
    assert TR.ppr_terms(0.05) == 10 and TR.ppr_terms(0.15) == 8 and TR.ppr_terms(1.0) == 1
    assert TR.ppr_terms(TR.ALPHA_MIN) == 16 and TR.ppr_terms(TR.ALPHA_MIN * 0.6) == 17      # alpha_min: J <= 16
    a = _adj(130, 1, 5)
    assert [TR.heat_exponent(a, t) for t in (1.0, 5.0, 10.0)] == [2, 4, 5]
    for rois, seed, knn in INPUTS:
        a = _adj(rois, seed, knn)
        for t in (1.0, 5.0, 10.0, 64.0):
            # the squarings the host launches without a read cover what any symmetric graph needs: |H|_1 <= sqrt(R)
            assert TR.heat_norm(a, t) <= t * np.sqrt(rois)
            nrm = TR.heat_norm(a, t) / 2.0 ** TR.heat_exponent(a, t)
            assert nrm <= 0.5
    star = np.zeros((512, 512))
    star[0, 1:] = star[1:, 0] = 1.0                      # the extreme: a hub joined to every other node
    assert TR.heat_norm(star, 64.0) / 2.0 ** TR.heat_exponent(star, 64.0) <= 0.5
    assert TR.heat_max_squarings(64.0, 512) == 12


def test_alpha_one_is_the_identity():
    a = _adj(17, 17, 5)
    assert np.array_equal(TR.ppr_matrix(a, 1.0), np.eye(17))


@pytest.mark.parametrize("rois,seed,knn", [(116, 116, 5), (130, 1, 5), (264, 264, 5), (512, 9, 9), (512, 512, 5)])
def test_named_inputs_are_far_from_a_flipped_decision(rois, seed, knn):
    a = _adj(rois, seed, knn).astype(np.float32)
    gaps = [HR.margins(HR.heat_matrix(a, 5.0), k=3)[0], HR.margins(OG.ppr_matrix(a.astype(np.float64), 0.05), k=3)[0]]
    print(f"R={rois} seed={seed}: top-3 gaps heat {gaps[0]:.3g}, ppr {gaps[1]:.3g}")
    assert min(gaps) >= 1e-6 > MARGIN


def test_unknown_route_is_refused_before_the_device():
    from igcn_amd import gdc
    from igcn_amd.loader import DeviceGdcFeeder
    adj = torch.rand(1, 6, 6)                            # CPU tensors: a launch would raise IgcnError instead
    for fn in (lambda: gdc.diffusion_routed(adj, kernel="heat", route="nonsense"),
               lambda: gdc.diffusion_topk(adj, route="nonsense"),
               lambda: gdc.batch_from_dense(adj, torch.rand(6, 3), route="nonsense"),
               lambda: DeviceGdcFeeder(torch.rand(4, 6, 6), {"x": torch.rand(4, 6, 3)}, 2, steps=1, route="nonsense")):
        with pytest.raises(ValueError, match="route must be one of"):
            fn()


def test_routes_and_their_default():
    import inspect
    from igcn_amd import gdc
    from igcn_amd.loader import DeviceGdcFeeder
    assert gdc.ROUTES == ("resident", "tiled", "auto")
    for fn in (gdc.diffusion_routed, gdc.diffusion_topk, gdc.batch_from_dense, DeviceGdcFeeder.__init__):
        p = inspect.signature(fn).parameters
        assert p["route"].default == "resident", fn
    for fn in (gdc.diffusion_routed, gdc.diffusion_topk, gdc.batch_from_dense):
        assert inspect.signature(fn).parameters["workspace_bytes"].default is None, fn
    assert gdc.DEFAULT_WORKSPACE_BYTES >= TR.workspace_bytes(1, TR.MAX_ROIS, "ppr")


def test_header_declares_the_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "igcn.h")) as fh:
        text = fh.read()
    for decl in (r"int\s+igcn_gdc_tiled_max_rois\(void\);", r"size_t\s+igcn_gdc_tiled_workspace_bytes\(int B, int R, int kernel\);",
                 r"int\s+igcn_gdc_diffuse_tiled\(int B, int R, int kernel, double param, int sparsify, int k, double eps,"):
        assert re.search(decl, text), decl
    from igcn_amd import _lib
    for name in ("igcn_gdc_tiled_max_rois", "igcn_gdc_tiled_workspace_bytes", "igcn_gdc_diffuse_tiled"):
        assert name in _lib.SIGNATURES, name
