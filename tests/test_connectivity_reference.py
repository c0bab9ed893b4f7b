"""CPU checks of the ROI x ROI connectivity maps (the dense form of cal_probability's edge mask,
kernel/sgcn_img_snp.py:133-151, and of the per-edge GATConv attention, kernel/sgcn.py:235-267): the restatement the GPU
tests compare with (tests/connectivity_ref.py) equals a brute-force loop and scipy's dense ``A``-shaped scatter, the GAT
maps behave as the definition says and rebuild the stand-in's layer outputs, the C ABI declares and binds the new entry
points, and the models and the cohort pass refuse what they must before anything is launched."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import connectivity_ref as C
from conftest import ROOT
from gat_standin import gat_conv
from igcn_amd import _lib

NAMES = ("igcn_edge_dense_map_supported", "igcn_edge_dense_map", "igcn_gat_stack_alpha_tile", "igcn_gat_stack_alpha")


# ---- 1. the dense-map restatement -------------------------------------------------------------------------------------
def test_dense_map_equals_the_brute_force_loop():
    ei, v = C.odd_batch()
    want, cnt = C.dense_map_loop(v, ei, 3, 7)
    got = C.dense_map(v, ei, 3, 7)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-15
    assert torch.equal(C.count_map(ei, 3, 7), cnt)
    assert float(cnt[0, 2, 5]) >= 3.0 and float(cnt[0, 4, 4]) >= 1.0                          # the copies; the self-loop
    assert float(got[1].abs().max()) == 0.0 and float(cnt[1].max()) == 0.0                    # the graph without edges
    assert int(cnt[0].sum()) == 13 and int(cnt[2].sum()) == 14                                # ragged
    # the fp32 stored-order mode: the bits of fp32 adds in stored order
    want32, _ = C.dense_map_loop(v.float(), ei, 3, 7, dtype=torch.float32)
    got32 = C.dense_map(v.float(), ei, 3, 7, stored_order_fp32=True)
    assert got32.dtype == torch.float32 and torch.equal(got32, want32)


def test_dense_map_has_the_orientation_of_A():
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(3)
    r = 11
    a = rng.random((r, r)) * (rng.random((r, r)) < 0.3)
    a[3, 8], a[8, 3] = 0.7, 0.0                                                 # asymmetric on purpose
    coo = sp.coo_matrix(a)
    ei = torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64))
    got = C.dense_map(torch.from_numpy(coo.data), ei, 1, r)[0]
    assert np.array_equal(got.numpy(), coo.toarray()) and np.array_equal(got.numpy(), a)
    assert float(got[3, 8]) == 0.7 and float(got[8, 3]) == 0.0


# ---- 2. the GAT map restatement ---------------------------------------------------------------------------------------
def _gat_case(seed=1, b=2, r=6, h0=3, f=4, layers=2):
    g = torch.Generator().manual_seed(seed)
    parts = []
    for k in range(b):
        e = torch.randint(0, r, (2, 12), generator=g)
        e = e[:, e[1] != 1]                                                     # nothing arrives at node 1
        e = torch.cat([e, e[:, :1], torch.tensor([[3], [3]])], 1)               # a duplicate and a stored self-loop
        parts.append(e + k * r)
    ei = torch.cat(parts, 1)
    ea = torch.rand(ei.shape[1], generator=g, dtype=torch.float64)
    x = torch.randn(b * r, h0, generator=g, dtype=torch.float64)
    par = []
    for l in range(layers):
        fin = h0 if l == 0 else f
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.7          # noqa: E731
        par.append((rnd(f, fin), rnd(f), rnd(f), rnd(f, 1), rnd(f), rnd(f) * 0.1))        # W, a_s, a_d, lin_edge, a_e, bias
    return x, ei, ea, par, b, r


def test_gat_maps_follow_the_definition_and_rebuild_the_layers():
    x, ei, ea, par, b, r = _gat_case()
    maps, outs = C.gat_maps(x, ei, ea, par, b, r)
    assert tuple(maps.shape) == (b, len(par), r, r)
    loops = ei[0] == ei[1]
    assert int(loops.sum()) >= b
    h = x
    for l, p in enumerate(par):
        g_l = maps[:, l]
        assert float((g_l.sum(1) - 1).abs().max()) <= 1e-12                     # every target column sums to 1
        out, alpha, (src, dst) = gat_conv(h, ei, ea, *p, return_alpha=True)
        n_kept = int((~loops).sum())
        assert torch.equal(src[n_kept:], torch.arange(b * r)) and torch.equal(dst[n_kept:], torch.arange(b * r))
        diag = torch.diagonal(g_l, dim1=1, dim2=2).reshape(-1)
        assert float((diag - alpha[n_kept:]).abs().max()) == 0.0                # the diagonal holds the added loop alone
        lonely = torch.arange(b) * r + 1
        assert float((diag[lonely] - 1).abs().max()) <= 1e-15                   # a target without incoming edges
        # stored self-loops hold 0: scattering the kept edges alone leaves the diagonal empty
        off = C.dense_map(alpha[:n_kept], torch.stack([src[:n_kept], dst[:n_kept]]), b, r)
        assert float(torch.diagonal(off, dim1=1, dim2=2).abs().max()) == 0.0
        assert float((off + torch.diag_embed(diag.view(b, r)) - g_l).abs().max()) <= 1e-15
        # the layer's output from its map
        h_lin = (h @ p[0].t()).view(b, r, -1)
        rebuilt = C.aggregate(g_l, h_lin, p[5]).reshape(b * r, -1)
        assert float((rebuilt - torch.relu(out)).abs().max()) <= 1e-12
        assert float((outs[l] - torch.relu(out)).abs().max()) == 0.0
        h = torch.relu(out)


# ---- 3. ABI -------------------------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "igcn.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name


def test_tile_widths_host_only():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    # the widest power-of-two tile of target columns with [R][tile] floats (two of them with counts) in 64 KB
    for r, cnt, tc in ((5, 1, 64), (90, 1, 64), (128, 1, 64), (129, 1, 32), (270, 1, 16), (512, 1, 16), (512, 0, 32),
                       (8192, 1, 1), (8193, 1, 0), (16384, 0, 1), (16385, 0, 0), (0, 0, 0)):
        assert lib.igcn_edge_dense_map_supported(r, cnt) == tc, (r, cnt)
    # beside the forward's LDS layout within 150 KB; outside the stack: nothing
    assert lib.igcn_gat_stack_alpha_tile(90, 270, 3, 16, 2) == 64
    assert lib.igcn_gat_stack_alpha_tile(90, 270, 3, 12, 2) == 0 and lib.igcn_gat_stack_alpha_tile(90, 270, 9, 16, 2) == 0
    assert lib.igcn_gat_stack_alpha_tile(90, 270, 3, 16, 5) == 0
    widths = set()
    for r, e in ((270, 810), (400, 1200), (480, 1440), (512, 4096)):
        tc = lib.igcn_gat_stack_alpha_tile(r, e, 3, 16, 2)
        base = lib.igcn_gat_stack_lds_bytes(r, e, 3, 16, 2, 0)
        widths.add(tc)
        if tc == 0:                                                             # not even one column fits
            assert base + r * 4 > 150 * 1024
            continue
        assert tc in (1, 2, 4, 8, 16, 32, 64) and base + r * tc * 4 <= 150 * 1024
        assert tc == 64 or base + r * 2 * tc * 4 > 150 * 1024
    assert 0 in widths and 64 in widths and len(widths) >= 3, widths


# ---- 4. refusals before any launch ------------------------------------------------------------------------------------
def _go_inputs():
    from igcn_amd import synth
    go_snps, adj, pool_dim = synth.go_hierarchy((60, 30, 20, 9, 1), seed=2)
    return synth.go_sparse_inputs(go_snps, adj, "cpu") + (pool_dim,)


def _batch_stub(rois=90, h0=3):
    return SimpleNamespace(x=torch.zeros(rois, h0), edge_index=torch.zeros(2, 0, dtype=torch.int64),
                           edge_attr=torch.zeros(0))


@pytest.mark.parametrize("gat", [False, True])
def test_unmasked_baseline_refuses_edge_importance(monkeypatch, gat):
    from calltrace import record_calls
    from igcn_amd.gcn_img_snp import GCN_IMGSNP
    a_g, a, pool_dim = _go_inputs()
    model = GCN_IMGSNP(2, 8, a_g, a, pool_dim, 32, "cpu", rois=90, H_0=3, num_classes=3, ifUseGAT=gat)
    seen = record_calls(monkeypatch)
    with pytest.raises(ValueError, match="edge_importance: GCN_IMGSNP trains no masks"):
        model.edge_importance(_batch_stub())
    with pytest.raises(ValueError, match="no masked pass"):
        model.gat_attention(_batch_stub(), isExplain=True)
    if not gat:
        with pytest.raises(ValueError, match="gat_attention: GCN_IMGSNP has GCNConv layers"):
            model.gat_attention(_batch_stub())
    assert seen == []


def test_gcnconv_models_refuse_gat_attention(monkeypatch):
    from calltrace import record_calls
    from igcn_amd.sgcn import SGCN_GCN, SGCN_Ori
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
    a_g, a, pool_dim = _go_inputs()
    models = [SGCN_GCN(None, 2, 8), SGCN_Ori(3, 8, 8, 8),
              SGCN_GCN_IMGSNP(2, 8, a_g, a, pool_dim, 32, "cpu", rois=90, H_0=3, num_classes=3),
              SGCN_GCN_CLUSTERLABEL(2, 8, a_g, a, pool_dim, 32, "cpu", H_0=3, num_features=3)]
    seen = record_calls(monkeypatch)
    for model in models:
        for mode in (True, False):
            model.train(mode)
            with pytest.raises(ValueError, match="gat_attention: .* has GCNConv layers"):
                model.gat_attention(_batch_stub())
            assert model.training == mode
        assert callable(model.edge_importance)
    assert seen == []


def test_guide_model_has_no_connectivity_methods():
    from igcn_amd.guide_img_snp import GUIDE_IMGSNP
    assert not hasattr(GUIDE_IMGSNP, "edge_importance") and not hasattr(GUIDE_IMGSNP, "gat_attention")


def test_connectivity_maps_refuses_before_any_launch(monkeypatch):
    from calltrace import record_calls
    from igcn_amd.sgcn import SGCN_GCN
    from igcn_amd.train import connectivity_maps
    model = SGCN_GCN(None, 2, 8)
    seen = record_calls(monkeypatch)
    with pytest.raises(ValueError, match="connectivity_maps: source='grad'"):
        connectivity_maps(model, [_batch_stub()], source="grad")
    with pytest.raises(ValueError, match="connectivity_maps: num_classes=0"):
        connectivity_maps(model, [_batch_stub()], num_classes=0)
    for source in ("mask", "gat"):
        with pytest.raises(ValueError, match="connectivity_maps: the loader is empty"):
            connectivity_maps(model, [], source=source)
    assert seen == []


def test_ops_shape_errors_raise_before_any_launch(monkeypatch):
    from calltrace import record_calls
    from igcn_amd import ops
    seen = record_calls(monkeypatch)
    plan = SimpleNamespace(n_nodes=14, n_edges=5, src32=torch.zeros(5, dtype=torch.int32), status=None,
                           _stack_dims=(7, 5))
    for values, rois in ((torch.zeros(5, dtype=torch.float64), 7), (torch.zeros(5, 1), 7), (torch.zeros(4), 7),
                         (torch.zeros(5), 4), (torch.zeros(5), 0), (torch.zeros(5), 7)):      # (the last: a CPU tensor)
        with pytest.raises(ValueError, match="edge_dense_map"):
            ops.edge_dense_map(values, plan, rois)
    par = [torch.zeros(4, 3)] + [torch.zeros(4)] * 5
    for x, ew, rois, pp in ((torch.zeros(14, 3), torch.zeros(5), 7, par[:5]), (torch.zeros(13, 3), torch.zeros(5), 7, par),
                            (torch.zeros(14, 3), torch.zeros(4), 7, par), (torch.zeros(14, 3), torch.zeros(5), 7, par)):
        with pytest.raises(ValueError, match="gat_stack_alpha"):
            ops.gat_stack_alpha(x, ew, plan, rois, *pp)
    assert seen == []
