"""CPU checks of the attention roll-out feature (go_model.py:208-251 rolled out to the SNPs; the ROI x SNP association
maps): the fp64 restatement the GPU tests compare with (tests/rollout_ref.py, sparse lists) equals a brute-force dense
formulation, its rows behave as the definition says, the C ABI declares and binds the new entry points, and the model
and the cohort pass refuse what they must before anything is launched."""
import os

import pytest
import torch

import rollout_ref as R
from conftest import ROOT
from igcn_amd import _lib

NAMES = ("igcn_go_attn_coeffs", "igcn_go_rollout_chunk", "igcn_go_rollout_layer")
POOL, S = (14, 8, 5, 2, 1), 54                                     # a 30-node hierarchy, two encoder layers


def _hierarchy(seed, every_node_has_a_snp):
    """(layers [(row_ptr, col, pool, N_l)], gene rows, gene cols) of a random 30-node hierarchy: lists of 0..4 entries,
    row 23 (kept by both layers) and row 3 without a list."""
    g = torch.Generator().manual_seed(seed)
    n = sum(POOL)
    adj = torch.rand(n, n, generator=g) < 0.08
    adj[23] = adj[3] = False
    adj[25, :5] = True                                             # reads nodes the first layer pools away
    layers, off = [], 0
    for l in range(2):
        sub = adj[off:, off:]
        rows, cols = sub.nonzero(as_tuple=True)
        row_ptr = torch.zeros(n - off + 1, dtype=torch.long)
        row_ptr[1:] = torch.bincount(rows, minlength=n - off).cumsum(0)
        layers.append((row_ptr, cols, POOL[l], n - off))
        off += POOL[l]
    gene = torch.rand(n, S, generator=g) < 0.1
    if every_node_has_a_snp:
        gene[torch.arange(n), torch.randint(0, S, (n,), generator=g)] = True
    else:
        gene[7] = gene[29] = False                                 # a leaf and the root without SNPs
    return layers, gene.nonzero(as_tuple=True)


def _inputs(seed, b=3, every_node_has_a_snp=False):
    g = torch.Generator().manual_seed(100 + seed)
    layers, (grow, gcol) = _hierarchy(seed, every_node_has_a_snp)
    ts = [torch.randn(grow.numel(), generator=g, dtype=torch.float64) for _ in range(2)]
    r0 = R.encoding_relevance(grow, gcol, ts, sum(POOL), S)
    coeffs, fin = [], 2
    for row_ptr, col, pool, n_l in layers:
        x = torch.randn(b, fin, n_l, generator=g, dtype=torch.float64)
        w_inc, w_s = torch.randn(5, fin, generator=g, dtype=torch.float64), torch.randn(5, fin, generator=g, dtype=torch.float64)
        a_in, a_s = torch.randn(10, generator=g, dtype=torch.float64), torch.randn(5, generator=g, dtype=torch.float64)
        alpha, beta = R.layer_coeffs(x, w_inc, w_s, a_in, a_s, row_ptr, col)
        coeffs.append((alpha, beta, row_ptr, col, pool, (x, w_inc, w_s, a_in, a_s)))
        fin = 5
    w = torch.softmax(torch.randn(b, 7, sum(POOL[2:]), generator=g, dtype=torch.float64), -1)
    return r0, coeffs, w


def _dense_rollout(r0, coeffs):
    """Brute force: per layer the dense N_l x N_l mixing matrix M_l (alpha on the list entries, beta on the diagonal,
    rows scaled to sum 1) from a dense restatement of the coefficients, sliced to the kept rows and multiplied."""
    b = coeffs[0][1].shape[0]
    r = r0.expand(b, *r0.shape)
    for _, _, row_ptr, col, pool, (x, w_inc, w_s, a_in, a_s) in coeffs:
        n = row_ptr.numel() - 1
        mask = torch.zeros(n, n, dtype=torch.bool)
        mask[R.row_of(row_ptr), col] = True
        x_in, x_s = (w_inc @ x).transpose(1, 2), (w_s @ x).transpose(1, 2)              # [B, N, f]
        score = torch.exp(torch.tanh((x_in @ a_in[:5])[:, :, None] + (x_in @ a_in[5:])[:, None, :]))
        score = torch.where(mask, score, torch.zeros_like(score))
        att = score / score.sum(-1, keepdim=True).clamp(min=1e-300)
        m = att + torch.diag_embed(torch.sigmoid(x_s @ a_s))
        m = m / m.sum(-1, keepdim=True)
        r = (m @ r)[:, pool:]
    return r


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_equals_dense_formulation(seed):
    r0, coeffs, w = _inputs(seed)
    rs = R.rollout(r0, [c[:5] for c in coeffs])
    want = _dense_rollout(r0, coeffs)
    assert tuple(rs[-1].shape) == (3, sum(POOL[2:]), S) == tuple(want.shape)
    assert float((rs[-1] - want).abs().max()) <= 1e-12
    assert float((R.association(w, rs[-1]) - w @ want).abs().max()) <= 1e-12


def test_rows_are_non_negative_and_sum_to_at_most_one():
    r0, coeffs, w = _inputs(0)
    assert float(r0[7].abs().max()) == 0.0 and float(r0[29].abs().max()) == 0.0      # no SNPs: the row stays 0
    rs = R.rollout(r0, [c[:5] for c in coeffs])
    assoc = R.association(w, rs[-1])
    for t in (rs[-1], assoc):
        assert float(t.min()) >= 0.0 and float(t.sum(-1).max()) <= 1.0 + 1e-12
    assert float(rs[-1].sum(-1).min()) < 1.0 - 1e-3                                  # (some mass is lost to those rows)


def test_rows_sum_to_one_when_every_node_has_a_snp():
    r0, coeffs, w = _inputs(1, every_node_has_a_snp=True)
    rs = R.rollout(r0, [c[:5] for c in coeffs])
    for t in (r0, rs[1], rs[-1], R.association(w, rs[-1])):
        assert float((t.sum(-1) - 1).abs().max()) <= 1e-12


def test_empty_row_passes_relevance_through():
    r0, coeffs, _ = _inputs(0)
    rs = R.rollout(r0, [c[:5] for c in coeffs])
    first, second = 23 - POOL[0], 23 - POOL[0] - POOL[1]          # node 23 as the first layer's output row, the second's
    for row_ptr, row in ((coeffs[0][2], 23), (coeffs[1][2], first)):
        assert int(row_ptr[row + 1] - row_ptr[row]) == 0
    assert torch.equal(rs[1][:, first], r0[23].expand(3, S))
    assert torch.equal(rs[2][:, second], r0[23].expand(3, S))


def test_header_and_binding_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "igcn.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name


def test_rollout_chunk_host_only():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    # the most relevance columns of one sample within 80 KB of LDS: 8 | 4 | 2 | 1, none above 20 480 nodes
    for n, ch in ((68, 8), (2560, 8), (2561, 4), (3000, 4), (5120, 4), (5121, 2), (10240, 2), (10241, 1), (20480, 1),
                  (20481, 0), (0, 0)):
        assert lib.igcn_go_rollout_chunk(n) == ch, n


def _cpu_model(**kw):
    from igcn_amd import synth
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    go_snps, adj, pool_dim = synth.go_hierarchy((60, 30, 20, 9, 1), seed=2)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cpu")
    return SGCN_GCN_IMGSNP(2, 8, a_g, a, pool_dim, 32, "cpu", rois=90, H_0=3, num_classes=3, **kw)


@pytest.mark.parametrize("kw", [dict(isImageOnly=True), dict(isCrossAtten=False, isImageOnly=False),
                                dict(isCrossAtten=True, isImageOnly=False, isSNPsOnly=True)])
def test_model_without_cross_attention_refuses_before_any_launch(monkeypatch, kw):
    from types import SimpleNamespace

    from calltrace import record_calls
    model = _cpu_model(**kw)
    seen = record_calls(monkeypatch)
    for mode in (True, False):
        model.train(mode)
        with pytest.raises(ValueError, match="snp_association: the model has no cross-attention"):
            model.snp_association(SimpleNamespace(x=torch.zeros(90, 3)))
        assert seen == [] and model.training == mode


def test_guide_model_has_no_snp_association():
    from igcn_amd.guide_img_snp import GUIDE_IMGSNP
    assert not hasattr(GUIDE_IMGSNP, "snp_association")
    from igcn_amd import guide_go_model
    with pytest.raises(NotImplementedError, match="GUIDE"):        # (its PReLU encoder is not the one rolled out)
        guide_go_model.Gene_ontology_network.attention_rollout(None, torch.zeros(1, 54))


def test_association_maps_refuses_an_empty_loader(monkeypatch):
    from calltrace import record_calls
    from igcn_amd.train import association_maps
    model = _cpu_model(isCrossAtten=True, isImageOnly=False)
    seen = record_calls(monkeypatch)
    with pytest.raises(ValueError, match="association_maps: the loader is empty"):
        association_maps(model, [])
    assert seen == []


def test_shape_errors_raise_before_any_launch(monkeypatch):
    from types import SimpleNamespace

    from calltrace import record_calls
    from igcn_amd import ops
    seen = record_calls(monkeypatch)
    csr = SimpleNamespace(n_rows=10, n_cols=10, nnz=7)
    f = torch.zeros
    with pytest.raises(ValueError, match="go_attention_coeffs"):
        ops.go_attention_coeffs(f(2, 2, 9), f(5, 2), f(5, 2), f(1, 10), f(1, 5), csr)          # 9 nodes, 10 rows
    with pytest.raises(ValueError, match="go_attention_coeffs"):
        ops.go_attention_coeffs(f(2, 2, 10), f(5, 2), f(5, 3), f(1, 10), f(1, 5), csr)         # w_s of another width
    with pytest.raises(ValueError, match="go_rollout_layer"):
        ops.go_rollout_layer(f(54, 10), f(2, 6), f(2, 10), csr, 4)                             # alpha: 6 of 7 entries
    with pytest.raises(ValueError, match="go_rollout_layer"):
        ops.go_rollout_layer(f(3, 54, 10), f(2, 7), f(2, 10), csr, 4)                          # 3 samples against 2
    with pytest.raises(ValueError, match="go_rollout_layer"):
        ops.go_rollout_layer(f(54, 10), f(2, 7), f(2, 10), csr, 10)                            # nothing left to keep
    with pytest.raises(ValueError, match="snp_association"):
        ops.snp_association(f(2, 90, 30), f(2, 29, 54))
    with pytest.raises(ValueError, match="snp_association"):
        ops.snp_association(f(2, 90, 30), f(3, 30, 54))
    assert seen == []
