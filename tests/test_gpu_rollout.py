"""GPU tests of the attention roll-out through the GO encoder and the ROI x SNP association maps (go_model.py:208-251
rolled out to the SNPs, times the cross-attention weights of kernel/sgcn_img_snp.py:240): igcn_go_attn_coeffs,
igcn_go_rollout_layer, ops.snp_association, Gene_ontology_network.attention_rollout, SGCN_GCN_IMGSNP.snp_association and
train.association_maps against the fp64 restatement tests/rollout_ref.py fed the same fp32 inputs.

Bound: |got - want| <= 1e-6 + 1e-4 want element-wise — the one tests/test_gpu_attn_weights.py holds the sibling weights
kernel to; every quantity here is a quotient or a sum of non-negative terms with |tanh| <= 1.  Every comparison
prints its error as a fraction of the bound before it asserts (rollout_ref.assert_close); measured, the largest
fraction any element uses: alpha 2.9e-3, beta 4.4e-3, a layer's R 4.6e-3 (N = 10 241), the product 3.2e-3, the models'
association 2.3e-3, the bare network's R_top 2.5e-3."""
import numpy as np
import pytest
import torch

import rollout_ref as R
from _weights import seeded_state
from conftest import assert_matches

pytestmark = pytest.mark.gpu

POOL, S = (37, 18, 9, 3, 1), 54                 # N = 68 (no multiple of 64), pool no multiple of 4, 13 top-level terms
HUB, EMPTY_KEPT, EMPTY_POOLED = 50, 40, 5       # rows of the first layer's structure (all three below N)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _structure(n, seed, hub=None, empty=(), p=0.05):
    """ops.Csr of a random n x n structure: a row lists each column with probability p; ``hub``: a row that lists every
    column but two (> 64 entries at n = 68: the whole-wave walk); ``empty``: rows without a list."""
    from igcn_amd import ops
    g = torch.Generator().manual_seed(seed)
    adj = torch.rand(n, n, generator=g) < p
    if hub is not None:
        adj[hub] = True
        adj[hub, [3, hub]] = False
    for r in empty:
        adj[r] = False
    rows, cols = adj.nonzero(as_tuple=True)
    return ops.Csr(rows, cols, n, n, "cuda")


def _layer_inputs(b, fin, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, fin, n, generator=g)
    par = [torch.randn(*s, generator=g) * 0.5 for s in ((5, fin), (5, fin), (1, 10), (1, 5))]
    return x, par


@pytest.fixture(scope="module")
def first_layer():
    csr = _structure(sum(POOL), 1, hub=HUB, empty=(EMPTY_KEPT, EMPTY_POOLED))
    row_ptr = csr.row_ptr.cpu()
    assert int(row_ptr[HUB + 1] - row_ptr[HUB]) == 66 and int(row_ptr[EMPTY_KEPT + 1] - row_ptr[EMPTY_KEPT]) == 0
    return csr


# ---- 1. the coefficients ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("fin", [2, 5])
def test_coeffs_vs_fp64(first_layer, fin, b):
    from igcn_amd import ops
    csr, n = first_layer, sum(POOL)
    x, par = _layer_inputs(b, fin, n, 10 + fin)
    alpha, beta = ops.go_attention_coeffs(x.cuda(), *(p.cuda() for p in par), csr)
    assert tuple(alpha.shape) == (b, csr.nnz) and tuple(beta.shape) == (b, n)
    want_a, want_b = R.layer_coeffs(x, *par, csr.row_ptr, csr.col)
    R.assert_close(alpha, want_a, f"alpha fin={fin} B={b}")
    R.assert_close(beta, want_b, f"beta fin={fin} B={b}")
    row_sums = torch.zeros(b, n, dtype=torch.float64).index_add_(1, R.row_of(csr.row_ptr.cpu()), alpha.double().cpu())
    has_list = (csr.row_ptr[1:] > csr.row_ptr[:-1]).cpu()
    assert float((row_sums[:, has_list] - 1).abs().max()) <= 1e-5 and float(row_sums[:, ~has_list].abs().max()) == 0.0
    again = ops.go_attention_coeffs(x.cuda(), *(p.cuda() for p in par), csr)
    assert torch.equal(again[0], alpha) and torch.equal(again[1], beta)


@pytest.mark.parametrize("fin", [2, 5])
def test_coeffs_rebuild_the_forward(first_layer, fin):
    """sum_e alpha_e x_in[col_e] + beta_r x_s[r], rebuilt on the host (fp64) from the kernel's alpha and beta, is
    igcn_go_attn_fwd's y — at the bound of that kernel's own parity test, tests/test_gpu_ops.py:590
    (assert_matches(y, y_ref, TOL = 1e-4): max |got - want| <= 1e-4 max |want|)."""
    from igcn_amd import ops
    csr, n, b = first_layer, sum(POOL), 3
    x, par = _layer_inputs(b, fin, n, 20 + fin)
    dev = [p.cuda() for p in par]
    alpha, beta = ops.go_attention_coeffs(x.cuda(), *dev, csr)
    y = ops.GoAttention.apply(x.cuda(), dev[0], dev[1], dev[2].view(-1), dev[3].view(-1), csr)
    rows, col = R.row_of(csr.row_ptr.cpu()), csr.col.cpu().long()[:csr.nnz]
    xd = x.double().transpose(1, 2)                                                     # [B, N, fin]
    x_in, x_s = xd @ par[0].double().t(), xd @ par[1].double().t()
    want = torch.zeros(b, n, 5, dtype=torch.float64).index_add_(1, rows, alpha.double().cpu()[:, :, None] * x_in[:, col])
    want += beta.double().cpu()[:, :, None] * x_s
    assert_matches(y.transpose(1, 2), want.numpy(), 1e-4, f"y from alpha, beta (fin={fin})")


# ---- 2. the roll-out, layer by layer, and the product ---------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3])
def test_two_layers_and_the_product_vs_fp64(first_layer, b):
    """The chain as the model runs it — (2, 5) on the 68-node structure (hub row, rows without a list), (5, 5) on the
    31 nodes it keeps — from a shared R_0 with rows of zeros, each stage against fp64 from the SAME fp32 inputs."""
    from igcn_amd import ops
    n0, n1 = sum(POOL), sum(POOL[1:])
    csrs = [first_layer, _structure(n1, 2, empty=(20,), p=0.12)]
    g = torch.Generator().manual_seed(3 + b)
    e = torch.rand(n0, S, generator=g) * (torch.rand(n0, S, generator=g) < 0.1)
    e[7] = e[HUB] = 0
    r0 = (e / e.sum(1, keepdim=True).clamp(min=1e-30)).float()                          # [N, S]: rows sum to 1 or 0
    r_dev, r_ref = r0.t().contiguous().cuda(), r0
    for l, (fin, n) in enumerate(((2, n0), (5, n1))):
        x, par = _layer_inputs(b, fin, n, 30 + l)
        alpha, beta = ops.go_attention_coeffs(x.cuda(), *(p.cuda() for p in par), csrs[l])
        out = ops.go_rollout_layer(r_dev, alpha, beta, csrs[l], POOL[l])
        assert tuple(out.shape) == (b, S, n - POOL[l])
        # the layer's mixing against fp64 on the kernel's own fp32 coefficients and input relevance ...
        want = R.rollout_layer(r_dev.transpose(-1, -2), alpha, beta, csrs[l].row_ptr, csrs[l].col, POOL[l])
        R.assert_close(out.transpose(1, 2), want, f"R_{l + 1} from the kernel's inputs, B={b}")
        # ... and the chain so far against fp64 end to end
        a64, b64 = R.layer_coeffs(x, *par, csrs[l].row_ptr, csrs[l].col)
        r_ref = R.rollout_layer(r_ref, a64, b64, csrs[l].row_ptr, csrs[l].col, POOL[l])
        R.assert_close(out.transpose(1, 2), r_ref, f"R_{l + 1} end to end, B={b}")
        assert torch.equal(ops.go_rollout_layer(r_dev, alpha, beta, csrs[l], POOL[l]), out)
        r_dev = out
    r_top = r_dev.transpose(1, 2)                                                        # [B, 13, 54]
    assert float(r_top.min()) >= 0.0 and float(r_top.sum(-1).max()) <= 1.0 + 1e-5
    w = torch.softmax(torch.randn(b, 7, POOL[2] + POOL[3] + POOL[4], generator=g), -1)
    assoc = ops.snp_association(w.cuda(), r_top)
    R.assert_close(assoc, R.association(w, r_top), f"association from the kernel's R_top, B={b}")
    R.assert_close(assoc, R.association(w, r_ref), f"association end to end, B={b}")
    assert float(assoc.min()) >= 0.0 and float(assoc.sum(-1).max()) <= 1.0 + 1e-5


def test_row_without_a_list_copies_its_relevance(first_layer):
    from igcn_amd import ops
    n, b = sum(POOL), 2
    x, par = _layer_inputs(b, 2, n, 40)
    alpha, beta = ops.go_attention_coeffs(x.cuda(), *(p.cuda() for p in par), first_layer)
    r = torch.rand(b, S, n, generator=torch.Generator().manual_seed(4)).cuda()
    out = ops.go_rollout_layer(r, alpha, beta, first_layer, POOL[0])
    assert torch.equal(out[:, :, EMPTY_KEPT - POOL[0]], r[:, :, EMPTY_KEPT])


@pytest.mark.parametrize("n,chunk", [(2561, 4), (5121, 2), (10241, 1)])
def test_rollout_layer_at_every_chunk_width(n, chunk):
    """The smallest node counts at which a workgroup keeps 4, 2 and 1 relevance columns in LDS (8 at the sizes above),
    read from the entry point's own helper; 5 columns: the last chunk is ragged at 4 and at 2.  Per-sample relevance (the
    second layer's form) and the shared table."""
    from igcn_amd import _lib, ops
    lib = _lib.load()
    assert lib.igcn_go_rollout_chunk(n) == chunk and lib.igcn_go_rollout_chunk(n - 1) == 2 * chunk
    b, s, pool = 2, 5, n // 2 + 1
    g = torch.Generator().manual_seed(n)
    deg = torch.randint(0, 4, (n,), generator=g)
    deg[n - 2] = 200                                                                     # one long list
    rows = torch.repeat_interleave(torch.arange(n), deg)
    first = torch.cumsum(deg, 0) - deg
    # a row's columns: a random start, then steps of 37 (coprime to all three n: no column twice in a row)
    cols = (torch.randint(0, n, (n,), generator=g)[rows] + (torch.arange(rows.numel()) - first[rows]) * 37) % n
    order = torch.argsort(rows * n + cols)
    rows, cols = rows[order], cols[order]
    csr = ops.Csr(rows, cols, n, n, "cuda")
    alpha = torch.rand(b, csr.nnz, generator=g) + 0.01
    z = torch.zeros(b, n).index_add_(1, rows, alpha)
    alpha = alpha / z[:, rows]
    beta = torch.rand(b, n, generator=g) * 0.98 + 0.01
    for r in (torch.rand(b, s, n, generator=g), torch.rand(s, n, generator=g)):
        out = ops.go_rollout_layer(r.cuda(), alpha.cuda(), beta.cuda(), csr, pool)
        want = R.rollout_layer(r.transpose(-1, -2), alpha, beta, csr.row_ptr, csr.col, pool)
        R.assert_close(out.transpose(1, 2), want, f"N={n} chunk={chunk} r_in {tuple(r.shape)}")


def test_rollout_layer_refuses_what_does_not_fit():
    from igcn_amd import _lib
    lib = _lib.load()
    n = 20481
    assert lib.igcn_go_rollout_chunk(n) == 0
    z = torch.zeros(4, device="cuda")
    zi = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.IgcnError, match="go_rollout_layer"):                        # (refused on the host: no launch)
        _lib.call("igcn_go_rollout_layer", 1, n, 1, 0, _lib.ptr(zi), _lib.ptr(zi), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z),
                  0, _lib.ptr(z), _lib.stream_ptr())


@pytest.mark.parametrize("rois", [7, 90])
@pytest.mark.parametrize("n_top", [13, 103])
def test_final_product_vs_fp64(rois, n_top):
    from igcn_amd import ops
    g = torch.Generator().manual_seed(rois + n_top)
    b = 3
    w = torch.softmax(2 * torch.randn(b, rois, n_top, generator=g), -1)
    r = torch.rand(b, S, n_top, generator=g) * (torch.rand(b, S, n_top, generator=g) < 0.3)
    r = (r / r.sum(1, keepdim=True).clamp(min=1e-30)).float()
    r_top = r.cuda().transpose(1, 2)                                                     # as the roll-out hands it over
    got = ops.snp_association(w.cuda(), r_top)
    assert tuple(got.shape) == (b, rois, S)
    R.assert_close(got, R.association(w, r.transpose(1, 2)), f"product rois={rois} Ntop={n_top}")
    assert torch.equal(ops.snp_association(w.cuda(), r_top.contiguous()), got)           # any strides, the same bits
    assert torch.equal(ops.snp_association(w.cuda(), r_top), got)


# ---- 3. the models ---------------------------------------------------------------------------------------------------
def _go(device="cuda"):
    from igcn_amd import synth
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=2)
    return synth.go_sparse_inputs(go_snps, adj, device) + (pool_dim,)


def _model(kind="imgsnp", seed=8):
    a_g, a, pool_dim = _go()
    if kind == "clusterlabel":
        from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
        model = SGCN_GCN_CLUSTERLABEL(2, 16, a_g, a, pool_dim, 32, "cuda", H_0=3, num_features=3, isCrossAtten=True).cuda()
    elif kind == "gcn_img_snp":
        from igcn_amd.gcn_img_snp import GCN_IMGSNP
        model = GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=90, H_0=3, num_classes=3, isCrossAtten=True,
                           num_regr=3, isImageOnly=False, isSNPsOnly=False).cuda()
    else:
        from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
        model = SGCN_GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=90, H_0=3, num_classes=3,
                                isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3,
                                isuseProb4Regr=True, isImageOnly=False, isSNPsOnly=False).cuda()
    model.load_state_dict(seeded_state({k: v.shape for k, v in model.state_dict().items()}, seed, model.state_dict()))
    return model


def _batch(n=4, seed=5):
    from igcn_amd import synth
    from igcn_amd.data import Batch
    return Batch.from_data_list(synth.brain_graph_list(n, seed=seed, rois=90, tsne_dim=16)).to("cuda")


def _reference_rollout(net, layer_inputs):
    """R_top [B, Ntop, 54] in fp64 from the network's parameters and the fp32 inputs its encoder layers saw."""
    pos = net.gene_csr.flat_pos.cpu()
    r = R.encoding_relevance(pos // S, pos % S, list(net.t), net.n_nodes, S)
    for j, x in enumerate(layer_inputs):
        csr = net.enc_csr[j]
        par = (net.w_inc[j].weight, net.w_s_loop[j].weight, net.w_att_in[j].weight, net.w_att_s[j].weight)
        alpha, beta = R.layer_coeffs(x, *par, csr.row_ptr, csr.col)
        r = R.rollout_layer(r, alpha, beta, csr.row_ptr, csr.col, net.pool[j])
    return r


def _capture_layer_inputs(monkeypatch):
    from igcn_amd import ops
    seen, orig = [], ops.go_attention_coeffs

    def spy(x, *a):
        seen.append(x.detach().clone())
        return orig(x, *a)

    monkeypatch.setattr(ops, "go_attention_coeffs", spy)
    return seen


@pytest.mark.parametrize("explain", [False, True])
def test_model_vs_fp64(monkeypatch, explain):
    model, data = _model(), _batch()
    seen = _capture_layer_inputs(monkeypatch)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for mode in (True, False):
        model.train(mode)
        del seen[:]
        got = model.snp_association(data, None, "cuda", isExplain=explain)
        assert model.training == mode and model.go_network.training == mode
    assert tuple(got.shape) == (4, 90, S) and got.dtype == torch.float32 and got.is_cuda
    assert len(seen) == 2 and tuple(seen[0].shape) == (4, 2, 68) and tuple(seen[1].shape) == (4, 5, 31)
    w = model.attention_weights(data, None, "cuda", isExplain=explain)
    want = R.association(w, _reference_rollout(model.go_network, seen))
    R.assert_close(got, want, f"model association explain={explain}")
    assert float(got.min()) >= 0.0 and float(got.sum(-1).max()) <= 1.0 + 1e-5
    assert torch.equal(model.snp_association(data, None, "cuda", isExplain=explain), got)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k


def _flat(o):
    if torch.is_tensor(o):
        return [o.detach().clone()]
    if isinstance(o, (list, tuple)):
        return [t for x in o for t in _flat(x)]
    return []


def test_model_state_and_random_stream_are_untouched():
    """attention_weights, a training forward (dropout on) and a train step after snp_association / attention_rollout
    give the bits a fresh model gives that never called them."""
    from igcn_amd.train import FlatAdam, train_step

    def run(touch):
        torch.manual_seed(7)
        model, data = _model(), _batch()
        model.train()
        if touch:
            model.snp_association(data, None, "cuda")
            model.snp_association(data, None, "cuda", isExplain=True)
            model.go_network.attention_rollout(data.snps_feat.view(-1, S).float(), return_coeffs=True)
        out = _flat(model.attention_weights(data, None, "cuda"))
        out += _flat(model(data, None, "cuda"))
        opt = FlatAdam(model.parameters(), lr=1e-3)
        out += _flat(train_step(model, opt, data))
        out += [v.detach().clone() for v in model.state_dict().values()]
        out += [torch.get_rng_state(), torch.cuda.get_rng_state()]
        return out

    fresh, touched = run(False), run(True)
    assert len(fresh) == len(touched) > 10
    for k, (a, c) in enumerate(zip(fresh, touched)):
        assert torch.equal(a, c), k


@pytest.mark.parametrize("kind", ["clusterlabel", "gcn_img_snp"])
def test_sibling_models(kind):
    model, data = _model(kind), _batch()
    got = model.snp_association(data, None, "cuda")
    assert tuple(got.shape) == (4, 90, S) and bool(torch.isfinite(got).all())
    assert float(got.min()) >= 0.0 and float(got.sum(-1).max()) <= 1.0 + 1e-5
    w = model.attention_weights(data, None, "cuda")
    r_top = model.go_network.attention_rollout(data.snps_feat.view(-1, S).float())
    R.assert_close(got, R.association(w, r_top), kind)


def test_bare_go_network(monkeypatch):
    """The genetics-only path: the GO network alone, its coefficients handed out as well."""
    from igcn_amd.go_model import Gene_ontology_network
    a_g, a, pool_dim = _go()
    net = Gene_ontology_network(a_g, a, 2, 2, [5, 5], pool_dim, 32, "cuda").cuda()
    net.load_state_dict(seeded_state({k: v.shape for k, v in net.state_dict().items()}, 3, net.state_dict()))
    snps = torch.rand(3, S, generator=torch.Generator().manual_seed(1)).cuda()
    seen = _capture_layer_inputs(monkeypatch)
    net.train()
    r_top, coeffs = net.attention_rollout(snps, return_coeffs=True)
    assert net.training and tuple(r_top.shape) == (3, POOL[2] + POOL[3] + POOL[4], S) and r_top.dtype == torch.float32
    assert [tuple(a_.shape) for a_, _ in coeffs] == [(3, net.enc_csr[0].nnz), (3, net.enc_csr[1].nnz)]
    assert [tuple(b_.shape) for _, b_ in coeffs] == [(3, 68), (3, 31)]
    R.assert_close(r_top, _reference_rollout(net, seen), "bare GO network R_top")
    assert torch.equal(net.attention_rollout(snps), r_top)


# ---- 4. the cohort pass ----------------------------------------------------------------------------------------------
def test_association_maps_vs_per_batch_means():
    from igcn_amd import _lib, synth
    from igcn_amd.data import Batch, DataLoader
    from igcn_amd.train import association_maps
    model = _model()
    graphs = synth.brain_graph_list(11, seed=5, rois=90, tsne_dim=16)
    labels = [0, 2, 2, 0, 2, 0, 0, 2, 2, 0, 2]                                          # class 1 has no subject
    for g_, lab in zip(graphs, labels):
        g_.y = torch.tensor([lab])
    r = association_maps(model, DataLoader(graphs, batch_size=4), device="cuda", top_k=4)       # 4 + 4 + 3
    assert set(r) == {"mean", "count", "overall", "go_to_snp", "go_rows", "top_snps", "n"} and r["n"] == 11
    sums, go_sum = torch.zeros(3, 90, S, dtype=torch.float64), torch.zeros(13, S, dtype=torch.float64)
    for lo, hi in ((0, 4), (4, 8), (8, 11)):
        d = Batch.from_data_list(graphs[lo:hi]).to("cuda")
        a = model.snp_association(d, None, "cuda").double().cpu()
        go_sum += model.go_network.attention_rollout(d.snps_feat.view(-1, S).float()).double().cpu().sum(0)
        for i in range(hi - lo):
            sums[labels[lo + i]] += a[i]
    cnt = torch.tensor([labels.count(c) for c in range(3)])
    assert r["count"].cpu().tolist() == cnt.tolist() == [5, 0, 6]
    mean = sums / cnt.clamp(min=1).view(3, 1, 1)
    # fp64 sums of the same fp32 maps, rounded to fp32 once: within an fp32 rounding of the host's
    for got, want, nm in ((r["mean"], mean, "mean"), (r["overall"], sums.sum(0) / 11, "overall"),
                          (r["go_to_snp"], go_sum / 11, "go_to_snp")):
        assert got.dtype == torch.float32 and got.shape == want.shape, nm
        assert torch.allclose(got.double().cpu(), want, rtol=2e-7, atol=1e-12), nm
    assert float(r["mean"][1].abs().max()) == 0.0
    assert r["go_rows"].cpu().tolist() == list(range(68 - 13, 68))
    assert tuple(r["top_snps"].shape) == (90, 4)
    assert torch.equal(r["top_snps"], torch.topk(r["overall"], 4, dim=1).indices)
    bad = labels.count(2)                                                               # 6 of the 11
    with pytest.raises(_lib.IgcnError, match=rf"association_maps: {bad} of 11 labels lie outside \[0, 2\)"):
        association_maps(model, DataLoader(graphs, batch_size=4), device="cuda", num_classes=2)
