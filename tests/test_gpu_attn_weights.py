"""GPU tests of the cross-attention WEIGHTS (the second output of ``self.multihead_attn(...)``,
kernel/sgcn_img_snp.py:240): igcn_attn_weights / igcn_attn_map_accumulate, ops.attention_weights,
SGCN_GCN_IMGSNP.attention_weights and train.attention_maps against torch's own module in fp64 on the CPU
(tests/attn_map_ref.py).  Bound: |got - want| <= 1e-6 + 1e-4 want element-wise, every row sums to 1 within 1e-5."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_map_ref as R
from _weights import seeded_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _qkv(b, d, lq, lk, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, lq, d, generator=g), torch.randn(b, lk, 2 * d, generator=g)


def _launch(q, kv, heads):
    from igcn_amd import ops
    return ops.attention_weights(q.cuda().contiguous(), kv.cuda().contiguous(), heads)


# ---- 1. the kernel against fp64 -------------------------------------------------------------------------------------
CASES = {"default_width": (32, 2, 90, 400), "unaligned_rows": (20, 2, 90, 29), "odd_width": (30, 2, 5, 1),
         "head_average": (96, 4, 33, 17), "padded_wide_head": (66, 2, 90, 53), "widest_head": (192, 2, 17, 53),
         "many_queries": (32, 2, 300, 64)}


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_vs_fp64(case, b):
    from igcn_amd import _lib
    d, h, lq, lk = CASES[case]
    lib = _lib.load()
    assert lib.igcn_attn_weights_supported(d, h, lq, lk) and lib.igcn_attn_weights_chunk_rows(d, h, lq, lk) == 0
    q, kv = _qkv(b, d, lq, lk, 11 + lq)
    got = _launch(q, kv, h)
    assert tuple(got.shape) == (b, lq, lk) and got.dtype == torch.float32
    R.assert_weights(got, R.weights_fp64(q, kv, h), f"{case} B={b}")
    if lk == 1:
        assert bool((got == 1).all())                            # one key: every weight is exactly 1


@pytest.mark.parametrize("b", [1, 3])
def test_kernel_streamed_keys_vs_fp64(b):
    """The one case that STREAMS the keys: head_dim 96 with two heads keeps 80 key rows per LDS chunk, so chunk + 5 = 85
    keys take two chunks, the second ragged (5 keys).  Every case of test_kernel_vs_fp64 is resident."""
    from igcn_amd import _lib
    lib = _lib.load()
    d, h, lq = 192, 2, 17
    ch = lib.igcn_attn_weights_chunk_rows(d, h, lq, 1 << 20)
    assert ch > 0 and ch % 16 == 0
    lk = ch + 5
    assert lib.igcn_attn_weights_chunk_rows(d, h, lq, lk) == ch   # this shape streams
    q, kv = _qkv(b, d, lq, lk, 5)
    R.assert_weights(_launch(q, kv, h), R.weights_fp64(q, kv, h), f"streamed Lk={lk} B={b}")


def test_kernel_large_scores_need_the_row_maximum():
    """q scaled until the largest |score| is 100: exp() of it overflows fp32 unless the row maximum is subtracted."""
    d, h, lq, lk = 32, 2, 90, 400
    q, kv = _qkv(2, d, lq, lk, 3)
    s = torch.einsum("bqhc,bkhc->bhqk", q.double().view(2, lq, h, 16), kv.double().view(2, lk, 2, h, 16)[:, :, 0]) / 4.0
    q = (q * (100.0 / float(s.abs().max()))).contiguous()
    R.assert_weights(_launch(q, kv, h), R.weights_fp64(q, kv, h), "scores up to 100")


def test_kernel_pointers_off_16_bytes():
    """q and kv as views one float into their buffers: rows are no longer 16-byte aligned (no vector loads)."""
    d, h, lq, lk, b = 32, 2, 90, 400, 2
    q, kv = _qkv(b, d, lq, lk, 4)
    qb, kb = torch.zeros(q.numel() + 1, device="cuda"), torch.zeros(kv.numel() + 1, device="cuda")
    qv, kvv = qb[1:].view(b, lq, d), kb[1:].view(b, lk, 2 * d)
    qv.copy_(q)
    kvv.copy_(kv)
    assert qv.data_ptr() % 16 == 4 and kvv.data_ptr() % 16 == 4 and qv.is_contiguous() and kvv.is_contiguous()
    from igcn_amd import ops
    R.assert_weights(ops.attention_weights(qv, kvv, h), R.weights_fp64(q, kv, h), "pointers off 16 bytes")


# ---- 2. a head the kernel does not cover ---------------------------------------------------------------------------
def test_unsupported_head_raises_and_ops_takes_the_composite():
    from igcn_amd import _lib, ops
    d, h, lq, lk, b = 200, 2, 33, 53, 2                          # head_dim 100
    q, kv = _qkv(b, d, lq, lk, 9)
    qc, kc = q.cuda(), kv.cuda()
    w = torch.empty(b, lq, lk, device="cuda")
    with pytest.raises(_lib.IgcnError, match="attn_weights"):
        _lib.call("igcn_attn_weights", b, d, h, lq, lk, _lib.ptr(qc), _lib.ptr(kc), _lib.ptr(w), _lib.stream_ptr())
    R.assert_weights(ops.attention_weights(qc, kc, h), R.weights_fp64(q, kv, h), "composite head_dim 100")


# ---- 3. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(32, 2, 90, 400), (192, 2, 17, 85)])
def test_two_launches_are_bit_identical(shape):
    d, h, lq, lk = shape
    q, kv = _qkv(3, d, lq, lk, 21)
    qc, kc = q.cuda(), kv.cuda()
    from igcn_amd import ops
    a, b2 = ops.attention_weights(qc, kc, h), ops.attention_weights(qc, kc, h)
    assert torch.equal(a, b2)


# ---- 4. per-class accumulation -------------------------------------------------------------------------------------
def test_map_accumulate_vs_numpy():
    from igcn_amd import ops
    lq, lk, c = 33, 17, 3                                        # 561 elements: three blocks, the last one ragged
    rng = np.random.default_rng(0)
    w1, y1 = rng.random((5, lq, lk), dtype=np.float32), np.array([0, 2, 2, 0, 7])
    w2, y2 = rng.random((4, lq, lk), dtype=np.float32), np.array([1, -1, 0, 2])
    sums = torch.zeros(c, lq, lk, dtype=torch.float64, device="cuda")
    counts = torch.zeros(c, dtype=torch.int64, device="cuda")
    state = torch.zeros(1, dtype=torch.int64, device="cuda")
    want, cnt = np.zeros((c, lq, lk)), np.zeros(c, dtype=np.int64)

    def host(w, y):
        for i, lab in enumerate(y):
            if 0 <= lab < c:
                want[lab] += w[i].astype(np.float64)
                cnt[lab] += 1

    ops.attention_map_accumulate(torch.from_numpy(w1).cuda(), torch.from_numpy(y1).cuda(), sums, counts, state)
    host(w1, y1)
    assert counts.tolist() == [2, 0, 2] == cnt.tolist() and int(state) == 1
    assert float(sums[1].abs().max()) == 0.0                     # class 1: no subject, zero sums (a zero mean)
    assert np.array_equal(sums.cpu().numpy(), want)              # fp64 sums of fp32 values in the same order: exact
    ops.attention_map_accumulate(torch.from_numpy(w2).cuda(), torch.from_numpy(y2).cuda(), sums, counts, state)
    host(w2, y2)
    assert counts.tolist() == [3, 1, 3] == cnt.tolist() and int(state) == 2
    assert np.array_equal(sums.cpu().numpy(), want)


# ---- 5. the model against fp64 -------------------------------------------------------------------------------------
POOL = (60, 30, 20, 9, 1)


def _model(layers, hidden, seed=8):
    from igcn_amd import synth
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=2)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    model = SGCN_GCN_IMGSNP(layers, hidden, a_g, a, pool_dim, 32, "cuda", rois=90, H_0=3, num_classes=3,
                            isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3,
                            isuseProb4Regr=True, isImageOnly=False, isSNPsOnly=False).cuda()
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, seed)
    model.load_state_dict(sd)
    return model, sd, (go_snps, adj)


def _oracle(sd, go, graphs, explain):
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from oracle import go_network as OG
    a_g_c, a_c = synth.go_sparse_inputs(*go)
    idx = OG.go_index_sets(a_g_c, a_c, list(POOL), 2)
    sd = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    d = Batch.from_data_list(graphs)
    for k in ("x", "edge_attr", "snps_feat"):
        setattr(d, k, getattr(d, k).double())
    with torch.no_grad():
        return R.model_weights_fp64(sd, SimpleNamespace(rois=90, heads=2), idx, d, explain)


@pytest.mark.parametrize("layers,hidden", [(2, 8), (4, 5)])
def test_model_vs_fp64(monkeypatch, layers, hidden):
    from calltrace import record_calls
    from igcn_amd import synth
    from igcn_amd.data import Batch
    model, sd, go = _model(layers, hidden)
    graphs = synth.brain_graph_list(8, seed=5, rois=90, tsne_dim=16)
    data = Batch.from_data_list(graphs).to("cuda")
    seen = record_calls(monkeypatch)

    def forward_calls():
        del seen[:]
        with torch.no_grad():
            model(data, None, "cuda")
        return list(seen)

    model.eval()
    forward_calls()                                              # (the first pass over a batch also builds its plan)
    before_calls = forward_calls()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for explain in (False, True):
        for mode in (True, False):
            model.train(mode)
            got = model.attention_weights(data, None, "cuda", isExplain=explain)
            assert model.training == mode
            assert model.last_edge_prob is None and model._handoff.reg is None and model._handoff.key[0] is None
        assert tuple(got.shape) == (8, 90, 30) and got.dtype == torch.float32 and got.is_cuda
        R.assert_weights(got, _oracle(sd, go, graphs, explain), f"model L={layers} h={hidden} explain={explain}")
    after = model.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k                       # parameters and buffers (num_batches_tracked included)
    model.eval()
    assert forward_calls() == before_calls                       # a forward launches what it launched before


# ---- 6. the loader-level product -----------------------------------------------------------------------------------
def test_attention_maps_vs_fp64():
    from igcn_amd import synth
    from igcn_amd.data import DataLoader
    from igcn_amd.train import attention_maps
    model, sd, go = _model(2, 8)
    graphs = synth.brain_graph_list(12, seed=5, rois=90, tsne_dim=16)
    r = attention_maps(model, DataLoader(graphs, batch_size=8), device="cuda", top_k=4)      # 8 + a ragged tail of 4
    assert set(r) == {"mean", "count", "overall", "go_rows", "top_terms", "n"} and r["n"] == 12
    want = torch.cat([_oracle(sd, go, graphs[lo:hi], False) for lo, hi in ((0, 8), (8, 12))])
    y = torch.cat([g.y.view(-1) for g in graphs])
    mean, cnt = torch.zeros(3, 90, 30, dtype=torch.float64), torch.zeros(3, dtype=torch.int64)
    for i in range(12):
        mean[y[i]] += want[i]
        cnt[y[i]] += 1
    assert cnt.min() > 0                                         # (every class has subjects: the means below are defined)
    mean /= cnt.view(3, 1, 1)
    assert r["count"].cpu().tolist() == cnt.tolist()
    assert r["mean"].dtype == torch.float32 and tuple(r["mean"].shape) == (3, 90, 30)
    R.assert_weights(r["mean"], mean, "class means")
    R.assert_weights(r["overall"][None], want.mean(0)[None], "overall")
    assert r["go_rows"].cpu().tolist() == list(range(90, 120))
    assert tuple(r["top_terms"].shape) == (90, 4)
    assert torch.equal(r["top_terms"], r["go_rows"][torch.topk(r["overall"], 4, dim=1).indices])
    # a class without subjects: zero mean; labels outside [0, C): refused after the pass
    r2 = attention_maps(model, DataLoader(graphs, batch_size=8), device="cuda", num_classes=5)
    assert r2["count"].cpu().tolist() == cnt.tolist() + [0, 0] and float(r2["mean"][3:].abs().max()) == 0.0
    from igcn_amd import _lib
    bad = int((y >= 2).sum())                                    # (> 0: class 2 has subjects, above)
    with pytest.raises(_lib.IgcnError, match=rf"attention_maps: {bad} of 12 labels lie outside \[0, 2\)"):
        attention_maps(model, DataLoader(graphs, batch_size=8), device="cuda", num_classes=2)


@pytest.mark.parametrize("kind", ["clusterlabel", "gcn_img_snp"])
def test_attention_maps_of_the_sibling_models(kind):
    from igcn_amd import synth
    from igcn_amd.data import DataLoader
    from igcn_amd.train import attention_maps
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=2)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    if kind == "clusterlabel":
        from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
        model = SGCN_GCN_CLUSTERLABEL(2, 8, a_g, a, pool_dim, 32, "cuda", H_0=3, num_features=3,
                                      isCrossAtten=True).cuda()
    else:
        from igcn_amd.gcn_img_snp import GCN_IMGSNP
        model = GCN_IMGSNP(2, 8, a_g, a, pool_dim, 32, "cuda", rois=90, H_0=3, num_classes=3, isCrossAtten=True,
                           num_regr=3, isImageOnly=False, isSNPsOnly=False).cuda()
    model.load_state_dict(seeded_state({k: v.shape for k, v in model.state_dict().items()}, 8, model.state_dict()))
    graphs = synth.brain_graph_list(12, seed=5, rois=90, tsne_dim=16)
    r = attention_maps(model, DataLoader(graphs, batch_size=8), device="cuda")
    assert tuple(r["mean"].shape) == (3, 90, 30) and tuple(r["overall"].shape) == (90, 30) and r["n"] == 12
    assert float((r["overall"].sum(-1) - 1).abs().max()) <= 1e-5
    live = r["count"] > 0
    assert float((r["mean"][live].sum(-1) - 1).abs().max()) <= 1e-5
