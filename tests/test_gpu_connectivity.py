"""GPU tests of the ROI x ROI connectivity maps: igcn_edge_dense_map (per-edge values -> dense [B, R, R], bit for bit
against the stored-order fp32 restatement), ``edge_importance`` of the mask-training models against cal_probability of
oracle/sgcn_img_snp.py in fp64, igcn_gat_stack_alpha against the fp64 GATConv stand-in (tests/connectivity_ref.py), the
models' ``gat_attention``, that nothing else moved, and train.connectivity_maps against plain torch.

Bounds: the dense map only moves and adds in a fixed order — ``torch.equal``.  The edge mask: assert_matches(1e-4), the
bound tests/test_gpu_ops.py holds ``e`` to.  The attention maps: |got - want| <= 1e-6 + 1e-4 alpha element-wise, the
bound tests/test_gpu_attn_weights.py holds softmax weights to; every comparison prints the largest fraction of it any
element uses (connectivity_ref.assert_alpha_close).  Rebuilding the forward from the maps: 1e-5 of max|xcat|, the bound
tests/test_gpu_gat.py holds xcat to."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import connectivity_ref as C
from conftest import assert_matches

pytestmark = pytest.mark.gpu

DATASET = SimpleNamespace(num_features=3, num_classes=2)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


# ---- 1. the dense-map kernel, bit for bit -----------------------------------------------------------------------------
def _incoming(rng, b, r, deg, block=None):
    """``deg`` distinct incoming edges per target, sources drawn inside the target's block of ``block`` nodes."""
    block = block or r
    src, dst = [], []
    for g in range(b):
        for j in range(r):
            lo = (j // block) * block
            for i in rng.choice(block, deg, replace=False):
                src.append(g * r + lo + int(i))
                dst.append(g * r + j)
    order = rng.permutation(len(src))
    return torch.from_numpy(np.stack([np.array(src)[order], np.array(dst)[order]])).long()


def _case(name):
    rng = np.random.default_rng(len(name))
    if name == "deg2":
        b, r = 1, 5
        ei = torch.tensor([[(j + 1) % 5 for j in range(5)] + [(j + 2) % 5 for j in range(5)], list(range(5)) * 2])
    elif name == "odd":
        b, r = 3, 7
        ei = C.odd_batch()[0]
    elif name == "top3":
        b, r, ei = 2, 90, _incoming(rng, 2, 90, 3)
    elif name == "fusion":
        b, r, ei = 2, 270, _incoming(rng, 2, 270, 3, block=90)
    else:
        b, r = 1, 512
        k = torch.arange(512 * 512)
        ei = torch.stack([k // 512, k % 512])
    return b, r, ei.contiguous(), torch.from_numpy(rng.random(ei.shape[1])).float()


def _raw_launch(values, plan, b, r, count):
    """igcn_edge_dense_map into buffers filled with NaN beforehand: whatever the launch does not write stays NaN."""
    from igcn_amd import _lib
    out = torch.full((b, r, r), float("nan"), device="cuda")
    cnt = torch.full((b, r, r), float("nan"), device="cuda") if count else None
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    _lib.call("igcn_edge_dense_map", b, r, plan.n_edges, _lib.ptr(values), _lib.ptr(plan.src32), _lib.ptr(plan.dst32),
              _lib.ptr(plan.tgt_ptr), _lib.ptr(plan.tgt_perm), _lib.ptr(out), _lib.ptr(cnt), _lib.ptr(status),
              _lib.stream_ptr())
    assert int(status[0]) == 0
    return out, cnt


@pytest.mark.parametrize("name", ["deg2", "odd", "top3", "fusion", "complete"])
def test_dense_map_bit_for_bit(name):
    from igcn_amd import ops
    b, r, ei, v = _case(name)
    plan = ops.GraphPlan(ei.cuda(), b * r)
    want, want_cnt = C.dense_map(v, ei, b, r, stored_order_fp32=True), C.count_map(ei, b, r)
    if name == "odd":
        assert float(want_cnt[0, 2, 5]) >= 3 and float(want_cnt[0, 4, 4]) >= 1 and float(want_cnt[1].max()) == 0
    for count in (True, False):
        got, cnt = _raw_launch(v.cuda(), plan, b, r, count)
        assert not bool(torch.isnan(got).any()), "an element of map was not written"
        assert torch.equal(got.cpu(), want)
        if count:
            assert not bool(torch.isnan(cnt).any()), "an element of cnt was not written"
            assert torch.equal(cnt.cpu(), want_cnt)
        again, cnt2 = _raw_launch(v.cuda(), plan, b, r, count)
        assert torch.equal(again, got) and (not count or torch.equal(cnt2, cnt))
    m, c = ops.edge_dense_map(v.cuda(), plan, r, want_count=True)
    assert torch.equal(m.cpu(), want) and torch.equal(c.cpu(), want_cnt)
    assert torch.equal(ops.edge_dense_map(v.cuda(), plan, r).cpu(), want)
    plan.check()


def test_dense_map_on_a_per_graph_plan():
    """The plan a Batch builds per graph in LDS (ragged edge counts, one graph without edges) gives the same bits."""
    from igcn_amd import ops
    ei, v = C.odd_batch()
    data = SimpleNamespace(x=torch.zeros(21, 1, device="cuda"), edge_index=ei.cuda(),
                           ptr=torch.tensor([0, 7, 14, 21]).cuda(), edge_ptr=torch.tensor([0, 13, 13, 27]).cuda(),
                           _max_nodes=7, _max_edges=14)
    plan = ops.plan_for(data)
    assert plan.segmented
    m, c = ops.edge_dense_map(v.cuda(), plan, 7, want_count=True)
    assert torch.equal(m.cpu(), C.dense_map(v, ei, 3, 7, stored_order_fp32=True))
    assert torch.equal(c.cpu(), C.count_map(ei, 3, 7))
    plan.check()


def test_edge_that_leaves_its_graph_is_flagged_and_not_written():
    """Valid node indices, but edge 3 runs from graph 0 into graph 1: the status word, no fault."""
    from igcn_amd import _lib, ops
    b, r = 2, 5
    ei = torch.tensor([[0, 1, 6, 2, 7], [1, 2, 7, 8, 9]])
    v = torch.arange(1, 6).float()
    plan = ops.GraphPlan(ei.cuda(), b * r)
    m, c = ops.edge_dense_map(v.cuda(), plan, r, want_count=True)
    keep = torch.tensor([True, True, True, False, True])
    assert torch.equal(m.cpu(), C.dense_map(v[keep], ei[:, keep], b, r, stored_order_fp32=True))
    assert torch.equal(c.cpu(), C.count_map(ei[:, keep], b, r))
    with pytest.raises(_lib.IgcnError, match="not block diagonal"):
        plan.check()


def test_dense_map_refuses_what_does_not_fit():
    from igcn_amd import _lib, ops
    r = 16385
    assert _lib.load().igcn_edge_dense_map_supported(r, 0) == 0
    z = torch.zeros(4, device="cuda")
    zi = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.IgcnError, match="edge_dense_map"):                         # (refused on the host: no launch)
        _lib.call("igcn_edge_dense_map", 1, r, 0, _lib.ptr(z), _lib.ptr(zi), _lib.ptr(zi), _lib.ptr(zi), _lib.ptr(zi),
                  _lib.ptr(z), None, None, _lib.stream_ptr())
    plan = SimpleNamespace(n_nodes=r, n_edges=4, src32=zi, status=None)
    with pytest.raises(ValueError, match="does not fit"):
        ops.edge_dense_map(z, plan, r)


# ---- 2. edge_importance against the fp64 oracle -----------------------------------------------------------------------
def _go():
    from igcn_amd import synth
    go_snps, adj, pool_dim = synth.go_hierarchy((37, 18, 9, 3, 1), seed=2)
    return synth.go_sparse_inputs(go_snps, adj, "cuda") + (pool_dim,)


def _mask_model(kind, rois, h0):
    torch.manual_seed(11)
    if kind == "imgsnp":
        from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
        a_g, a, pool_dim = _go()
        return SGCN_GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=rois, H_0=h0, num_classes=3).cuda()
    if kind == "clusterlabel":
        from igcn_amd.sgcn_img_snp_clusterlabel import SGCN_GCN_CLUSTERLABEL
        a_g, a, pool_dim = _go()
        return SGCN_GCN_CLUSTERLABEL(2, 16, a_g, a, pool_dim, 32, "cuda", rois=rois, H_0=h0, num_features=h0,
                                     isCrossAtten=True).cuda()
    from igcn_amd.sgcn import SGCN_GCN
    return SGCN_GCN(None, 2, 16, rois=rois, H_0=h0, num_features=h0).cuda()


def _brain_batch(n, rois, h0, seed=5):
    from igcn_amd import synth
    from igcn_amd.data import Batch
    return Batch.from_data_list(synth.brain_graph_list(n, seed=seed, rois=rois, h0=h0, top_k=3, tsne_dim=4)).to("cuda")


@pytest.mark.parametrize("h0", [1, 3])
@pytest.mark.parametrize("rois", [7, 90])
@pytest.mark.parametrize("kind", ["imgsnp", "clusterlabel", "image_only"])
def test_edge_importance_vs_fp64_oracle(kind, rois, h0):
    from igcn_amd import ops
    from oracle import sgcn_img_snp as OS
    model, data = _mask_model(kind, rois, h0), _brain_batch(3, rois, h0)
    with torch.no_grad():                                                # masks of O(1) on both sides of 1/2
        model.prob.normal_()
        model.prob_bias.normal_()
    ei = data.edge_index.cpu()
    sd = {"prob": model.prob.detach().double().cpu(), "prob_bias": model.prob_bias.detach().double().cpu()}
    _, ewm, e = OS.edge_and_region_masks(sd, data.x.detach().double().cpu(), ei, data.edge_attr.double().cpu(), rois)
    own = model.cal_probability(data.x, data.edge_index, data.edge_attr, plan=ops.plan_for(data))
    b = 3
    s, d = ei[0], ei[1]
    for weighted, want_e, own_e in ((False, e, own[3]), (True, ewm, own[1])):
        got, cnt = model.edge_importance(data, weighted=weighted, return_count=True)
        assert tuple(got.shape) == (b, rois, rois) and got.dtype == torch.float32 and got.is_cuda
        assert_matches(got, C.dense_map(want_e, ei, b, rois).numpy(), 1e-4, f"{kind} weighted={weighted}")
        assert torch.equal(cnt.cpu(), C.count_map(ei, b, rois)) and float(cnt.max()) == 1.0
        # at the stored positions: the model's own cal_probability, bit for bit; 0 everywhere else
        assert torch.equal(got.cpu()[s // rois, s % rois, d % rois], own_e.detach().reshape(-1).cpu())
        assert torch.equal(got.cpu(), C.dense_map(own_e.detach().reshape(-1), ei, b, rois, stored_order_fp32=True))
        assert torch.equal(model.edge_importance(data, weighted=weighted), got)


def test_edge_importance_on_complete_graphs():
    """A dense-block batch (complete row-major graphs, whose forward runs on the dense kernels) takes the generic mask
    launch and the map launch: every position is stored once, the map is ``e`` reshaped."""
    from igcn_amd import ops, synth
    from oracle import sgcn_img_snp as OS
    rois, b = 64, 2
    model = _mask_model("imgsnp", rois, 3)
    data = synth.brain_batch(b, seed=1, rois=rois, tsne_dim=8, dense=True).to("cuda")
    assert ops.plan_for(data).dense_blocks
    with torch.no_grad():
        model.prob_bias.normal_()
    got, cnt = model.edge_importance(data, return_count=True)
    assert bool((cnt == 1).all())
    ei = data.edge_index.cpu()
    sd = {"prob": model.prob.detach().double().cpu(), "prob_bias": model.prob_bias.detach().double().cpu()}
    e = OS.edge_and_region_masks(sd, data.x.detach().double().cpu(), ei, data.edge_attr.double().cpu(), rois)[2]
    assert_matches(got, e.view(b, rois, rois).numpy(), 1e-4, "complete graphs")
    own = model.cal_probability(data.x, data.edge_index, data.edge_attr, plan=ops.plan_for(data))[3]
    assert torch.equal(got, own.detach().view(b, rois, rois))
    ops.plan_for(data).check()


# ---- 3. the attention maps of the GAT stack -----------------------------------------------------------------------------
def _convs(layers, h0, hidden, seed):
    from igcn_amd.gcn_img_snp import GATConv
    torch.manual_seed(seed)
    convs = [GATConv(h0 if l == 0 else hidden, hidden) for l in range(layers)]
    with torch.no_grad():
        for c in convs:                                            # every parameter non-trivial, logits of O(1)
            c.lin_src.weight.copy_(torch.randn_like(c.lin_src.weight) / c.in_channels ** 0.5)
            for p in (c.att_src, c.att_dst, c.att_edge, c.lin_edge.weight):
                p.copy_(0.5 * torch.randn_like(p))
            c.bias.copy_(0.1 * torch.randn_like(c.bias))
    return [c.cuda() for c in convs]


def _standin_params(convs):
    return [(c.lin_src.weight, c.att_src, c.att_dst, c.lin_edge.weight, c.att_edge, c.bias) for c in convs]


def _gat_batch(b, r, h0, seed):
    from igcn_amd.data import Batch, Data
    graphs, lonely = C.gat_graphs(b, r, h0, seed)
    data = Batch.from_data_list([Data(x=x, edge_index=ei, edge_attr=ea) for x, ei, ea in graphs]).to("cuda")
    return data, lonely


def _check_maps(got, data, convs, b, r, lonely, x_in=None, ew_in=None, what=""):
    """The kernel's maps against the fp64 restatement fed the same fp32 inputs, and the properties of the definition."""
    x_in = data.x if x_in is None else x_in
    ew_in = data.edge_attr if ew_in is None else ew_in
    layers = len(convs)
    assert tuple(got.shape) == (b, layers, r, r) and got.dtype == torch.float32
    want, outs = C.gat_maps(x_in, data.edge_index, ew_in, _standin_params(convs), b, r)
    frac = C.assert_alpha_close(got, want, what)
    g = got.double().cpu()
    assert float((g.sum(2) - 1).abs().max()) <= 1e-5                                    # every target column sums to 1
    ei = data.edge_index.cpu()
    for k, lone in enumerate(lonely):
        assert bool((g[k, :, lone, lone] == 1.0).all())                                 # no incoming edge: the loop alone
        col = g[k, :, :, lone].clone()
        col[:, lone] = 0
        assert float(col.abs().max()) == 0.0
    # stored self-loops hold exactly 0: the diagonal is the added loop's alpha and nothing else — position by position
    # the map is 0 wherever neither a kept edge nor the diagonal lies
    kept = ei[:, ei[0] != ei[1]]
    free = C.count_map(kept, b, r) == 0
    free &= ~torch.eye(r, dtype=torch.bool)
    assert float(g[free[:, None].expand_as(g)].abs().max()) == 0.0
    return frac, want, outs


@pytest.mark.parametrize("rois,h0", [(5, 1), (90, 3)])
@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("f", [4, 32])
def test_gat_stack_alpha_vs_fp64(f, layers, rois, h0):
    from igcn_amd import ops
    from igcn_amd.gcn_img_snp import gat_padded_params, gat_stack
    b = 3
    data, lonely = _gat_batch(b, rois, h0, seed=10 * f + layers + rois)
    convs = _convs(layers, h0, f, seed=f + layers)
    params = gat_padded_params(convs)[2]
    plan = ops.plan_for(data)
    with torch.no_grad():
        before = gat_stack(convs, data.x, data.edge_attr, plan, rois)
        got = ops.gat_stack_alpha(data.x, data.edge_attr, plan, rois, *params)
        after = gat_stack(convs, data.x, data.edge_attr, plan, rois)
    assert torch.equal(before, after)                                                   # the forward against itself
    assert torch.equal(ops.gat_stack_alpha(data.x, data.edge_attr, plan, rois, *params), got)
    _check_maps(got, data, convs, b, rois, lonely, what=f"G F={f} L={layers} R={rois}")
    # the maps rebuild the forward: relu(G_l^T-aggregation of x_l W_l^T + bias) is xcat's slice l
    xcat = before.double().cpu().view(b, rois, layers * f)
    x_l = data.x.double().cpu().view(b, rois, h0)
    for l, c in enumerate(convs):
        h_lin = x_l @ c.lin_src.weight.detach().double().cpu().t()
        rebuilt = C.aggregate(got[:, l].cpu(), h_lin, c.bias.detach().cpu())
        x_l = xcat[:, :, l * f:(l + 1) * f]
        scale = max(float(xcat.abs().max()), 1e-30)
        err = float((rebuilt - x_l).abs().max())
        print(f"rebuilt layer {l}: err {err:.3e} of scale {scale:.3e}")
        assert err <= 1e-5 * scale, (l, err, scale)
    plan.check()


def test_gat_stack_alpha_at_a_narrow_tile():
    """400 nodes: the map tile beside the stack is narrower than 64 columns (several tiles, more threads per column)."""
    from igcn_amd import _lib, ops
    from igcn_amd.gcn_img_snp import gat_padded_params
    rois, h0, f, layers = 400, 3, 16, 2
    data, lonely = _gat_batch(1, rois, h0, seed=4)
    tc = _lib.load().igcn_gat_stack_alpha_tile(rois, data._max_edges, h0, f, layers)
    assert 0 < tc < 64
    convs = _convs(layers, h0, f, seed=9)
    got = ops.gat_stack_alpha(data.x, data.edge_attr, ops.plan_for(data), rois, *gat_padded_params(convs)[2])
    _check_maps(got, data, convs, 1, rois, lonely, what=f"G R=400 tile={tc}")


def test_gat_stack_alpha_refuses_what_the_stack_refuses():
    from igcn_amd import _lib, ops
    data, _ = _gat_batch(2, 5, 1, seed=1)
    plan = ops.plan_for(data)
    par = [torch.zeros(12, 1, device="cuda")] + [torch.zeros(12, device="cuda")] * 5
    with pytest.raises(ValueError, match="gat_stack_alpha: needs F in"):
        ops.gat_stack_alpha(data.x, data.edge_attr, plan, 5, *par)
    import ctypes
    pp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in par])
    g = torch.zeros(2, 1, 5, 5, device="cuda")
    for name, out in (("igcn_gat_stack_alpha", g), ("igcn_gat_stack_fwd", torch.zeros(10, 12, device="cuda"))):
        with pytest.raises(_lib.IgcnError, match=r"rc=-3"):                             # (refused on the host: no launch)
            _lib.call(name, 2, 5, data._max_edges, 1, 12, 1, _lib.ptr(data.x), _lib.ptr(data.edge_attr),
                      _lib.ptr(plan.src32), _lib.ptr(plan.dst32), _lib.ptr(plan.tgt_ptr), _lib.ptr(plan.tgt_perm), pp,
                      _lib.ptr(out), _lib.ptr(plan.status), _lib.stream_ptr())


# ---- 4. the models -------------------------------------------------------------------------------------------------------
def _sgcn_gat(layers=2, hidden=16, seed=3):
    from igcn_amd.sgcn import SGCN_GAT
    torch.manual_seed(seed)
    model = SGCN_GAT(DATASET, layers, hidden, rois=90, H_0=3).cuda()
    with torch.no_grad():
        for c in [model.conv1, *model.convs]:
            for p in (c.att_src, c.att_dst, c.att_edge, c.lin_edge.weight):
                p.copy_(0.5 * torch.randn_like(p))
            c.bias.copy_(0.1 * torch.randn_like(c.bias))
    return model


def _gcn_img_snp_gat():
    from igcn_amd.gcn_img_snp import GCN_IMGSNP
    torch.manual_seed(4)
    a_g, a, pool_dim = _go()
    return GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=90, H_0=3, num_classes=3, isCrossAtten=True, num_regr=3,
                      isImageOnly=False, isSNPsOnly=False, ifUseGAT=True).cuda()


@pytest.mark.parametrize("hidden", [16, 10])
@pytest.mark.parametrize("explain", [False, True])
def test_sgcn_gat_attention_vs_restatement(explain, hidden):
    """Against the restatement fed the pass's own inputs: data.x and edge_attr, or what cal_probability makes of them.
    hidden = 10 runs padded to 16 inside the kernel; the maps are those of the 10-wide layers."""
    from igcn_amd import ops
    model, data = _sgcn_gat(hidden=hidden), _brain_batch(3, 90, 3)
    x_in, ew_in = data.x, data.edge_attr
    if explain:
        with torch.no_grad():
            x_in, ew_in = model.cal_probability(data.x, data.edge_index, data.edge_attr, plan=ops.plan_for(data))[:2]
    for mode in (True, False):
        model.train(mode)
        got = model.gat_attention(data, isExplain=explain)
        assert model.training == mode
    _check_maps(got, data, [model.conv1, *model.convs], 3, 90, [], x_in, ew_in, what=f"SGCN_GAT explain={explain}")
    assert torch.equal(model.gat_attention(data, isExplain=explain), got)


def test_gcn_img_snp_gat_attention():
    model, data = _gcn_img_snp_gat(), _brain_batch(3, 90, 3)
    got = model.gat_attention(data)
    _check_maps(got, data, model._gcn_convs, 3, 90, [], what="GCN_IMGSNP(ifUseGAT)")
    with pytest.raises(ValueError, match="no masked pass"):
        model.gat_attention(data, isExplain=True)
    with pytest.raises(ValueError, match="trains no masks"):
        model.edge_importance(data)


# ---- 5. nothing else moved -------------------------------------------------------------------------------------------
def _flat(o):
    if torch.is_tensor(o):
        return [o.detach().clone()]
    if isinstance(o, (list, tuple)):
        return [t for x in o for t in _flat(x)]
    return []


def _forward(model, data, explain):
    if hasattr(model, "go_network"):
        if getattr(model, "single_pass", False):
            return model(data, None, "cuda")
        return model(data, None, "cuda", isExplain=explain)
    return model(data, isExplain=explain)


KINDS = ["sgcn_gat", "gcn_img_snp_gat", "imgsnp", "image_only"]


def _any_model(kind):
    return {"sgcn_gat": _sgcn_gat, "gcn_img_snp_gat": _gcn_img_snp_gat}.get(kind, lambda: _mask_model(kind, 90, 3))()


def _touch(model, data, kind):
    if kind != "gcn_img_snp_gat":
        model.edge_importance(data)
        model.edge_importance(data, weighted=True, return_count=True)
    if kind in ("sgcn_gat", "gcn_img_snp_gat"):
        model.gat_attention(data)
    if kind == "sgcn_gat":
        model.gat_attention(data, isExplain=True)


@pytest.mark.parametrize("kind", KINDS)
def test_forward_after_the_new_calls_launches_and_returns_what_it_did(monkeypatch, kind):
    """On one model and one batch: parameters, buffers, the training flag, the dropout counter and the CUDA random state
    are what they were before the new calls, and the forward after them makes the library calls of the forward before
    them and returns the same bits (evaluation mode: two forwards of one model draw no masks)."""
    from calltrace import record_calls
    model, data = _any_model(kind), _brain_batch(3, 90, 3)
    explain = kind != "gcn_img_snp_gat"
    model.train()
    _forward(model, data, explain)                                                      # the plan, the dropout counter
    seen = record_calls(monkeypatch)
    model.eval()
    first = _flat(_forward(model, data, explain))
    calls = list(seen)
    for mode in (True, False):
        model.train(mode)
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        rng, host_rng = torch.cuda.get_rng_state(), torch.get_rng_state()
        drop = getattr(getattr(model, "go_network", None), "_drop_state", None)
        counter = None if drop is None else drop.state.clone()
        _touch(model, data, kind)
        assert all(m.training == mode for m in model.modules())
        assert torch.equal(torch.cuda.get_rng_state(), rng) and torch.equal(torch.get_rng_state(), host_rng)
        assert counter is None or torch.equal(model.go_network._drop_state.state, counter)
        for k, v in model.state_dict().items():
            assert torch.equal(v, state[k]), k
    del seen[:]
    second = _flat(_forward(model, data, explain))
    assert len(calls) > 0 and list(seen) == calls
    assert len(first) == len(second) > 0
    for k, (a, c) in enumerate(zip(first, second)):
        assert torch.equal(a, c), k


@pytest.mark.parametrize("kind", KINDS)
def test_training_forward_after_the_new_calls_gives_a_fresh_model_s_bits(kind):
    """A training forward (dropout on) after the new calls gives the bits of a fresh model that never made them."""
    def run(touch):
        torch.manual_seed(7)
        model, data = _any_model(kind), _brain_batch(3, 90, 3)
        torch.manual_seed(7)
        model.train()
        if touch:
            _touch(model, data, kind)
        out = _flat(_forward(model, data, kind != "gcn_img_snp_gat"))
        out += [v.detach().clone() for v in model.state_dict().values()]
        return out + [torch.get_rng_state(), torch.cuda.get_rng_state()]

    fresh, touched = run(False), run(True)
    assert len(fresh) == len(touched) > 3
    for k, (a, c) in enumerate(zip(fresh, touched)):
        assert torch.equal(a, c), k


# ---- 6. the cohort pass ----------------------------------------------------------------------------------------------
def _cohort(model, source, symmetric, **kw):
    """train.connectivity_maps over 7 subjects in batches of 3 (3 + 3 + 1), labels in {0, 2} of 3 classes, against plain
    torch in fp64 on the per-sample maps of the same batches."""
    from igcn_amd import synth
    from igcn_amd.data import Batch, DataLoader
    from igcn_amd.train import connectivity_maps
    graphs = synth.brain_graph_list(7, seed=6, rois=90, h0=3, top_k=3, tsne_dim=4)
    labels = [0, 2, 2, 0, 2, 0, 2]                                                      # class 1 has no subject
    for g_, lab in zip(graphs, labels):
        g_.y = torch.tensor([lab])
    r = connectivity_maps(model, DataLoader(graphs, batch_size=3), source=source, symmetric=symmetric, num_classes=3,
                          top_k=5, device="cuda", **kw)
    maps, cnts = [], []
    for lo, hi in ((0, 3), (3, 6), (6, 7)):
        d = Batch.from_data_list(graphs[lo:hi]).to("cuda")
        if source == "mask":
            m, c = model.edge_importance(d, return_count=True, **kw)
            cnts.append(c.double().cpu())
        else:
            m = model.gat_attention(d, **kw)
        maps.append(m.double().cpu())
    maps = torch.cat(maps)                                                               # [7, R, R] or [7, L, R, R]
    y = torch.tensor(labels)
    sym = (lambda t: (t + t.transpose(-1, -2)) / 2) if symmetric else (lambda t: t)
    mean = torch.stack([maps[y == c].mean(0) if bool((y == c).any()) else torch.zeros_like(maps[0]) for c in range(3)])
    overall = maps.mean(0)
    want = {"mean": sym(mean), "overall": sym(overall)}
    keys = {"mean", "count", "overall", "strength", "top_edges", "n"}
    if source == "mask":
        present = torch.cat(cnts).mean(0)
        want["present"] = sym(present)
        want["mean_present"] = sym(torch.where(present > 0, overall / present.clamp(min=1e-300), torch.zeros_like(overall)))
        keys |= {"present", "mean_present"}
    flat = want["overall"] if source == "mask" else want["overall"].mean(0)
    want["strength"] = (flat.sum(1) + flat.sum(0)) / 2
    assert set(r) == keys and r["n"] == 7 and r["count"].cpu().tolist() == [3, 0, 4]
    for k, w in want.items():
        got = r[k]
        assert got.dtype == torch.float32 and got.shape == w.shape, k
        assert torch.allclose(got.double().cpu(), w, rtol=1e-6, atol=1e-12), k
    assert float(r["mean"][1].abs().max()) == 0.0
    # the largest entries of the returned table, largest first, as (source, target)
    got_flat = r["overall"] if source == "mask" else r["overall"].double().mean(0).float()
    top = r["top_edges"].cpu()
    assert tuple(top.shape) == (5, 2) and top.dtype == torch.int64
    vals = got_flat.cpu()[top[:, 0], top[:, 1]]
    assert torch.equal(vals, torch.topk(got_flat.cpu().reshape(-1), 5).values)
    want_vals = torch.topk(flat.reshape(-1), 5).values
    assert torch.allclose(vals.double(), want_vals, rtol=1e-6, atol=1e-12)
    return r


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_connectivity_maps_from_the_masks(weighted, symmetric):
    model = _mask_model("imgsnp", 90, 3)
    with torch.no_grad():
        model.prob_bias.normal_()
    r = _cohort(model, "mask", symmetric, weighted=weighted)
    assert tuple(r["mean"].shape) == (3, 90, 90) and tuple(r["present"].shape) == (90, 90)
    if symmetric:
        assert torch.equal(r["overall"], r["overall"].t()) and torch.equal(r["present"], r["present"].t())


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("explain", [False, True])
def test_connectivity_maps_from_the_gat_attention(explain, symmetric):
    r = _cohort(_sgcn_gat(), "gat", symmetric, isExplain=explain)
    assert tuple(r["mean"].shape) == (3, 2, 90, 90) and tuple(r["overall"].shape) == (2, 90, 90)
    assert tuple(r["strength"].shape) == (90,)
    if not symmetric:                                                                   # columns of a mean of maps sum to 1
        assert float((r["overall"].double().sum(1) - 1).abs().max()) <= 1e-5


def test_connectivity_maps_label_outside_the_classes_and_default_classes():
    from igcn_amd import _lib, synth
    from igcn_amd.data import DataLoader
    from igcn_amd.train import connectivity_maps
    graphs = synth.brain_graph_list(4, seed=6, rois=90, h0=3, top_k=3, tsne_dim=4)
    for g_, lab in zip(graphs, (0, 1, 5, 1)):
        g_.y = torch.tensor([lab])
    model = _mask_model("image_only", 90, 3)
    with pytest.raises(_lib.IgcnError, match="1 of 4 labels lie outside"):
        connectivity_maps(model, DataLoader(graphs, batch_size=3), device="cuda")       # lin2: 2 classes
    graphs[2].y = torch.tensor([0])
    for kind, c in (("image_only", 2), ("imgsnp", 3), ("clusterlabel", 3)):
        r = connectivity_maps(_mask_model(kind, 90, 3), DataLoader(graphs, batch_size=3), device="cuda")
        assert tuple(r["mean"].shape) == (c, 90, 90) and r["count"].cpu().tolist()[:2] == [2, 2]
    from igcn_amd.sgcn import SGCN_Ori
    r = connectivity_maps(SGCN_Ori(3, 8, 8, 8).cuda(), DataLoader(graphs, batch_size=3), device="cuda")
    assert tuple(r["mean"].shape) == (2, 90, 90)
