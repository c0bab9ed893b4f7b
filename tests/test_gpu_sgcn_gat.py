"""GPU checks of SGCN_GAT (kernel/sgcn.py:154-270) and of the edge-attribute gradient of the GAT stack
(igcn_gat_stack_bwd_ew):
  * the stack kernels with ``ew_in`` trained against the float64 GATConv stand-in (tests/golden/gat_standin.py);
  * the stacked (plain | masked) pair against two single passes;
  * the model against the fixture captured from the reference (tests/golden/sgcn_gat.npz: GATConv is the unpinned
    stand-in there), the edge path in isolation, the train step, the captured step and its launch count;
  * the model against its float64 restatement (tests/sgcn_gat_ref.py) at the benchmark shape;
  * the refusal of shapes outside the kernels, and the unchanged backward of GCN_IMGSNP(ifUseGAT=True)."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import assert_matches, golden_group
from _weights import seeded_state
from gat_standin import gat_conv

pytestmark = pytest.mark.gpu

TAGS = ["l2h16", "l3h10"]
DATASET = SimpleNamespace(num_features=3, num_classes=2)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _probe(outs, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal(tuple(o.shape))).float() for o in outs]


# ---- the stack kernels against the float64 stand-in (helpers as in tests/test_gpu_gat.py) ---------------------------
def _odd_graphs(n_graphs, rois, h0, seed):
    """Uniform graphs whose edge lists hold stored self-loops, duplicate edges and a node without incoming edges."""
    from igcn_amd import synth
    from igcn_amd.data import Data
    rng = np.random.default_rng(seed)
    out = []
    for g in synth.brain_graph_list(n_graphs, seed=seed, rois=rois, h0=h0, top_k=3, tsne_dim=4):
        ei, ew = g.edge_index, g.edge_attr
        lonely = int(rng.integers(rois))
        keep = ei[1] != lonely                                     # nothing arrives at ``lonely``
        ei, ew = ei[:, keep], ew[keep]
        dup = torch.from_numpy(rng.choice(ei.shape[1], 3, replace=False))
        loops = torch.from_numpy(rng.choice(rois, 2, replace=False))
        ei = torch.cat([ei, ei[:, dup], torch.stack([loops, loops]), torch.tensor([[lonely], [lonely]])], 1)
        ew = torch.cat([ew, ew[dup], torch.from_numpy(rng.random(3)).float()])
        out.append(Data(x=g.x, edge_index=ei.contiguous(), edge_attr=ew.contiguous()))
    return out


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
    return convs


@pytest.mark.parametrize("h0", [1, 3])
@pytest.mark.parametrize("hidden", [5, 10, 16, 32])
@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_gat_stack_edge_gradient_vs_fp64_standin(layers, hidden, h0):
    """The grid and the graphs of test_gat_stack_vs_fp64_standin with ``ew_in`` requiring a gradient: xcat 1e-5, dx 1e-4,
    parameter gradients 1e-4 of the layer's scale, dew 1e-4 of max|dew| (the fp32 stand-in is within 1.2e-6 of the fp64
    one on this grid), and exactly 0 at every stored self-loop."""
    from igcn_amd import ops
    from igcn_amd.data import Batch
    from igcn_amd.gcn_img_snp import gat_stack
    rois = 20
    data = Batch.from_data_list(_odd_graphs(6, rois, h0, seed=100 * layers + hidden + h0)).to("cuda")
    convs = [c.cuda() for c in _convs(layers, h0, hidden, seed=layers + hidden)]
    x = data.x.clone().requires_grad_(True)
    ew = data.edge_attr.clone().requires_grad_(True)
    xcat = gat_stack(convs, x, ew, ops.plan_for(data), rois)
    cot = torch.randn(xcat.shape, generator=torch.Generator().manual_seed(7)).double()
    (xcat.double() * cot.cuda()).sum().backward()

    xd = data.x.detach().cpu().double().requires_grad_(True)
    ei = data.edge_index.cpu()
    ea = data.edge_attr.cpu().double().requires_grad_(True)
    ref = {k: p.detach().cpu().double().requires_grad_(True) for k, p in
           ((f"{l}.{n}", p) for l, c in enumerate(convs) for n, p in c.named_parameters())}
    h, hs = xd, []
    for l in range(layers):
        h = torch.relu(gat_conv(h, ei, ea, ref[f"{l}.lin_src.weight"], ref[f"{l}.att_src"], ref[f"{l}.att_dst"],
                                ref[f"{l}.lin_edge.weight"], ref[f"{l}.att_edge"], ref[f"{l}.bias"]))
        hs.append(h)
    want = torch.cat(hs, 1)
    (want * cot).sum().backward()
    assert_matches(xcat, want.detach().numpy(), 1e-5, "xcat")
    assert_matches(x.grad, xd.grad.numpy(), 1e-4, "dx")
    for l, c in enumerate(convs):
        scale = max(float(ref[f"{l}.{n}"].grad.abs().max()) for n, _ in c.named_parameters())
        for n, p in c.named_parameters():
            assert_matches(p.grad, ref[f"{l}.{n}"].grad.numpy(), 1e-4, f"d {l}.{n}", floor=scale)
    assert ew.grad is not None and ew.grad.shape == ew.shape
    dew, dea = ew.grad.cpu(), ea.grad
    err = float((dew.double() - dea).abs().max())
    print(f"dew: max {float(dea.abs().max()):.3e}, err {err:.3e} ({err / float(dea.abs().max()):.2e} of max), "
          f"{float((dea.abs() > 1e-3 * dea.abs().max()).double().mean()):.2f} of entries above 1e-3 of max")
    assert float(dea.abs().max()) > 0
    assert_matches(ew.grad, dea.numpy(), 1e-4, "dew")
    loops = ei[0] == ei[1]
    assert int(loops.sum()) >= 6 * 3 and bool((dew[loops] == 0.0).all()) and bool((dea[loops] == 0.0).all())


@pytest.mark.parametrize("layers,hidden", [(2, 16), (3, 10)])
def test_stacked_pair_equals_two_passes(layers, hidden):
    """gat_stack on plan.replicate(2) with (plain | masked)-like stacked inputs against two g = 1 calls: one workgroup per
    graph and no cross-graph arithmetic, so xcat, dx and dew are expected bit for bit; the parameter gradients are sums
    over 12 instead of 6 + 6 per-graph rows (another summation order), held to 1e-6 of the layer's scale."""
    from igcn_amd import ops
    from igcn_amd.data import Batch
    from igcn_amd.gcn_img_snp import gat_stack
    rois, h0 = 20, 3
    data = Batch.from_data_list(_odd_graphs(6, rois, h0, seed=41)).to("cuda")
    plan = ops.plan_for(data)
    gen = torch.Generator().manual_seed(3)
    xs = [data.x.clone(), (data.x * torch.rand(data.x.shape, generator=gen).cuda()).contiguous()]
    ews = [data.edge_attr.clone(), (data.edge_attr * torch.rand(data.edge_attr.shape, generator=gen).cuda()).contiguous()]
    cot = torch.randn(2 * data.x.shape[0], layers * hidden, generator=gen).cuda()
    n = data.x.shape[0]

    convs = [c.cuda() for c in _convs(layers, h0, hidden, seed=9)]
    x2 = torch.cat(xs).requires_grad_(True)
    ew2 = torch.cat(ews).requires_grad_(True)
    xcat2 = gat_stack(convs, x2, ew2, plan.replicate(2), rois)
    (xcat2 * cot).sum().backward()
    pair = {k: p.grad.clone() for k, p in ((f"{l}.{m}", p) for l, c in enumerate(convs) for m, p in c.named_parameters())}

    single = {k: torch.zeros_like(v) for k, v in pair.items()}
    bitwise = True
    for k in range(2):
        for c in convs:
            c.zero_grad()
        x1, ew1 = xs[k].clone().requires_grad_(True), ews[k].clone().requires_grad_(True)
        xcat1 = gat_stack(convs, x1, ew1, plan, rois)
        (xcat1 * cot[k * n:(k + 1) * n]).sum().backward()
        ne = ew1.shape[0]
        for what, a, b in (("xcat", xcat2[k * n:(k + 1) * n], xcat1), ("dx", x2.grad[k * n:(k + 1) * n], x1.grad),
                           ("dew", ew2.grad[k * ne:(k + 1) * ne], ew1.grad)):
            assert_matches(a, b.detach().cpu().numpy(), 1e-6, f"{what} half {k}")
            bitwise &= bool(torch.equal(a, b))
        for l, c in enumerate(convs):
            for m, p in c.named_parameters():
                single[f"{l}.{m}"] += p.grad
    assert bitwise, "per-graph outputs of the stacked pair differ from the single passes in some bit"
    for l in range(layers):
        scale = max(float(v.abs().max()) for k, v in single.items() if k.startswith(f"{l}."))
        for k, v in single.items():
            if k.startswith(f"{l}."):
                assert_matches(pair[k], v.cpu().numpy(), 1e-6, "d " + k, floor=scale)


# ---- SGCN_GAT against the reference fixture ---------------------------------------------------------------------------
def _model(store, tag):
    from igcn_amd import synth
    from igcn_amd.sgcn import SGCN_GAT
    rois, hidden, layers, bsz, seed, top_k = [int(v) for v in store[f"{tag}/cfg"]]
    model = SGCN_GAT(DATASET, layers, hidden, rois=rois, H_0=3).cuda()
    assert sorted(model.state_dict().keys()) == sorted(store[f"{tag}/state_keys"].tolist())
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, seed, model.state_dict())
    model.load_state_dict(sd)                                      # reference-keyed state, strict
    model._dropout_enabled = False
    graphs = synth.brain_graph_list(bsz, seed=seed + 10, rois=rois, top_k=top_k, tsne_dim=16, num_classes=2)
    return model, graphs, seed


def _batch(graphs):
    from igcn_amd.data import Batch
    return Batch.from_data_list(graphs).to("cuda")


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("explain", [False, True])
def test_sgcn_gat_vs_reference_golden(golden, tag, mode, explain):
    store = golden("sgcn_gat")
    model, graphs, seed = _model(store, tag)
    model.train(mode == "train")
    data = _batch(graphs)
    out = model(data, explain)
    assert model.input is data.x and data.x.requires_grad
    sub = f"{tag}/{mode}/explain{int(explain)}"
    assert_matches(out, golden_group(store, sub + "/out")["logp"], 1e-4, "logp")
    (out * _probe([out], seed + 3)[0].cuda()).sum().backward()
    wg = golden_group(store, sub + "/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), 1e-3, "grad data.x")
    params = dict(model.named_parameters())
    assert ("prob_bias" in wg) == explain
    for k, w in wg.items():
        assert params[k].grad is not None, k
        assert_matches(params[k].grad, w, 1e-3, "grad " + k, floor=1e-4)


@pytest.mark.parametrize("tag", TAGS)
def test_edge_path_alone_vs_reference_golden(golden, tag):
    """The gradients of hp.lamda_mi * mi alone: ``prob_bias`` is reached through the edge attributes of the GATConv layers
    only (logit term + mean-valued loop), ``prob`` partly.  Both to 1e-3 of their own maximum, no floor (the reference's
    fp32 run agrees with an fp64 one to 6e-7 of it); a dropped dew gives prob_bias.grad == 0 and fails."""
    import torch.nn.functional as F
    from igcn_amd.train import HP
    store = golden("sgcn_gat")
    model, graphs, _ = _model(store, tag)
    model.train(True)
    data = _batch(graphs)
    (HP.lamda_mi * F.nll_loss(model(data, True), data.y.view(-1))).backward()
    wg = golden_group(store, f"{tag}/mi_only/grad")
    for k in ("prob_bias", "prob"):
        g, w = model.get_parameter(k).grad, wg[k]
        assert g is not None and float(np.abs(w).max()) > 0
        err = float((g.cpu().double() - torch.from_numpy(w).double()).abs().max())
        print(f"{tag} mi_only {k}: max {float(np.abs(w).max()):.3e}, err {err:.3e} "
              f"({err / float(np.abs(w).max()):.2e} of max)")
        assert_matches(g, w, 1e-3, "grad " + k)
    assert_matches(data.x.grad, wg["data.x"], 1e-3, "grad data.x")


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("batched", [True, False])
def test_sgcn_gat_train_step_vs_reference_golden(golden, tag, batched):
    """train() of kernel/train_eval_sgcn.py:296-313: loss terms, gradients and the post-Adam parameters (bounds of
    test_sgcn_only_train_step_vs_reference_golden)."""
    from igcn_amd.train import FlatAdam, losses
    store = golden("sgcn_gat")
    model, graphs, _ = _model(store, tag)
    model.train(True)
    model.batched_passes = batched
    data = _batch(graphs)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss, terms, _ = losses(model, data)
    ref = float(store[f"{tag}/step/loss"])
    assert abs(float(loss.detach()) - ref) <= 1e-4 * max(1.0, abs(ref))
    assert set(terms) == {"ce", "mi", "prob"}
    for k, v in terms.items():
        assert abs(float(v) - float(store[f"{tag}/step/term/{k}"])) <= 1e-4, k
    loss.backward()
    params = dict(model.named_parameters())
    wg = golden_group(store, f"{tag}/step/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), 1e-3, "grad data.x")
    for k, w in wg.items():
        assert_matches(params[k].grad, w, 1e-3, "grad " + k, floor=1e-5)
    opt.step()
    for k, w in golden_group(store, f"{tag}/step/param_after").items():
        p = params[k].detach().cpu()
        if isinstance(w, tuple):
            assert_matches(p, w, 2.5e-3, "param " + k, floor=1.0)
            continue
        assert float((p - torch.from_numpy(w)).abs().max()) <= 2.01e-3, "param " + k
        if k in wg and not isinstance(wg[k], tuple):
            g = torch.from_numpy(wg[k])
            solid = g.abs() > 5e-2 * g.abs().max()
            if solid.any():
                assert float((p - torch.from_numpy(w)).abs()[solid].max()) <= 5e-5, "param " + k


def test_graphed_step_equals_eager_steps_and_launches_one_pair(golden, monkeypatch):
    """Three GraphedTrainStep replays against three eager train_steps (parameters after each step, the tolerance of
    test_graphed_step_equals_eager_steps), then one recorded eager step: one igcn_gat_stack_fwd and one
    igcn_gat_stack_bwd_ew for the stacked pair, no GCN stack."""
    from calltrace import record_calls
    from igcn_amd import _lib
    from igcn_amd.train import FlatAdam, GraphedTrainStep, assert_nothing_pending, eval_acc, eval_loss, train_step
    from igcn_amd.data import DataLoader
    store = golden("sgcn_gat")
    m1, graphs, _ = _model(store, "l2h16")
    m2, _, _ = _model(store, "l2h16")
    m1.train(True)
    m2.train(True)
    batches = [_batch(graphs), _batch(graphs[::-1]), _batch(graphs[2:] + graphs[:2])]
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    static = copy.copy(batches[0])
    for k in ("x", "edge_index", "edge_attr", "y", "ptr", "edge_ptr", "batch"):
        if getattr(batches[0], k, None) is not None:
            setattr(static, k, getattr(batches[0], k).clone())
    static._igcn_plan = None
    step = GraphedTrainStep(m2, o2, static, warmup=1)
    p1, p2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    for b in batches:
        l1 = float(train_step(m1, o1, b))
        step.load(b)
        l2 = float(step())
        assert abs(l1 - l2) <= 1e-5 * max(1.0, abs(l1)), (l1, l2)
        for k in p1:
            assert_matches(p2[k], p1[k].detach().cpu().numpy(), 1e-5, k, floor=1e-3)
    # the evaluation loops of the image-only trainer run on the model as they do for SGCN_GCN
    acc = eval_acc(m1, DataLoader(graphs, batch_size=2), device="cuda")
    lo = eval_loss(m1, DataLoader(graphs, batch_size=2), device="cuda")
    assert 0.0 <= float(acc) <= 1.0 and np.isfinite(float(lo[0] if isinstance(lo, (tuple, list)) else lo))
    m1.train(True)
    monkeypatch.setattr(_lib, "_DEBUG_SYNC", True)
    seen = record_calls(monkeypatch)
    train_step(m1, o1, batches[0])
    names = [c[0] for c in seen]
    assert names.count("igcn_gat_stack_fwd") == 1 and names.count("igcn_gat_stack_bwd_ew") == 1, names
    assert "igcn_gat_stack_bwd" not in names
    assert not any(n.startswith("igcn_sgcn_stack") or n.startswith("igcn_gcn_") for n in names), names
    assert_nothing_pending("test")


def _gcn_twin(seed=72):
    from igcn_amd.sgcn import SGCN_GCN
    model = SGCN_GCN(None, 3, 10, rois=90, H_0=3, num_features=3, num_classes=2).cuda()
    model.load_state_dict(seeded_state({k: v.shape for k, v in model.state_dict().items()}, seed, model.state_dict()))
    model._dropout_enabled = False
    return model


@pytest.mark.parametrize("kind", ["SGCN_GAT", "SGCN_GCN"])
def test_fit_epoch_equals_the_eager_loop(golden, kind):
    """Two epochs of 4 + 4 + 2 graphs through fit_epoch (eager, captured and replayed steps, a tail shape) against the
    same six steps through the eager train_step on a twin model.  The first captured step follows an EAGER step of the
    same model: the shared forward must let go of that step's edge mask (and with it of its autograd graph) before it
    builds the next one — for SGCN_GCN, which shares that code, as for SGCN_GAT."""
    from igcn_amd import synth
    from igcn_amd.data import DataLoader
    from igcn_amd.train import FlatAdam, fit_epoch, train_step
    store = golden("sgcn_gat")
    if kind == "SGCN_GAT":
        m1, _, _ = _model(store, "l3h10")
        m2, _, _ = _model(store, "l3h10")
    else:
        m1, m2 = _gcn_twin(), _gcn_twin()
    m1.train(True)
    m2.train(True)
    graphs = synth.brain_graph_list(10, seed=77, rois=90, top_k=3, tsne_dim=16, num_classes=2)
    loader = DataLoader(graphs, 4, shuffle=False)
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    for epoch in range(2):
        got = fit_epoch(m1, o1, loader, device="cuda")
        total = 0.0
        for data in loader:
            data = data.to("cuda")
            total += float(train_step(m2, o2, data)) * data.num_graphs
        assert got == pytest.approx(total / len(graphs), rel=1e-4), (epoch, got, total / len(graphs))
    assert int(o1.step_count.item()) == int(o2.step_count.item()) == 6
    p2 = dict(m2.named_parameters())
    for k, p in m1.named_parameters():
        assert_matches(p, p2[k].detach().cpu().numpy(), 1e-5, k, floor=1e-3)


@pytest.mark.parametrize("bsz", [32, 256])
def test_sgcn_gat_vs_fp64_at_bench_shape(bsz):
    """B = 32 and B = 256, L = 2, hidden 16, both passes, against the float64 restatement tests/sgcn_gat_ref.py: logp 1e-4,
    data.x.grad and every parameter gradient 3e-3 on the tensor's own scale (a d att_dst that is 0 in exact arithmetic: see
    below)."""
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from igcn_amd.sgcn import SGCN_GAT
    from sgcn_gat_ref import model_forward
    model = SGCN_GAT(DATASET, 2, 16, rois=90, H_0=3).cuda().eval()
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, 6)
    model.load_state_dict(sd)
    graphs = synth.brain_graph_list(bsz, seed=1000, rois=90, tsne_dim=16, num_classes=2)
    for explain in (False, True):
        data = Batch.from_data_list(graphs).to("cuda")
        model.zero_grad()
        out = model(data, explain)
        cot = _probe([out], 4)[0]
        (out * cot.cuda()).sum().backward()
        ref_sd = {k: p.detach().cpu().double().requires_grad_(True) for k, p in model.named_parameters()}
        dcpu = Batch.from_data_list(graphs)
        dcpu.x = dcpu.x.double().requires_grad_(True)
        dcpu.edge_attr = dcpu.edge_attr.double()
        ref = model_forward(ref_sd, 90, dcpu, explain)
        (ref * cot.double()).sum().backward()
        assert_matches(out, ref.detach().numpy(), 1e-4, "logp")
        assert_matches(data.x.grad, dcpu.x.grad.numpy(), 3e-3, "grad data.x")
        for k, p in model.named_parameters():
            w = ref_sd[k].grad
            if w is None:
                assert p.grad is None or not bool(p.grad.abs().max() > 0), k
                continue
            own = float(w.abs().max())
            err = float((p.grad.cpu().double() - w).abs().max())
            print(f"B={bsz} explain={int(explain)} grad {k}: max {own:.3e} err {err:.3e} ({err / max(own, 1e-300):.2e} "
                  "of max)")
            if k.endswith(".att_dst"):
                # Where every logit of a layer sits on one side of the leaky ReLU, a_d[i] shifts all logits of target i's
                # softmax alike and d att_dst is 0 in exact arithmetic: the float64 figure is then rounding noise (1e-17),
                # no scale to judge on.  ONLY there (float64 value below 1e-12 of the layer's largest gradient) the kernel's
                # value is held to 3e-3 of the layer's scale, as test_gat_stack_vs_fp64_standin judges it; every other
                # att_dst gradient is held to its own maximum like any parameter.
                layer = max(float(g.grad.abs().max()) for n, g in ref_sd.items()
                            if n.startswith(k[:-len("att_dst")]) and g.grad is not None)
                if own < 1e-12 * layer:
                    assert float(p.grad.abs().max()) <= 3e-3 * layer, (k, float(p.grad.abs().max()), layer)
                    continue
            assert_matches(p.grad, w.numpy(), 3e-3, f"grad {k} (explain={explain})")


# ---- limits ----------------------------------------------------------------------------------------------------------
def test_shapes_outside_the_stack_raise_value_error():
    from igcn_amd import synth
    from igcn_amd.sgcn import SGCN_GAT
    data = _batch(synth.brain_graph_list(2, seed=5, rois=90, tsne_dim=16, num_classes=2))
    wide = SGCN_GAT(DATASET, 2, 64, rois=90, H_0=3).cuda()
    for explain in (False, True):
        with pytest.raises(ValueError, match="F in"):
            wide(data, explain)
    with pytest.raises(ValueError, match="F in"):
        wide.forward_pair(data)
    # graphs of 80 and 100 nodes: 180 nodes in all, but not uniform graphs of 90
    from igcn_amd.data import Data
    uneven = _batch([Data(x=g.x, edge_index=g.edge_index, edge_attr=g.edge_attr, y=g.y)
                     for g in synth.brain_graph_list(1, seed=5, rois=80, tsne_dim=16, num_classes=2)
                     + synth.brain_graph_list(1, seed=6, rois=100, tsne_dim=16, num_classes=2)])
    model = SGCN_GAT(DATASET, 2, 16, rois=90, H_0=3).cuda()
    with pytest.raises(ValueError, match="uniform graphs"):
        model(uneven, True)
    torch.cuda.synchronize()


def test_gcn_imgsnp_gat_backward_keeps_its_entry_point(golden, monkeypatch):
    """GCN_IMGSNP(ifUseGAT=True): the edge attributes are data there, the backward is igcn_gat_stack_bwd as before."""
    from calltrace import record_calls
    from igcn_amd import synth
    from igcn_amd.gcn_img_snp import GCN_IMGSNP
    from igcn_amd.train import FlatAdam, train_step
    store = golden("gcn_imgsnp_gat")
    rois, hidden, layers, bsz, seed, top_k = [int(v) for v in store["l2h16/cfg"]]
    go_snps, adj, pool_dim = synth.go_hierarchy(tuple(store["pool"].tolist()), seed=seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    model = GCN_IMGSNP(layers, hidden, a_g, a, pool_dim, 32, "cuda", rois=rois, H_0=3, num_classes=3,
                       isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseFeat4Regr=True,
                       isImageOnly=False, isSNPsOnly=False, ifUseGAT=True).cuda()
    model.train(True)
    data = _batch(synth.brain_graph_list(8, seed=seed + 10, rois=rois, top_k=top_k, tsne_dim=16))
    opt = FlatAdam(model.parameters(), lr=1e-3)
    seen = record_calls(monkeypatch)
    train_step(model, opt, data, store["lam_alt"].tolist())
    names = [c[0] for c in seen]
    assert names.count("igcn_gat_stack_bwd") == 1 and "igcn_gat_stack_bwd_ew" not in names, names
    torch.cuda.synchronize()
