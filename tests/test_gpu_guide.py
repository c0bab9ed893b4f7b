"""GPU checks of GUIDE_IMGSNP and its kernels (csrc/guide.hip):
  * the PReLU forms (LayerNorm over nodes, BatchNorm1d on [B, C], per-node linear + BatchNorm) against float64 torch,
    dropout on, slopes 0.25 / negative / above 1, and bit-identical d slope from two identical calls;
  * the gate + encoder_i_N kernel against a float64 restatement (tests/guide_ref.py) with imposed noise, and eval;
  * the generator contract: the kernel's draws rebuilt on the host, successive counters, no draw in eval;
  * the model and the stand-alone GUIDE GO network against the fixtures captured from the reference;
  * GraphedTrainStep against eager train_step, the epoch functions, and Evaluator's refusal."""
import copy

import numpy as np
import pytest
import torch

import guide_ref
from conftest import assert_matches, golden_group
from _weights import seeded_state

pytestmark = pytest.mark.gpu

TAGS = ["h16", "h10"]
NAMES = ["logp", "x_hat", "latent", "lin_f", "reg", "img", "decoded", "prob"]
TERMS = ("ce", "reg", "recon", "recon_img", "sparsity")
SLOPES = [0.25, -0.3, 1.7]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _prelu(u, a):
    return torch.where(u > 0, u, a * u)


def _keep(shape, p, gen):
    return ((torch.rand(shape, generator=gen) >= p).double() / (1 - p))


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


# ---- the PReLU forms against float64 torch ---------------------------------------------------------------------------
@pytest.mark.parametrize("a", SLOPES)
def test_nodes_ln_prelu_vs_fp64(a):
    from igcn_amd import ops
    g = torch.Generator().manual_seed(1)
    b, f, n, pool = 4, 5, 37, 6
    y = torch.randn(b, f, n, generator=g, dtype=torch.float64)
    gamma = 1 + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
    beta = 0.2 * torch.randn(n, generator=g, dtype=torch.float64)
    keep = _keep((b, n), 0.4, g)
    slope = torch.tensor([a], dtype=torch.float64)
    cot = torch.randn(b, f, n - pool, generator=g, dtype=torch.float64)
    ref = [_leaf(t) for t in (y, gamma, beta, slope)]
    mu = ref[0].mean(-1, keepdim=True)
    var = ref[0].var(-1, unbiased=False, keepdim=True)
    z = _prelu((ref[0] - mu) / torch.sqrt(var + 1e-5) * ref[1] + ref[2], ref[3]) * keep.unsqueeze(1)
    z = z[..., pool:]
    (z * cot).sum().backward()
    das = []
    for _ in range(2):
        got = [_leaf(t.float().cuda()) for t in (y, gamma, beta, slope)]
        zg = ops.NodesLayerNormPReLU.apply(*got, keep.float().cuda(), pool, 1e-5)
        (zg * cot.float().cuda()).sum().backward()
        das.append(got[3].grad.clone())
    assert_matches(zg, z.detach().numpy(), 1e-5, "z")
    for r, t, w in zip(ref, got, ("dy", "dgamma", "dbeta", "dslope")):
        assert_matches(t.grad, r.grad.numpy(), 1e-4, w)
    assert torch.equal(das[0], das[1])


@pytest.mark.parametrize("a", SLOPES)
@pytest.mark.parametrize("f", [0, 5])
def test_bn_prelu_vs_fp64(a, f):
    from igcn_amd import ops
    g = torch.Generator().manual_seed(2 + f)
    b, c = 64, 40
    x = torch.randn((b, c) if f == 0 else (b, f, c), generator=g, dtype=torch.float64)
    w = torch.randn(1, f, generator=g, dtype=torch.float64) if f else None
    bn = torch.nn.BatchNorm1d(c).double()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(c, generator=g, dtype=torch.float64))
        bn.bias.copy_(0.2 * torch.randn(c, generator=g, dtype=torch.float64))
    bn_gpu = copy.deepcopy(bn).float().cuda()
    keep = _keep((b, c), 0.5, g)
    slope = torch.tensor([a], dtype=torch.float64)
    cot = torch.randn(b, c, generator=g, dtype=torch.float64)
    xr, sr = _leaf(x), _leaf(slope)
    wr = _leaf(w) if f else None
    pre = xr if f == 0 else torch.einsum("of,bfc->bc", wr, xr)
    out = _prelu(bn(pre), sr) * keep
    (out * cot).sum().backward()
    das = []
    for _ in range(2):
        bg = copy.deepcopy(bn_gpu)
        xg, sg = _leaf(x.float().cuda()), _leaf(slope.float().cuda())
        wg = _leaf(w.float().cuda()) if f else None
        og = ops.BatchNormPReLU.apply(xg, wg, bg.weight, bg.bias, sg, bg, True, keep.float().cuda())
        (og * cot.float().cuda()).sum().backward()
        das.append(sg.grad.clone())
    assert_matches(og, out.detach().numpy(), 1e-5, "y")
    assert_matches(xg.grad, xr.grad.numpy(), 1e-4, "dx")
    assert_matches(sg.grad, sr.grad.numpy(), 1e-4, "dslope")
    assert_matches(bg.weight.grad, bn.weight.grad.numpy(), 1e-4, "dgamma")
    assert_matches(bg.bias.grad, bn.bias.grad.numpy(), 1e-4, "dbeta")
    if f:
        assert_matches(wg.grad, wr.grad.numpy(), 1e-4, "dW")
    assert_matches(bg.running_mean, bn.running_mean.numpy(), 1e-5, "running_mean")
    assert_matches(bg.running_var, bn.running_var.numpy(), 1e-5, "running_var")
    assert torch.equal(das[0], das[1])


def test_node_linear_bn_prelu_wide_forward_vs_fp64():
    """conc_for_attention's form (D > 1): output and running statistics only."""
    from igcn_amd import ops
    g = torch.Generator().manual_seed(4)
    b, f, c, d = 16, 5, 80, 16
    x = torch.randn(b, f, c, generator=g, dtype=torch.float64)
    w = torch.randn(d, f, generator=g, dtype=torch.float64)
    bn = torch.nn.BatchNorm1d(c).double()
    bn_gpu = copy.deepcopy(bn).float().cuda()
    out = _prelu(bn(torch.einsum("df,bfc->bcd", w, x)), -0.2)
    y, _, _ = ops.bn_prelu_forward(x.float().cuda(), w.float().cuda(), bn_gpu, torch.tensor([-0.2], device="cuda"), True)
    assert_matches(y, out.detach().numpy(), 1e-5, "y")
    assert_matches(bn_gpu.running_var, bn.running_var.detach().numpy(), 1e-5, "running_var")


# ---- the gate + encoder kernel ---------------------------------------------------------------------------------------
def _gate_inputs(b=8, k=270, h=32, l=32, seed=5):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(b, k, generator=g, dtype=torch.float64)
    bias = 0.1 * (2 * torch.rand(k, 2, generator=g, dtype=torch.float64) - 1)
    w1 = torch.randn(h, k, generator=g, dtype=torch.float64) / k ** 0.5
    w2 = torch.randn(l, h, generator=g, dtype=torch.float64) / h ** 0.5
    keep = _keep((b, h), 0.4, g)
    noise = torch.from_numpy(guide_ref.gumbel_noise(77, b, k)).double()
    return img, bias, w1, w2, keep, noise


@pytest.mark.parametrize("training", [True, False])
def test_gate_encoder_vs_fp64(training):
    from igcn_amd import ops
    img, bias, w1, w2, keep, noise = _gate_inputs()
    a, tau = torch.tensor([-0.3], dtype=torch.float64), 0.1
    s, _ = guide_ref.soft_sample(bias, noise, tau)
    far = ((s[..., 1] - s[..., 0]).abs() > 1e-5).all()
    assert bool(far)                                   # (no decision within fp32 rounding of a tie at this seed)
    ref = [_leaf(t) for t in (img, bias, w1, a, w2)]
    lat, imp1 = guide_ref.gate_encoder(*ref[:3], ref[3], ref[4], keep, tau, noise, training)
    g = torch.Generator().manual_seed(9)
    c1, c2 = torch.randn(lat.shape, generator=g, dtype=torch.float64), torch.randn(imp1.shape, generator=g, dtype=torch.float64)
    ((lat * c1).sum() + (imp1 * c2).sum()).backward()
    got = [_leaf(t.float().cuda()) for t in (img, bias, w1, a, w2)]
    tau_t = torch.tensor(tau, device="cuda")
    lg, ig, gate = ops.GuideGate.apply(*got, keep.float().cuda(), tau_t, training, noise.float().cuda(), None)
    ((lg * c1.float().cuda()).sum() + (ig * c2.float().cuda()).sum()).backward()
    assert_matches(lg, lat.detach().numpy(), 1e-4, "latent_n")
    assert_matches(ig, imp1.detach().numpy(), 1e-5, "imp1")
    for r, t, w in zip(ref, got, ("d img", "d bias_n", "dW1", "d slope", "dW2")):
        assert_matches(t.grad, r.grad.numpy(), 1e-3, w)
    if training:
        _, z1 = guide_ref.soft_sample(bias, noise, tau)
        assert torch.equal((gate[..., 0] > 0.5).cpu(), z1 > 0.5)
    else:
        assert gate is None


def test_gate_generator_contract():
    from igcn_amd import ops
    img, bias, w1, w2, keep, _ = _gate_inputs(b=16, seed=6)
    args = [t.float().cuda() for t in (img, bias, w1)] + [torch.tensor([0.25], device="cuda"), w2.float().cuda()]
    state = ops.DropoutState("cuda")
    c0 = int(state.state[0].item())
    for step in range(2):
        _, _, gate = ops.GuideGate.apply(*args, None, 0.1, True, None, state)
        assert int(state.state[0].item()) == c0 + step + 1 and int(state.state[1].item()) == 0
        s, z1 = guide_ref.soft_sample(bias, torch.from_numpy(guide_ref.gumbel_noise(c0 + step, 16, 270)).double(), 0.1)
        far = (s[..., 1] - s[..., 0]).abs() > 1e-6
        got = (gate[..., 0] > 0.5).cpu()
        assert bool(far.float().mean() > 0.99)
        assert torch.equal(got[far], (z1 > 0.5)[far]), "kernel draws differ from the host rebuild"
    ops.GuideGate.apply(*args, None, 0.1, False, None, state)
    assert int(state.state[0].item()) == c0 + 2                     # an eval forward draws nothing


def test_gate_limits_match_the_model_constants():
    from igcn_amd import guide_img_snp, ops
    k, h = guide_img_snp.GATE_K_MAX, guide_img_snp.GATE_H_MAX
    assert ops.guide_gate_supported(k, h, 32) and not ops.guide_gate_supported(k + 1, h, 32)
    assert not ops.guide_gate_supported(k, h + 1, 32)


# ---- the model against the reference fixtures ------------------------------------------------------------------------
def _model(store, tag):
    from igcn_amd import synth
    from igcn_amd.guide_img_snp import GUIDE_IMGSNP
    rois, hidden, bsz, seed, ncls, hl = [int(v) for v in store[f"{tag}/cfg"]]
    go_snps, adj, pool_dim = synth.go_hierarchy(tuple(store["pool"].tolist()), seed=seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    model = GUIDE_IMGSNP(2, hidden, a_g, a, pool_dim, 32, "cuda", rois=rois, H_0=3, num_classes=ncls, num_regr=3,
                         hidden_linear=hl).cuda()
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, seed, model.state_dict())
    model.load_state_dict(sd)
    model._dropout_enabled = False
    model.go_network._dropout_enabled = False
    graphs = synth.brain_graph_list(bsz, seed=seed + 10, rois=rois, top_k=3, tsne_dim=16)
    return model, graphs


def _batch(graphs):
    from igcn_amd.data import Batch
    return Batch.from_data_list(graphs).to("cuda")


def _named(o):
    return dict(zip(NAMES, (o[0], o[1], o[2], o[4], o[5], o[6][0], o[6][1], o[7][0])))


@pytest.mark.parametrize("tag", TAGS)
def test_model_eval_vs_reference_golden(golden, tag):
    store = golden("guide_imgsnp")
    model, graphs = _model(store, tag)
    model.eval()
    with torch.no_grad():
        outs = _named(model(_batch(graphs), torch.tensor(0.1, device="cuda"), "cuda"))
    want = golden_group(store, f"{tag}/eval")
    for n in NAMES:
        assert_matches(outs[n], want[n], 1e-4, n)


@pytest.mark.parametrize("tag", TAGS)
def test_model_train_vs_reference_golden(golden, tag):
    from igcn_amd.train import losses
    store = golden("guide_imgsnp")
    model, graphs = _model(store, tag)
    model.train()
    model._gate_noise = torch.from_numpy(store[f"{tag}/noise"]).cuda()
    data = _batch(graphs)
    loss, terms, outs = losses(model, data, temperature=torch.tensor(float(store["tau"]), device="cuda"))
    want = golden_group(store, f"{tag}/train")
    for n, o in _named(outs).items():
        assert_matches(o, want[n], 1e-4, n)
    for k in TERMS:
        ref = float(store[f"{tag}/term/{k}"])
        assert abs(float(terms[k]) - ref) <= 1e-4 * max(1.0, abs(ref)), (k, float(terms[k]), ref)
    ref = float(store[f"{tag}/loss"])
    assert abs(float(loss) - ref) <= 1e-4 * max(1.0, abs(ref))
    sd = model.state_dict()
    for k, w in golden_group(store, f"{tag}/running").items():      # conc_for_attention.1 included
        assert_matches(sd[k].float(), np.asarray(w, dtype=np.float32), 1e-4, k)
    loss.backward()
    wg = golden_group(store, f"{tag}/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), 1e-3, "grad data.x")
    params = dict(model.named_parameters())
    go_scale = max(float(np.abs(w).max()) for k, w in wg.items() if k.startswith("go_network.") and not isinstance(w, tuple))
    for k, w in wg.items():
        assert params[k].grad is not None, k
        floor = 1e-5
        sib = wg.get(k[:-5] + ".weight") if k.endswith(".bias") else None
        if sib is not None and not isinstance(sib, tuple):
            floor = max(floor, 0.5 * float(np.abs(sib).max()))
        if k.startswith("go_network."):
            floor = max(floor, go_scale)
        assert_matches(params[k].grad, w, 1e-3, "grad " + k, floor=floor)
    no_grad = set(store[f"{tag}/no_grad"].tolist())
    for k, p in params.items():                # nothing the reference leaves without a gradient gets one here
        if k in no_grad:
            assert p.grad is None or not bool(p.grad.abs().max() > 0), "unexpected grad " + k


def test_guide_go_network_vs_reference_golden(golden):
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from igcn_amd.guide_go_model import Gene_ontology_network
    store = golden("guide_imgsnp")
    bsz, seed, atten = [int(v) for v in store["go/cfg"]]
    go_snps, adj, pool_dim = synth.go_hierarchy(tuple(store["pool"].tolist()), seed=seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    net = Gene_ontology_network(a_g, a, 2, 2, [5, 5], pool_dim, 32, "cuda", dim_snps_atten=atten).cuda()
    net.load_state_dict(seeded_state({k: v.shape for k, v in net.state_dict().items()}, seed, net.state_dict()))
    net._dropout_enabled = False
    net.train()
    snps = Batch.from_data_list(synth.brain_graph_list(bsz, seed=seed + 10, rois=90, top_k=3, tsne_dim=16)).snps_feat
    latent, x_d, _, atten_out = net(snps.cuda(), None, "cuda")
    want = golden_group(store, "go/out")
    for n, o in (("latent", latent), ("x_d", x_d), ("atten_out", atten_out)):
        assert_matches(o, want[n], 1e-4, n)
    sd = net.state_dict()
    for k, w in golden_group(store, "go/running").items():
        assert_matches(sd[k].float(), np.asarray(w, dtype=np.float32), 1e-4, k)
    ((latent * torch.from_numpy(store["go/c1"]).cuda()).sum() + (x_d * torch.from_numpy(store["go/c2"]).cuda()).sum()).backward()
    wg = golden_group(store, "go/grad")
    # judged on the scale of the branch, as tests/test_gpu_gat.py judges the GO network: its LayerNorm scales take gradients
    # far below the branch's largest, and fp32 rounding through the attention moves them by a few 1e-3 of their own size
    scale = max(float(np.abs(w).max()) for w in wg.values() if not isinstance(w, tuple))
    params = dict(net.named_parameters())
    for k, w in wg.items():
        assert_matches(params[k].grad, w, 1e-3, "grad " + k, floor=scale)
    for k in store["go/no_grad"].tolist():
        assert params[k].grad is None, k


# ---- the captured step, the epoch functions ---------------------------------------------------------------------------
def test_graphed_step_equals_eager_steps_with_dropout_and_gate(golden):
    from igcn_amd import ops
    from igcn_amd.train import FlatAdam, GraphedTrainStep, train_step
    store = golden("guide_imgsnp")
    m1, graphs = _model(store, "h16")
    for m in (m1, m1.go_network):
        m._dropout_enabled = True
    m1.train()
    m2 = copy.deepcopy(m1)
    tau = torch.tensor(0.1, device="cuda")
    batches = [_batch(graphs[k::2] * 2) for k in range(2)] + [_batch(graphs[8:] + graphs[:8])]
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    static = _batch(graphs)
    step = GraphedTrainStep(m1, o1, static, warmup=2, temperature=tau)
    for src, dst in ((m1.go_network, m2.go_network), (m1, m2)):      # twins' generators aligned after the capture
        name = "_drop_state" if src is m1.go_network else "_gate_state"
        st = ops.DropoutState("cuda")
        st.state.copy_(getattr(src, name).state)
        setattr(dst, name, st)
    for b in batches:
        step.load(b)
        l1 = float(step())
        l2 = float(train_step(m2, o2, b, temperature=tau))
        assert abs(l1 - l2) <= 1e-4 * max(1.0, abs(l2)), (l1, l2)
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        d = (p1.detach() - p2.detach()).abs()
        tol = torch.full_like(d, 2e-4) if p2.grad is None else torch.where(p2.grad.abs() > 1e-6, 2e-4, 3.5e-3)
        assert bool((d <= tol).all()), (k, float(d.max()))


def test_epoch_functions_and_evaluator_refusal(golden):
    from igcn_amd.train import Evaluator, FlatAdam, eval_acc, eval_loss, eval_outputs, fit_epoch
    store = golden("guide_imgsnp")
    model, graphs = _model(store, "h10")
    for m in (model, model.go_network):
        m._dropout_enabled = True
    loader = [_batch(graphs[:6]), _batch(graphs[6:12]), _batch(graphs[12:])]       # the last batch has 4 graphs
    opt = FlatAdam(model.parameters(), lr=1e-3)
    tau = torch.tensor(0.1, device="cuda")
    losses = [fit_epoch(model, opt, loader, tau) for _ in range(3)]
    assert all(np.isfinite(losses)), losses
    tr = next(iter(opt._igcn_epoch_trainers.values()))
    assert tr.counts["captured"] == 2 and tr.counts["replayed"] > 0
    assert np.isfinite(eval_loss(model, loader, temperature=tau))
    assert 0.0 <= eval_acc(model, loader, tau) <= 1.0
    out = eval_outputs(model, loader, tau)
    assert out["logp"].shape == (16, 3) and out["reg"].shape == (16, 3) and out["linear_outf"].shape == (16, 32)
    with pytest.raises(ValueError, match="GUIDE_IMGSNP"):
        Evaluator(model)
