"""GPU checks of GUIDE_IMGSNP and its kernels (csrc/guide.hip; the LayerNorm form: csrc/nodes_ln.hip):
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


# ---- edge sweeps of the three kernel families against float64 torch ---------------------------------------------------
# Inputs are held off the PReLU kink: an fp32 pre-activation within rounding of 0 may take the other branch, and the
# derivative jumps there (1 -> a).  _off_kink nudges the shift beta of the affected columns / nodes until no fp64
# pre-activation lies within KINK of 0; the gate draws its inputs afresh instead.
KINK = 1e-4
SWEEP_SLOPES = [0.0, 1.0, 0.25, -0.3, 1.7]


def _off_kink(u_of, beta, axis_other):
    for _ in range(20):
        near = u_of(beta).abs() < KINK
        if not bool(near.any()):
            return beta
        beta = beta + 4e-3 * near.any(dim=axis_other).double()
    raise AssertionError("inputs did not leave the PReLU kink")


def _ln_u(y, gamma):
    mu = y.mean(-1, keepdim=True)
    xh = (y - mu) / torch.sqrt(y.var(-1, unbiased=False, keepdim=True) + 1e-5)
    return lambda beta: xh * gamma + beta


# (b, f, N, pool): rows b f = 1 / 64 / 65 / 1280, N around the 64-node tiles and LN_T = 256 threads, the bench's 1200 /
# 3000-node layers (20 chunks of LN_RC = 64 rows), pool 0 and pool = N - 1
LN_SHAPES = [(1, 1, 63, 0), (8, 8, 64, 63), (13, 5, 65, 7), (4, 16, 256, 0), (5, 13, 257, 256), (256, 5, 1200, 800),
             (256, 5, 3000, 1800), (2, 3, 4100, 100), (1, 1, 4100, 4099)]


@pytest.mark.parametrize("a", SWEEP_SLOPES)
@pytest.mark.parametrize("keep_on", [True, False], ids=["keep", "nokeep"])
@pytest.mark.parametrize("b,f,n,pool", LN_SHAPES)
def test_nodes_ln_prelu_sweep_vs_fp64(b, f, n, pool, keep_on, a):
    from igcn_amd import ops
    g = torch.Generator().manual_seed(n + 7 * pool + b)
    y = torch.randn(b, f, n, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma = 1 + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
    beta = _off_kink(_ln_u(y, gamma), 0.2 * torch.randn(n, generator=g, dtype=torch.float64), (0, 1))
    keep = _keep((b, n), 0.4, g) if keep_on else None
    slope = torch.tensor([a], dtype=torch.float64)
    cot = torch.randn(b, f, n - pool, generator=g, dtype=torch.float64)
    ref = [_leaf(t) for t in (y, gamma, beta, slope)]
    mu = ref[0].mean(-1, keepdim=True)
    var = ref[0].var(-1, unbiased=False, keepdim=True)
    z = _prelu((ref[0] - mu) / torch.sqrt(var + 1e-5) * ref[1] + ref[2], ref[3])
    if keep_on:
        z = z * keep.unsqueeze(1)
    z = z[..., pool:]
    (z * cot).sum().backward()
    das = []
    for _ in range(2):
        got = [_leaf(t.float().cuda()) for t in (y, gamma, beta, slope)]
        zg = ops.NodesLayerNormPReLU.apply(*got, keep.float().cuda() if keep_on else None, pool, 1e-5)
        (zg * cot.float().cuda()).sum().backward()
        das.append(got[3].grad.clone())
    assert_matches(zg, z.detach().numpy(), 1e-5, "z")
    for r, t, w in zip(ref, got, ("dy", "dgamma", "dbeta", "dslope")):
        assert_matches(t.grad, r.grad.numpy(), 1e-4, w)
    assert torch.equal(das[0], das[1])


def _bn_case(f, b, c, d, seed, training, off_kink=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, c) if f == 0 else (b, f, c), generator=g, dtype=torch.float64) * 1.5 + 0.3
    w = torch.randn(d, f, generator=g, dtype=torch.float64) if f else None
    if b == 2 and d == 1:
        # two samples: (pre_0 - pre_1) / 2 is the column's standard deviation; hold it >= 1/2, away from the
        # cancellation of two nearly equal numbers (there the fp32 output is ill-conditioned: 1 / |pre_0 - pre_1|)
        pre = x if f == 0 else torch.einsum("of,bfc->bc", w, x)
        delta = pre[0] - pre[1]
        t = torch.where(delta.abs() < 1.0, delta - torch.where(delta >= 0, 1.0, -1.0), torch.zeros_like(delta))
        if f == 0:
            x[1] += t
        else:
            x[1] += t[None, :] * (w[0] / (w[0] ** 2).sum())[:, None]
    bn = torch.nn.BatchNorm1d(c).double()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(c, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(0.3 * torch.randn(c, generator=g, dtype=torch.float64))
        bn.running_var.copy_(0.5 + torch.rand(c, generator=g, dtype=torch.float64))
        pre = x if f == 0 else torch.einsum("df,bfc->bcd", w, x)
        if training:
            m, v = pre.mean((0, -1) if f else 0), pre.var((0, -1) if f else 0, unbiased=False)
        else:
            m, v = bn.running_mean, bn.running_var
        if f:
            xh = (pre - m[:, None]) / torch.sqrt(v[:, None] + 1e-5)
            u_of = lambda beta: xh * bn.weight[:, None] + beta[:, None]      # noqa: E731
            other = (0, 2)
        else:
            xh = (pre - m) / torch.sqrt(v + 1e-5)
            u_of = lambda beta: xh * bn.weight + beta                        # noqa: E731
            other = (0,)
        beta = 0.2 * torch.randn(c, generator=g, dtype=torch.float64)
        bn.bias.copy_(_off_kink(u_of, beta, other) if off_kink else beta)
    return g, x, w, bn


# F = 0 (a column of x), 1, 5 and GD_FMAX = 8 channels of the per-node linear; B = 2 (the smallest batch a training
# BatchNorm takes), 3, and around the GD_T = 256 threads of a column; C = 1, 32, the bench's 400 (B) and 3000 (B_D)
@pytest.mark.parametrize("keep_on", [True, False], ids=["keep", "nokeep"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("c", [1, 32, 400, 3000])
@pytest.mark.parametrize("b", [2, 3, 255, 256, 257, 512])
@pytest.mark.parametrize("f", [0, 1, 5, 8])
def test_bn_prelu_sweep_vs_fp64(f, b, c, training, keep_on):
    """Scale-relative bounds of test_bn_prelu_vs_fp64.  Three quantities are sums whose exact value may cancel far below
    their terms — measured rounding cases, each judged on the scale its terms set (floors, computed in float64):
    dx, whose exact value in a training BatchNorm over B = 2 samples is O(eps) (x hat = +-1 whatever x is), on the largest
    gamma rstd e; d W, which in training is orthogonal to W (the BatchNorm is blind to W's scale: exactly 0 at F = 1, and
    all of it O(eps) at B = 2), on the root-sum-square of its B C summands gamma rstd e x before the batch means cancel
    them; and d slope on the root-sum-square of its summands u dy."""
    from igcn_amd import ops
    a = [0.25, -0.3, 1.7, 0.0][(f + b + c) % 4]
    g, x, w, bn = _bn_case(f, b, c, 1, 11 * f + b + c, training)
    bn.train(training)
    bn_gpu = copy.deepcopy(bn).float().cuda()
    keep = _keep((b, c), 0.5, g) if keep_on else None
    slope = torch.tensor([a], dtype=torch.float64)
    cot = torch.randn(b, c, generator=g, dtype=torch.float64)
    xr, sr = _leaf(x), _leaf(slope)
    wr = _leaf(w) if f else None
    pre = xr if f == 0 else torch.einsum("of,bfc->bc", wr, xr)
    pre.retain_grad()
    u = bn(pre)
    u.retain_grad()
    out = _prelu(u, sr)
    if keep_on:
        out = out * keep
    (out * cot).sum().backward()
    with torch.no_grad():
        up = cot * keep if keep_on else cot
        gre = u.grad * bn.weight / torch.sqrt((bn.running_var if not training else pre.var(0, unbiased=False)) + 1e-5)
        fl_dx = float(gre.abs().max())
        fl_da = float(((u * up)[u <= 0] ** 2).sum().sqrt())
        fl_dw = float(((gre.unsqueeze(1) * x) ** 2).sum((0, 2)).sqrt().max()) if f else 0.0
    das = []
    for _ in range(2):
        bg = copy.deepcopy(bn_gpu)
        xg, sg = _leaf(x.float().cuda()), _leaf(slope.float().cuda())
        wg = _leaf(w.float().cuda()) if f else None
        og = ops.BatchNormPReLU.apply(xg, wg, bg.weight, bg.bias, sg, bg, training,
                                      keep.float().cuda() if keep_on else None)
        (og * cot.float().cuda()).sum().backward()
        das.append(sg.grad.clone())
    assert_matches(og, out.detach().numpy(), 1e-5, "y")
    assert_matches(xg.grad, xr.grad.numpy(), 1e-4, "dx", floor=fl_dx if (training and b == 2) else 0.0)
    assert_matches(sg.grad, sr.grad.numpy(), 1e-4, "dslope", floor=fl_da)
    assert_matches(bg.weight.grad, bn.weight.grad.numpy(), 1e-4, "dgamma")
    assert_matches(bg.bias.grad, bn.bias.grad.numpy(), 1e-4, "dbeta")
    if f:
        assert_matches(wg.grad, wr.grad.numpy(), 1e-4, "dW", floor=fl_dw if training else 0.0)
    assert_matches(bg.running_mean, bn.running_mean.numpy(), 1e-5, "running_mean")
    assert_matches(bg.running_var, bn.running_var.numpy(), 1e-5, "running_var")
    assert torch.equal(das[0], das[1])


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("d", [5, 10, 16, 32])
def test_node_linear_bn_prelu_wide_sweep_vs_fp64(d, training):
    """conc_for_attention's form (D > 1) at the bench's n_top = 400 nodes and B = 256: output and running statistics."""
    from igcn_amd import ops
    g, x, w, bn = _bn_case(5, 256, 400, d, 90 + d, training, off_kink=False)     # (values only: continuous at the kink)
    bn.train(training)
    bn_gpu = copy.deepcopy(bn).float().cuda()
    with torch.no_grad():
        out = _prelu(bn(torch.einsum("df,bfc->bcd", w, x)), 0.35)
    y, _, _ = ops.bn_prelu_forward(x.float().cuda(), w.float().cuda(), bn_gpu, torch.tensor([0.35], device="cuda"),
                                   training)
    assert_matches(y, out.numpy(), 1e-5, "y")
    assert_matches(bn_gpu.running_mean, bn.running_mean.numpy(), 1e-5, "running_mean")
    assert_matches(bn_gpu.running_var, bn.running_var.numpy(), 1e-5, "running_var")


def test_bn_prelu_refusals_launch_nothing():
    """F = 9 > GD_FMAX, keep with D > 1 and a training call with B D = 1 raise, and nothing is written."""
    from igcn_amd import _lib, ops
    from igcn_amd._lib import IgcnError

    def fwd(b, c, f, d, keep, training):
        x = torch.randn((b, c) if f == 0 else (b, f, c), device="cuda")
        w = torch.randn(d, f, device="cuda") if f else None
        bn = torch.nn.BatchNorm1d(c).cuda()
        y = torch.full((b, c, d), float("nan"), device="cuda")
        mean, rstd = torch.full((c,), 7.0, device="cuda"), torch.full((c,), 7.0, device="cuda")
        k = torch.ones(b, c, device="cuda") if keep else None
        with pytest.raises(IgcnError, match="bn_prelu_fwd"):
            _lib.call("igcn_bn_prelu_fwd", b, c, f, d, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bn.weight), _lib.ptr(bn.bias),
                      _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), int(training), 0.1, 1e-5, _lib.ptr(k),
                      _lib.ptr(torch.tensor([0.25], device="cuda")), _lib.ptr(y), _lib.ptr(mean), _lib.ptr(rstd),
                      _lib.stream_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all()) and bool((mean == 7).all()) and bool((rstd == 7).all())
        assert bool((bn.running_mean == 0).all()) and bool((bn.running_var == 1).all())

    fwd(8, 16, 9, 1, False, True)          # F = 9
    fwd(8, 16, 5, 4, True, True)           # keep with D > 1
    fwd(1, 16, 0, 1, False, True)          # training, B D = 1
    fwd(1, 16, 5, 1, False, True)
    # the backward refuses F = 9 too, before anything is written
    b, c, f = 8, 16, 9
    x, w = torch.randn(b, f, c, device="cuda"), torch.randn(1, f, device="cuda")
    ones = torch.ones(c, device="cuda")
    dx, dw = torch.full_like(x, float("nan")), torch.full_like(w, float("nan"))
    dg, db, da = torch.full_like(ones, float("nan")), torch.full_like(ones, float("nan")), torch.full((1,), float("nan"), device="cuda")
    scratch = torch.full((c * (f + 1) + 64,), float("nan"), device="cuda")
    with pytest.raises(IgcnError, match="bn_prelu_bwd"):
        _lib.call("igcn_bn_prelu_bwd", b, c, f, 1, _lib.ptr(x), _lib.ptr(w), _lib.ptr(ones), _lib.ptr(ones),
                  _lib.ptr(torch.tensor([0.25], device="cuda")), _lib.ptr(ones), _lib.ptr(ones),
                  _lib.ptr(torch.ones(b, c, device="cuda")), None, _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(dg),
                  _lib.ptr(db), _lib.ptr(da), _lib.ptr(scratch), _lib.stream_ptr())
    torch.cuda.synchronize()
    for t in (dx, dw, dg, db, da, scratch):
        assert bool(torch.isnan(t).all())
    # and the autograd entry points
    bn = torch.nn.BatchNorm1d(16).cuda()
    with pytest.raises(IgcnError):
        ops.BatchNormPReLU.apply(torch.randn(8, 9, 16, device="cuda"), torch.randn(1, 9, device="cuda"), bn.weight,
                                 bn.bias, torch.tensor([0.25], device="cuda"), bn, True, None)
    with pytest.raises(IgcnError):
        ops.bn_prelu_forward(torch.randn(8, 5, 16, device="cuda"), torch.randn(4, 5, device="cuda"), bn,
                             torch.tensor([0.25], device="cuda"), True, torch.ones(8, 16, device="cuda"))
    with pytest.raises(IgcnError):
        ops.BatchNormPReLU.apply(torch.randn(1, 16, device="cuda"), None, bn.weight, bn.bias,
                                 torch.tensor([0.25], device="cuda"), bn, True, None)
    torch.cuda.synchronize()
    assert bool((bn.running_mean == 0).all()) and bool((bn.running_var == 1).all())


def _gate_case(b, k, h, l, training, seed, tau):
    """Gate inputs whose fp64 hidden pre-activations all lie off the PReLU kink (by 1e-5 of the largest), and noise
    whose hard decisions sit 1e-3 (tempered-logit units) off a tie, as tests/golden/make_golden_guide.py moves them."""
    for s in range(seed, seed + 20):
        g = torch.Generator().manual_seed(s)
        img = torch.randn(b, k, generator=g, dtype=torch.float64)
        bias = 0.1 * (2 * torch.rand(k, 2, generator=g, dtype=torch.float64) - 1)
        w1 = torch.randn(h, k, generator=g, dtype=torch.float64) / k ** 0.5
        w2 = torch.randn(l, h, generator=g, dtype=torch.float64) / h ** 0.5
        keep = _keep((b, h), 0.4, g)
        noise = torch.from_numpy(guide_ref.gumbel_noise(s, b, k)).double()
        logit = torch.log(torch.softmax(bias, 1))
        wt = (logit.unsqueeze(0) + noise) / tau
        noise[..., 1] += torch.where((wt[..., 1] - wt[..., 0]).abs() < 1e-3, 0.05, 0.0)
        _, z1 = guide_ref.soft_sample(bias, noise, tau)
        pre = (img * z1 if training else img) @ w1.t()
        if not bool(((pre.abs() <= 1e-5 * pre.abs().max()) & (pre != 0)).any()):      # (exact zeros agree)
            return img, bias, w1, w2, keep, noise
    raise AssertionError("no gate inputs off the PReLU kink")


# K = 1 .. GG_KMAX = 1024 (the LDS row xin[K] full), K < GD_T = 256 and the model's 270; H, L = 1, 32 and their limit 64;
# B = 1, 8 and 256 workgroups.  Each shape runs in training and eval and in four variants: dropout keep on / off, tau as
# a device scalar / a number, a cotangent on imp1 (the sparsity term's path into bias_n through the b == 0 block) or not.
GATE_SHAPES = [(k, h, l, (1, 8, 256)[(i + j + m) % 3]) for i, k in enumerate((1, 64, 255, 270, 1024))
               for j, h in enumerate((1, 32, 64)) for m, l in enumerate((1, 32, 64))]
GATE_VARIANTS = {"keep-dev-imp": (True, True, True), "nokeep-num-imp": (False, False, True),
                 "keep-num-noimp": (True, False, False), "nokeep-dev-noimp": (False, True, False)}


@pytest.mark.parametrize("variant", list(GATE_VARIANTS))
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("k,h,l,b", GATE_SHAPES)
def test_gate_encoder_sweep_vs_fp64(k, h, l, b, training, variant):
    from igcn_amd import ops
    keep_on, tau_dev, imp_cot = GATE_VARIANTS[variant]
    tau = 0.1
    img, bias, w1, w2, keep, noise = _gate_case(b, k, h, l, training, 1000 * k + 10 * h + l + b, tau)
    keep = keep if keep_on else None
    a = torch.tensor([[-0.3, 0.25, 0.0, 1.0, 1.7][(k + h + l) % 5]], dtype=torch.float64)
    ref = [_leaf(t) for t in (img, bias, w1, a, w2)]
    lat, imp1 = guide_ref.gate_encoder(*ref[:3], ref[3], ref[4], keep, tau, noise, training)
    g = torch.Generator().manual_seed(9)
    c1, c2 = torch.randn(lat.shape, generator=g, dtype=torch.float64), torch.randn(imp1.shape, generator=g, dtype=torch.float64)
    obj = (lat * c1).sum() + ((imp1 * c2).sum() if imp_cot else 0.0)
    obj.backward()
    grads = []
    for _ in range(2):
        got = [_leaf(t.float().cuda()) for t in (img, bias, w1, a, w2)]
        tau_arg = torch.tensor(tau, device="cuda") if tau_dev else tau
        lg, ig, gate = ops.GuideGate.apply(*got, keep.float().cuda() if keep_on else None, tau_arg, training,
                                           noise.float().cuda(), None)
        og = (lg * c1.float().cuda()).sum() + ((ig * c2.float().cuda()).sum() if imp_cot else 0.0)
        og.backward()
        grads.append(got[3].grad.clone())
    assert_matches(lg, lat.detach().numpy(), 1e-4, "latent_n")
    assert_matches(ig, imp1.detach().numpy(), 1e-5, "imp1")
    # d bias_n from the gate alone is sum_b s0 s1 img d img / tau, and d img = W1^T dpre an H-term sum that may cancel:
    # with one summand (B = K = 1) scale-relative turns self-relative.  A measured rounding case: d bias_n is judged on
    # the scale of those sums' terms, sum_b s0 s1 |img| sum_j |W1[j, k] dpre[b, j]| / tau (float64)
    fl_b = 0.0
    if training and not imp_cot:
        with torch.no_grad():
            s, z1 = guide_ref.soft_sample(bias, noise, tau)
            pre = (img * z1) @ w1.t()
            up = (c1 @ w2) * (keep if keep_on else 1.0)
            dpre = torch.where(pre > 0, up, a * up)
            fl_b = float((s[..., 0] * s[..., 1] * img.abs() * (dpre.abs() @ w1.abs())).sum(0).max() / tau)
    for r, t, w in zip(ref, got, ("d img", "d bias_n", "dW1", "d slope", "dW2")):
        if r.grad is None:                    # (bias_n in eval with no cotangent on imp1: nothing reaches it)
            assert not bool(t.grad.abs().max() > 0), w
            continue
        assert_matches(t.grad, r.grad.numpy(), 1e-3, w, floor=fl_b if w == "d bias_n" else 0.0)
    assert torch.equal(grads[0], grads[1])
    if training:
        _, z1 = guide_ref.soft_sample(bias, noise, tau)
        assert torch.equal(gate[..., 0].cpu() > 0.5, z1 > 0.5)
    else:
        assert gate is None


def test_gate_generator_contract_b256_k1024():
    """256 workgroups race to advance the counter: one training launch advances it by exactly one, and its draws at
    K = GG_KMAX = 1024 equal the host rebuild."""
    from igcn_amd import ops
    b, k = 256, 1024
    img, bias, w1, w2, _, _ = _gate_case(b, k, 64, 64, False, 17, 0.1)
    args = [t.float().cuda() for t in (img, bias, w1)] + [torch.tensor([0.25], device="cuda"), w2.float().cuda()]
    state = ops.DropoutState("cuda")
    c0 = int(state.state[0].item())
    for step in range(3):
        _, _, gate = ops.GuideGate.apply(*args, None, torch.tensor(0.1, device="cuda"), True, None, state)
        torch.cuda.synchronize()
        assert int(state.state[0].item()) == c0 + step + 1 and int(state.state[1].item()) == 0
        s, z1 = guide_ref.soft_sample(bias, torch.from_numpy(guide_ref.gumbel_noise(c0 + step, b, k)).double(), 0.1)
        far = (s[..., 1] - s[..., 0]).abs() > 1e-6
        got = (gate[..., 0] > 0.5).cpu()
        assert bool(far.float().mean() > 0.99)
        assert torch.equal(got[far], (z1 > 0.5)[far]), "kernel draws differ from the host rebuild"
        # the soft part of the gate is the draw's too: s0 s1 of the rebuild
        prod = (s[..., 0] * s[..., 1]).float()
        assert_matches(gate[..., 1], prod.numpy(), 1e-4, "s0 s1")
