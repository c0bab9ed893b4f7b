"""GPU checks of SGCN_Ori (kernel/sgcn.py:11-151) and of its LDS-resident graph stack (igcn_sgcn_ori_*):
  * the two kernels against the float64 restatement (tests/sgcn_ori_ref.py), the Grad-CAM tap bit for bit, determinism;
  * the fused and the per-layer route through the model against float64;
  * the model against the fixture captured from the reference (tests/golden/sgcn_ori.npz), the train step included;
  * forward_pair against two calls, the captured step against eager steps, fit_epoch, dropout, and the refusals."""
import copy

import numpy as np
import pytest
import torch

from conftest import assert_matches, golden_group
from _weights import seeded_state

import sgcn_ori_ref as REF

pytestmark = pytest.mark.gpu

TOL = 1e-4                                  # the bound tests/test_gpu_ops.py holds igcn_sgcn_stack_* to
TAGS = ["h32_5", "h16_8"]
WIDTHS = [(3, 32, 5), (1, 4, 4), (8, 16, 32), (3, 5, 10)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _probe(outs, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal(tuple(o.shape))).float() for o in outs]


# ---- the stack kernels -------------------------------------------------------------------------------------------------
def _hand_graphs(h0, rng):
    """Three graphs of 7 nodes: (a) no stored loop at all, node 6 isolated, one duplicated edge; (b) two stored loops at
    node 2 (the last one counts), one at node 4, a duplicated edge, node 0 without incoming edges; (c) a ring with a
    loop on every node."""
    from igcn_amd.data import Data
    lists = [
        [(0, 1), (1, 0), (1, 2), (2, 3), (3, 1), (4, 5), (5, 4), (1, 2), (3, 5), (0, 4)],
        [(2, 2), (0, 1), (1, 3), (2, 2), (3, 4), (4, 4), (5, 6), (6, 5), (1, 3), (0, 2), (6, 1), (4, 2)],
        [(i, (i + 1) % 7) for i in range(7)] + [(i, i) for i in range(7)],
    ]
    out = []
    for edges in lists:
        ei = torch.tensor(edges, dtype=torch.long).t().contiguous()
        out.append(Data(x=torch.from_numpy(rng.random((7, h0))).float(), edge_index=ei,
                        edge_attr=torch.from_numpy(rng.random(ei.shape[1]) + 0.05).float()))
    return out


def _graph_set(kind, h0, seed):
    from igcn_amd import synth
    rng = np.random.default_rng(seed)
    if kind == "r7":
        return _hand_graphs(h0, rng), 7
    n = {"r90x1": 1, "r90x3": 3}[kind]
    return synth.brain_graph_list(n, seed=seed, rois=90, h0=h0, top_k=3, tsne_dim=4), 90


def _overwritten_loops(edge_index):
    """Stored self-loops that a later stored loop of the same node replaces (PyG keeps the last): their weight reaches
    nothing, d(loss)/d(weight) is 0 — the float64 restatement's index_put hands them the survivor's gradient instead."""
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    last, over = {}, torch.zeros(len(src), dtype=torch.bool)
    for k, (s, d) in enumerate(zip(src, dst)):
        if s == d:
            if s in last:
                over[last[s]] = True
            last[s] = k
    return over


_STACK_CACHE = {}


def _stack_case(widths, kind):
    """One launch pair per (widths, graph set), shared by the tests that read it; the float64 reference beside it."""
    key = (widths, kind)
    if key in _STACK_CACHE:
        return _STACK_CACHE[key]
    from igcn_amd import ops
    from igcn_amd.data import Batch
    h0, f1, f3 = widths
    graphs, rois = _graph_set(kind, h0, seed=11 * f1 + f3 + h0)
    batch = Batch.from_data_list(graphs).to("cuda")
    plan = ops.plan_for(batch)
    plan.check()
    assert ops.sgcn_ori_supported(plan, rois, h0, f1, f3)
    rng = np.random.default_rng(f1 * 100 + f3)
    w1 = torch.from_numpy(rng.standard_normal((f1, h0)) / np.sqrt(h0)).float()
    w3 = torch.from_numpy(rng.standard_normal((f3, f1)) / np.sqrt(f1)).float()
    b1 = torch.from_numpy(0.3 * rng.standard_normal(f1)).float()
    b3 = torch.from_numpy(0.3 * rng.standard_normal(f3)).float()
    g = len(graphs)
    cot = torch.from_numpy(rng.standard_normal((g, rois * (f1 + f3)))).float()
    # float64
    xd = batch.x.cpu().double().requires_grad_(True)
    ewd = batch.edge_attr.cpu().double().requires_grad_(True)
    pd = [t.double().requires_grad_(True) for t in (w1, b1, w3, b3)]
    zd, actsd, _ = REF.stack(xd, batch.edge_index.cpu(), ewd, *pd, rois)
    actsd.retain_grad()
    (zd * cot.double()).sum().backward()
    # HIP
    xg = batch.x.clone().requires_grad_(True)
    ewg = batch.edge_attr.clone().requires_grad_(True)
    pg = [t.cuda().requires_grad_(True) for t in (w1, b1, w3, b3)]
    tap = ops.TapGrads()
    z, acts = ops.SgcnOriStack.apply(xg, ewg, plan, rois, tap, *pg)
    (z * cot.cuda()).sum().backward()
    plan.check()
    case = dict(rois=rois, g=g, batch=batch, plan=plan, cot=cot, z=z.detach(), acts=acts.detach(), tap=tap, xg=xg, ewg=ewg,
                pg=pg, zd=zd.detach(), actsd=actsd, xd=xd, ewd=ewd, pd=pd)
    _STACK_CACHE[key] = case
    return case


@pytest.mark.parametrize("kind", ["r90x1", "r90x3", "r7"])
@pytest.mark.parametrize("widths", WIDTHS)
def test_stack_kernels_vs_fp64(widths, kind):
    """igcn_sgcn_ori_fwd / _bwd against the float64 restatement: z, acts, dx, d(edge weight), dW1, db1, dW3, db3 and the
    gradient at the tap, all at the bound of test_fused_sgcn_stack_fwd_bwd."""
    c = _stack_case(widths, kind)
    assert_matches(c["z"], c["zd"].numpy(), TOL, "z")
    assert_matches(c["acts"], c["actsd"].detach().numpy(), TOL, "acts")
    assert_matches(c["xg"].grad, c["xd"].grad.numpy(), TOL, "dx")
    over = _overwritten_loops(c["batch"].edge_index.cpu())
    want_dew = c["ewd"].grad.clone()
    want_dew[over] = 0.0
    assert kind != "r7" or int(over.sum()) == 1
    assert_matches(c["ewg"].grad, want_dew.numpy(), TOL, "dew")
    assert bool((c["ewg"].grad.cpu()[over] == 0.0).all())
    for name, got, want in zip(("dW1", "db1", "dW3", "db3"), c["pg"], c["pd"]):
        assert_matches(got.grad, want.grad.numpy(), TOL, name, floor=1e-6)
    assert_matches(c["tap"].grads, c["actsd"].grad.numpy(), TOL, "dacts")
    frac = float((c["actsd"] < 0).double().mean())
    assert 0.02 < frac < 0.98, f"the tap of this case has one sign only ({frac})"


@pytest.mark.parametrize("kind", ["r90x3", "r7"])
@pytest.mark.parametrize("widths", WIDTHS)
def test_tap_is_exact(widths, kind):
    """dacts == dz's h3 block where acts > 0 and 0.0 elsewhere; z's h3 block == max(acts, 0): exact, not to a bound."""
    c = _stack_case(widths, kind)
    h0, f1, f3 = widths
    rois, g = c["rois"], c["g"]
    acts = c["acts"]
    dz_h3 = c["cot"].cuda()[:, rois * f1:].reshape(g * rois, f3)
    want = torch.where(acts > 0, dz_h3, torch.zeros_like(dz_h3))
    assert torch.equal(c["tap"].grads, want)
    assert bool((c["tap"].grads[acts <= 0] == 0.0).all())
    assert torch.equal(c["z"][:, rois * f1:].reshape(g * rois, f3), torch.clamp(acts, min=0.0))
    assert int((acts > 0).sum()) > 0 and int((acts < 0).sum()) > 0


def test_gradient_on_acts_joins_at_the_tap():
    """A loss that reads final_conv_acts itself: its gradient is added at the tap (and is part of what the tap reports)."""
    from igcn_amd import ops
    c = _stack_case((3, 5, 10), "r7")
    rois, g = c["rois"], c["g"]
    rng = np.random.default_rng(5)
    cot_a = torch.from_numpy(rng.standard_normal(tuple(c["acts"].shape))).float()
    xd = c["xd"].detach().clone().requires_grad_(True)
    ewd = c["ewd"].detach().clone().requires_grad_(True)
    pd = [t.detach().clone().requires_grad_(True) for t in c["pd"]]
    zd, actsd, _ = REF.stack(xd, c["batch"].edge_index.cpu(), ewd, *pd, rois)
    actsd.retain_grad()
    ((zd * c["cot"].double()).sum() + (actsd * cot_a.double()).sum()).backward()
    xg = c["batch"].x.clone().requires_grad_(True)
    pg = [t.detach().clone().requires_grad_(True) for t in c["pg"]]
    tap = ops.TapGrads()
    z, acts = ops.SgcnOriStack.apply(xg, c["batch"].edge_attr.clone(), c["plan"], rois, tap, *pg)
    ((z * c["cot"].cuda()).sum() + (acts * cot_a.cuda()).sum()).backward()
    assert_matches(xg.grad, xd.grad.numpy(), TOL, "dx")
    assert_matches(tap.grads, actsd.grad.numpy(), TOL, "dacts")
    for name, got, want in zip(("dW1", "db1", "dW3", "db3"), pg, pd):
        assert_matches(got.grad, want.grad.numpy(), TOL, name, floor=1e-6)
    # and acts alone (no gradient on z at all)
    xg2 = c["batch"].x.clone().requires_grad_(True)
    _, acts2 = ops.SgcnOriStack.apply(xg2, c["batch"].edge_attr.clone(), c["plan"], rois, None, *c["pg"])
    (acts2 * cot_a.cuda()).sum().backward()
    xd2 = c["xd"].detach().clone().requires_grad_(True)
    _, actsd2, _ = REF.stack(xd2, c["batch"].edge_index.cpu(), c["ewd"].detach(), *[t.detach() for t in c["pd"]], rois)
    (actsd2 * cot_a.double()).sum().backward()
    assert_matches(xg2.grad, xd2.grad.numpy(), TOL, "dx (acts only)")


def _raw_launches(c, widths, with_dacts=True):
    """One forward and one backward launch through the C ABI on fresh output buffers -> every output tensor."""
    from igcn_amd import _lib
    from igcn_amd._lib import call, ptr, stream_ptr
    h0, f1, f3 = widths
    rois, g, plan, batch = c["rois"], c["g"], c["plan"], c["batch"]
    n, e = batch.x.shape[0], batch.edge_attr.shape[0]
    f = dict(dtype=torch.float32, device="cuda")
    x, ew = batch.x.contiguous(), batch.edge_attr.contiguous()
    w1, b1, w3, b3 = [t.detach() for t in c["pg"]]
    # buffers start as NaN: an element the kernels do not write shows
    z, acts = torch.full((g, rois * (f1 + f3)), float("nan"), **f), torch.full((n, f3), float("nan"), **f)
    emax = plan._stack_dims[1]
    call("igcn_sgcn_ori_fwd", g, rois, emax, h0, f1, f3, ptr(x), ptr(ew), ptr(plan.src32), ptr(plan.dst32),
         ptr(plan.tgt_ptr), ptr(plan.tgt_perm), ptr(plan.loop_edge), ptr(w1), ptr(b1), ptr(w3), ptr(b3), ptr(z), ptr(acts),
         ptr(plan.status), stream_ptr())
    npar = int(_lib.load().igcn_sgcn_ori_param_floats(h0, f1, f3))
    dz = c["cot"].cuda().contiguous()
    dacts = torch.full((n, f3), float("nan"), **f) if with_dacts else None
    dx, dew = torch.full((n, h0), float("nan"), **f), torch.full((e,), float("nan"), **f)
    dpar, scratch = torch.full((npar,), float("nan"), **f), torch.full((g * npar,), float("nan"), **f)
    call("igcn_sgcn_ori_bwd", g, rois, emax, h0, f1, f3, ptr(x), ptr(ew), ptr(plan.src32), ptr(plan.dst32),
         ptr(plan.tgt_ptr), ptr(plan.tgt_perm), ptr(plan.src_ptr), ptr(plan.src_perm), ptr(plan.loop_edge), ptr(w1), ptr(b1),
         ptr(w3), ptr(b3), ptr(dz), None, ptr(dacts), ptr(dx), ptr(dew), ptr(dpar), ptr(scratch), ptr(plan.status),
         stream_ptr())
    torch.cuda.synchronize()
    return dict(z=z, acts=acts, dacts=dacts, dx=dx, dew=dew, dpar=dpar, scratch=scratch)


@pytest.mark.parametrize("widths,kind", [((3, 32, 5), "r90x3"), ((3, 5, 10), "r7"), ((8, 16, 32), "r90x1")])
def test_launches_are_deterministic_and_write_everything(widths, kind):
    """Two identical launch pairs give identical bytes; dacts = NULL changes no other output; no output element is left
    unwritten (the buffers start as NaN)."""
    c = _stack_case(widths, kind)
    a, b = _raw_launches(c, widths), _raw_launches(c, widths)
    nod = _raw_launches(c, widths, with_dacts=False)
    for k, t in a.items():
        assert not bool(torch.isnan(t).any()), f"{k}: unwritten elements"
        assert torch.equal(t.view(torch.int32), b[k].view(torch.int32)), k
        if k != "dacts":
            assert torch.equal(t.view(torch.int32), nod[k].view(torch.int32)), k + " (dacts = NULL)"
    assert torch.equal(a["z"], c["z"]) and torch.equal(a["dacts"], c["tap"].grads)


@pytest.mark.parametrize("kind", ["r7", "r90x3"])
@pytest.mark.parametrize("f1", [4, 8, 16, 32])
def test_first_layer_equals_the_uniform_stack_bit_for_bit(f1, kind):
    """Both stacks run gcn_norm and the by-target walk of csrc/gcn_lds.h and the same first transform, one workgroup per
    graph, sums in list order: the h1 block of SgcnOriStack's z IS SgcnStack's output with L = 1, F = F1 on the same x,
    edge weights, W1, b1 — equal bits, not a bound (measured equal on the commit that still had the two copies)."""
    from igcn_amd import ops
    from igcn_amd.data import Batch
    h0, f3 = 3, 5
    graphs, rois = _graph_set(kind, h0, seed=40 + f1)
    batch = Batch.from_data_list(graphs).to("cuda")
    plan = ops.plan_for(batch)
    plan.check()
    assert ops.sgcn_ori_supported(plan, rois, h0, f1, f3) and ops.sgcn_stack_supported(plan, rois, h0, f1, 1)
    rng = np.random.default_rng(f1)
    w1 = torch.from_numpy(rng.standard_normal((f1, h0)) / np.sqrt(h0)).float().cuda()
    b1 = torch.from_numpy(0.3 * rng.standard_normal(f1)).float().cuda()
    w3 = torch.from_numpy(rng.standard_normal((f3, f1)) / np.sqrt(f1)).float().cuda()
    b3 = torch.from_numpy(0.3 * rng.standard_normal(f3)).float().cuda()
    with torch.no_grad():
        z, _ = ops.SgcnOriStack.apply(batch.x, batch.edge_attr, plan, rois, None, w1, b1, w3, b3)
        y = ops.SgcnStack.apply(batch.x, batch.edge_attr, plan, rois, w1, b1)
    plan.check()
    h1 = z[:, :rois * f1].reshape(len(graphs) * rois, f1)
    assert y.shape == h1.shape and int((h1 > 0).sum()) > 0 and int((h1 == 0).sum()) > 0
    assert torch.equal(h1, y)


def test_too_many_edges_sets_status_bit_1():
    from igcn_amd._lib import call, ptr, stream_ptr
    c = _stack_case((3, 5, 10), "r7")
    plan, batch = c["plan"], c["batch"]
    w1, b1, w3, b3 = [t.detach() for t in c["pg"]]
    z = torch.full((3, 7 * 15), 7.0, device="cuda")
    acts = torch.full((21, 10), 7.0, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    call("igcn_sgcn_ori_fwd", 3, 7, 11, 3, 5, 10, ptr(batch.x), ptr(batch.edge_attr), ptr(plan.src32), ptr(plan.dst32),
         ptr(plan.tgt_ptr), ptr(plan.tgt_perm), ptr(plan.loop_edge), ptr(w1), ptr(b1), ptr(w3), ptr(b3), ptr(z), ptr(acts),
         ptr(status), stream_ptr())
    assert int(status.item()) == 2
    # graph 0 (10 edges) is computed, graphs 1 and 2 (12 and 14 edges) are refused and left as they were
    assert torch.equal(z[0], c["z"][0]) and bool((z[1:] == 7.0).all()) and bool((acts[7:] == 7.0).all())


# ---- the model ---------------------------------------------------------------------------------------------------------
def _cfg(store, tag):
    rois, h0, h1, h2, h3, b_eval, b_train, seed, top_k = [int(v) for v in store[f"{tag}/cfg"]]
    return rois, (h0, h1, h2, h3), b_eval, b_train, seed, top_k


def _model(store, tag, bsz=None, train=False):
    from igcn_amd import synth
    from igcn_amd.sgcn import SGCN_Ori
    rois, dims, b_eval, b_train, seed, top_k = _cfg(store, tag)
    model = SGCN_Ori(*dims, rois=rois).cuda()
    assert sorted(model.state_dict().keys()) == sorted(store[f"{tag}/state_keys"].tolist())
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, seed, model.state_dict())
    model.load_state_dict(sd)                                      # reference-keyed state, strict
    model._dropout_enabled = False
    model.train(train)
    bsz = bsz or (b_train if train else b_eval)
    graphs = synth.brain_graph_list(bsz, seed=seed + 10, rois=rois, top_k=top_k, tsne_dim=16, num_classes=2)
    return model, graphs, seed


def _batch(graphs):
    from igcn_amd.data import Batch
    return Batch.from_data_list(graphs).to("cuda")


def _names(monkeypatch, fn):
    from calltrace import record_calls
    with monkeypatch.context() as mp:
        seen = record_calls(mp)
        out = fn()
    return out, [c[0] for c in seen]


@pytest.mark.parametrize("route", ["fused", "per_layer"])
@pytest.mark.parametrize("explain", [False, True])
def test_both_routes_vs_fp64_in_eval_mode(monkeypatch, golden, route, explain):
    """Each route against the float64 restatement (logp 1e-4, gradients 1e-3, the tap and its gradient alike), and each
    launches what it says: one igcn_sgcn_ori_* pair, or gcn_norm once + two propagations."""
    store = golden("sgcn_ori")
    if route == "per_layer":
        monkeypatch.setenv("IGCN_NO_FUSED_SGCN", "1")
    model, graphs, seed = _model(store, "h32_5", bsz=6)
    data = _batch(graphs)
    out, fwd_names = _names(monkeypatch, lambda: model(data, explain))
    cot = _probe([out], 4)[0]
    _, bwd_names = _names(monkeypatch, lambda: (out * cot.cuda()).sum().backward())
    if route == "fused":
        assert fwd_names.count("igcn_sgcn_ori_fwd") == 1 and bwd_names.count("igcn_sgcn_ori_bwd") == 1
        assert not any(n.startswith("igcn_gcn_") for n in fwd_names + bwd_names)
    else:
        assert fwd_names.count("igcn_gcn_norm_fwd") == 1 and fwd_names.count("igcn_gcn_propagate_fwd") == 2
        assert not any(n.startswith("igcn_sgcn_ori") for n in fwd_names + bwd_names)
    assert not any(n.startswith("igcn_sgcn_stack") for n in fwd_names + bwd_names)
    from igcn_amd.data import Batch
    sd = {k: (v.detach().cpu().double().requires_grad_(True) if v.dtype.is_floating_point and "running_" not in k
              else v.detach().cpu()) for k, v in model.state_dict(keep_vars=True).items()}
    dcpu = Batch.from_data_list(graphs)
    dcpu.x = dcpu.x.double().requires_grad_(True)
    dcpu.edge_attr = dcpu.edge_attr.double()
    taps = {}
    ref = REF.model_forward(sd, 90, dcpu, explain, training=False, taps=taps)
    (ref * cot.double()).sum().backward()
    assert_matches(out, ref.detach().numpy(), 1e-4, "logp")
    assert_matches(model.final_conv_acts, taps["acts"].detach().numpy(), 1e-4, "final_conv_acts")
    assert_matches(model.final_conv_grads, taps["acts"].grad.numpy(), 1e-3, "final_conv_grads")
    assert_matches(data.x.grad, dcpu.x.grad.numpy(), 1e-3, "grad data.x")
    for k, p in model.named_parameters():
        w = sd[k].grad
        if w is None:
            assert p.grad is None or not bool(p.grad.abs().max() > 0), k
            continue
        assert_matches(p.grad, w.numpy(), 1e-3, "grad " + k, floor=1e-4)


def test_train_mode_with_dropout_vs_fp64_under_the_recorded_factors(monkeypatch, golden):
    """TRAINING mode with dropout ON at B = 6, masked pass: the two ``keep`` tensors ``_bn`` hands ops.BatchNorm1dGrouped
    (ReLU flag 0) are recorded at the op's ``apply`` — Dropout(0.5) behind bn1, Dropout(0.7) behind bn2: their non-zero
    value is 1 / (1 - p) of the right p — and the float64 restatement multiplies by them at the same two places: logp at
    1e-4, every gradient at 1e-3 (the bounds of the eval-mode check above)."""
    from igcn_amd import ops
    from igcn_amd.data import Batch
    store = golden("sgcn_ori")
    model, graphs, seed = _model(store, "h32_5", bsz=6, train=True)
    model._dropout_enabled = True
    torch.manual_seed(seed)
    data = _batch(graphs)
    keeps = []
    real = ops.BatchNorm1dGrouped.apply

    def spy(*a):
        assert a[8] == 0 and a[10] is not None                    # ReLU flag 0, factors present
        keeps.append(a[10].detach().cpu())
        return real(*a)
    sd = {k: (v.detach().cpu().double().requires_grad_(True) if v.dtype.is_floating_point and "running_" not in k
              else v.detach().cpu().clone()) for k, v in model.state_dict(keep_vars=True).items()}
    with monkeypatch.context() as mp:
        mp.setattr(ops.BatchNorm1dGrouped, "apply", spy)
        out = model(data, True)
    cot = _probe([out], 4)[0]
    (out * cot.cuda()).sum().backward()
    assert [tuple(k.shape) for k in keeps] == [(6, 64), (6, 16)]
    for k, p in zip(keeps, (0.5, 0.7)):
        vals = np.unique(k.numpy())
        assert len(vals) == 2 and vals[0] == 0.0 and abs(float(vals[1]) - 1.0 / (1.0 - p)) <= 1e-6 / (1.0 - p), (p, vals)
    dcpu = Batch.from_data_list(graphs)
    dcpu.x = dcpu.x.double().requires_grad_(True)
    dcpu.edge_attr = dcpu.edge_attr.double()
    taps = {}
    ref = REF.model_forward(sd, 90, dcpu, True, training=True, taps=taps, keeps=keeps)
    (ref * cot.double()).sum().backward()
    assert_matches(out, ref.detach().numpy(), 1e-4, "logp")
    assert_matches(model.final_conv_grads, taps["acts"].grad.numpy(), 1e-3, "final_conv_grads")
    assert_matches(data.x.grad, dcpu.x.grad.numpy(), 1e-3, "grad data.x")
    for k, p in model.named_parameters():
        w = sd[k].grad
        if w is None:
            assert p.grad is None or not bool(p.grad.abs().max() > 0), k
            continue
        assert_matches(p.grad, w.numpy(), 1e-3, "grad " + k, floor=1e-4)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("explain", [False, True])
def test_sgcn_ori_vs_reference_golden(golden, tag, mode, explain):
    """Outputs 1e-4, gradients 1e-3, scale-relative."""
    store = golden("sgcn_ori")
    model, graphs, seed = _model(store, tag, train=(mode == "train"))
    data = _batch(graphs)
    out = model(data, explain)
    assert model.input is data.x and data.x.requires_grad and model.final_conv_grads is None
    sub = f"{tag}/{mode}/explain{int(explain)}"
    assert_matches(out, golden_group(store, sub + "/out")["logp"], 1e-4, "logp")
    (out * _probe([out], seed + 3)[0].cuda()).sum().backward()
    cam = golden_group(store, sub + "/cam")
    assert_matches(model.final_conv_acts, cam["final_conv_acts"], 1e-4, "final_conv_acts")
    assert_matches(model.final_conv_grads, cam["final_conv_grads"], 1e-3, "final_conv_grads")
    assert model.final_conv_grads.shape == model.final_conv_acts.shape
    assert bool((model.final_conv_grads[model.final_conv_acts <= 0] == 0.0).all())
    wg = golden_group(store, sub + "/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), 1e-3, "grad data.x")
    params = dict(model.named_parameters())
    assert ("prob_bias" in wg) == explain
    for k, w in wg.items():
        assert params[k].grad is not None, k
        assert_matches(params[k].grad, w, 1e-3, "grad " + k, floor=1e-4)
    assert params["conv2.bias"].grad is None and params["edge_prob"].grad is None
    assert int(model.bn1.num_batches_tracked) == int(model.bn2.num_batches_tracked) == (1 if mode == "train" else 0)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("batched", [True, False])
def test_sgcn_ori_train_step_vs_reference_golden(golden, tag, batched):
    """train() of kernel/train_eval_sgcn.py:303-308 at the bounds of test_sgcn_gat_train_step_vs_reference_golden, plus the
    BatchNorm buffers (1e-4 of max(scale, 1e-2): they are means of outputs) and the Grad-CAM attributes the step leaves."""
    from igcn_amd.train import FlatAdam, losses
    store = golden("sgcn_ori")
    model, graphs, _ = _model(store, tag, train=True)
    model.batched_passes = batched
    data = _batch(graphs)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss, terms, _ = losses(model, data)
    ref = float(store[f"{tag}/step/loss"])
    assert abs(float(loss.detach()) - ref) <= 1e-4 * max(1.0, abs(ref))
    assert set(terms) == {"ce", "mi", "prob"}
    for k, v in terms.items():
        assert abs(float(v.detach()) - float(store[f"{tag}/step/term/{k}"])) <= 1e-4, k
    loss.backward()
    params = dict(model.named_parameters())
    wg = golden_group(store, f"{tag}/step/grad")
    assert_matches(data.x.grad, wg.pop("data.x"), 1e-3, "grad data.x")
    for k, w in wg.items():
        assert_matches(params[k].grad, w, 1e-3, "grad " + k, floor=1e-5)
    cam = golden_group(store, f"{tag}/step/cam")
    assert_matches(model.final_conv_acts, cam["final_conv_acts"], 1e-4, "final_conv_acts (masked pass)")
    assert_matches(model.final_conv_grads, cam["final_conv_grads"], 1e-3, "final_conv_grads (plain pass)")
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
    bufs = dict(model.named_buffers())
    for k, w in golden_group(store, f"{tag}/step/buffers").items():
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(w) == 2, k
        else:
            assert_matches(bufs[k], w, 1e-4, "buffer " + k, floor=1e-2)


@pytest.mark.parametrize("tag", TAGS)
def test_forward_pair_equals_two_calls(golden, tag):
    """One stacked sweep against model(data), model(data, True) in training mode: outputs, running statistics and
    num_batches_tracked, the tap (bit for bit: one workgroup per graph either way) and which pass each Grad-CAM attribute
    holds afterwards — final_conv_acts the masked pass's, final_conv_grads the plain pass's."""
    store = golden("sgcn_ori")
    m1, graphs, seed = _model(store, tag, bsz=8, train=True)
    m2, _, _ = _model(store, tag, bsz=8, train=True)
    d1, d2 = _batch(graphs), _batch(graphs)
    o1, p1 = m1.forward_pair(d1)
    o2, p2 = m2(d2), None
    acts2_plain = m2.final_conv_acts
    p2 = m2(d2, True)
    acts2_masked = m2.final_conv_acts
    cots = [c.cuda() for c in _probe([o1, p1], seed)]
    ((o1 * cots[0]).sum() + (p1 * cots[1]).sum()).backward()
    ((o2 * cots[0]).sum() + (p2 * cots[1]).sum()).backward()
    assert_matches(o1, o2.detach().cpu().numpy(), 1e-5, "plain logp")
    assert_matches(p1, p2.detach().cpu().numpy(), 1e-5, "masked logp")
    b2 = dict(m2.named_buffers())
    for k, b in m1.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(b2[k]) == 2, k
        else:
            assert_matches(b, b2[k].cpu().numpy(), 1e-5, "buffer " + k, floor=1e-2)
    assert torch.equal(m1.final_conv_acts, acts2_masked) and torch.equal(m1.final_conv_acts, m2.final_conv_acts)
    pair = m1.final_conv_pair
    assert len(pair) == 2 and torch.equal(pair[0][0], acts2_plain) and torch.equal(pair[1][0], acts2_masked)
    assert pair[0][1] is not None and pair[0][1].data_ptr() == m1.final_conv_grads.data_ptr()
    # two calls: both backward nodes write the attribute and the plain pass's runs last
    assert_matches(m1.final_conv_grads, m2.final_conv_grads.cpu().numpy(), 1e-5, "final_conv_grads (plain pass)")
    assert bool((m2.final_conv_grads[acts2_plain <= 0] == 0.0).all()) and bool((pair[1][1][acts2_masked <= 0] == 0.0).all())
    assert not torch.equal(pair[0][1], pair[1][1])
    p2d = dict(m2.named_parameters())
    for k, p in m1.named_parameters():
        if p.grad is None:
            assert p2d[k].grad is None, k
            continue
        assert_matches(p.grad, p2d[k].grad.cpu().numpy(), 1e-5, "grad " + k, floor=1e-4)
    assert_matches(d1.x.grad, d2.x.grad.cpu().numpy(), 1e-5, "grad data.x")


def test_graphed_step_equals_eager_steps(golden):
    """Three GraphedTrainStep replays against three eager train_steps on a twin (loss 1e-5, parameters 1e-5 with floor
    1e-3: the bound of the image-only siblings' test of this kind), the Grad-CAM attributes after each replay, and the
    evaluation loops of the image-only trainer."""
    from igcn_amd.data import DataLoader
    from igcn_amd.train import FlatAdam, GraphedTrainStep, assert_nothing_pending, eval_acc, eval_loss, eval_outputs, train_step
    store = golden("sgcn_ori")
    m1, graphs, _ = _model(store, "h32_5", bsz=8, train=True)
    m2, _, _ = _model(store, "h32_5", bsz=8, train=True)
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
        assert_matches(m2.final_conv_acts, m1.final_conv_acts.detach().cpu().numpy(), 1e-5, "final_conv_acts")
        assert_matches(m2.final_conv_grads, m1.final_conv_grads.cpu().numpy(), 1e-5, "final_conv_grads", floor=1e-6)
    b1, b2 = dict(m1.named_buffers()), dict(m2.named_buffers())
    assert int(b1["bn1.num_batches_tracked"]) == int(b2["bn1.num_batches_tracked"]) == 6
    for k in ("bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var"):
        assert_matches(b2[k], b1[k].cpu().numpy(), 1e-5, k, floor=1e-2)
    acc = eval_acc(m1, DataLoader(graphs, batch_size=4), device="cuda")
    lo = eval_loss(m1, DataLoader(graphs, batch_size=4), device="cuda")
    cols = eval_outputs(m1, DataLoader(graphs, batch_size=4), device="cuda")
    assert 0.0 <= float(acc) <= 1.0 and np.isfinite(float(lo)) and cols["logp"].shape == (8, 2)
    assert_nothing_pending("test")


def test_fit_epoch_equals_the_eager_loop(golden):
    """Three epochs of 8 + 8 + 5 graphs (a ragged tail) through fit_epoch — eager, captured and replayed steps — with the
    rate halved after the second, against the same nine steps through the eager train_step on a twin."""
    from igcn_amd import synth
    from igcn_amd.data import DataLoader
    from igcn_amd.train import FlatAdam, fit_epoch, train_step
    store = golden("sgcn_ori")
    m1, _, _ = _model(store, "h16_8", train=True)
    m2, _, _ = _model(store, "h16_8", train=True)
    graphs = synth.brain_graph_list(21, seed=77, rois=90, top_k=3, tsne_dim=16, num_classes=2)
    loader = DataLoader(graphs, 8, shuffle=False)
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    for epoch in range(3):
        if epoch == 2:
            for o in (o1, o2):
                o.param_groups[0]["lr"] *= 0.5
        got = fit_epoch(m1, o1, loader, device="cuda")
        total = 0.0
        for data in loader:
            data = data.to("cuda")
            total += float(train_step(m2, o2, data)) * data.num_graphs
        assert got == pytest.approx(total / len(graphs), rel=1e-4), (epoch, got, total / len(graphs))
    assert int(o1.step_count.item()) == int(o2.step_count.item()) == 9
    p2 = dict(m2.named_parameters())
    for k, p in m1.named_parameters():
        assert_matches(p, p2[k].detach().cpu().numpy(), 1e-5, k, floor=1e-3)
    b2 = dict(m2.named_buffers())
    for k, b in m1.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(b2[k]) == 18, k
        else:
            assert_matches(b, b2[k].cpu().numpy(), 1e-5, k, floor=1e-2)


def test_dropout_in_the_captured_step(golden):
    """Two replays of a captured step from identical state draw different masks (different losses); with
    _dropout_enabled = False they are identical; eval mode never drops."""
    from igcn_amd.train import FlatAdam, GraphedTrainStep
    store = golden("sgcn_ori")

    def two_replays(dropout):
        model, graphs, _ = _model(store, "h32_5", bsz=8, train=True)
        model._dropout_enabled = dropout
        state = copy.deepcopy(model.state_dict())
        opt = FlatAdam(model.parameters(), lr=0.0)
        step = GraphedTrainStep(model, opt, _batch(graphs), warmup=1)
        out = []
        for _ in range(2):
            model.load_state_dict(state)
            out.append(float(step()))
        return out, model, graphs

    (a, b), model, graphs = two_replays(True)
    assert a != b and np.isfinite(a) and np.isfinite(b), (a, b)
    model.eval()
    data = _batch(graphs)
    with torch.no_grad():
        assert torch.equal(model(data), model(data))
    (a, b), _, _ = two_replays(False)
    assert a == b, (a, b)


def test_refusals(golden):
    from igcn_amd import _lib
    from igcn_amd.sgcn import SGCN_Ori
    from igcn_amd.train import Evaluator
    from calltrace import record_calls
    store = golden("sgcn_ori")
    model, graphs, _ = _model(store, "h32_5", bsz=2)
    data = _batch(graphs)
    odd = SGCN_Ori(3, 32, 16, 5, rois=90).cuda()
    with pytest.MonkeyPatch.context() as mp:
        seen = record_calls(mp)
        with pytest.raises(ValueError, match="H_1=32 != H_2=16"):
            odd(data)
        with pytest.raises(ValueError, match="H_1=32 != H_2=16"):
            odd.forward_pair(data)
        assert seen == []                                           # raised before any launch
    with pytest.raises(ValueError, match="SGCN_GCN_IMGSNP models only"):
        Evaluator(model)
    with pytest.raises(_lib.IgcnError):
        _lib.ptr(torch.zeros(3))
    # widths the kernels do not cover fall to the per-layer route
    wide = SGCN_Ori(3, 40, 40, 5, rois=90).cuda().eval()
    with pytest.MonkeyPatch.context() as mp:
        seen = record_calls(mp)
        out = wide(data)
        names = [c[0] for c in seen]
    assert out.shape == (2, 2) and names.count("igcn_gcn_propagate_fwd") == 2 and "igcn_sgcn_ori_fwd" not in names
    torch.cuda.synchronize()
