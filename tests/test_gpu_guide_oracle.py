"""GPU checks of GUIDE_IMGSNP against the float64 oracle (oracle/guide.py, pinned on the CPU by tests/test_oracle_guide.py)
at the shapes it runs: 90 ROIs, H_0 3, hidden_linear 32, the bench's 3000-node GO DAG (1800, 800, 300, 99, 1); hidden 16
at B = 256 graphs (the captured step of tools/guide_bench.py) and hidden 10 at B = 32.

Training mode, the gate's Gumbel noise imposed; dropout off — and, in one configuration of its own (hidden 10, B = 8), ON
with the oracle fed the masks the step drew (oracle.dropout.MaskFeed, the five sites of this model by name).  Gumbel noise (guide_ref.gumbel_noise, moved 1e-3 off a hard-decision tie):
the five loss terms and the loss to 1e-4, every gradient (data.x included) to 1e-3 on the scales of
tests/test_gpu_guide.py's fixture test.  An fp32 pre-activation within rounding of a PReLU's kink may take the other
branch, where the derivative jumps (1 -> a): the model's slopes are set to seeded positive values, so that the HIP path's
decisions can be read off the signs of the kernels' outputs (recorded in call order), and the oracle takes those decisions
inside a band of 2e-5 of the site's largest pre-activation.  Outside the band the two must agree; the flips are counted,
printed and capped.  The gate's hidden PReLU (encoder_i_N.1) is internal to its kernel and is not observed: there the
oracle's own decisions stand.  The heads' ReLU of lin1 is imposed likewise from linear_outf (conftest.relu_forced).

Eval mode: the outputs to 1e-4.  And GraphedTrainStep against eager train_step over three steps at B = 256 with dropout
and the gate drawing."""
import copy
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dropout_cases as DC
import guide_ref
from conftest import assert_matches, relu_forced
from _weights import seeded_state

pytestmark = pytest.mark.gpu

POOL = (1800, 800, 300, 99, 1)
ROIS, H0, HL, TAU = 90, 3, 32, 0.1
CONFIGS = {"h16_b256": dict(hidden=16, bsz=256, seed=81), "h10_b32": dict(hidden=10, bsz=32, seed=82)}
NAMES = ["logp", "x_hat", "latent", "lin_f", "reg", "img", "decoded", "prob"]
TERMS = ("ce", "reg", "recon", "recon_img", "sparsity")
BAND = 2e-5
MAX_FLIPS = 16
# the HIP path's PReLU launches in call order (guide_go_model.forward, then guide_img_snp.forward)
LN_SITES = ["go_network.w_act.0", "go_network.w_act.1", "go_network.w_act_out.0", "go_network.w_act_out.1"]
BN_SITES = ["go_network.conc_for_attention.2", "go_network.B.1", "go_network.B_D.1", "go_network.latent.2",
            "decoder_i_N.1", "decoder_i_N.5"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()
    torch.set_num_threads(16)


_SETUP = {}


DROPOUT = "h10_b8_dropout"          # dropout on: dropout_cases.GUIDE (its own seed), not part of CONFIGS


def _setup(tag):
    """(model on cuda, float32 state, index sets, graphs, noise [B, K, 2]) of a configuration; built once per module."""
    if tag in _SETUP:
        return _SETUP[tag]
    if tag == DROPOUT:
        g = DC.GUIDE
        assert (g["pool"], g["rois"], g["h0"], g["hidden_linear"], g["tau"]) == (POOL, ROIS, H0, HL, TAU)
        _SETUP[tag] = DC.guide_setup(g["hidden"], g["bsz"], g["seed"], "cuda")
        return _SETUP[tag]
    from igcn_amd import synth
    from igcn_amd.guide_img_snp import GUIDE_IMGSNP
    from oracle import go_network as OG
    c = CONFIGS[tag]
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=c["seed"])
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    model = GUIDE_IMGSNP(2, c["hidden"], a_g, a, pool_dim, 32, "cuda", rois=ROIS, H_0=H0, num_classes=3, num_regr=3,
                         hidden_linear=HL).cuda()
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, c["seed"], model.state_dict())
    rng = np.random.default_rng(c["seed"] + 1)
    for k in sorted(sd):                                 # every PReLU slope positive: its decisions show in its output
        if k.endswith(".weight") and tuple(sd[k].shape) == (1,):
            sd[k] = torch.tensor([rng.uniform(0.1, 0.6)], dtype=torch.float32)
    a_gc, a_c = synth.go_sparse_inputs(go_snps, adj)
    idx = OG.go_index_sets(a_gc, a_c, list(POOL), 2)
    graphs = synth.brain_graph_list(c["bsz"], seed=c["seed"] + 10, rois=ROIS, top_k=3, tsne_dim=16)
    k = ROIS * H0
    g = guide_ref.gumbel_noise(c["seed"] + 20, c["bsz"], k).astype(np.float64)
    logit = np.log(torch.softmax(sd["bias_n.0"].double(), 1).numpy())
    w = (logit[None] + g) / TAU
    g[..., 1] += np.where(np.abs(w[..., 1] - w[..., 0]) < 1e-3, 0.05, 0.0)  # as tests/golden/make_golden_guide.py
    _SETUP[tag] = (model, sd, idx, graphs, g.astype(np.float32))
    return _SETUP[tag]


def _fresh(tag, dropout=False):
    model, sd, idx, graphs, noise = _setup(tag)
    model.load_state_dict(sd)
    model.zero_grad(set_to_none=True)
    model._dropout_enabled = dropout
    model.go_network._dropout_enabled = dropout
    return model, sd, idx, graphs, noise


def _named(o):
    return dict(zip(NAMES, (o[0], o[1], o[2], o[4], o[5], o[6][0], o[6][1], o[7][0])))


class _recorded_prelus:
    """Record the outputs of the HIP path's PReLU launches, in call order (dropout off: the PReLU itself; dropout on: the
    PReLU times the site's factors — a dropped entry shows nothing and goes into ``decisions``' skip mask)."""

    def __init__(self, monkeypatch):
        from igcn_amd import ops
        self.ln, self.bn = [], []
        orig_ln, orig_bn = ops.NodesLayerNormPReLU, ops.bn_prelu_forward
        rec = self

        class LN:
            @staticmethod
            def apply(*args):
                z = orig_ln.apply(*args)
                rec.ln.append((z.detach().clone(), args[5]))
                return z

        def bn(*args, **kw):
            y, m, r = orig_bn(*args, **kw)
            rec.bn.append(y.detach().clone())
            return y, m, r
        monkeypatch.setattr(ops, "NodesLayerNormPReLU", LN)
        monkeypatch.setattr(ops, "bn_prelu_forward", bn)

    def decisions(self, dropped=None):
        """site -> (bool tensor of u > 0 in the oracle's layout, entries nothing downstream reads or None).  ``dropped``
        {site: bool array, True = zero factor}: [B, N] for the LayerNorm sites (whole nodes), the site's shape otherwise."""
        dropped = dropped or {}
        assert len(self.ln) == len(LN_SITES) and len(self.bn) == len(BN_SITES), (len(self.ln), len(self.bn))
        out = {}
        for site, (z, pool) in zip(LN_SITES, self.ln):           # HIP [B, f, N - pool] -> oracle [B, N, f]
            b, f, m = z.shape
            want = torch.zeros(b, m + pool, f, dtype=torch.bool)
            want[:, pool:, :] = (z > 0).permute(0, 2, 1).cpu()
            skip = torch.zeros_like(want)
            skip[:, :pool, :] = True                              # pooled-away nodes
            if site in dropped:
                skip |= torch.from_numpy(dropped[site]).unsqueeze(2)
            out[site] = (want, skip)
        for site, y in zip(BN_SITES, self.bn):                    # HIP [B, C, D] -> [B, C, D] (D > 1) or [B, C]
            w = (y > 0).cpu()
            w = w if w.shape[-1] > 1 else w[..., 0]
            out[site] = (w, torch.from_numpy(dropped[site]).reshape(w.shape) if site in dropped else None)
        return out


class _imposed_prelus:
    """Replace oracle.guide.prelu: inside BAND the HIP decision replaces the oracle's; outside it they must agree."""

    def __init__(self, monkeypatch, decided):
        from oracle import guide as OGD
        self.flips, self.mismatch, self.total = 0, 0, 0
        orig = OGD.prelu

        def prelu(site, u, a):
            if site not in decided:
                return orig(site, u, a)
            want, skip = decided[site]
            assert tuple(want.shape) == tuple(u.shape), (site, tuple(want.shape), tuple(u.shape))
            mag = u.detach().abs()
            near = mag <= BAND * mag.max()
            differ = (u.detach() > 0) != want
            if skip is not None:
                differ = differ & ~skip
            self.mismatch += int((differ & ~near).sum())
            flip = differ & near
            self.flips += int(flip.sum())
            self.total += u.numel()
            return torch.where(flip, torch.where(want, u, a * u), orig(site, u, a))
        monkeypatch.setattr(OGD, "prelu", prelu)


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_model_train_vs_fp64_oracle(tag, monkeypatch):
    from igcn_amd.data import Batch
    from igcn_amd.train import GUIDE_LAMBDA, losses
    from oracle import guide as OGD
    from oracle import sgcn_img_snp as OS
    model, sd, idx, graphs, noise = _fresh(tag)
    model.train()
    model._gate_noise = torch.from_numpy(noise).cuda()
    data = Batch.from_data_list(graphs).to("cuda")
    rec = _recorded_prelus(monkeypatch)
    loss, terms, outs = losses(model, data, temperature=torch.tensor(TAU, device="cuda"))
    loss.backward()
    model._gate_noise = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sdo = OS.make_leaf_state(sd, torch.float64)
    cpu = OGD.batch_data(Batch.from_data_list(graphs))
    imp = _imposed_prelus(monkeypatch, rec.decisions())
    lin_f = _named(outs)["lin_f"]
    with relu_forced({0: (lin_f > 0).cpu()}, band=BAND) as rf:
        loss_o, terms_o, outs_o = OGD.train_losses(sdo, SimpleNamespace(rois=ROIS), idx, cpu, TAU,
                                                   torch.from_numpy(noise).double(), GUIDE_LAMBDA)
    loss_o.backward()
    print(f"\n[{tag}] oracle {time.perf_counter() - t0:.1f} s; imposed {imp.flips} of {imp.total} PReLU decisions "
          f"and {rf.flips} of {lin_f.numel()} lin1 ReLU decisions")
    assert imp.mismatch == 0 and rf.mismatch_outside == 0, (imp.mismatch, rf.mismatch_outside)
    assert imp.flips + rf.flips <= MAX_FLIPS, (imp.flips, rf.flips)
    want = _named(outs_o)
    for n, o in _named(outs).items():
        assert_matches(o, want[n].detach().numpy(), 1e-4, n)
    for k in TERMS:
        ref = float(terms_o[k].detach())
        assert abs(float(terms[k]) - ref) <= 1e-4 * max(1.0, abs(ref)), (k, float(terms[k]), ref)
    ref = float(loss_o.detach())
    assert abs(float(loss) - ref) <= 1e-4 * max(1.0, abs(ref)), (float(loss), ref)
    msd = model.state_dict()
    for k, v in sdo.items():
        if "running_" in k:
            assert_matches(msd[k].float(), v.numpy(), 1e-4, k)
        elif k.endswith("num_batches_tracked"):
            assert int(msd[k]) == int(v), k
    assert_matches(data.x.grad, cpu.x.grad.numpy(), 1e-3, "grad data.x")
    params = dict(model.named_parameters())
    wg = {k: v.grad.numpy() for k, v in sdo.items() if v.requires_grad and v.grad is not None}
    go_scale = max(float(np.abs(w).max()) for k, w in wg.items() if k.startswith("go_network."))
    for k, w in wg.items():                    # the floors of test_model_train_vs_reference_golden
        assert params[k].grad is not None, k
        floor = 1e-5
        sib = wg.get(k[:-5] + ".weight") if k.endswith(".bias") else None
        if sib is not None:
            floor = max(floor, 0.5 * float(np.abs(sib).max()))
        if k.startswith("go_network."):
            floor = max(floor, go_scale)
        assert_matches(params[k].grad, w, 1e-3, "grad " + k, floor=floor)
    for k, p in params.items():                # nothing the oracle leaves without a gradient gets one here
        if k not in wg:
            assert p.grad is None or not bool(p.grad.abs().max() > 0), "unexpected grad " + k


def test_model_train_with_dropout_vs_fp64_oracle_under_the_steps_own_masks(monkeypatch):
    """Dropout on in the model and in its GO network (hidden 10, B = 8, the module's pool): the one mask launch of the
    forward is recorded, equals oracle.dropout.masks(recorded sites, counter) bit for bit, and the oracle takes those
    factors by site name — the GO network's seven sites and encoder_i_N.1, decoder_i_N.1, decoder_i_N.5 (p = 0.4), lin1
    (0.5), lin1_regr (0.3).  The five terms and the loss at 1e-4, every gradient at 1e-3 on the floors of the dropout-off
    test; PReLU decisions of dropped entries are skipped (a PReLU output times a zero factor shows nothing), MAX_FLIPS and
    BAND as everywhere.  Negative control: the oracle under the masks of counter + 1 is dropout_cases.MARGIN away."""
    from igcn_amd.data import Batch
    from igcn_amd.train import GUIDE_LAMBDA, losses
    from oracle import dropout as OD
    from oracle import guide as OGD
    from oracle import sgcn_img_snp as OS
    model, sd, idx, graphs, noise = _fresh(DROPOUT, dropout=True)
    model.train()
    model._gate_noise = torch.from_numpy(noise).cuda()
    data = Batch.from_data_list(graphs).to("cuda")
    rec = _recorded_prelus(monkeypatch)
    counter = int(DC.set_counter(model.go_network).state[0].item())
    with monkeypatch.context() as mp:
        drawn = DC.recorded_masks(mp)
        loss, terms, outs = losses(model, data, temperature=torch.tensor(TAU, device="cuda"))
    loss.backward()
    model._gate_noise = None
    torch.cuda.synchronize()
    assert len(drawn.calls) == 1 and not drawn.calls[0][2]
    sites, arrays = drawn.calls[0][0], drawn.arrays(0)
    DC.assert_masks_rebuilt(sites, arrays, counter, "GUIDE_IMGSNP")
    assert int(model.go_network._drop_state.state[0].item()) == counter + 1
    names = OD.go_site_names(2, OD.GUIDE_EXTRA)
    zero = {n: a == 0 for n, a in zip(names, arrays)}
    dropped = {("go_network." + n if n in OD.go_site_names(2) else n): z for n, z in zero.items()}
    t0 = time.perf_counter()
    sdo = OS.make_leaf_state(sd, torch.float64)
    cpu = OGD.batch_data(Batch.from_data_list(graphs))
    imp = _imposed_prelus(monkeypatch, rec.decisions(dropped))
    lin_f = _named(outs)["lin_f"]
    noise64 = torch.from_numpy(noise).double()
    with relu_forced({0: (lin_f > 0).cpu()}, band=BAND) as rf:
        loss_o, terms_o, outs_o = OGD.train_losses(sdo, SimpleNamespace(rois=ROIS), idx, cpu, TAU, noise64, GUIDE_LAMBDA,
                                                   dropout=OD.feed_of(sites, arrays, names))
    loss_o.backward()
    print(f"\n[{DROPOUT}] oracle {time.perf_counter() - t0:.1f} s; imposed {imp.flips} of {imp.total} PReLU decisions "
          f"and {rf.flips} of {lin_f.numel()} lin1 ReLU decisions")
    assert imp.mismatch == 0 and rf.mismatch_outside == 0, (imp.mismatch, rf.mismatch_outside)
    assert imp.flips + rf.flips <= MAX_FLIPS, (imp.flips, rf.flips)
    for k in TERMS:
        ref = float(terms_o[k].detach())
        assert abs(float(terms[k]) - ref) <= 1e-4 * max(1.0, abs(ref)), (k, float(terms[k]), ref)
    ref = float(loss_o.detach())
    assert abs(float(loss) - ref) <= 1e-4 * max(1.0, abs(ref)), (float(loss), ref)
    want = _named(outs_o)
    for n, o in _named(outs).items():
        assert_matches(o, want[n].detach().numpy(), 1e-4, n)
    assert_matches(data.x.grad, cpu.x.grad.numpy(), 1e-3, "grad data.x")
    params = dict(model.named_parameters())
    wg = {k: v.grad.numpy() for k, v in sdo.items() if v.requires_grad and v.grad is not None}
    go_scale = max(float(np.abs(w).max()) for k, w in wg.items() if k.startswith("go_network."))
    for k, w in wg.items():                    # the floors of test_model_train_vs_fp64_oracle
        assert params[k].grad is not None, k
        floor = 1e-5
        sib = wg.get(k[:-5] + ".weight") if k.endswith(".bias") else None
        if sib is not None:
            floor = max(floor, 0.5 * float(np.abs(sib).max()))
        if k.startswith("go_network."):
            floor = max(floor, go_scale)
        assert_matches(params[k].grad, w, 1e-3, "grad " + k, floor=floor)
    # negative control (values only): the same HIP loss against the oracle under the NEXT launch's masks
    monkeypatch.undo()
    with torch.no_grad():
        other = OGD.train_losses(OS.make_leaf_state(sd, torch.float64), SimpleNamespace(rois=ROIS), idx,
                                 OGD.batch_data(Batch.from_data_list(graphs)), TAU, noise64, GUIDE_LAMBDA,
                                 dropout=OD.feed_of(sites, OD.masks(sites, counter + 1), names))[:2]
    gap = DC.gap((loss, terms), other)
    print(f"[control] HIP loss against the oracle under the masks of counter + 1: {gap:.5f} (margin {DC.MARGIN})")
    assert gap > DC.MARGIN, gap


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_model_eval_vs_fp64_oracle(tag):
    from igcn_amd.data import Batch
    from oracle import guide as OGD
    from oracle import sgcn_img_snp as OS
    model, sd, idx, graphs, _ = _fresh(tag)
    model.eval()
    with torch.no_grad():
        outs = _named(model(Batch.from_data_list(graphs).to("cuda"), torch.tensor(TAU, device="cuda"), "cuda"))
    sdo = OS.make_leaf_state(sd, torch.float64)
    with torch.no_grad():
        want = _named(OGD.model_forward(sdo, SimpleNamespace(rois=ROIS), idx, OGD.batch_data(Batch.from_data_list(graphs)),
                                        training=False))
    for n in NAMES:
        assert_matches(outs[n], want[n].detach().numpy(), 1e-4, n)


def test_graphed_step_equals_eager_steps_at_bench_shape():
    """Three steps at B = 256 on the 3000-node DAG, dropout on and the gate drawing: the captured step equals the eager
    one (the bounds of tests/test_gpu_guide.py::test_graphed_step_equals_eager_steps_with_dropout_and_gate)."""
    from igcn_amd import ops, synth
    from igcn_amd.data import Batch
    from igcn_amd.train import FlatAdam, GraphedTrainStep, train_step
    m1, sd, _, graphs, _ = _fresh("h16_b256")
    m1 = copy.deepcopy(m1)
    for m in (m1, m1.go_network):
        m._dropout_enabled = True
    m1.train()
    m2 = copy.deepcopy(m1)
    tau = torch.tensor(TAU, device="cuda")
    more = synth.brain_graph_list(256, seed=CONFIGS["h16_b256"]["seed"] + 11, rois=ROIS, top_k=3, tsne_dim=16)
    batches = [Batch.from_data_list(more).to("cuda"), Batch.from_data_list(graphs[128:] + more[:128]).to("cuda"),
               Batch.from_data_list(graphs[::-1]).to("cuda")]
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    step = GraphedTrainStep(m1, o1, Batch.from_data_list(graphs).to("cuda"), warmup=2, temperature=tau)
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
