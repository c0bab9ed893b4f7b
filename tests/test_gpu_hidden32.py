"""The hidden-32 rows of the reference's default search (main.py:141-145): SGCN_GCN_IMGSNP(L, 32) for L = 2..5, attention
width L * 32 = 64, 96, 128, 160 — the GO read-out on the wide kernels of csrc/readout.hip (64: the row-coalesced `_q`
kernels; 96..160: the strip kernels), the cross-attention on igcn_attn_core_* at head_dim 32..80.

  * eval forward (isExplain=True) and every gradient against the fp64 oracle, the body and the bounds of
    test_sweep_widths_off_the_kernel_grid_vs_oracle (outputs 1e-4, data.x.grad 3e-3, parameter gradients 5e-3, floor 1e-6);
  * training mode through test_gpu_model.train_mode_vs_oracle at (3, 32), its own bounds, both step formulations;
  * the captured step against the eager one at (3, 32), three steps, nothing left pending on the stream;
  * the entry points one forward + backward of (3, 32) calls: the read-out with D = 96, the attention core, and not the
    batched-GEMM + softmax composite."""
from types import SimpleNamespace

import pytest
import torch

from calltrace import record_calls
from conftest import assert_matches
from _weights import seeded_state
from test_gpu_model import NAMES, _probe, train_mode_vs_oracle

pytestmark = pytest.mark.gpu

POOL = (60, 30, 20, 9, 1)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _model(layers, go_seed, torch_seed=None):
    from igcn_amd import synth
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=go_seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    if torch_seed is not None:
        torch.manual_seed(torch_seed)
    model = SGCN_GCN_IMGSNP(layers, 32, a_g, a, pool_dim, 32, "cuda", rois=90, H_0=3, num_classes=3,
                            isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3,
                            isuseProb4Regr=True, isImageOnly=False, isSNPsOnly=False).cuda()
    return model, (go_snps, adj)


@pytest.mark.parametrize("layers", [2, 3, 4, 5])
def test_hidden32_vs_oracle(layers):
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from oracle import go_network as OG, sgcn_img_snp as OS
    model, (go_snps, adj) = _model(layers, 1)
    model.eval()
    sd = seeded_state({k: v.shape for k, v in model.state_dict().items()}, 6)
    model.load_state_dict(sd)
    graphs = synth.brain_graph_list(8, seed=78, rois=90, tsne_dim=16)
    data = Batch.from_data_list(graphs).to("cuda")
    outs = model(data, None, "cuda", isExplain=True)
    assert outs[2].shape == (8, 90 * layers * 32)
    cot = _probe(outs, 9)
    sum((o * c.cuda()).sum() for o, c in zip(outs, cot)).backward()
    a_g_c, a_c = synth.go_sparse_inputs(go_snps, adj)
    idx = OG.go_index_sets(a_g_c, a_c, list(POOL), 2)
    sdo = OS.make_leaf_state(sd, dtype=torch.float64)
    dcpu = Batch.from_data_list(graphs)
    dcpu.x = dcpu.x.double().requires_grad_(True)
    dcpu.edge_attr, dcpu.snps_feat = dcpu.edge_attr.double(), dcpu.snps_feat.double()
    cfg = SimpleNamespace(num_layers=layers, rois=90, image_only=False, rbf_gamma=0.01)
    ref = OS.model_forward(sdo, cfg, idx, dcpu, True, training=False)
    sum((o * c.double()).sum() for o, c in zip(ref, cot)).backward()
    for n, o, r in zip(NAMES, outs, ref):
        assert_matches(o, r.detach().numpy(), 1e-4, n)
    assert_matches(data.x.grad, dcpu.x.grad.numpy(), 3e-3, "grad data.x")
    params = dict(model.named_parameters())
    for k in OS.trainable_keys(sdo):
        if sdo[k].grad is None:
            continue
        assert_matches(params[k].grad, sdo[k].grad.numpy(), 5e-3, "grad " + k, floor=1e-6)


def test_hidden32_train_mode_vs_oracle(monkeypatch):
    """(3, 32) in TRAINING mode at the 500-node GO DAG and B = 32 of the multifusion cases: the seven loss terms at 1e-4,
    every gradient at 1e-3 against the fp64 oracle, the stacked sweep and the two-call formulation."""
    train_mode_vs_oracle(monkeypatch, 90, (300, 120, 60, 19, 1), 32, maps=("default",), layers=3, hidden=32)


def test_hidden32_graphed_train_step_matches_eager():
    """test_graphed_train_step_matches_eager[90-False] with SGCN_GCN_IMGSNP(3, 32, ...)."""
    import copy
    from igcn_amd import synth
    from igcn_amd.data import Batch
    from igcn_amd.train import FlatAdam, GraphedTrainStep, stream_pending, train_step
    m1, _ = _model(3, 2, torch_seed=3)
    m1.train()
    for m in (m1, m1.go_network):
        m._dropout_enabled = False
    m2 = copy.deepcopy(m1)
    gkw = dict(rois=90, tsne_dim=16, dense=False, num_classes=3, num_regr=3)
    batches = [Batch.from_data_list(synth.brain_graph_list(6, seed=50 + i, **gkw)).to("cuda") for i in range(3)]
    lam = [1.0, 1.0, 0.5, 1.5e-6, 0.1, 0.2]
    o1, o2 = FlatAdam(m1.parameters(), lr=1e-3), FlatAdam(m2.parameters(), lr=1e-3)
    static = Batch.from_data_list(synth.brain_graph_list(6, seed=50, **gkw)).to("cuda")
    static.x.requires_grad_(True)
    snap = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    step = GraphedTrainStep(m1, o1, static, lam, warmup=2)
    assert step.plan_in_graph and not step.plan._tiled
    for k, v in m1.state_dict().items():                 # the constructor's warm-up steps left no trace
        assert torch.equal(v, snap[k]), k
    assert int(o1.step_count.item()) == 0 and not bool(o1.exp_avg.any())
    for b in batches:
        step.load(b)
        l1 = float(step())
        l2 = float(train_step(m2, o2, b, lam))
        assert abs(l1 - l2) <= 1e-4 * max(1.0, abs(l2)), (l1, l2)
        assert stream_pending() == 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        # (see test_graphed_train_step_matches_eager: an element whose gradient is rounding noise moves by up to lr per step)
        d = (p1.detach() - p2.detach()).abs()
        tol = torch.full_like(d, 2e-4) if p2.grad is None else torch.where(p2.grad.abs() > 1e-6, 2e-4, 3.5e-3)
        assert bool((d <= tol).all()), (k, float(d.max()))


def test_hidden32_calls_the_wide_readout_and_the_attention_core(monkeypatch):
    from igcn_amd import ops, synth
    from igcn_amd.data import Batch
    model, _ = _model(3, 1, torch_seed=0)
    model.eval()
    data = Batch.from_data_list(synth.brain_graph_list(4, seed=78, rois=90, tsne_dim=16)).to("cuda")
    seen = record_calls(monkeypatch)

    def composite(*a, **k):
        raise AssertionError("the batched-GEMM + softmax composite ran: ops.InProj is only used there")
    monkeypatch.setattr(ops.InProj, "apply", composite)
    outs = model(data, None, "cuda", isExplain=True)
    sum(o.sum() for o in outs).backward()
    torch.cuda.synchronize()
    # (name, B, F, N, D, ...) forward and backward
    wide = {nm: [c for c in seen if c[0] == nm and c[4] == 96] for nm in ("igcn_node_linear_bn_fwd", "igcn_node_linear_bn_bwd")}
    for nm, calls in wide.items():
        assert len(calls) == 1 and calls[0][1:3] == (4, 5), (nm, calls)
    names = [c[0] for c in seen]
    assert "igcn_node_linear_bn_pair_fwd" not in names            # (paired launches are built for D1 = 32 only)
    assert any(nm.startswith("igcn_attn_core_fwd") for nm in names), sorted(set(names))
    assert any(nm.startswith("igcn_attn_core_bwd") for nm in names), sorted(set(names))
