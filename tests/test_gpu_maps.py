"""GPU test of what the cohort map passes (igcn_amd.maps) launch: the igcn_attn_map_accumulate calls of every pass, per
batch and in order, as (B, Lq, Lk, C).  What the tables hold is tested next to each pass's model method
(test_gpu_attn_weights, test_gpu_rollout, test_gpu_connectivity, test_gpu_saliency)."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

ROIS, S, C = 90, 54, 3
POOL = (37, 18, 9, 3, 1)                        # the smallest synthetic GO DAG of the sibling GPU tests
N_TOP = POOL[2] + POOL[3] + POOL[4]             # (the encoder drops the two deepest levels)
BATCHES = (3, 3, 1)                             # 7 subjects in batches of 3: a ragged last batch


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _imgsnp():
    from igcn_amd import synth
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=2)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    torch.manual_seed(11)
    return SGCN_GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=ROIS, H_0=3, num_classes=C, isSoftSimilarity=True,
                           rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseProb4Regr=True, isImageOnly=False,
                           isSNPsOnly=False).cuda()


def _sgcn_gat():
    from igcn_amd.sgcn import SGCN_GAT
    torch.manual_seed(3)
    return SGCN_GAT(SimpleNamespace(num_features=3, num_classes=C), 2, 16, rois=ROIS, H_0=3).cuda()


def _per_batch(*shapes):
    return [(b,) + s for b in BATCHES for s in shapes]


CASES = {
    "attention": ("imgsnp", "attention_maps", {}, _per_batch((ROIS, N_TOP, C))),
    "association": ("imgsnp", "association_maps", {}, _per_batch((ROIS, S, C), (N_TOP, S, 1))),
    "connectivity_mask": ("imgsnp", "connectivity_maps", {"source": "mask"}, _per_batch((ROIS, ROIS, C), (ROIS, ROIS, 1))),
    "connectivity_gat": ("sgcn_gat", "connectivity_maps", {"source": "gat"}, _per_batch((2 * ROIS, ROIS, C))),
    "saliency_both": ("imgsnp", "saliency_maps", {"inputs": "both"}, _per_batch((ROIS, 3, C), (ROIS, 1, C), (S, 1, C))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_accumulate_launches_per_batch(monkeypatch, case):
    """One igcn_attn_map_accumulate call per quantity and batch, the labelled quantities first (C classes), then the
    ones averaged over everybody (1 class); nothing else reaches that entry point."""
    from calltrace import record_calls
    from igcn_amd import maps, synth
    from igcn_amd.data import DataLoader
    kind, name, kw, want = CASES[case]
    model = _imgsnp() if kind == "imgsnp" else _sgcn_gat()
    graphs = synth.brain_graph_list(sum(BATCHES), seed=6, rois=ROIS, h0=3, top_k=3, tsne_dim=16, num_classes=C)
    seen = record_calls(monkeypatch)
    r = getattr(maps, name)(model, DataLoader(graphs, batch_size=BATCHES[0]), device="cuda", **kw)
    got = [c[1:5] for c in seen if c[0] == "igcn_attn_map_accumulate"]
    assert got == want and r["n"] == sum(BATCHES)
    assert int(r["count"].sum()) == sum(BATCHES) and r["count"].numel() == C
