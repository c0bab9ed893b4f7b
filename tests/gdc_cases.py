"""What the GDC tests on the GPU share (tests/test_gpu_gdc_heat.py, tests/test_gpu_gdc_tiled.py, tests/test_gpu_feeders.py,
tests/test_gdc.py): the inputs, the fp64 expectations, the entry points called raw into poisoned buffers, and the edge
comparison with its bounds — edge_ptr and edge_index exact, weights rtol 3e-7: an fp64 value correct to << 2^-24, rounded
once to fp32.  A plain module: nothing here is collected."""
import numpy as np
import pytest
import torch

import gdc_heat_ref as HR
from gdc_heat_ref import MARGIN

RTOL = 3e-7
PPR, HEAT, TOPK, THRESHOLD = 0, 1, 0, 1
KERNEL_ID = {"ppr": PPR, "heat": HEAT}
PARAM = {"heat": 5.0, "ppr": 0.05}
EPS = {"heat": 0.02, "ppr": 0.03}
# what a feeder's batch is compared on, and the per-subject columns a dense feeder gathers
KEYS = ("x", "edge_index", "edge_attr", "snps_feat", "y", "clini_score", "tsne_fdim", "clust_y", "batch", "ptr", "edge_ptr")
COLS = ("x", "snps_feat", "y", "clini_score", "tsne_fdim", "clust_y")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    """Imported by a GPU test module: skips it without a GPU, loads the library once."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


_ADJ, _S = {}, {}


def adjacencies(bsz, rois, seed, knn=5):
    key = (bsz, rois, seed, knn)
    if key not in _ADJ:
        rng = np.random.default_rng(seed)
        _ADJ[key] = [HR.synthetic_adjacency(rng, rois, knn).astype(np.float32) for _ in range(bsz)]
    return _ADJ[key]


def matrices(tag, adjs, kernel, param):
    """The dense fp64 diffusion matrices of a named input, computed once and shared (never modified)."""
    key = (tag, kernel, param)
    if key not in _S:
        _S[key] = [HR.diffusion_matrix(a, kernel, param) for a in adjs]
        for s in _S[key]:
            s.setflags(write=False)
    return _S[key]


def want(mats, k=None, eps=None):
    """(edge_index with graph g offset by g*R, edge_attr, edge_ptr) of a batch from its diffusion matrices, after
    asserting the margin of every decision."""
    gap_k, gap_e = zip(*[HR.margins(s, k=k, eps=eps) for s in mats])
    assert min(gap_k) >= MARGIN and min(gap_e) >= MARGIN, (min(gap_k), min(gap_e))
    eis, ews, ptr, off = [], [], [0], 0
    for s in mats:
        ei, ew = HR.coo(HR.OG.top_k_matrix(s, k) if eps is None else HR.clipped_matrix(s, eps))
        eis.append(ei + off)
        ews.append(ew)
        off += s.shape[0]
        ptr.append(ptr[-1] + ei.shape[1])
    return np.concatenate(eis, axis=1), np.concatenate(ews), np.asarray(ptr, dtype=np.int64)


def assert_edges(got, want, what=""):
    (ei, ew, edge_ptr), (want_ei, want_ew, want_ptr) = got, want
    assert edge_ptr.tolist() == list(want_ptr), what
    assert np.array_equal(ei.cpu().numpy(), want_ei), what                              # bit-exact indexing
    err = np.abs(ew.cpu().numpy().astype(np.float64) - want_ew) / np.abs(want_ew)
    print(f"{what}: edges {want_ei.shape[1]}, largest relative weight error {err.max() if err.size else 0.0:.3g}")
    np.testing.assert_allclose(ew.cpu().numpy(), want_ew, rtol=RTOL, atol=0)


def ws_need(bsz, rois, kernel):
    """Bytes of workspace the tiled route asks for."""
    from igcn_amd import _lib
    return int(_lib.load().igcn_gdc_tiled_workspace_bytes(bsz, rois, kernel))


def poisoned(b, r, cap):
    """Outputs of ``b`` graphs full of -7 / NaN: (edge_index [2, slots], edge_attr [slots], counts [b])."""
    slots = b * r * cap
    return (torch.full((2, slots), -7, dtype=torch.int64, device="cuda"),
            torch.full((slots,), float("nan"), dtype=torch.float32, device="cuda"),
            torch.full((b,), -7, dtype=torch.int32, device="cuda"))


def poisoned_workspace(nbytes):
    return torch.full(((nbytes + 7) // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")


def assert_written(ei, ew, counts):
    """No word of ``poisoned`` outputs is left."""
    assert not bool(torch.isnan(ew).any()) and not bool((ei == -7).any()) and not bool((counts == -7).any())


def raw(route, adj, kernel, param, sparsify, k, eps, subject=None, n_subjects=None, bsz=None, ws_bytes=None):
    """The entry point of ``route`` itself ('resident': igcn_gdc_diffuse, 'tiled': igcn_gdc_diffuse_tiled) on outputs full
    of NaN / -7 and, on the tiled route, a workspace full of NaN of the size the library asks for (``ws_bytes``: another
    size): (edge_index [2, slots], edge_attr [slots], counts [B]) with the padding left in."""
    from igcn_amd._lib import call, ptr, stream_ptr
    r = adj.shape[1]
    b = adj.shape[0] if bsz is None else bsz
    ei, ew, counts = poisoned(b, r, k if sparsify == TOPK else r)
    args = (b, r, kernel, float(param), sparsify, int(k), float(eps), ptr(adj),
            adj.shape[0] if n_subjects is None else n_subjects, ptr(subject), ptr(ei), ptr(ew), ptr(counts))
    if route == "tiled":
        nbytes = ws_need(b, r, kernel) if ws_bytes is None else ws_bytes
        ws = poisoned_workspace(nbytes)
        call("igcn_gdc_diffuse_tiled", *args, ptr(ws), nbytes, stream_ptr())
    else:
        assert route == "resident" and ws_bytes is None
        call("igcn_gdc_diffuse", *args, stream_ptr())
    return ei, ew, counts


def subjects(n, rois):
    """(graphs with their dense A, the same without it) of ``n`` synthetic subjects: a module's ``subjects`` fixture."""
    from igcn_amd import synth
    from igcn_amd.data import Data
    graphs = synth.brain_graph_list(n, seed=5, rois=rois, tsne_dim=16)
    slim = [Data(**{k: v for k, v in g.__dict__.items() if k != "A"}) for g in graphs]
    return graphs, slim


def batch_of_drawn(adj, cols, idx, **kw):
    """``batch_from_dense(check=True, **kw)`` of the subjects ``idx`` of ``adj`` [S,R,R] and of the columns ``cols``: what
    a DeviceGdcFeeder's batch is held to."""
    from igcn_amd.gdc import batch_from_dense
    b = int(idx.numel())
    sel = {k: torch.index_select(v, 0, idx) for k, v in cols.items()}
    x = sel.pop("x")
    per = {k: (v.reshape(b, -1) if k in ("snps_feat", "tsne_fdim", "clini_score") else v.reshape(-1))
           for k, v in sel.items()}
    return batch_from_dense(torch.index_select(adj, 0, idx), x, check=True, **kw, **per)


def same_batch(got, want, keys=KEYS):
    for k in keys:
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8)), k
