"""On-device batch construction: the reference's per-subject GDC pre-transform
``preprocess_diffusion_imgs_snps`` (util_gdc.py:71-101: personalised-PageRank or heat-kernel diffusion, top-k per column
or epsilon threshold, column normalisation, COO) and the block-diagonal collation of ``Batch.from_data_list``
(batch.py:24-123), for a whole batch of dense adjacencies in one kernel launch (igcn_gdc_topk / igcn_gdc_diffuse, fp64
in LDS).

The reference runs the transform once per subject in numpy at dataset-build time and collates in a Python loop per
batch; at >= 100 k graphs/s of train-step throughput both are far too slow to feed the GPU.
"""
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .data import Batch, Data


KERNELS = {"ppr": 0, "heat": 1}                       # include/igcn.h IGCN_GDC_PPR / IGCN_GDC_HEAT
_TOPK, _THRESHOLD = 0, 1                                # IGCN_GDC_TOPK / IGCN_GDC_THRESHOLD


def _diffuse(adj, cap, check, launch):
    """The launch common to every kernel / sparsifier pair: outputs of ``cap`` slots per column, ``launch(b, r, adj, ei,
    ew, counts)``, the edge offsets, and — with ``check`` — the squeeze of the padding."""
    if adj.dim() != 3 or adj.shape[1] != adj.shape[2]:
        raise _lib.IgcnError("adj must be [B,R,R]")
    adj = adj.to(torch.float32).contiguous()
    b, r, _ = adj.shape
    slots = b * r * cap
    ei = torch.empty(2, slots, dtype=torch.int64, device=adj.device)
    ew = torch.empty(slots, dtype=torch.float32, device=adj.device)
    counts = torch.empty(b, dtype=torch.int32, device=adj.device)
    launch(b, r, adj, ei, ew, counts)
    edge_ptr = torch.zeros(b + 1, dtype=torch.int64, device=adj.device)
    torch.cumsum(counts, 0, out=edge_ptr[1:])
    # pre-transform time, not the train step: one host read decides whether padding slots must be squeezed out
    if check and int(edge_ptr[-1]) != slots:
        valid = ei[0] >= 0
        ei, ew = ei[:, valid].contiguous(), ew[valid].contiguous()
    return ei, ew, edge_ptr


def diffusion_topk(adj, top_k=3, alpha=0.05, check=True):
    """adj [B,R,R] f32 (device) -> (edge_index [2,E] int64 with graph g's nodes offset by g*R, edge_attr [E] f32,
    edge_ptr [B+1] int64).  Edges of a graph are in (row, col) order as scipy's coo_matrix emits them.
    ``check=False``: no host read — for inputs known to keep ``top_k`` entries in every column (a PPR matrix of a
    connected graph is dense), as a per-step producer in front of the graphed train step; a column that kept fewer
    leaves -1 slots behind, which the per-graph plan build reports in its status word."""
    return _diffuse(adj, top_k, check, lambda b, r, a, ei, ew, counts: call(
        "igcn_gdc_topk", b, r, int(top_k), float(alpha), ptr(a), ptr(ei), ptr(ew), ptr(counts), stream_ptr()))


def diffusion(adj, kernel="ppr", alpha=0.05, t=5.0, top_k=3, eps=None, check=True):
    """All of util_gdc.py for a batch: ``kernel`` 'ppr' (get_ppr_matrix :7-14, ``alpha``) or 'heat' (get_heat_matrix
    :16-23, ``t`` in (0, 64]); ``eps=None`` keeps the ``top_k`` largest entries of every column (get_top_k_matrix
    :25-31), otherwise the entries >= ``eps`` (get_clipped_matrix :33-38) and ``top_k`` is ignored.  Same result layout
    as ``diffusion_topk``.  The threshold allocates R*R slots per graph and always squeezes the padding out (one host
    read), so it cannot run with ``check=False``."""
    if kernel not in KERNELS:
        raise ValueError(f"kernel must be 'ppr' or 'heat', got {kernel!r}")
    if eps is not None and not check:
        raise ValueError("the eps threshold keeps a data-dependent number of edges: it needs check=True")
    if kernel == "ppr" and eps is None:
        return diffusion_topk(adj, top_k, alpha, check)
    param = float(alpha if kernel == "ppr" else t)
    mode, eps_arg = (_TOPK, 0.0) if eps is None else (_THRESHOLD, float(eps))
    cap = int(top_k) if eps is None else int(adj.shape[-1])
    return _diffuse(adj, cap, check, lambda b, r, a, ei, ew, counts: call(
        "igcn_gdc_diffuse", b, r, KERNELS[kernel], param, mode, int(top_k), eps_arg, ptr(a), b, None, ptr(ei), ptr(ew),
        ptr(counts), stream_ptr()))


def batch_from_dense(adj, x, top_k=3, alpha=0.05, check=True, kernel="ppr", t=5.0, eps=None, **per_graph):
    """A ``Batch`` (the attribute surface of data.Batch.from_data_list) straight from device tensors:
    adj [B,R,R], x [B*R,H0] or [B,R,H0]; ``per_graph`` tensors with leading dim B (snps_feat [B,54], y [B],
    clini_score [B,n] -> flattened like the reference's collation, tsne_fdim [B,F], clust_y [B], sbjID [B]).
    ``kernel``, ``t``, ``eps``: see ``diffusion``."""
    b, r, _ = adj.shape
    if kernel == "ppr" and eps is None:
        ei, ew, edge_ptr = diffusion_topk(adj, top_k, alpha, check)
    else:
        ei, ew, edge_ptr = diffusion(adj, kernel, alpha, t, top_k, eps, check)
    out = Batch()
    out.x = x.reshape(b * r, -1).contiguous()
    out.edge_index, out.edge_attr = ei, ew
    out.A = adj.reshape(b * r, r)
    out.batch = torch.arange(b, device=adj.device).repeat_interleave(r)
    for key, val in per_graph.items():
        if key == "clini_score" or key == "demographics":
            val = val.reshape(-1)                       # 1-D per-graph attributes concatenate (batch.py:110)
        setattr(out, key, val)
    out._num_graphs = b
    out.ptr = torch.arange(b + 1, device=adj.device, dtype=torch.int64) * r
    out.edge_ptr = edge_ptr
    out._max_nodes = r
    if eps is None:
        out._max_edges = r * top_k
    else:                                               # data-dependent: the largest graph of this batch
        out._max_edges = int((edge_ptr[1:] - edge_ptr[:-1]).max()) if b else 0
    return out


def preprocess_diffusion_imgs_snps(data, isPPr=True, isTopK=True, top_k=5, alpha=0.05):
    """util_gdc.py:71-101 for one ``Data`` (its dense ``A`` [R,R]), on the device ``A`` lives on: the same signature,
    the same field list.  ``isPPr=False`` is the heat kernel at the reference's default t = 5.0 (:77)."""
    if not isTopK:
        raise ValueError("isTopK=False is not reproduced: util_gdc.py:82 applies get_heat_matrix to the diffusion "
                         "matrix and never reaches get_clipped_matrix; use gdc.diffusion(..., eps=) for the threshold")
    ei, ew, _ = diffusion(data.A[None], "ppr" if isPPr else "heat", alpha=alpha, t=5.0, top_k=top_k)
    return Data(x=data.x, edge_index=ei, edge_attr=ew, y=data.y, A=data.A, snps_feat=data.snps_feat,
                clust_y=data.clust_y, sbjID=data.sbjID, tsne_fdim=data.tsne_fdim, clini_score=data.clini_score,
                demographics=data.demographics)
