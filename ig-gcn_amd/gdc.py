"""On-device batch construction: the reference's per-subject GDC pre-transform
``preprocess_diffusion_imgs_snps`` (util_gdc.py:71-101: personalised-PageRank or heat-kernel diffusion, top-k per column
or epsilon threshold, column normalisation, COO) and the block-diagonal collation of ``Batch.from_data_list``
(batch.py:24-123), for a whole batch of dense adjacencies in one kernel launch (igcn_gdc_diffuse, fp64 in LDS).  Graphs
beyond the LDS limit (up to 512 regions) take the tiled route: igcn_gdc_diffuse_tiled, fp64 products on the matrix cores
over a global-memory workspace (``route=``).  ``launch_into`` alone names an entry point; ``diffusion_routed`` is the body.

The reference runs the transform once per subject in numpy at dataset-build time and collates in a Python loop per
batch; at >= 100 k graphs/s of train-step throughput both are far too slow to feed the GPU.
"""
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .data import Batch, Data


KERNELS = {"ppr": 0, "heat": 1}                       # include/igcn.h IGCN_GDC_PPR / IGCN_GDC_HEAT
_TOPK, _THRESHOLD = 0, 1                                # IGCN_GDC_TOPK / IGCN_GDC_THRESHOLD


ROUTES = ("resident", "tiled", "auto")
# what one launch sequence of the tiled route may hold in its workspace unless the caller says otherwise: a batch that
# needs more is processed in chunks of graphs (32 PPR graphs of 512 regions need 256 MiB)
DEFAULT_WORKSPACE_BYTES = 512 << 20


def _check_route(route):
    if route not in ROUTES:
        raise ValueError(f"route must be one of {ROUTES}, got {route!r}")


def _check_kernel(kernel):
    if kernel not in KERNELS:
        raise ValueError(f"kernel must be 'ppr' or 'heat', got {kernel!r}")


def _resolve_route(route, rois, kernel):
    """'auto': the LDS-resident kernels wherever the graph fits them (they are the faster ones there), the tiled
    global-memory route (csrc/gdc_tiled.hip) above that.  ``route`` has passed ``_check_route``."""
    if route != "auto":
        return route
    return "resident" if rois <= _lib.load().igcn_gdc_max_rois(KERNELS[kernel]) else "tiled"


def tiled_workspace_bytes(graphs, rois, kernel):
    """Bytes of workspace the tiled route needs for ``graphs`` graphs of ``rois`` regions (linear in ``graphs``)."""
    return int(_lib.load().igcn_gdc_tiled_workspace_bytes(int(graphs), int(rois), KERNELS[kernel]))


def _empty(shape, dtype, device):
    """Every device buffer the GDC kernels write comes from here: the outputs of either route, and the tiled route's
    workspace (``loader.DeviceGdcFeeder`` takes its own from here too)."""
    return torch.empty(shape, dtype=dtype, device=device)


def tiled_workspace(graphs, rois, kernel, device):
    """(uint8 tensor, bytes) for ``graphs`` graphs on the tiled route."""
    need = tiled_workspace_bytes(graphs, rois, kernel)
    return _empty((max(need, 16),), torch.uint8, device), need


def launch_into(route, kernel, param, mode, top_k, eps, adj, n_subjects, subject, b, ei, ew, counts, ws=None, ws_bytes=0):
    """The C entry point of a resolved ``route`` ('resident' / 'tiled' with its workspace) on the current stream, and nothing
    more: graph g of the ``b`` is matrix ``subject[g]`` (``None``: g) of the ``n_subjects`` in ``adj``.  Allocates nothing."""
    args = (b, int(adj.shape[-1]), KERNELS[kernel], float(param), mode, int(top_k), float(eps), ptr(adj), int(n_subjects),
            ptr(subject), ptr(ei), ptr(ew), ptr(counts))
    if route == "tiled":
        call("igcn_gdc_diffuse_tiled", *args, ptr(ws), int(ws_bytes), stream_ptr())
    else:
        call("igcn_gdc_diffuse", *args, stream_ptr())


def _tiled_launch(kernel, param, mode, top_k, eps_arg, workspace_bytes):
    """The ``launch`` of ``_diffuse`` for the tiled route.  The workspace is one allocation of at most ``workspace_bytes``
    (default DEFAULT_WORKSPACE_BYTES); a batch that needs more goes through it in chunks of graphs, each chunk into
    buffers of its own size whose slots are then copied behind one another with the node offset of the chunk's first
    graph added.  Graphs do not depend on each other, so the chunk size changes no bit of the result.  A cap below one
    graph's need is handed to the library as it is, which refuses it with the number of bytes needed."""
    def launch(b, r, a, ei, ew, counts):
        cap_bytes = DEFAULT_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
        cap = (ei.shape[1] // (b * r)) if b else 0
        one = tiled_workspace_bytes(1, r, kernel)
        chunk = b if one == 0 else max(1, min(b, cap_bytes // one))
        have = min(cap_bytes, tiled_workspace_bytes(chunk, r, kernel)) if one else 0
        ws = _empty((max(have, 16),), torch.uint8, a.device)

        def run(g0, n, out_ei, out_ew, out_counts):
            launch_into("tiled", kernel, param, mode, top_k, eps_arg, a[g0:g0 + n], n, None, n, out_ei, out_ew, out_counts,
                        ws, have)

        if chunk >= b:
            run(0, b, ei, ew, counts)
            return
        for g0 in range(0, b, chunk):
            n = min(chunk, b - g0)
            part_ei = _empty((2, n * r * cap), torch.int64, a.device)
            lo, hi = g0 * r * cap, (g0 + n) * r * cap
            run(g0, n, part_ei, ew[lo:hi], counts[g0:g0 + n])
            ei[:, lo:hi] = torch.where(part_ei >= 0, part_ei + g0 * r, part_ei)
    return launch


def _diffuse(adj, cap, check, launch):
    """The launch common to every kernel / sparsifier pair: outputs of ``cap`` slots per column, ``launch(b, r, adj, ei,
    ew, counts)``, the edge offsets, and — with ``check`` — the squeeze of the padding."""
    adj = adj.to(torch.float32).contiguous()
    b, r, _ = adj.shape
    slots = b * r * cap
    ei = _empty((2, slots), torch.int64, adj.device)
    ew = _empty((slots,), torch.float32, adj.device)
    counts = _empty((b,), torch.int32, adj.device)
    launch(b, r, adj, ei, ew, counts)
    edge_ptr = torch.zeros(b + 1, dtype=torch.int64, device=adj.device)
    torch.cumsum(counts, 0, out=edge_ptr[1:])
    # pre-transform time, not the train step: one host read decides whether padding slots must be squeezed out
    if check and int(edge_ptr[-1]) != slots:
        valid = ei[0] >= 0
        ei, ew = ei[:, valid].contiguous(), ew[valid].contiguous()
    return ei, ew, edge_ptr


def diffusion_topk(adj, top_k=3, alpha=0.05, check=True, route="resident", workspace_bytes=None):
    """adj [B,R,R] f32 (device) -> (edge_index [2,E] int64 with graph g's nodes offset by g*R, edge_attr [E] f32,
    edge_ptr [B+1] int64).  Edges of a graph are in (row, col) order as scipy's coo_matrix emits them.
    ``check=False``: no host read — for inputs known to keep ``top_k`` entries in every column (a PPR matrix of a
    connected graph is dense), as a per-step producer in front of the graphed train step; a column that kept fewer
    leaves -1 slots behind, which the per-graph plan build reports in its status word.
    ``route``, ``workspace_bytes``: see ``diffusion_routed``."""
    return diffusion_routed(adj, "ppr", alpha, top_k=top_k, check=check, route=route, workspace_bytes=workspace_bytes)


def diffusion(adj, kernel="ppr", alpha=0.05, t=5.0, top_k=3, eps=None, check=True):
    """All of util_gdc.py for a batch: ``kernel`` 'ppr' (get_ppr_matrix :7-14, ``alpha``) or 'heat' (get_heat_matrix
    :16-23, ``t`` in (0, 64]); ``eps=None`` keeps the ``top_k`` largest entries of every column (get_top_k_matrix
    :25-31), otherwise the entries >= ``eps`` (get_clipped_matrix :33-38) and ``top_k`` is ignored.  Same result layout
    as ``diffusion_topk``.  The threshold allocates R*R slots per graph and always squeezes the padding out (one host
    read), so it cannot run with ``check=False``.  The LDS-resident kernels (R <= igcn_gdc_max_rois(kernel));
    ``diffusion_routed`` is the same call with a choice of route."""
    return diffusion_routed(adj, kernel, alpha, t, top_k, eps, check)


def diffusion_routed(adj, kernel="ppr", alpha=0.05, t=5.0, top_k=3, eps=None, check=True, route="resident",
                     workspace_bytes=None):
    """``diffusion`` with a choice of kernels.  ``route``:
      'resident'  one workgroup per graph, the fp64 system in LDS (csrc/gdc.hip): R <= 96 (heat) / 128 (PPR), refused
                  above that.  The default, and what ``diffusion`` runs.
      'tiled'     the fp64 system in a global-memory workspace, products on the fp64 matrix cores (csrc/gdc_tiled.hip):
                  any R <= 512, t in (0, 64], alpha in [0.001, 1].  Same edges; weights equal to the last fp32 bit or two.
      'auto'      'resident' wherever the graph fits it, 'tiled' above.
    ``workspace_bytes``: the cap on the tiled route's workspace (default DEFAULT_WORKSPACE_BYTES = 512 MiB; a graph of
    512 regions needs 8 MiB for PPR, 6 MiB for heat).  A batch that needs more is processed in chunks of graphs; the
    result does not depend on the chunk size.  Any other ``route`` raises ValueError before the device is touched."""
    _check_route(route)
    _check_kernel(kernel)
    if eps is not None and not check:
        raise ValueError("the eps threshold keeps a data-dependent number of edges: it needs check=True")
    if adj.dim() != 3 or adj.shape[1] != adj.shape[2]:
        raise _lib.IgcnError("adj must be [B,R,R]")
    param = float(alpha if kernel == "ppr" else t)
    mode, eps_arg = (_TOPK, 0.0) if eps is None else (_THRESHOLD, float(eps))
    cap = int(top_k) if eps is None else int(adj.shape[-1])
    if _resolve_route(route, adj.shape[-1], kernel) == "tiled":
        return _diffuse(adj, cap, check, _tiled_launch(kernel, param, mode, top_k, eps_arg, workspace_bytes))
    return _diffuse(adj, cap, check, lambda b, r, a, ei, ew, counts: launch_into(
        "resident", kernel, param, mode, top_k, eps_arg, a, b, None, b, ei, ew, counts))


def batch_from_dense(adj, x, top_k=3, alpha=0.05, check=True, kernel="ppr", t=5.0, eps=None, route="resident",
                     workspace_bytes=None, **per_graph):
    """A ``Batch`` (the attribute surface of data.Batch.from_data_list) straight from device tensors:
    adj [B,R,R], x [B*R,H0] or [B,R,H0]; ``per_graph`` tensors with leading dim B (snps_feat [B,54], y [B],
    clini_score [B,n] -> flattened like the reference's collation, tsne_fdim [B,F], clust_y [B], sbjID [B]).
    ``kernel``, ``t``, ``eps``: see ``diffusion``; ``route``, ``workspace_bytes``: see ``diffusion_routed``."""
    _check_route(route)
    b, r, _ = adj.shape
    ei, ew, edge_ptr = diffusion_routed(adj, kernel, alpha, t, top_k, eps, check, route, workspace_bytes)
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
    the same field list.  ``isPPr=False`` is the heat kernel at the reference's default t = 5.0 (:77).  Route 'auto':
    graphs beyond the LDS-resident kernels (up to 512 regions) take the tiled route."""
    if not isTopK:
        raise ValueError("isTopK=False is not reproduced: util_gdc.py:82 applies get_heat_matrix to the diffusion "
                         "matrix and never reaches get_clipped_matrix; use gdc.diffusion(..., eps=) for the threshold")
    ei, ew, _ = diffusion_routed(data.A[None], "ppr" if isPPr else "heat", alpha=alpha, t=5.0, top_k=top_k, route="auto")
    return Data(x=data.x, edge_index=ei, edge_attr=ew, y=data.y, A=data.A, snps_feat=data.snps_feat,
                clust_y=data.clust_y, sbjID=data.sbjID, tsne_fdim=data.tsne_fdim, clini_score=data.clini_score,
                demographics=data.demographics)
