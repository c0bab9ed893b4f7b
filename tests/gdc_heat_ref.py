"""fp64 restatement of the heat-kernel and threshold halves of the GDC pre-transform (TEST INFRASTRUCTURE ONLY),
written from the formulas:

    H = D^-1/2 A D^-1/2,  D = diag(row sums of A)           S_heat = expm(-t (I - H))
    threshold(S, eps): entries below eps become 0, every column is divided by its sum (a sum <= 0: left as it is)
    COO: the non-zeros in row-major order, edge_index = [row; col] int64, edge_attr float32

The PPR matrix and the top-k rule are oracle/gdc.py's.  Pinned to the reference's own functions by
tests/golden/gdc_heat.npz (tests/test_gdc_heat_reference.py).
"""
import numpy as np
from scipy.linalg import expm

from oracle import gdc as OG


def heat_matrix(adj, t=5.0):
    adj = np.asarray(adj, dtype=np.float64)
    d = 1.0 / np.sqrt(adj.sum(axis=1))
    h = (d[:, None] * adj) * d[None, :]
    return expm(-t * (np.eye(adj.shape[0]) - h))


def diffusion_matrix(adj, kernel, param):
    """kernel 'ppr' (param = alpha) or 'heat' (param = t) -> dense fp64 S."""
    if kernel == "ppr":
        return OG.ppr_matrix(np.asarray(adj, dtype=np.float64), param)
    return heat_matrix(adj, param)


def clipped_matrix(s, eps):
    s = np.where(s < eps, 0.0, s)
    norm = s.sum(axis=0)
    norm[norm <= 0] = 1
    return s / norm


def coo(res):
    r, c = np.nonzero(res)
    return np.vstack([r, c]).astype(np.int64), res[r, c].astype(np.float32)


def diffusion(adj, kernel="heat", param=5.0, top_k=3, eps=None):
    """-> (edge_index [2,E], edge_attr [E] f32) of one graph."""
    s = diffusion_matrix(adj, kernel, param)
    return coo(OG.top_k_matrix(s, top_k) if eps is None else clipped_matrix(s, eps))


def diffusion_batch(adjs, kernel="heat", param=5.0, top_k=3, eps=None):
    """-> (edge_index [2,E] with graph g offset by g*R, edge_attr [E], edge_ptr [B+1])."""
    eis, ews, ptr, off = [], [], [0], 0
    for a in adjs:
        ei, ew = diffusion(a, kernel, param, top_k, eps)
        eis.append(ei + off)
        ews.append(ew)
        off += a.shape[0]
        ptr.append(ptr[-1] + ei.shape[1])
    return np.concatenate(eis, axis=1), np.concatenate(ews), np.asarray(ptr, dtype=np.int64)


def margins(s, k=None, eps=None):
    """How far the decisions on S are from flipping: (smallest relative gap between the k-th and the (k+1)-th largest
    entry of a column, smallest relative distance of an entry to eps); inf where the question does not arise."""
    s = np.asarray(s, dtype=np.float64)
    gap_k = gap_e = np.inf
    if k is not None and k < s.shape[0]:
        v = -np.sort(-s, axis=0)
        gap_k = float(np.min((v[k - 1] - v[k]) / np.abs(v[k - 1])))
    if eps is not None:
        gap_e = float(np.min(np.abs(s - eps)) / abs(eps))
    return gap_k, gap_e


def synthetic_adjacency(rng, rois, knn=5):
    """Symmetric non-negative connectivity with a connected kNN support (as tests/golden/make_golden.py's)."""
    s = rng.random((rois, rois))
    s = (s + s.T) / 2
    np.fill_diagonal(s, 0.0)
    nbr = np.argsort(-s, axis=1)[:, :knn]
    a = np.zeros((rois, rois))
    rows = np.repeat(np.arange(rois), knn)
    a[rows, nbr.ravel()] = s[rows, nbr.ravel()]
    return np.maximum(a, a.T)


# ---- the cases of tests/golden/gdc_heat.npz ----------------------------------------------------------------
N_TOPK, N_THRESHOLD = 6, 4
MARGIN = 1e-8          # a condition on the INPUTS: a correct fp64 kernel errs near 1e-14, so no decision may flip


def topk_cases(store):
    for c in range(N_TOPK):
        rois, k, _ = [int(v) for v in store[f"topk{c}/cfg"]]
        yield c, rois, k, float(store[f"topk{c}/t"]), store[f"topk{c}/A"], store[f"topk{c}/edge_index"], \
            store[f"topk{c}/edge_attr"]


def threshold_cases(store):
    for c in range(N_THRESHOLD):
        src, kernel, empty = [int(v) for v in store[f"thr{c}/cfg"]]
        yield c, ("ppr", "heat")[kernel], float(store[f"thr{c}/param"]), float(store[f"thr{c}/eps"]), empty, \
            store[f"topk{src}/A"], store[f"thr{c}/edge_index"], store[f"thr{c}/edge_attr"]
