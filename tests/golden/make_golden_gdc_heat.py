"""Regenerates tests/golden/gdc_heat.npz: the reference's own util_gdc.py functions (get_heat_matrix, get_ppr_matrix,
get_top_k_matrix, get_clipped_matrix) and scipy's coo_matrix, executed on CPU (numpy float64) on seeded adjacencies —
the heat-kernel and threshold halves of the pre-transform, next to gdc.npz (make_golden.py::capture_gdc) for PPR top-k.

    python tests/golden/make_golden_gdc_heat.py

The reference functions write into their argument, so each call gets a copy.  Arrays only.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gdc_heat_ref import margins, synthetic_adjacency  # noqa: E402

SEED = 78
# (R, k, t, knn); knn None: dense and NOT symmetric
TOPK_CASES = [(90, 3, 5.0, 5), (90, 5, 5.0, 8), (12, 3, 5.0, 3), (33, 2, 1.0, None), (96, 4, 5.0, 9), (90, 3, 10.0, 5)]
# (matrix of top-k case, kernel 0 = PPR | 1 = heat, alpha | t, eps); eps None: chosen so that some column keeps nothing
THRESHOLD_CASES = [(0, 1, 5.0, 0.01), (3, 1, 1.0, 0.01), (0, 0, 0.05, 1e-4), (2, 1, 5.0, None)]


def _reference():
    tg = types.ModuleType("torch_geometric")
    tgd = types.ModuleType("torch_geometric.data")
    tgd.Data, tgd.InMemoryDataset = object, object
    tg.data = tgd
    sys.modules.setdefault("torch_geometric", tg)
    sys.modules["torch_geometric.data"] = tgd
    spec = importlib.util.spec_from_file_location("util_gdc", os.path.join(REF, "util_gdc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _coo(res):
    from scipy.sparse import coo_matrix
    coo = coo_matrix(res)
    return np.vstack([coo.row, coo.col]).astype(np.int64), torch.from_numpy(coo.data).float().numpy()


def main():
    gdc = _reference()
    rng = np.random.default_rng(SEED)
    store, mats = {}, []
    for c, (rois, k, t, knn) in enumerate(TOPK_CASES):
        if knn is None:
            a = rng.random((rois, rois)).astype(np.float32)
        else:
            a = synthetic_adjacency(rng, rois, knn).astype(np.float32)
        mats.append(a)
        s = gdc.get_heat_matrix(a.astype(np.float64).copy(), t=t)
        print("topk case", c, (rois, k, t, knn), "margin %.3g" % margins(s, k=k)[0])
        ei, ew = _coo(gdc.get_top_k_matrix(s.copy(), k=k))
        store[f"topk{c}/cfg"] = np.array([rois, k, -1 if knn is None else knn])
        store[f"topk{c}/t"] = np.array(t)
        store[f"topk{c}/A"] = a
        store[f"topk{c}/edge_index"], store[f"topk{c}/edge_attr"] = ei, ew
    for c, (src, kernel, param, eps) in enumerate(THRESHOLD_CASES):
        a = mats[src].astype(np.float64)
        s = gdc.get_heat_matrix(a.copy(), t=param) if kernel else gdc.get_ppr_matrix(a.copy(), alpha=param)
        if eps is None:
            # between the column maxima: the columns whose largest entry lies below keep nothing
            top = np.sort(s.max(axis=0))
            eps = float(np.float32((top[1] + top[2]) / 2))
        ei, ew = _coo(gdc.get_clipped_matrix(s.copy(), eps=eps))
        empty = s.shape[0] - len(np.unique(ei[1]))
        print("threshold case", c, (src, kernel, param, eps), "margin %.3g" % margins(s, eps=eps)[1], "edges",
              ei.shape[1], "empty columns", empty)
        store[f"thr{c}/cfg"] = np.array([src, kernel, empty])
        store[f"thr{c}/param"] = np.array(param)
        store[f"thr{c}/eps"] = np.array(eps)
        store[f"thr{c}/edge_index"], store[f"thr{c}/edge_attr"] = ei, ew
    path = os.path.join(HERE, "gdc_heat.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
