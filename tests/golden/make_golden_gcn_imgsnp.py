#!/usr/bin/env python3
"""Generate tests/golden/gcn_imgsnp_{gcn,gat}.npz by EXECUTING THE REFERENCE's kernel/gcn_img_snp.py (read-only).

Run in the build container only:  python tests/golden/make_golden_gcn_imgsnp.py
The GPU box never has the reference; it only sees the committed .npz files.

The reference is loaded as make_golden.py loads it (same module substitutions, its helpers imported, not edited), plus:
  torch_geometric.nn.GATConv -> gat_standin.GATConvModule   (PyG 2.0.2 GATConv restated from its source: UNPINNED)
which every fixture's ``meta`` states.  Each fixture holds two configurations of GCN_IMGSNP (B = 32, R = 90,
cross-attention on, isuseFeat4Regr on, seeded weights, dropout off, training mode): ``l2h16`` (L = 2, hidden 16) and
``l3h10`` (L = 3, hidden 10).  Per configuration: the forward 6-tuple, the five loss terms of train()
(kernel/train_eval_gcn_img_snps.py:450-484, restated below on the model's own methods) and every parameter gradient of
their sum at the trainer's default lambda (main.py:73-78), the terms at a second lambda whose ``ce`` / ``orth`` weights are
non-zero, and the sorted state_dict keys.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (adds the repository and this folder to sys.path)
from gat_standin import STATED, GATConvModule  # noqa: E402
from igcn_amd import synth  # noqa: E402
from igcn_amd.data import Batch  # noqa: E402
from _weights import seeded_state  # noqa: E402

LAM_DEFAULT = [0.0, 1.0, 0.5, 1.5e-6, 0.1, 0.0]        # main.py:73-78
LAM_ALT = [1.0, 1.0, 0.5, 1.5e-6, 0.1, 0.2]
LAMDA_CE = 1.0                                          # sgcn_hyperparameters.py: hp.lamda_ce
CONFIGS = {"l2h16": dict(layers=2, hidden=16, seed=61), "l3h10": dict(layers=3, hidden=10, seed=62)}
BSZ, ROIS, POOL = 32, 90, (300, 120, 60, 19, 1)


def load_gcn_img_snp():
    MG._load_reference()
    sys.modules["torch_geometric.nn"].GATConv = GATConvModule
    spec = importlib.util.spec_from_file_location("kernel.gcn_img_snp", os.path.join(MG.REF, "kernel/gcn_img_snp.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["kernel.gcn_img_snp"] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_losses(model, data, lam, outs):
    """train() :455-479 on the reference model's own methods (isSoftSimilarity=True)."""
    out, snps_hat, out_feat, _, _, reg = outs
    mse = torch.nn.MSELoss(reduction="none")
    t = {"ce": lam[0] * F.nll_loss(out, data.y.view(-1)),
         "reg": lam[1] * F.mse_loss(reg.view(-1), data.clini_score.view(-1)),
         "recon": lam[3] * torch.sum(mse(snps_hat, data.snps_feat)),
         "cluster": lam[4] * model.consist_loss(out_feat, data.tsne_fdim),
         "orth": lam[5] * model.OrthogonalConstraint(out_feat)}
    if lam[0] == 0:
        t["ce"], t["orth"] = 0.0, 0.0
    loss = LAMDA_CE * t["ce"] + t["reg"] + t["recon"] + t["cluster"] + t["orth"]
    return loss, t


def capture(mod, name, gat):
    store = {"meta": np.array(
        "reference kernel/gcn_img_snp.py + kernel/go_model.py executed on CPU; " + (STATED + "; " if gat else "")
        + "GCNConv/to_dense_batch = oracle.pyg_ops (PyG 2.0.2 absent: unpinned), torch_scatter.scatter -> index_add_; "
        f"dropout p=0; training mode; torch {torch.__version__}; weights = seeded_state(shapes, seed); "
        f"graphs = synth.brain_graph_list({BSZ}, seed=seed+10, rois={ROIS}, top_k=3, tsne_dim=16); "
        f"GO = synth.go_hierarchy({list(POOL)}, seed=seed); loss = train() kernel/train_eval_gcn_img_snps.py:450-484"),
        "gat": np.array(int(gat)), "pool": np.array(POOL), "lam": np.array(LAM_DEFAULT),
        "lam_alt": np.array(LAM_ALT)}
    for tag, c in CONFIGS.items():
        layers, hidden, seed = c["layers"], c["hidden"], c["seed"]
        go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=seed)
        a_g, a = synth.go_sparse_inputs(go_snps, adj)
        torch.manual_seed(seed)
        model = mod.GCN_IMGSNP(layers, hidden, a_g, a, pool_dim, 32, "cpu", rois=ROIS, H_0=3, num_classes=3,
                               isSoftSimilarity=True, rbf_gamma=0.01, isCrossAtten=True, num_regr=3,
                               model4eachregr=False, isuseFeat4Regr=True, isImageOnly=False, isSNPsOnly=False,
                               ifUseGAT=gat)
        ref_sd = model.state_dict()
        sd = seeded_state({k: v.shape for k, v in ref_sd.items()}, seed, ref_sd)
        graphs = synth.brain_graph_list(BSZ, seed=seed + 10, rois=ROIS, top_k=3, tsne_dim=16)
        store[f"{tag}/cfg"] = np.array([ROIS, hidden, layers, BSZ, seed, 3])
        store[f"{tag}/state_keys"] = np.array(sorted(ref_sd.keys()))
        for lam, sub in ((LAM_ALT, "alt"), (LAM_DEFAULT, "step")):
            model.load_state_dict(sd)
            model.train(True)
            MG._no_dropout(model)
            model.zero_grad()
            data = Batch.from_data_list(graphs)
            outs = model(data, torch.tensor(0.1), "cpu")
            loss, terms = reference_losses(model, data, lam, outs)
            store[f"{tag}/{sub}/loss"] = np.array(float(loss))
            for k, v in terms.items():
                store[f"{tag}/{sub}/term/{k}"] = np.array(float(v))
            if sub == "step":
                MG._pack(f"{tag}/out", dict(zip(["logp", "x_hat", "out_z", "out_lin", "lin_f", "reg"], outs)), store)
                loss.backward()
                MG._pack(f"{tag}/step/grad",
                         {"data.x": data.x.grad, **{k: p.grad for k, p in model.named_parameters()}}, store)
        print("wrote", name, tag, "loss", float(loss), {k: float(v) for k, v in terms.items()})
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **store)


def main():
    torch.manual_seed(0)
    mod = load_gcn_img_snp()
    want = set(sys.argv[1:])
    for name, gat in (("gcn_imgsnp_gcn", False), ("gcn_imgsnp_gat", True)):
        if name in want or not want:
            capture(mod, name, gat)


if __name__ == "__main__":
    main()
