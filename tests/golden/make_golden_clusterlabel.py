#!/usr/bin/env python3
"""Generate tests/golden/clusterlabel.npz by EXECUTING THE REFERENCE's kernel/sgcn_img_snp_clusterlabel.py (read-only).

Run in the build container only:  python tests/golden/make_golden_clusterlabel.py
The GPU box never has the reference; it only sees the committed .npz file.

The reference is loaded as make_golden.py loads it (same module substitutions, seeded weights, dropout off).  Its trainer
module imports the absent data stack, so the six-term combination of train()
(kernel/train_eval_sgcn_clusterlabel.py:375-393; criterion_recon = MSELoss(reduction='none'), lambda0 = 1e-5 of :188,
lambda1 = 0 of :191 — the per-cluster consist_loss is weighted by it and never added) is restated below on top of the
model's own ``forward`` and ``loss_probability``; Adam is torch.optim.Adam(lr=1e-3, weight_decay=0).

Configurations of SGCN_GCN_CLUSTERLABEL(2, 16, ..., isCrossAtten=True) on the (300, 120, 60, 19, 1) DAG, 90 ROIs:
  h0_1       the reference's defaults (H_0 = num_features = 1, 3 classes, 2 clusters)
  h0_3       H_0 = num_features = 3 — only here does the ``* H_0`` normalisation of loss_probability differ from the
             headline model's mean
  nopredict  isPredictCluster=False
Per configuration: ``eval`` (B = 4, eval mode) and ``train`` (B = 32, training mode), each with the outputs of both
isExplain modes and the gradients of a seeded probe of them; ``step``: one train() iteration on the B = 32 batch (loss, six
terms, gradients, the parameters after one Adam step, the BatchNorm buffers); the sorted state_dict keys and shapes.
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
from igcn_amd import synth  # noqa: E402
from igcn_amd.data import Batch  # noqa: E402
from oracle import sgcn_img_snp as OS  # noqa: E402
from _weights import seeded_state  # noqa: E402

LAMBDA0 = 1e-5
POOL, ROIS, LAYERS, HIDDEN, L_DIM = (300, 120, 60, 19, 1), 90, 2, 16, 32
CONFIGS = {"h0_1": dict(seed=81, h0=1, predict=True),
           "h0_3": dict(seed=82, h0=3, predict=True),
           "nopredict": dict(seed=83, h0=1, predict=False)}
SIZES = {"eval": 4, "train": 32}
NAMES = ("logp", "logp_cluster", "x_hat", "out_z")
# three configurations x (four probed groups + a step) of ~70 tensors each — 1500 archive members, whose headers alone
# would pass the size limit: a group goes through ``MG._pack`` (summaries for what is large; here: more than 256 elements,
# the GO network's own tensors being pinned in full by go_b32 / full_b32) and is then stored as FOUR members — names,
# sizes, the values back to back, the summaries stacked (``clusterlabel_ref.group`` restores ``golden_group``'s dict)
MG.BIG = 256


def _pack(prefix, tensors, store):
    tmp = {}
    MG._pack("g", tensors, tmp)
    full = {k[2:]: v for k, v in tmp.items() if not k.endswith("#summary")}
    summ = {k[2:-8]: v for k, v in tmp.items() if k.endswith("#summary")}
    store[prefix + "#names"] = np.array(list(full) + list(summ))
    store[prefix + "#shapes"] = np.array([",".join(str(d) for d in v.shape) for v in full.values()] + [""] * len(summ))
    store[prefix + "#values"] = (np.concatenate([np.asarray(v, dtype=np.float32).reshape(-1) for v in full.values()])
                                 if full else np.zeros(0, np.float32))
    store[prefix + "#summaries"] = (np.stack([np.asarray(v) for v in summ.values()]) if summ else np.zeros((0, 3)))


def load_clusterlabel():
    MG._load_reference()
    spec = importlib.util.spec_from_file_location("kernel.sgcn_img_snp_clusterlabel",
                                                  os.path.join(MG.REF, "kernel/sgcn_img_snp_clusterlabel.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_losses(model, data, hp, o1, o2, predict, lambda0=LAMBDA0):
    """train() :375-393 on the reference model's own methods."""
    out, out_cluster, snps_hat, _ = o1
    out_prob, out_cluster_prob, snps_hat_prob, _ = o2
    mse = torch.nn.MSELoss(reduction="none")
    t = {"ce": F.nll_loss(out, data.y.view(-1)), "ce_cluster": F.nll_loss(out_cluster, data.clust_y.view(-1)),
         "mi": F.nll_loss(out_prob, data.y.view(-1)), "mi_cluster": F.nll_loss(out_cluster_prob, data.clust_y.view(-1)),
         "prob": model.loss_probability(data.x, data.edge_index, data.edge_attr, hp),
         "recon": (lambda0 * torch.sum(mse(snps_hat, data.snps_feat))
                   + lambda0 * torch.sum(mse(snps_hat_prob, data.snps_feat))) / 2}
    if predict:
        loss = hp.lamda_ce * (t["ce"] + t["ce_cluster"]) / 2 + hp.lamda_mi * (t["mi"] + t["mi_cluster"]) / 2 \
            + t["prob"] + t["recon"]
    else:
        loss = hp.lamda_ce * t["ce"] + hp.lamda_mi * t["mi"] + t["prob"] + t["recon"]
    return loss, t


def graphs_of(tag, mode, seed, h0):
    return synth.brain_graph_list(SIZES[mode], seed=seed + (10 if mode == "train" else 11), rois=ROIS, h0=h0, top_k=3,
                                  tsne_dim=16)


def capture(mod, tag, cfg, store):
    seed, h0, predict = cfg["seed"], cfg["h0"], cfg["predict"]
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj)
    torch.manual_seed(seed)
    model = mod.SGCN_GCN_CLUSTERLABEL(LAYERS, HIDDEN, a_g, a, pool_dim, L_DIM, "cpu", H_0=h0, num_features=h0,
                                      isCrossAtten=True, isPredictCluster=predict)
    ref_sd = model.state_dict()
    sd = seeded_state({k: v.shape for k, v in ref_sd.items()}, seed, ref_sd)
    keys = sorted(ref_sd)
    store[f"{tag}/cfg"] = np.array([seed, h0, int(predict)])
    store[f"{tag}/state_keys"] = np.array(keys)
    store[f"{tag}/state_shapes"] = np.array([",".join(str(d) for d in ref_sd[k].shape) for k in keys])
    big = Batch.from_data_list(graphs_of(tag, "train", seed, h0))
    if sorted(set(big.clust_y.view(-1).tolist())) != [0, 1] or sorted(set(big.y.view(-1).tolist())) != [0, 1, 2]:
        raise SystemExit(f"{tag}: the B = {SIZES['train']} batch must hold both cluster labels and all three classes")
    for mode in ("eval", "train"):
        for explain in (False, True):
            model.load_state_dict(sd)
            model.train(mode == "train")
            MG._no_dropout(model)
            model.zero_grad()
            data = Batch.from_data_list(graphs_of(tag, mode, seed, h0))
            outs = model(data, torch.tensor(0.1), "cpu", isExplain=explain)
            cot = MG._probe_weights(outs, seed + 3)
            sum((o * c).sum() for o, c in zip(outs, cot)).backward()
            grp = f"{tag}/{mode}/explain{int(explain)}"
            _pack(grp + "/out", dict(zip(NAMES, outs)), store)
            _pack(grp + "/grad", {"data.x": data.x.grad, **{k: p.grad for k, p in model.named_parameters()}}, store)
    # one optimisation step (training mode, dropout off)
    model.load_state_dict(sd)
    model.train(True)
    MG._no_dropout(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0)
    opt.zero_grad()
    data = Batch.from_data_list(graphs_of(tag, "train", seed, h0))
    o1 = model(data, torch.tensor(0.1), "cpu")
    o2 = model(data, torch.tensor(0.1), "cpu", isExplain=True)
    loss, terms = reference_losses(model, data, OS.HP, o1, o2, predict)
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    _pack(f"{tag}/step/grad", {"data.x": data.x.grad, **grads}, store)
    store[f"{tag}/step/no_grad"] = np.array(sorted(k for k, g in grads.items() if g is None))
    opt.step()
    store[f"{tag}/step/loss"] = np.array(float(loss))
    for k, v in terms.items():
        store[f"{tag}/step/term/{k}"] = np.array(float(v))
    _pack(f"{tag}/step/param_after", dict(model.named_parameters()), store)
    _pack(f"{tag}/step/buffers_after", {k: v for k, v in model.state_dict().items() if "running" in k}, store)
    print("wrote", tag, "loss", float(loss), {k: float(v) for k, v in terms.items()})


def main():
    mod = load_clusterlabel()
    store = {"meta": np.array(
        "reference kernel/sgcn_img_snp_clusterlabel.py + kernel/go_model.py executed on CPU; GCNConv/to_dense_batch = "
        "oracle.pyg_ops (PyG 2.0.2 absent: unpinned), torch_scatter.scatter -> index_add_; dropout p=0; "
        f"torch {torch.__version__}; weights = seeded_state(shapes, seed); graphs = synth.brain_graph_list(B, "
        f"seed=seed+10 (B=32) / seed+11 (B=4), rois={ROIS}, h0=H_0, top_k=3, tsne_dim=16); GO = synth.go_hierarchy("
        f"{list(POOL)}, seed=seed); loss = train() kernel/train_eval_sgcn_clusterlabel.py:375-393, lambda0={LAMBDA0}"),
        "pool": np.array(POOL), "lambda0": np.array(LAMBDA0), "dims": np.array([ROIS, LAYERS, HIDDEN, L_DIM])}
    for tag, cfg in CONFIGS.items():
        capture(mod, tag, cfg, store)
    path = os.path.join(HERE, "clusterlabel.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("clusterlabel.npz:", size, "bytes")
    if size > 300 * 1024:
        raise SystemExit("clusterlabel.npz is over 300 KB")


if __name__ == "__main__":
    main()
