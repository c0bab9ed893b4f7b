#!/usr/bin/env python3
"""Generate tests/golden/sgcn_gat.npz by EXECUTING THE REFERENCE's kernel/sgcn.py SGCN_GAT (read-only).

Run in the build container only:  python tests/golden/make_golden_sgcn_gat.py
The GPU box never has the reference; it only sees the committed .npz file.

The reference is loaded as make_golden.py loads it (same module substitutions, its helpers imported, not edited), plus:
  torch_geometric.nn.GATConv -> gat_standin.GATConvModule   (PyG 2.0.2 GATConv restated from its source: UNPINNED)
which the fixture's ``meta`` states.  Two configurations of SGCN_GAT — ``l2h16`` (L = 2, hidden 16) and ``l3h10`` (L = 3,
hidden 10) — on B = 4 graphs of 90 ROIs (the batch shape of sgcn_only.npz; top_k = 3 stores one self-loop per node, which
GATConv drops and replaces by a mean-valued loop), seeded weights, dropout off.  Per configuration:
  {eval, train}/explain{0, 1}/{out, grad}   log_softmax and every gradient of a probed sum (``data.x`` included);
  step/...                                  train() of kernel/train_eval_sgcn.py:303-308: loss, the three terms, every
                                            gradient, the parameters after one Adam step (lr = 1e-3);
  mi_only/grad                              the gradients of ``hp.lamda_mi * mi`` alone — the masked pass, whose edge
                                            attribute edge_weight * edge_prob is the only path into ``prob_bias``;
  state_keys                                the sorted state_dict keys.
"""
import importlib.util
import os
import sys
from types import SimpleNamespace

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

CONFIGS = {"l2h16": dict(layers=2, hidden=16, seed=71), "l3h10": dict(layers=3, hidden=10, seed=72)}
BSZ, ROIS, TOP_K = 4, 90, 3
DATASET = SimpleNamespace(num_features=3, num_classes=2)


def load_sgcn():
    MG._load_reference()
    sys.modules["torch_geometric.nn"].GATConv = GATConvModule
    spec = importlib.util.spec_from_file_location("kernel.sgcn", os.path.join(MG.REF, "kernel/sgcn.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["kernel.sgcn"] = mod
    spec.loader.exec_module(mod)
    return mod


def _grads(model, data):
    return {"data.x": data.x.grad, **{k: p.grad for k, p in model.named_parameters()}}


def capture(mod, name):
    hp = MG.OS.HP
    store = {"meta": np.array(
        "reference kernel/sgcn.py SGCN_GAT executed on CPU; " + STATED + "; to_dense_batch = oracle.pyg_ops (PyG 2.0.2 "
        f"absent: unpinned); dropout p=0; torch {torch.__version__}; weights = seeded_state(shapes, seed); "
        f"graphs = synth.brain_graph_list({BSZ}, seed=seed+10, rois={ROIS}, top_k={TOP_K}, tsne_dim=16, num_classes=2); "
        "dataset = SimpleNamespace(num_features=3, num_classes=2); step = train() kernel/train_eval_sgcn.py:303-308, "
        "Adam lr=1e-3")}
    for tag, c in CONFIGS.items():
        layers, hidden, seed = c["layers"], c["hidden"], c["seed"]
        model = mod.SGCN_GAT(DATASET, layers, hidden, rois=ROIS, H_0=3)
        ref_sd = model.state_dict()
        sd = seeded_state({k: v.shape for k, v in ref_sd.items()}, seed, ref_sd)
        graphs = synth.brain_graph_list(BSZ, seed=seed + 10, rois=ROIS, top_k=TOP_K, tsne_dim=16, num_classes=2)
        store[f"{tag}/cfg"] = np.array([ROIS, hidden, layers, BSZ, seed, TOP_K])
        store[f"{tag}/state_keys"] = np.array(sorted(ref_sd.keys()))
        for mode in ("eval", "train"):
            for explain in (False, True):
                model.load_state_dict(sd)
                model.train(mode == "train")
                MG._no_dropout(model)
                model.zero_grad()
                data = Batch.from_data_list(graphs)
                out = model(data, explain)
                cot = MG._probe_weights([out], seed + 3)[0]
                (out * cot).sum().backward()
                sub = f"{tag}/{mode}/explain{int(explain)}"
                MG._pack(sub + "/out", {"logp": out}, store)
                MG._pack(sub + "/grad", _grads(model, data), store)
        # the masked pass's term alone
        model.load_state_dict(sd)
        model.train(True)
        MG._no_dropout(model)
        model.zero_grad()
        data = Batch.from_data_list(graphs)
        (hp.lamda_mi * F.nll_loss(model(data, True), data.y.view(-1))).backward()
        MG._pack(f"{tag}/mi_only/grad", _grads(model, data), store)
        # one step of train()
        model.load_state_dict(sd)
        model.zero_grad()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0)
        opt.zero_grad()
        data = Batch.from_data_list(graphs)
        y = data.y.view(-1)
        out, out_p = model(data), model(data, True)
        terms = {"ce": F.nll_loss(out, y), "mi": F.nll_loss(out_p, y),
                 "prob": model.loss_probability(data.x, data.edge_index, data.edge_attr, hp)}
        loss = hp.lamda_ce * terms["ce"] + terms["prob"] + hp.lamda_mi * terms["mi"]
        loss.backward()
        MG._pack(f"{tag}/step/grad", _grads(model, data), store)
        opt.step()
        store[f"{tag}/step/loss"] = np.array(float(loss.detach()))
        for k, v in terms.items():
            store[f"{tag}/step/term/{k}"] = np.array(float(v.detach()))
        MG._pack(f"{tag}/step/param_after", dict(model.named_parameters()), store)
        print("wrote", name, tag, "loss", float(loss.detach()), {k: float(v.detach()) for k, v in terms.items()},
              "max|d prob_bias| (mi only)", float(np.abs(store[f"{tag}/mi_only/grad/prob_bias"]).max()))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **store)


def main():
    torch.manual_seed(0)
    capture(load_sgcn(), "sgcn_gat")


if __name__ == "__main__":
    main()
