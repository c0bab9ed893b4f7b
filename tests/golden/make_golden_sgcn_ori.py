#!/usr/bin/env python3
"""Generate tests/golden/sgcn_ori.npz by EXECUTING THE REFERENCE's kernel/sgcn.py SGCN_Ori (read-only).

Run in the build container only:  python tests/golden/make_golden_sgcn_ori.py
The GPU box never has the reference; it only sees the committed .npz file.

The reference is loaded as make_golden.py loads it (same module substitutions, its helpers imported, not edited).  Two
configurations of SGCN_Ori(H_0, H_1, H_2, H_3) — ``h32_5`` = (3, 32, 32, 5), the reference's hyper-parameters
(sgcn_hyperparameters.py:8-11), and ``h16_8`` = (3, 16, 16, 8) — on graphs of 90 ROIs (top_k = 3), seeded weights, dropout
off.  Evaluation-mode groups use B = 4; training-mode and step groups B = 32 (BatchNorm over 4 rows amplifies fp32
rounding).  Per configuration:
  {eval, train}/explain{0, 1}/{out, grad, cam}   log_softmax; every gradient of a probed sum (``data.x`` included);
                                                 final_conv_acts / final_conv_grads and the share of negative acts;
  step/...                                       train() of kernel/train_eval_sgcn.py:303-308: loss, the three terms, every
                                                 gradient, the parameters after one Adam step (lr = 1e-3), the BatchNorm
                                                 buffers, and the Grad-CAM attributes the two calls leave;
  state_keys, state_shapes                       the state_dict's sorted keys and their shapes.
The Grad-CAM tap is only exercised when final_conv_acts has both signs: the script refuses to write unless between 20 %
and 80 % of it is negative in every pass.
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
from _weights import seeded_state  # noqa: E402

CONFIGS = {"h32_5": dict(dims=(3, 32, 32, 5), seed=6), "h16_8": dict(dims=(3, 16, 16, 8), seed=7)}
ROIS, TOP_K, B_EVAL, B_TRAIN = 90, 3, 4, 32
NEG_LO, NEG_HI = 0.2, 0.8


def load_sgcn():
    MG._load_reference()
    spec = importlib.util.spec_from_file_location("kernel.sgcn", os.path.join(MG.REF, "kernel/sgcn.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["kernel.sgcn"] = mod
    spec.loader.exec_module(mod)
    return mod


def _grads(model, data):
    return {"data.x": data.x.grad, **{k: p.grad for k, p in model.named_parameters()}}


def _neg_frac(acts, where):
    frac = float((acts.detach() < 0).double().mean())
    if not NEG_LO <= frac <= NEG_HI:
        raise SystemExit(f"{where}: {100 * frac:.1f} % of final_conv_acts is negative (need {100 * NEG_LO:.0f}-"
                         f"{100 * NEG_HI:.0f} %): the tap would not be tested; nothing written")
    return frac


def _graphs(bsz, seed):
    return synth.brain_graph_list(bsz, seed=seed + 10, rois=ROIS, top_k=TOP_K, tsne_dim=16, num_classes=2)


def capture(mod, name):
    hp = MG.OS.HP
    store = {"meta": np.array(
        "reference kernel/sgcn.py SGCN_Ori executed on CPU; GCNConv / to_dense_batch = oracle.pyg_ops (PyG 2.0.2 absent: "
        f"unpinned); dropout p=0; torch {torch.__version__}; weights = seeded_state(shapes, seed); graphs = "
        f"synth.brain_graph_list(B, seed=seed+10, rois={ROIS}, top_k={TOP_K}, tsne_dim=16, num_classes=2), B = {B_EVAL} "
        f"(eval groups) / {B_TRAIN} (train and step groups); step = train() kernel/train_eval_sgcn.py:303-308, Adam "
        "lr=1e-3; after the step's two calls final_conv_acts is the masked pass's and final_conv_grads the plain pass's")}
    for tag, c in CONFIGS.items():
        dims, seed = c["dims"], c["seed"]
        model = mod.SGCN_Ori(*dims, rois=ROIS)
        ref_sd = model.state_dict()
        sd = seeded_state({k: v.shape for k, v in ref_sd.items()}, seed, ref_sd)
        store[f"{tag}/cfg"] = np.array([ROIS, *dims, B_EVAL, B_TRAIN, seed, TOP_K])
        store[f"{tag}/state_keys"] = np.array(sorted(ref_sd.keys()))
        store[f"{tag}/state_shapes"] = np.array([",".join(str(d) for d in ref_sd[k].shape) for k in sorted(ref_sd)])
        fracs = {}
        for mode, bsz in (("eval", B_EVAL), ("train", B_TRAIN)):
            graphs = _graphs(bsz, seed)
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
                fracs[sub] = _neg_frac(model.final_conv_acts, sub)
                store[sub + "/cam/neg_frac"] = np.array(fracs[sub])
                MG._pack(sub + "/out", {"logp": out}, store)
                MG._pack(sub + "/grad", _grads(model, data), store)
                MG._pack(sub + "/cam", {"final_conv_acts": model.final_conv_acts,
                                        "final_conv_grads": model.final_conv_grads}, store)
        # one step of train()
        model.load_state_dict(sd)
        model.train(True)
        MG._no_dropout(model)
        model.zero_grad()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0)
        opt.zero_grad()
        data = Batch.from_data_list(_graphs(B_TRAIN, seed))
        y = data.y.view(-1)
        out = model(data)
        acts_plain = model.final_conv_acts
        out_p = model(data, True)
        terms = {"ce": F.nll_loss(out, y), "mi": F.nll_loss(out_p, y),
                 "prob": model.loss_probability(data.x, data.edge_index, data.edge_attr, hp)}
        loss = hp.lamda_ce * terms["ce"] + terms["prob"] + hp.lamda_mi * terms["mi"]
        loss.backward()
        fracs[f"{tag}/step/plain"] = _neg_frac(acts_plain, f"{tag}/step plain")
        fracs[f"{tag}/step/masked"] = _neg_frac(model.final_conv_acts, f"{tag}/step masked")
        store[f"{tag}/step/cam/neg_frac"] = np.array([fracs[f"{tag}/step/plain"], fracs[f"{tag}/step/masked"]])
        MG._pack(f"{tag}/step/out", {"logp": out, "logp_p": out_p}, store)
        MG._pack(f"{tag}/step/grad", _grads(model, data), store)
        MG._pack(f"{tag}/step/cam", {"final_conv_acts": model.final_conv_acts,
                                     "final_conv_grads": model.final_conv_grads}, store)
        opt.step()
        store[f"{tag}/step/loss"] = np.array(float(loss.detach()))
        for k, v in terms.items():
            store[f"{tag}/step/term/{k}"] = np.array(float(v.detach()))
        MG._pack(f"{tag}/step/param_after", dict(model.named_parameters()), store)
        MG._pack(f"{tag}/step/buffers", dict(model.named_buffers()), store)
        print("wrote", name, tag, "loss", float(loss.detach()), {k: float(v.detach()) for k, v in terms.items()},
              "negative share of final_conv_acts", {k: round(v, 3) for k, v in fracs.items()})
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **store)


def main():
    torch.manual_seed(0)
    capture(load_sgcn(), "sgcn_ori")


if __name__ == "__main__":
    main()
