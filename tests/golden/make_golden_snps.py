#!/usr/bin/env python3
"""Generate tests/golden/snps_only.npz by EXECUTING THE REFERENCE's kernel/go_model.py (read-only), its ``classification``
module included.

Run in the build container only:  python tests/golden/make_golden_snps.py
The GPU box never has the reference; it only sees the committed .npz file.

The reference is loaded as make_golden.py loads it (same module substitutions, seeded weights, dropout off).  Its trainer
module kernel/train_eval_snps.py imports the absent data stack, so the batch body of train() (:314-320: criterion_class =
BCELoss(reduction='none'), criterion_recon = MSELoss(reduction='none'), lambda0 = 1e-5 of :169) is restated below on top
of the model's own ``forward`` and ``classification``; as shipped :314 unpacks three values from forward's four-tuple and
raises — the first two are taken.  Adam is torch.optim.Adam(lr=1e-3, weight_decay=0).

Configurations of Gene_ontology_network(A_g, A, 2, 2, [5, 5], pool_dim, l_dim, 'cpu') (tests/snps_ref.py: CONFIGS):
  main20   the shape of go_model.py's __main__: 20 GO nodes, pool (3, 6, 11), l_dim 5, B = 30, on a seeded DAG
  b32      synth.go_hierarchy((300, 120, 60, 19, 1)), l_dim 32, B = 32
Inputs: seeded integers in {0, 1, 2} as floats; labels: seeded Bernoulli(0.5).  Per configuration: ``eval`` (eval mode) and
``train`` (training mode) with the outputs (latent, x_hat, y_hat), the loss and both terms and all parameter gradients (``no_grad``: the
parameters the loss does not reach — the attention read-out, whose output this trainer drops);
``step``: the parameters and BatchNorm buffers after one Adam step of the training-mode loss; the sorted state_dict keys.
Groups are stored as make_golden_clusterlabel.py stores them (``clusterlabel_ref.group`` reads them).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (adds the repository and this folder to sys.path)
import make_golden_clusterlabel as MC  # noqa: E402  (its group packing; sets MG.BIG = 256)
import snps_ref as REF  # noqa: E402
from igcn_amd import synth  # noqa: E402
from _weights import seeded_state  # noqa: E402

LAMBDA0 = 1e-5


def reference_losses(model, data, label, lambda0=LAMBDA0):
    """train() :314-320 on the reference model's own methods."""
    latent, x_hat = model(data, torch.tensor(0.1), "cpu")[:2]
    y_hat = model.classification(torch.cat((latent, data), -1))
    class_loss = torch.sum(torch.nn.BCELoss(reduction="none")(y_hat.view(-1), label.view(-1)))
    recon_loss = lambda0 * torch.sum(torch.nn.MSELoss(reduction="none")(x_hat, data))
    return class_loss + recon_loss, {"class": class_loss, "recon": recon_loss}, (latent, x_hat, y_hat.view(-1))


def capture(go_mod, tag, store):
    c = REF.CONFIGS[tag]
    go_snps, adj, pool_dim = REF.hierarchy(tag)
    a_g, a = synth.go_sparse_inputs(go_snps, adj)
    torch.manual_seed(c["seed"])
    model = go_mod.Gene_ontology_network(a_g, a, 2, 2, [5, 5], pool_dim, c["l_dim"], "cpu")
    ref_sd = model.state_dict()
    sd = seeded_state({k: v.shape for k, v in ref_sd.items()}, c["seed"], ref_sd)
    store[f"{tag}/cfg"] = np.array([c["seed"], c["l_dim"], c["bsz"]] + list(c["pool"]))
    store[f"{tag}/state_keys"] = np.array(sorted(ref_sd))
    for mode in ("eval", "train"):
        model.load_state_dict(sd)
        model.train(mode == "train")
        MG._no_dropout(model)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0)
        opt.zero_grad()
        data, label = REF.inputs(tag, mode)
        if sorted(set(label.tolist())) != [0.0, 1.0]:
            raise SystemExit(f"{tag}/{mode}: the batch must hold both labels")
        loss, terms, outs = reference_losses(model, data, label)
        loss.backward()
        grads = {k: p.grad for k, p in model.named_parameters()}
        # (atten_out feeds nothing in this trainer: the conc_for_attention parameters are the ones left without)
        store[f"{tag}/{mode}/no_grad"] = np.array(sorted(k for k, g in grads.items() if g is None))
        MC._pack(f"{tag}/{mode}/out", dict(zip(("latent", "x_hat", "y_hat"), outs)), store)
        MC._pack(f"{tag}/{mode}/grad", grads, store)
        store[f"{tag}/{mode}/loss"] = np.array(float(loss))
        for k, v in terms.items():
            store[f"{tag}/{mode}/term/{k}"] = np.array(float(v))
        if mode == "train":
            opt.step()
            MC._pack(f"{tag}/step/param_after", dict(model.named_parameters()), store)
            MC._pack(f"{tag}/step/buffers_after", {k: v for k, v in model.state_dict().items() if "running" in k}, store)
        print("wrote", tag, mode, "loss", float(loss), {k: float(v) for k, v in terms.items()})


def main():
    go_mod, _ = MG._load_reference()
    store = {"meta": np.array(
        "reference kernel/go_model.py (forward + classification) executed on CPU; torch_scatter.scatter -> index_add_; "
        f"dropout p=0; torch {torch.__version__}; weights = seeded_state(shapes, seed); GO = synth.go_hierarchy(pool, "
        "seed=seed); data = integers in {0,1,2}, label = Bernoulli(0.5), default_rng(seed+10 train / seed+11 eval); loss = "
        f"train() kernel/train_eval_snps.py:314-320, lambda0={LAMBDA0}"),
        "lambda0": np.array(LAMBDA0)}
    for tag in REF.CONFIGS:
        capture(go_mod, tag, store)
    path = os.path.join(HERE, "snps_only.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print("snps_only.npz:", size, "bytes")
    if size > os.path.getsize(os.path.join(HERE, "clusterlabel.npz")):
        raise SystemExit("snps_only.npz is larger than clusterlabel.npz")


if __name__ == "__main__":
    main()
