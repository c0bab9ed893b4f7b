#!/usr/bin/env python3
"""Generate tests/golden/guide_imgsnp.npz by EXECUTING THE REFERENCE's kernel/guide_img_snp.py and
kernel/guide_go_model.py (read-only).

Run in the build container only:  python tests/golden/make_golden_guide.py
The GPU box never has the reference; it only sees the committed .npz file.

The reference is loaded as make_golden.py loads it (same module substitutions, its helpers imported, not edited).  Its
gate draws from torch's global generator (``F.gumbel_softmax(..., hard=True)``); during the capture that function is
replaced by torch's own formula applied to STORED noise, which the tests impose on the HIP gate
(``GUIDE_IMGSNP._gate_noise``).  Noise within 1e-3 of a hard-decision tie is moved off it, so that fp32 rounding cannot
flip a decision.  Configurations ``h16`` / ``h10`` (hidden 16 / 10) of GUIDE_IMGSNP on the (300, 120, 60, 19, 1) DAG,
B = 16 graphs of 90 ROIs, 3 classes, hidden_linear 32, seeded weights (``_weights.seeded_state``).  Per configuration:
the eval-mode outputs; then in training mode, every dropout off and the noise imposed: the outputs, the five loss terms of
train() (kernel/train_eval_guide_img_snps.py:450-487, restated below) at the trainer's default lambda, every parameter
gradient and data.x.grad of their sum, the parameters left without a gradient, the BatchNorm running statistics after
that forward, and the sorted state_dict keys with their shapes.  ``go``: the stand-alone GUIDE Gene_ontology_network
(dim_snps_atten 16) in training mode with dropout off — latent, x_D, atten_out, the running statistics, and the gradients
of sum(latent * c1) + sum(x_D * c2) for seeded cotangents c1, c2.
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

LAM = [1.0, 1.0, 2.5e-6, 0.2, 0.2]                      # kernel/train_eval_guide_img_snps.py:163-164
LAMDA_CE = 1.0                                          # sgcn_hyperparameters.py: hp.lamda_ce
PROB_REF, EPS = 0.001, 1e-10
CONFIGS = {"h16": dict(hidden=16, seed=71), "h10": dict(hidden=10, seed=72)}
GO_SEED = 73
BSZ, ROIS, H0, POOL, TAU, HL = 16, 90, 3, (300, 120, 60, 19, 1), 0.1, 32


def load_guide():
    MG._load_reference()
    mods = []
    for name, rel in (("kernel.guide_go_model", "kernel/guide_go_model.py"),
                      ("kernel.guide_img_snp", "kernel/guide_img_snp.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(MG.REF, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


class imposed_gumbel:
    """``F.gumbel_softmax`` = torch's formula (torch.nn.functional.gumbel_softmax) on ``noise`` instead of a draw."""

    def __init__(self, noise):
        self.noise = noise

    def __enter__(self):
        self.orig = F.gumbel_softmax
        noise = self.noise

        def gumbel_softmax(logits, tau=1, hard=False, eps=1e-10, dim=-1):
            y_soft = ((logits + noise.reshape(logits.shape)) / tau).softmax(dim)
            if not hard:
                return y_soft
            index = y_soft.max(dim, keepdim=True)[1]
            y_hard = torch.zeros_like(logits).scatter_(dim, index, 1.0)
            return y_hard - y_soft.detach() + y_soft
        F.gumbel_softmax = gumbel_softmax
        return self

    def __exit__(self, *exc):
        F.gumbel_softmax = self.orig
        return False


def gate_noise(bias, seed):
    """Gumbel noise [B, K, 2] whose hard decisions sit at least 1e-3 (in units of the tempered logits) from a tie."""
    rng = np.random.default_rng(seed)
    u = rng.random((BSZ, bias.shape[0], 2))
    g = -np.log(-np.log(np.clip(u, 1e-12, 1 - 1e-12)))
    logit = np.log(torch.softmax(bias.double(), 1).numpy())
    w = (logit[None] + g) / TAU
    near = np.abs(w[..., 1] - w[..., 0]) < 1e-3
    g[..., 1] += np.where(near, 0.05, 0.0)
    return g.astype(np.float32)


def reference_losses(data, outs, lam=LAM):
    """train() :455-483 on the reference model's outputs (criterion_recon = MSELoss(reduction='none'))."""
    out, snps_hat, _, _, _, reg, surrogate, prob = outs
    mse = torch.nn.MSELoss(reduction="none")
    s2 = 0.0
    for p in prob:
        rho = torch.FloatTensor([PROB_REF for _ in range(p.size()[0])])
        s1 = torch.mean(p * (torch.log(p + EPS) - torch.log(rho + EPS)))
        s2 += torch.mean((1 - p) * (torch.log(1 - p + EPS) - torch.log(1 - rho + EPS))) + s1
    t = {"ce": lam[0] * F.nll_loss(out, data.y.view(-1)),
         "reg": lam[1] * F.mse_loss(reg.view(-1), data.clini_score.view(-1)),
         "recon": lam[2] * torch.sum(mse(snps_hat, data.snps_feat)),
         "recon_img": lam[3] * torch.sum(mse(surrogate[0], surrogate[1])),
         "sparsity": lam[4] * s2}
    if lam[0] == 0:
        t["ce"] = 0.0
    loss = LAMDA_CE * t["ce"] + t["reg"] + t["recon"] + t["recon_img"] + t["sparsity"]
    return loss, t


def _named(outs):
    return {"logp": outs[0], "x_hat": outs[1], "latent": outs[2], "lin_f": outs[4], "reg": outs[5],
            "img": outs[6][0], "decoded": outs[6][1], "prob": outs[7][0]}


def _keys(prefix, sd, store):
    keys = sorted(sd)
    store[f"{prefix}/state_keys"] = np.array(keys)
    store[f"{prefix}/state_shapes"] = np.array([",".join(str(d) for d in sd[k].shape) for k in keys])


def _running(model):
    return {k: v for k, v in model.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}


def capture_model(gd, store):
    for tag, c in CONFIGS.items():
        hidden, seed = c["hidden"], c["seed"]
        go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=seed)
        a_g, a = synth.go_sparse_inputs(go_snps, adj)
        torch.manual_seed(seed)
        model = gd.GUIDE_IMGSNP(2, hidden, a_g, a, pool_dim, 32, "cpu", hidden_linear=HL, rois=ROIS, H_0=H0,
                                num_classes=3, num_regr=3)
        ref_sd = model.state_dict()
        sd = seeded_state({k: v.shape for k, v in ref_sd.items()}, seed, ref_sd)
        graphs = synth.brain_graph_list(BSZ, seed=seed + 10, rois=ROIS, top_k=3, tsne_dim=16)
        noise = gate_noise(sd["bias_n.0"], seed + 20)
        store[f"{tag}/cfg"] = np.array([ROIS, hidden, BSZ, seed, 3, HL])
        store[f"{tag}/noise"] = noise
        _keys(tag, ref_sd, store)
        model.load_state_dict(sd)
        model.eval()
        with torch.no_grad():
            outs = model(Batch.from_data_list(graphs), torch.tensor(TAU), "cpu")
        MG._pack(f"{tag}/eval", _named(outs), store)
        model.load_state_dict(sd)
        model.train(True)
        MG._no_dropout(model)
        model.zero_grad()
        data = Batch.from_data_list(graphs)
        with imposed_gumbel(torch.from_numpy(noise)):
            outs = model(data, torch.tensor(TAU), "cpu")
        MG._pack(f"{tag}/train", _named(outs), store)
        MG._pack(f"{tag}/running", _running(model), store)
        loss, terms = reference_losses(data, outs)
        store[f"{tag}/loss"] = np.array(float(loss))
        for k, v in terms.items():
            store[f"{tag}/term/{k}"] = np.array(float(v))
        loss.backward()
        grads = {k: p.grad for k, p in model.named_parameters()}
        MG._pack(f"{tag}/grad", {"data.x": data.x.grad, **grads}, store)
        store[f"{tag}/no_grad"] = np.array(sorted(k for k, g in grads.items() if g is None))
        print("wrote", tag, "loss", float(loss), {k: float(v) for k, v in terms.items()})


def capture_go(gm, store):
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=GO_SEED)
    a_g, a = synth.go_sparse_inputs(go_snps, adj)
    torch.manual_seed(GO_SEED)
    net = gm.Gene_ontology_network(a_g, a, 2, 2, [5, 5], pool_dim, 32, "cpu", dim_snps_atten=16)
    ref_sd = net.state_dict()
    sd = seeded_state({k: v.shape for k, v in ref_sd.items()}, GO_SEED, ref_sd)
    net.load_state_dict(sd)
    net.train(True)
    MG._no_dropout(net)
    snps = Batch.from_data_list(synth.brain_graph_list(BSZ, seed=GO_SEED + 10, rois=ROIS, top_k=3,
                                                       tsne_dim=16)).snps_feat
    latent, x_d, _, atten = net(snps, torch.tensor(TAU), "cpu")
    rng = np.random.default_rng(GO_SEED + 30)
    c1 = torch.from_numpy(rng.standard_normal(tuple(latent.shape)).astype(np.float32))
    c2 = torch.from_numpy(rng.standard_normal(tuple(x_d.shape)).astype(np.float32))
    ((latent * c1).sum() + (x_d * c2).sum()).backward()
    store["go/cfg"] = np.array([BSZ, GO_SEED, 16])
    _keys("go", ref_sd, store)
    store["go/c1"], store["go/c2"] = c1.numpy(), c2.numpy()
    MG._pack("go/out", {"latent": latent, "x_d": x_d, "atten_out": atten}, store)
    MG._pack("go/running", _running(net), store)
    MG._pack("go/grad", {k: p.grad for k, p in net.named_parameters()}, store)
    store["go/no_grad"] = np.array(sorted(k for k, p in net.named_parameters() if p.grad is None))
    print("wrote go")


def main():
    torch.manual_seed(0)
    gm, gd = load_guide()
    store = {"meta": np.array(
        "reference kernel/guide_img_snp.py + kernel/guide_go_model.py executed on CPU; to_dense_batch = "
        "oracle.pyg_ops (PyG 2.0.2 absent: unpinned), torch_scatter.scatter -> index_add_; F.gumbel_softmax = torch's "
        "formula on the stored noise; dropout p=0 in training mode; "
        f"torch {torch.__version__}; weights = seeded_state(shapes, seed); graphs = synth.brain_graph_list({BSZ}, "
        f"seed=seed+10, rois={ROIS}, top_k=3, tsne_dim=16); GO = synth.go_hierarchy({list(POOL)}, seed=seed); "
        "loss = train() kernel/train_eval_guide_img_snps.py:450-487"),
        "pool": np.array(POOL), "lam": np.array(LAM), "tau": np.array(TAU)}
    capture_model(gd, store)
    capture_go(gm, store)
    np.savez_compressed(os.path.join(HERE, "guide_imgsnp.npz"), **store)


if __name__ == "__main__":
    main()
