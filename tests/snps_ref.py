"""CPU restatement (TEST INFRASTRUCTURE ONLY) of the genetics-only trainer kernel/train_eval_snps.py:298-335 on
``Gene_ontology_network``: ``oracle.go_network.go_forward`` as it is, plus what the trainer adds — the ``classification``
module (kernel/go_model.py:148-157) on cat(latent, data), ``sum BCELoss(y_hat, label)`` and ``lambda0 sum (x_hat -
data)^2`` (:314-320) — functional over a flat state_dict with the reference's key names, in whatever dtype the state has
(float64 unless the caller converts).  Dropout is off unless the caller asks for it or feeds the masks
(oracle.dropout.MaskFeed; the head's sites are ``classification.2`` and ``classification.5``).

Also the float64 reference of the fused launches (``head_loss``: igcn_snps_head_loss_fwd / _bwd), whose keep masks are
arguments.
"""
import torch
import torch.nn.functional as F

from oracle import go_network as G

LAMBDA0 = 1e-5                                                    # kernel/train_eval_snps.py:169
TERMS = ("class", "recon")
HEAD_SITES = ("classification.2", "classification.5")


class _BCE(torch.autograd.Function):
    """torch.nn.BCELoss(reduction='none') restated: -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)), with ITS
    gradient (p - y) / max(p (1 - p), 1e-12) — not the derivative of the clamped logarithms.  log(1 - p) is log1p(-p), as
    torch's: for a small p it is -p, where log(1 - p) in fp32 is 0."""

    @staticmethod
    def forward(ctx, p, y):
        ctx.save_for_backward(p, y)
        return -(y * torch.log(p).clamp(min=-100.0) + (1 - y) * torch.log1p(-p).clamp(min=-100.0))

    @staticmethod
    def backward(ctx, g):
        p, y = ctx.saved_tensors
        return g * (p - y) / (p * (1 - p)).clamp(min=1e-12), None


def bce(p, y):
    return _BCE.apply(p, y)


def classification(sd, latent, snps, training=False, dropout=False, prefix="", keeps=None):
    """``model.classification(cat(latent, snps))`` [B] (kernel/go_model.py:148-157; kernel/train_eval_snps.py:315).
    ``keeps`` = (keep1 [B, l_dim + 54] or None, keep2 [B, 16] or None): the two dropouts multiply by these factors instead of
    asking ``dropout``.  In training mode the running statistics in ``sd`` are updated in place, as the module's."""
    sdp = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)} if prefix else sd
    x = torch.cat((latent, snps), -1)
    a = torch.relu(G._batch_norm(sdp, "classification.0", x, training))
    if keeps is not None:
        a = a if keeps[0] is None else a * keeps[0]
    else:
        a = G._dropout(a, 0.5, training, dropout, HEAD_SITES[0])
    h = torch.relu(a @ sdp["classification.3.weight"].t())
    if keeps is not None:
        h = h if keeps[1] is None else h * keeps[1]
    else:
        h = G._dropout(h, 0.3, training, dropout, HEAD_SITES[1])
    z = h @ sdp["classification.6.weight"].t() + sdp["classification.6.bias"]
    return torch.sigmoid(z).view(-1)


def losses(sd, idx, data, label, lambda0=LAMBDA0, training=False, dropout=False):
    """train() :314-320 for one batch.  Returns (loss, {"class", "recon"}, (latent, x_hat, y_hat)).  The reference unpacks
    three values from forward's four-tuple and raises; the first two outputs are what it means."""
    latent, x_hat, _ = G.go_forward(sd, idx, data, training, dropout)
    y_hat = classification(sd, latent, data, training, dropout)
    t = {"class": bce(y_hat, label.view(-1).to(y_hat.dtype)).sum(), "recon": lambda0 * ((x_hat - data) ** 2).sum()}
    return t["class"] + t["recon"], t, (latent, x_hat, y_hat)


def trainable_keys(sd):
    return [k for k, v in sd.items() if v.dtype.is_floating_point and "running_" not in k]


def train_step(sd, idx, data, label, lr=1e-3, lambda0=LAMBDA0, dropout=False):
    """One iteration of train() :305-330: zero_grad, forward, loss, backward, Adam(weight_decay=0)."""
    opt = torch.optim.Adam([sd[k] for k in trainable_keys(sd)], lr=lr)
    opt.zero_grad()
    loss, terms, outs = losses(sd, idx, data, label, lambda0, True, dropout)
    loss.backward()
    opt.step()
    return loss.detach(), terms, outs


def head_loss(latent, snps, x_hat, label, gamma, beta, running_mean, running_var, w1, w2, b2, keep1=None, keep2=None,
              lambda0=LAMBDA0, training=True, momentum=0.1, eps=1e-5, upstream=1.0, dtype=torch.float64):
    """igcn_snps_head_loss_fwd + _bwd in ``dtype`` torch: every input is converted; latent, x_hat and the five parameters
    become leaves.  Returns a dict: y_hat, loss, class, recon, the gradients dlatent, dxhat, dgamma, dbeta, dW1, dW2, db2 for
    the upstream gradient ``upstream``, and the running statistics after the call."""
    f = lambda t: None if t is None else t.detach().to(dtype).cpu().clone()          # noqa: E731
    latent, snps, x_hat, label, gamma, beta, rm, rv, w1, w2, b2, keep1, keep2 = (
        f(t) for t in (latent, snps, x_hat, label, gamma, beta, running_mean, running_var, w1, w2, b2, keep1, keep2))
    leaves = [latent, x_hat, gamma, beta, w1, w2, b2]
    for t in leaves:
        t.requires_grad_(True)
    x = torch.cat((latent, snps), -1)
    a = torch.relu(F.batch_norm(x, rm, rv, gamma, beta, training, momentum, eps))
    a = a if keep1 is None else a * keep1
    h = torch.relu(a @ w1.t())
    h = h if keep2 is None else h * keep2
    y_hat = torch.sigmoid(h @ w2.t() + b2).view(-1)
    cls = bce(y_hat, label.view(-1)).sum()
    rec = lambda0 * ((x_hat - snps) ** 2).sum() if lambda0 != 0 else torch.zeros((), dtype=dtype)
    loss = cls + rec
    grads = torch.autograd.grad(loss * upstream, leaves, allow_unused=True)
    out = {"y_hat": y_hat.detach(), "loss": loss.detach(), "class": cls.detach(), "recon": rec.detach(),
           "running_mean": rm, "running_var": rv}
    out.update(dict(zip(("dlatent", "dxhat", "dgamma", "dbeta", "dW1", "dW2", "db2"), grads)))
    if out["dxhat"] is None:
        out["dxhat"] = torch.zeros_like(x_hat)
    return out


# ---- the fixture -------------------------------------------------------------------------------------------------
CONFIGS = {"main20": dict(seed=91, pool=(3, 6, 11), l_dim=5, bsz=30),          # the shape of go_model.py's __main__
           "b32": dict(seed=92, pool=(300, 120, 60, 19, 1), l_dim=32, bsz=32)}


def hierarchy(tag):
    """(go_snps, adj, pool_dim) of a configuration.  b32: ``synth.go_hierarchy`` on its pool.  main20: a seeded DAG on 20
    nodes in which any deeper node may be the child of any later one (adj[parent, child] = 1 with probability 1/2 for parent
    > child) — a strict level hierarchy of three levels leaves the decoder's first layer without edges, which the
    reference cannot run; the root row of go_snps is all ones, as the hierarchies' is."""
    import numpy as np
    from igcn_amd import synth
    c = CONFIGS[tag]
    if tag != "main20":
        return synth.go_hierarchy(c["pool"], seed=c["seed"])
    rng = np.random.default_rng(c["seed"])
    n = sum(c["pool"])
    adj = np.tril((rng.random((n, n)) < 0.5).astype(np.float32), -1)
    go_snps = (rng.random((n, G.N_SNPS)) < 0.3).astype(np.float32)
    go_snps[n - 1, :] = 1.0
    return go_snps, adj, [list(c["pool"])]


def inputs(tag, mode="train"):
    """(data [B, 54] float32 with seeded integers in {0, 1, 2}, label [B] float32 seeded Bernoulli(0.5))."""
    import numpy as np
    c = CONFIGS[tag]
    rng = np.random.default_rng(c["seed"] + (10 if mode == "train" else 11))
    data = torch.from_numpy(rng.integers(0, 3, (c["bsz"], G.N_SNPS)).astype(np.float32))
    label = torch.from_numpy((rng.random(c["bsz"]) < 0.5).astype(np.float32))
    return data, label


def fixture_setup(store, tag):
    """(cfg, go index sets, seeded fp32 state) of configuration ``tag`` of snps_only.npz, rebuilt from seeds as
    tests/golden/make_golden_snps.py built them; the state's keys are checked against the reference's ``state_dict()``."""
    from types import SimpleNamespace
    from _weights import seeded_state
    from igcn_amd import synth
    c = CONFIGS[tag]
    assert [int(v) for v in store[f"{tag}/cfg"]] == [c["seed"], c["l_dim"], c["bsz"]] + list(c["pool"])
    go_snps, adj, pool_dim = hierarchy(tag)
    a_g, a = synth.go_sparse_inputs(go_snps, adj)
    idx = G.go_index_sets(a_g, a, list(c["pool"]), 2)
    shapes = G.go_param_shapes(idx, l_dim=c["l_dim"])
    keys = store[f"{tag}/state_keys"].tolist()
    assert sorted(shapes) == keys, sorted(set(shapes) ^ set(keys))
    cfg = SimpleNamespace(a_g=a_g, a=a, pool_dim=pool_dim, lambda0=float(store["lambda0"]), **c)
    return cfg, idx, seeded_state(shapes, c["seed"])


# ---- the inputs of the GPU tests of the launch (tests/test_gpu_snps.py), built here so that the CPU suite can check
# the condition they rest on (tests/test_snps_reference.py: no ReLU decision of the float64 reference within rounding) ----
HEAD_SHAPES = ((2, 5), (3, 32), (30, 5), (32, 32), (257, 32))      # (B, L): see tests/test_gpu_snps.py
H = 16


def head_case(b, l, seed=None, const_col=None, soft=False, masks=False):
    """Seeded inputs of one head launch as a dict of float32 tensors: latent [b, l] (post-ReLU like: about half zeros), snps
    [b, 54] integers in {0, 1, 2} (``const_col``: that SNP column constant over the batch), x_hat, label (Bernoulli(0.5), or
    ``soft`` uniform in [0, 1]), the BatchNorm's gamma / beta / running statistics, W1 [16, l + 54], W2 [1, 16], b2 [1] and,
    ``masks``, keep1 / keep2 = {0, 1/(1-p)} factors at p = 0.5 / 0.3 (else None)."""
    import numpy as np
    rng = np.random.default_rng(5000 if seed is None else seed)
    k1 = l + G.N_SNPS
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))                  # noqa: E731
    snps = rng.integers(0, 3, (b, G.N_SNPS))
    if const_col is not None:
        snps[:, const_col] = 2
    c = {"latent": f(np.maximum(rng.standard_normal((b, l)), 0.0)), "snps": f(snps),
         "x_hat": f(rng.standard_normal((b, G.N_SNPS)) + 1.0),
         "label": f(rng.random(b)) if soft else f(rng.random(b) < 0.5),
         "gamma": f(1.0 + 0.2 * rng.standard_normal(k1)), "beta": f(0.1 * rng.standard_normal(k1)),
         "running_mean": f(0.5 + 0.3 * rng.standard_normal(k1)), "running_var": f(0.5 + rng.random(k1)),
         "w1": f(rng.uniform(-1, 1, (H, k1)) / np.sqrt(k1)), "w2": f(rng.uniform(-1, 1, (1, H)) / np.sqrt(H) * 4),
         "b2": f(0.1 * rng.standard_normal(1)), "keep1": None, "keep2": None}
    if masks:
        for name, shape, p in (("keep1", (b, k1), 0.5), ("keep2", (b, H), 0.3)):
            scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
            c[name] = f(np.where(rng.random(shape) < p, np.float32(0.0), scale))
    return c


def head_cases():
    """Every (name, inputs, training) the GPU tests of the launch compare with ``head_loss``.  The seeds are ones at which
    the float64 reference has no ReLU decision within rounding (tests/test_snps_reference.py checks it)."""
    out = []
    for b, l in HEAD_SHAPES:
        out.append((f"B{b}L{l}/eval", head_case(b, l), False))
        out.append((f"B{b}L{l}/train", head_case(b, l), True))
        out.append((f"B{b}L{l}/train+masks", head_case(b, l, masks=True), True))
    out.append(("const_col", head_case(30, 5, seed=6000, const_col=7), True))
    out.append(("soft", head_case(32, 32, seed=7001, soft=True, masks=True), True))
    return out


def head_loss_of(c, training, **kw):
    """``head_loss`` on a ``head_case`` dict."""
    return head_loss(c["latent"], c["snps"], c["x_hat"], c["label"], c["gamma"], c["beta"], c["running_mean"],
                     c["running_var"], c["w1"], c["w2"], c["b2"], c["keep1"], c["keep2"], training=training, **kw)


DROPOUT_TAG = "b32"                              # the dropout-on step of tests/test_gpu_snps.py runs this configuration


def dropout_sites(tag):
    """The site list of the GO network's one mask launch for a training forward of ``losses_snps`` on configuration ``tag``:
    the network's own sites, then the head's two ([B, l_dim + 54] at p = 0.5, [B, 16] at p = 0.3)."""
    from dropout_cases import go_sites
    c = CONFIGS[tag]
    return go_sites(c["pool"], c["bsz"], [((c["bsz"], c["l_dim"] + G.N_SNPS), 0.5), ((c["bsz"], H), 0.3)])
