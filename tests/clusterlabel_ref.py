"""CPU restatement (TEST INFRASTRUCTURE ONLY) of what SGCN_GCN_CLUSTERLABEL adds to the shared body of the family —
kernel/sgcn_img_snp_clusterlabel.py:114-144 (loss_probability with its own normalisations), :217-228 (the two
classification heads) and train() of kernel/train_eval_sgcn_clusterlabel.py:375-393 (the six-term loss) — functional over
a flat state_dict with the reference's key names, in whatever dtype the state has (the tests use float64); dropout is
off unless the caller asks for it or feeds the masks (oracle.dropout.MaskFeed).  The masks,
GCNConv, the GO network and the attention are ``oracle``'s.

Also the float64 references of the two new launches: ``head_loss`` (igcn_cluster_head_loss_fwd) and ``mask_reg3``
(igcn_mask_reg3_*).
"""
import torch
import torch.nn.functional as F

from oracle import go_network as G
from oracle import sgcn_img_snp as OS
from oracle.pyg_ops import gcn_conv, to_dense_batch

HP = OS.HP
LAMBDA0 = 1e-5                                                    # kernel/train_eval_sgcn_clusterlabel.py:188
TERMS = ("ce", "ce_cluster", "mi", "mi_cluster", "prob", "recon")


def param_shapes(num_layers, hidden, h0=1, num_features=1, l_dim=32, num_classes=3, num_cluster=2, hidden_linear=64,
                 rois=90):
    """Top-level parameter and buffer shapes of SGCN_GCN_CLUSTERLABEL(isCrossAtten=True) (:15-67)."""
    d = num_layers * hidden
    shp = {"prob": (rois, h0), "prob_bias": (2 * h0, 1), "edge_prob": (rois, rois), "snps_prob": (1, 54),
           "conv1.bias": (hidden,), "conv1.lin.weight": (hidden, num_features)}
    for i in range(num_layers - 1):
        shp[f"convs.{i}.bias"] = (hidden,)
        shp[f"convs.{i}.lin.weight"] = (hidden, hidden)
    shp.update({"multihead_attn.in_proj_weight": (3 * d, d), "multihead_attn.in_proj_bias": (3 * d,),
                "multihead_attn.out_proj.weight": (d, d), "multihead_attn.out_proj.bias": (d,)})
    lin_in = 90 * d + l_dim                                        # the literal 90 of :46,50
    for head, c in (("classify", num_classes), ("cluster", num_cluster)):
        shp[f"lin1_{head}.weight"] = (hidden_linear, lin_in)
        shp[f"lin1_{head}.bias"] = (hidden_linear,)
        shp[f"lin2_{head}.weight"] = (c, hidden_linear)
        shp[f"lin2_{head}.bias"] = (c,)
    shp.update({"batch_norm.weight": (d,), "batch_norm.bias": (d,), "batch_norm.running_mean": (d,),
                "batch_norm.running_var": (d,), "batch_norm.num_batches_tracked": ()})
    return shp


def model_forward(sd, rois, go_idx, data, is_explain=False, training=False, predict=True, faithful=False, dropout=False):
    """forward :157-228 with isCrossAtten=True.  ``dropout``: False (off), True (drawn, as the reference does), or an
    oracle.dropout.MaskFeed holding this pass's factors: the GO network's sites and the two heads' (:221,225, both
    p = 0.5), ``lin1_classify`` and ``lin1_cluster``.  Returns the reference's 4-tuple."""
    x, ei, batch, ew, snps = data.x, data.edge_index, data.batch, data.edge_attr, data.snps_feat
    if is_explain:
        xm, ewm, _, snpsm = OS.edge_and_region_masks(sd, x, ei, ew, rois, snps)
    else:
        xm, ewm, snpsm = x, ew, snps
    hs = [torch.relu(gcn_conv(xm, ei, ewm, sd["conv1.lin.weight"], sd["conv1.bias"]))]
    i = 0
    while f"convs.{i}.lin.weight" in sd:
        hs.append(torch.relu(gcn_conv(hs[-1], ei, ewm, sd[f"convs.{i}.lin.weight"], sd[f"convs.{i}.bias"])))
        i += 1
    xcat = torch.cat(hs, dim=1)
    dense, _ = to_dense_batch(xcat, batch, float(xcat.min()) - 1)
    bsz = dense.shape[0]
    img_out = dense.reshape(bsz, -1)
    latent, x_hat, atten_out = G.go_forward(sd, go_idx, snpsm, training, dropout, faithful, prefix="go_network.")
    cross = torch.relu(OS._mha(sd, dense, atten_out)).reshape(bsz, -1)
    out_z = torch.cat([(img_out + cross) / 2, latent], dim=-1)                            # :208
    z_cluster = out_z if predict else torch.zeros_like(out_z)                              # :217-220
    h_cluster = torch.relu(z_cluster @ sd["lin1_cluster.weight"].t() + sd["lin1_cluster.bias"])
    h_cluster = G._dropout(h_cluster, 0.5, training, dropout, "lin1_cluster")
    s_cluster = h_cluster @ sd["lin2_cluster.weight"].t() + sd["lin2_cluster.bias"]
    h = torch.relu(out_z @ sd["lin1_classify.weight"].t() + sd["lin1_classify.bias"])
    h = G._dropout(h, 0.5, training, dropout, "lin1_classify")
    s = h @ sd["lin2_classify.weight"].t() + sd["lin2_classify.bias"]
    return F.log_softmax(s, dim=-1), F.log_softmax(s_cluster, dim=-1), x_hat, out_z


def _entropy(p, eps):
    return -(p * torch.log(p + eps) + (1 - p) * torch.log((1 - p) + eps)).sum() / p.numel()


def loss_probability(sd, x, edge_index, edge_weight, rois, hp=HP, eps=1e-6):
    """:114-144 — the L1 term of sigma(prob) is divided by its ROWS and that of sigma(snps_prob) by its one row; the edge
    term and the three entropies are means."""
    _, _, e = OS.edge_and_region_masks(sd, x, edge_index, edge_weight, rois)
    p = torch.sigmoid(sd["prob"])
    s = torch.sigmoid(sd["snps_prob"])
    f_sum = p.abs().sum(dim=-1).sum() / p.shape[0]
    e_sum = e.abs().sum() / e.shape[0]
    s_sum = s.abs().sum(dim=-1).sum() / s.shape[0]
    return (hp.lamda_x_l1 * f_sum + hp.lamda_e_l1 * e_sum + hp.lamda_x_ent * _entropy(p, eps)
            + hp.lamda_e_ent * _entropy(e, eps) + hp.lamda_x_l1 * s_sum + hp.lamda_x_ent * _entropy(s, eps))


def combine(t, predict, hp=HP):
    """:391 / :393."""
    if predict:
        return hp.lamda_ce * (t["ce"] + t["ce_cluster"]) / 2 + hp.lamda_mi * (t["mi"] + t["mi_cluster"]) / 2 \
            + t["prob"] + t["recon"]
    return hp.lamda_ce * t["ce"] + hp.lamda_mi * t["mi"] + t["prob"] + t["recon"]


def train_losses(sd, rois, go_idx, data, lambda0=LAMBDA0, predict=True, hp=HP, faithful=False, dropout=False):
    """The loss of train() :375-393 (model in training mode).  ``dropout``: False, True, or an oracle.dropout.MaskFeed of
    2B rows per site (plain pass rows [0, B), masked pass rows [B, 2B)), which must be used up.
    Returns (loss, terms, (o1, o2))."""
    y, cy = data.y.view(-1), data.clust_y.view(-1)
    d1, d2 = OS.pass_feeds(dropout, y.numel())
    o1 = model_forward(sd, rois, go_idx, data, False, True, predict, faithful, d1)
    o2 = model_forward(sd, rois, go_idx, data, True, True, predict, faithful, d2)
    if OS.is_feed(dropout):
        dropout.close()
    t = {"ce": F.nll_loss(o1[0], y), "ce_cluster": F.nll_loss(o1[1], cy),
         "mi": F.nll_loss(o2[0], y), "mi_cluster": F.nll_loss(o2[1], cy),
         "prob": loss_probability(sd, data.x, data.edge_index, data.edge_attr, rois, hp),
         "recon": (lambda0 * ((o1[2] - data.snps_feat) ** 2).sum() + lambda0 * ((o2[2] - data.snps_feat) ** 2).sum()) / 2}
    return combine(t, predict, hp), t, (o1, o2)


def train_step(sd, rois, go_idx, data, lr=1e-3, lambda0=LAMBDA0, predict=True, faithful=False):
    """One iteration of train() :369-398: zero_grad, two forwards, the loss, backward, Adam(wd=0)."""
    opt = torch.optim.Adam([sd[k] for k in OS.trainable_keys(sd)], lr=lr)
    opt.zero_grad()
    data.x.requires_grad_(True)
    loss, terms, outs = train_losses(sd, rois, go_idx, data, lambda0, predict, faithful=faithful)
    loss.backward()
    opt.step()
    return loss.detach(), terms, outs


def fixture_setup(store, tag):
    """(cfg, go index sets, seeded fp32 state, {mode: graph list}) of configuration ``tag`` of clusterlabel.npz, rebuilt
    from seeds as tests/golden/make_golden_clusterlabel.py built them; the state's keys and shapes are checked against
    the ones the reference's ``state_dict()`` had."""
    from types import SimpleNamespace
    from _weights import seeded_state
    from igcn_amd import synth
    seed, h0, predict = (int(v) for v in store[f"{tag}/cfg"])
    rois, layers, hidden, l_dim = (int(v) for v in store["dims"])
    pool = store["pool"].tolist()
    go_snps, adj, pool_dim = synth.go_hierarchy(pool, seed=seed)
    a_g, a = synth.go_sparse_inputs(go_snps, adj)
    idx = G.go_index_sets(a_g, a, pool, 2)
    shapes = dict(param_shapes(layers, hidden, h0=h0, num_features=h0, l_dim=l_dim, rois=rois))
    shapes.update({"go_network." + k: v for k, v in G.go_param_shapes(idx, l_dim=l_dim, d_att=layers * hidden).items()})
    keys = store[f"{tag}/state_keys"].tolist()
    assert sorted(shapes) == keys, sorted(set(shapes) ^ set(keys))
    want = [tuple(int(d) for d in sh.split(",")) if sh else () for sh in store[f"{tag}/state_shapes"].tolist()]
    assert [tuple(shapes[k]) for k in keys] == want
    graphs = {"train": synth.brain_graph_list(32, seed=seed + 10, rois=rois, h0=h0, top_k=3, tsne_dim=16),
              "eval": synth.brain_graph_list(4, seed=seed + 11, rois=rois, h0=h0, top_k=3, tsne_dim=16)}
    cfg = SimpleNamespace(seed=seed, h0=h0, predict=bool(predict), rois=rois, layers=layers, hidden=hidden, l_dim=l_dim,
                          pool=pool, a_g=a_g, a=a, pool_dim=pool_dim, lambda0=float(store["lambda0"]))
    return cfg, idx, seeded_state(shapes, seed), graphs


# ---- float64 references of the two launches ---------------------------------------------------------------------
def head_loss(x1, keep1, w1, b1, x2, keep2, w2, b2, y, cy, x_hat, snps, prob, hp_ce, hp_mi, lambda0, predict):
    """igcn_cluster_head_loss_fwd + igcn_cluster_loss_final in float64 torch: every input is converted, the features,
    weights, x_hat and ``prob`` become leaves.  Returns a dict: logp1, logp2, the six terms, loss, and the gradients dx1,
    dx2, dW1, db1, dW2, db2, dxhat, dprob (None where the loss does not depend on the input)."""
    f = lambda t: None if t is None else t.detach().double().cpu()          # noqa: E731
    x1, keep1, w1, b1, x2, keep2, w2, b2, x_hat, snps, prob = (f(t) for t in (x1, keep1, w1, b1, x2, keep2, w2, b2,
                                                                               x_hat, snps, prob))
    y, cy = y.cpu(), cy.cpu()
    leaves = [x1, w1, b1, x2, w2, b2, x_hat, prob]
    for t in leaves:
        t.requires_grad_(True)
    b = y.numel()
    s1 = (x1 if keep1 is None else x1 * keep1) @ w1.t() + b1
    s2 = (x2 if keep2 is None else x2 * keep2) @ w2.t() + b2
    logp1, logp2 = F.log_softmax(s1, dim=-1), F.log_softmax(s2, dim=-1)
    t = {"ce": F.nll_loss(logp1[:b], y), "ce_cluster": F.nll_loss(logp2[:b], cy),
         "mi": F.nll_loss(logp1[b:], y), "mi_cluster": F.nll_loss(logp2[b:], cy), "prob": prob.sum(),
         "recon": lambda0 * (((x_hat[:b] - snps) ** 2).sum() + ((x_hat[b:] - snps) ** 2).sum()) / 2}
    hp = type(HP)(lamda_ce=hp_ce, lamda_mi=hp_mi)
    loss = combine(t, predict, hp)
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    out = {"logp1": logp1.detach(), "logp2": logp2.detach(), "loss": loss.detach(),
           **{k: v.detach() for k, v in t.items()}}
    out.update(dict(zip(("dx1", "dW1", "db1", "dx2", "dW2", "db2", "dxhat", "dprob"), grads)))
    return out


def mask_reg3(prob, e, snps, l1_x, ent_x, l1_e, ent_e, l1_s, ent_s, eps):
    """igcn_mask_reg3_{fwd,bwd} in float64: (loss, dprob, de, dsnps); a group without elements contributes nothing."""
    prob, e, snps = (t.detach().double().cpu().requires_grad_(True) for t in (prob, e, snps))

    def group(p, l1, ent):
        if p.numel() == 0:
            return p.sum()
        return l1 * p.abs().sum() / p.numel() + ent * _entropy(p, eps)
    loss = group(torch.sigmoid(prob), l1_x, ent_x) + group(e, l1_e, ent_e) + group(torch.sigmoid(snps), l1_s, ent_s)
    return (loss.detach(), *torch.autograd.grad(loss, [prob, e, snps], allow_unused=True))


# ---- the fixture's groups ---------------------------------------------------------------------------------------
def group(store, prefix):
    """``conftest.golden_group``'s dict ({name: array or ('summary', array)}) for a group of tests/golden/clusterlabel.npz,
    which stores a group as four archive members: the names (tensors kept in full first, then the summarised ones), the
    shapes of the full ones, their values back to back, and the summaries stacked."""
    names, shapes = store[prefix + "#names"].tolist(), store[prefix + "#shapes"].tolist()
    values, summaries = store[prefix + "#values"], store[prefix + "#summaries"]
    n_full = len(names) - summaries.shape[0]
    out, at = {}, 0
    for name, shape in zip(names[:n_full], shapes):
        dims = tuple(int(d) for d in shape.split(",")) if shape else ()
        n = int(torch.Size(dims).numel())
        out[name] = values[at:at + n].reshape(dims)
        at += n
    assert at == values.size, prefix
    for name, s in zip(names[n_full:], summaries):
        out[name] = ("summary", s)
    return out
