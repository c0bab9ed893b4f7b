"""CPU restatement of GUIDE_IMGSNP + its loss (TEST INFRASTRUCTURE ONLY).

Follows /root/reference:
  kernel/guide_go_model.py:97-144     the GUIDE GO network: nn.PReLU() for every activation, the latent MLP
                                      Linear -> BN(32) -> PReLU -> Dropout -> Linear with nothing behind it
  kernel/guide_go_model.py:203-285    its forward                   -> go_forward (oracle.go_network.go_forward with
                                                                       act = prelu, latent_out = False)
  kernel/guide_img_snp.py:43-67       heads, encoder_i_N, decoder_i_N, bias_n
  kernel/guide_img_snp.py:94-100      the gate (F.gumbel_softmax(..., hard=True) on imposed noise) -> gate
  kernel/guide_img_snp.py:78-135      forward                       -> model_forward
  kernel/train_eval_guide_img_snps.py:450-487  train()'s loss       -> train_losses

Functional over a flat state_dict with the reference's key names (``bias_n.0``, ``encoder_i_N.0.weight``,
``go_network.w_act.0.weight`` ...).  Every PReLU goes through the module-level ``prelu`` (``site`` = the module's key), so
that a test can observe or impose its decisions by replacing it.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import go_network as G
from .dropout import is_feed

LAMBDA = (1.0, 1.0, 2.5e-6, 0.2, 0.2)        # kernel/train_eval_guide_img_snps.py:163-164
PROB_REF, EPS = 0.001, 1e-10                 # train()'s prob_ref / eps (:450)
LAMDA_CE = 1                                 # sgcn_hyperparameters.py: hp.lamda_ce
# the BatchNorms a training forward runs (their num_batches_tracked advance; classification.0 and batch_norm never run)
GO_BNS = ("conc_for_attention.1", "B.0", "B_D.0", "latent.1")
MODEL_BNS = ("decoder_i_N.0", "decoder_i_N.4")


def prelu(site, u, a):
    """nn.PReLU() with its single slope ``a`` [1]: u > 0 ? u : a u.  ``site``: the module's state_dict key (the
    decisions of one site can be told from another's by a test that replaces this function)."""
    return torch.where(u > 0, u, a * u)


def _act(sd, prefix):
    return lambda site, t: prelu(prefix + site, t, sd[prefix + site + ".weight"])


def _batch_norm(sd, name, x, training):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"],
                        sd[name + ".bias"], training, 0.1, 1e-5)


def _count_batches(sd, names):
    for n in names:
        sd[n + ".num_batches_tracked"] += 1


def go_forward(sd, idx, snps, training=False, dropout=False, prefix=""):
    """guide_go_model.py:203-285.  snps [B,54] -> (latent [B,l_dim], x_D [B,54], atten_out [B,Ntop,d_att])."""
    out = G.go_forward(sd, idx, snps, training, dropout, False, prefix, act=_act(sd, prefix), latent_out=False)
    if training:
        _count_batches(sd, [prefix + n for n in GO_BNS])
    return out


def gate(bias, noise, tau, b):
    """guide_img_snp.py:94-100: (imp_N = softmax(bias_n) [K,2], z_N[:, 1] [b, K]) with z_N the straight-through hard
    sample of F.gumbel_softmax(log imp_N.repeat(b, 1), tau, hard=True), whose noise [b, K, 2] is imposed (torch's formula:
    y_hard - y_soft.detach() + y_soft, the hard index from max)."""
    imp = torch.softmax(bias, dim=1)
    logits = torch.log(imp.repeat(b, 1))
    y_soft = ((logits + noise.reshape(logits.shape).to(logits.dtype)) / tau).softmax(-1)
    index = y_soft.max(-1, keepdim=True)[1]
    y_hard = torch.zeros_like(logits).scatter_(-1, index, 1.0)
    return imp, (y_hard - y_soft.detach() + y_soft)[:, 1].reshape(b, -1)


def model_forward(sd, cfg, idx, data, tau=None, noise=None, training=False, dropout=False):
    """GUIDE_IMGSNP.forward :78-135.  cfg: SimpleNamespace(rois); data: x [B*rois, H_0] (every graph has rois nodes:
    to_dense_batch :86-89 is a reshape), snps_feat.  ``noise`` [B, K, 2]: the gate's Gumbel noise (training needs it).
    ``dropout``: True (draw), False, or an oracle.dropout.MaskFeed (the GO network's sites, ``encoder_i_N.1``,
    ``decoder_i_N.1``, ``decoder_i_N.5``, ``lin1``, ``lin1_regr``).
    Returns the reference's 8-tuple (log_softmax, x_hat, latent, latent, linear_outf, our_reg, [img_out, decoded],
    [imp_N[:, 1]])."""
    x = data.x
    b = x.shape[0] // cfg.rois
    img = x.reshape(b, -1)                                                    # :86-89
    if training:                                                              # :94-102
        if noise is None or tau is None:
            raise ValueError("oracle.guide: a training forward needs the temperature and the imposed noise")
        imp, z1 = gate(sd["bias_n.0"], noise, tau, b)
        x_in = img * z1
    else:
        imp = torch.softmax(sd["bias_n.0"], dim=1)
        x_in = img
    latent_g, x_hat, _ = go_forward(sd, idx, data.snps_feat, training, dropout, prefix="go_network.")     # :105
    h = prelu("encoder_i_N.1", x_in @ sd["encoder_i_N.0.weight"].t(), sd["encoder_i_N.1.weight"])           # :49-55,110
    h = G._dropout(h, 0.4, training, dropout, "encoder_i_N.1")
    latent_n = h @ sd["encoder_i_N.3.weight"].t()
    latent = (latent_g + latent_n) / 2                                        # :113
    d = prelu("decoder_i_N.1", _batch_norm(sd, "decoder_i_N.0", latent, training), sd["decoder_i_N.1.weight"])  # :57-66
    d = G._dropout(d, 0.4, training, dropout, "decoder_i_N.1") @ sd["decoder_i_N.3.weight"].t()
    d = prelu("decoder_i_N.5", _batch_norm(sd, "decoder_i_N.4", d, training), sd["decoder_i_N.5.weight"])
    decoded = G._dropout(d, 0.4, training, dropout, "decoder_i_N.5") @ sd["decoder_i_N.7.weight"].t()
    if training:
        _count_batches(sd, MODEL_BNS)
    lin_f = torch.relu(latent @ sd["lin1.weight"].t() + sd["lin1.bias"])     # :127-133
    logits = G._dropout(lin_f, 0.5, training, dropout, "lin1") @ sd["lin2.weight"].t() + sd["lin2.bias"]
    r = torch.relu(latent @ sd["lin1_regr.weight"].t() + sd["lin1_regr.bias"])
    reg = G._dropout(r, 0.3, training, dropout, "lin1_regr") @ sd["lin2_regr.weight"].t() + sd["lin2_regr.bias"]
    return F.log_softmax(logits, dim=-1), x_hat, latent, latent, lin_f, reg, [img, decoded], [imp[:, 1]]


def sparsity(p, prob_ref=PROB_REF, eps=EPS):
    """train() :465-474 for one importance vector: the KL divergence of Bernoulli(p) against Bernoulli(prob_ref), rho a
    FloatTensor there (its log rounds in fp32)."""
    rho = torch.full(p.shape, prob_ref, dtype=torch.float32).to(p.dtype)
    s1 = torch.mean(p * (torch.log(p + eps) - torch.log(rho + eps)))
    return torch.mean((1 - p) * (torch.log(1 - p + eps) - torch.log(1 - rho + eps))) + s1


def train_losses(sd, cfg, idx, data, tau, noise, lam=LAMBDA, dropout=False):
    """train() :460-483 (model in training mode; criterion_recon = MSELoss(reduction='none')).
    Returns (loss, dict of the five terms, outputs)."""
    outs = model_forward(sd, cfg, idx, data, tau, noise, training=True, dropout=dropout)
    if is_feed(dropout):
        dropout.close()                                                       # (every mask of the launch was consumed)
    logp, x_hat, _, _, _, reg, (img, decoded), prob = outs
    s2 = 0.0
    for p in prob:
        s2 = s2 + sparsity(p)
    t = {"ce": lam[0] * F.nll_loss(logp, data.y.view(-1)),
         "reg": lam[1] * F.mse_loss(reg.view(-1), data.clini_score.view(-1)),
         "recon": lam[2] * torch.sum((x_hat - data.snps_feat) ** 2),
         "recon_img": lam[3] * torch.sum((img - decoded) ** 2),
         "sparsity": lam[4] * s2}
    if lam[0] == 0:                                                           # :481-482
        t["ce"] = 0.0
    loss = LAMDA_CE * t["ce"] + t["reg"] + t["recon"] + t["recon_img"] + t["sparsity"]
    return loss, t, outs


def batch_data(data, dtype=torch.float64):
    """The fields model_forward / train_losses read, floating ones in ``dtype``; x a leaf that takes a gradient."""
    return SimpleNamespace(x=data.x.detach().to(dtype).requires_grad_(True), snps_feat=data.snps_feat.detach().to(dtype),
                           y=data.y.detach(), clini_score=data.clini_score.detach().to(dtype))
