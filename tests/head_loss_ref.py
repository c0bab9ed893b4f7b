"""CPU restatement (TEST INFRASTRUCTURE ONLY), in float64 torch, of what closes a train step of SGCN_GCN_IMGSNP: the two
output layers lin2 / lin2_regr on their (dropout-scaled) features (kernel/sgcn_img_snp.py:289-290,300-301), log_softmax
(:305) and the seven terms of train() with their weighted sum (kernel/train_eval_sgcn_img_snps.py:525-543), the
``lambda_loss[0] == 0`` rule of :540-542 included.  The references of ops.HeadLoss (``head_loss``: igcn_head_loss_fwd,
igcn_head_loss_gram_fwd, igcn_loss_final) and of ops.LossHead (``loss_head``: igcn_loss_head_*).

Every floating input is converted to float64 (``dtype``) on the CPU and becomes a leaf; the gradients are autograd's.
"""
import torch
import torch.nn.functional as F

TERMS = ("ce", "mi", "reg", "prob", "recon", "cluster", "orth")


def _leaf(t, dtype):
    if t is None:
        return None
    if not torch.is_tensor(t):
        t = torch.tensor(t)
    return t.detach().to("cpu", dtype).clone().requires_grad_(True)


def _seven_terms(logp, reg, y, clin, x_hat, snps, gram, prob, lam):
    """The terms of :525-538, lam-weighted, on the stacked outputs (rows [0, B) the plain pass, [B, 2B) the isExplain
    pass).  ``gram``: [2, 2] = (consist, orth) per pass, or partial rows [r, 4] whose column sums are
    (consist_1, orth_1, consist_2, orth_2); ``prob``: the mask regulariser, a scalar or partial rows that sum to it."""
    b = y.numel()
    clin = clin.reshape(-1)
    if gram.dim() == 2 and gram.shape[1] == 4:
        g = gram.sum(0)
        c1, o1, c2 = g[0], g[1], g[2]
    else:
        c1, o1, c2 = gram[0, 0], gram[0, 1], gram[1, 0]
    t = [lam[0] * F.nll_loss(logp[:b], y), lam[0] * F.nll_loss(logp[b:], y),
         lam[1] * (F.mse_loss(reg[:b].reshape(-1), clin) + F.mse_loss(reg[b:].reshape(-1), clin)) / 2,
         lam[2] * prob.sum(),
         lam[3] * (((x_hat[:b] - snps) ** 2).sum() + ((x_hat[b:] - snps) ** 2).sum()) / 2,
         lam[4] * (c1 + c2) / 2, lam[5] * o1]
    if lam[0] == 0:                                                   # :540-542: the class terms are the constant 0.0
        t[0] = t[1] = torch.zeros((), dtype=reg.dtype)
    return t


def _finish(t, hp_ce, hp_mi, upstream, leaves, out):
    loss = hp_ce * t[0] + hp_mi * t[1] + t[2] + t[3] + t[4] + t[5] + t[6]            # :543
    names = [k for k, v in leaves.items() if v is not None]
    grads = torch.autograd.grad(loss * float(upstream), [leaves[k] for k in names], allow_unused=True)
    out.update(loss=loss.detach(), terms=torch.stack([v.detach() for v in t]),
               grads={k: (None if k not in names else grads[names.index(k)]) for k in leaves})
    return out


def loss_head(scores, y, reg, clin, x_hat, snps, gram, prob, lam, hp_ce=1.0, hp_mi=1.0, upstream=1.0, from_logits=True,
              dtype=torch.float64):
    """ops.LossHead.  ``scores`` [2B, C]: the raw class scores (``from_logits``) or log-probabilities taken as given.
    Returns {logp, loss, terms [7], grads: {scores, reg, x_hat, gram, prob}} — d (upstream * loss) / d input; a gradient
    is None where the loss does not depend on the input (the class scores when lam[0] == 0).  ``dtype``: float64, the
    reference; float32 gives the plain torch composite whose own error a bound may be taken from."""
    scores, reg, x_hat, gram, prob = (_leaf(v, dtype) for v in (scores, reg, x_hat, gram, prob))
    clin, snps = clin.detach().to("cpu", dtype), snps.detach().to("cpu", dtype)
    y = y.detach().cpu().view(-1)
    logp = F.log_softmax(scores, dim=-1) if from_logits else scores
    t = _seven_terms(logp, reg.view(2 * y.numel(), -1), y, clin, x_hat, snps, gram, prob, [float(v) for v in lam])
    return _finish(t, hp_ce, hp_mi, upstream, dict(scores=scores, reg=reg, x_hat=x_hat, gram=gram, prob=prob),
                   dict(logp=logp.detach()))


def head_loss(hf, keep1, w2, b2, hr, keep2, w2r, b2r, y, clin, x_hat, snps, gram, prob, lam, hp_ce=1.0, hp_mi=1.0,
              upstream=1.0, dtype=torch.float64):
    """ops.HeadLoss.  ``hf`` / ``hr`` [2B, K]: the classifier's and the regression head's features, ``keep*`` their
    dropout factors or None, (``w2``, ``b2``) = lin2 (bias may be None), (``w2r``, ``b2r``) = lin2_regr.
    Returns {logp [2B, C], reg [2B, NR], loss, terms [7], grads: {hf, w2, b2, hr, w2r, b2r, x_hat, gram, prob}}."""
    hf, w2, b2, hr, w2r, b2r, x_hat, gram, prob = (_leaf(v, dtype)
                                                   for v in (hf, w2, b2, hr, w2r, b2r, x_hat, gram, prob))
    fixed = lambda v: None if v is None else v.detach().to("cpu", dtype)          # noqa: E731
    keep1, keep2, clin, snps = fixed(keep1), fixed(keep2), fixed(clin), fixed(snps)
    y = y.detach().cpu().view(-1)
    scores = F.linear(hf if keep1 is None else hf * keep1, w2, b2)
    reg = F.linear(hr if keep2 is None else hr * keep2, w2r, b2r)
    logp = F.log_softmax(scores, dim=-1)
    t = _seven_terms(logp, reg, y, clin, x_hat, snps, gram, prob, [float(v) for v in lam])
    leaves = dict(hf=hf, w2=w2, b2=b2, hr=hr, w2r=w2r, b2r=b2r, x_hat=x_hat, gram=gram, prob=prob)
    return _finish(t, hp_ce, hp_mi, upstream, leaves, dict(logp=logp.detach(), reg=reg.detach()))
