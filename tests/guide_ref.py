"""Restatements for the GUIDE_IMGSNP tests: the gate's generator contract in numpy (include/igcn.h, igcn_guide_gate_fwd)
and the gate + encoder_i_N of kernel/guide_img_snp.py:88-100,112 in float64 torch."""
import numpy as np
import torch

from oracle import dropout as OD


def gumbel_from_draws(r):
    """g = -log(-log u), u = (r + 1/2) 2^-24 exactly, for 24-bit draws r (float64 arithmetic, float32 result; the kernel
    forms log u in fp32, so the two agree to a few ulps)."""
    u = (np.asarray(r, dtype=np.float64) + 0.5) / 16777216.0
    return (-np.log(-np.log(u))).astype(np.float32)


def gumbel_noise(counter, b, k):
    """The noise [b, k, 2] the kernel draws at stream counter ``counter``: element (b, k, j) at flat index 2 (b k + k) + j,
    r = the 24-bit draw of the dropout generator there (oracle.dropout.uniforms = r / 2^24)."""
    r = np.round(OD.uniforms(counter, 2 * b * k).astype(np.float64) * 16777216.0)
    return gumbel_from_draws(r).reshape(b, k, 2)


def soft_sample(bias, noise, tau):
    """(s [B, K, 2], hard z1 [B, K]) of gumbel_softmax(log softmax(bias), tau, hard=True) in float64; ties -> class 0."""
    logit = torch.log(torch.softmax(torch.as_tensor(bias, dtype=torch.float64), 1))
    w = (logit.unsqueeze(0) + torch.as_tensor(noise, dtype=torch.float64)) / float(tau)
    s = torch.softmax(w, -1)
    return s, (s[..., 1] > s[..., 0]).to(torch.float64)


def gate_encoder(img, bias, w1, a, w2, keep, tau, noise, training):
    """float64 autograd restatement: (latent_n, imp1).  ``training``: the straight-through hard gate on ``noise``."""
    imp = torch.softmax(bias, 1)
    x = img
    if training:
        logits = torch.log(imp).repeat(img.shape[0], 1)
        y_soft = ((logits + noise.reshape(logits.shape)) / tau).softmax(-1)
        index = y_soft.max(-1, keepdim=True)[1]
        y_hard = torch.zeros_like(logits).scatter_(-1, index, 1.0)
        z = (y_hard - y_soft.detach() + y_soft)[:, 1].reshape(img.shape)
        x = img * z
    pre = x @ w1.t()
    h = torch.where(pre > 0, pre, a * pre)
    if keep is not None:
        h = h * keep
    return h @ w2.t(), imp[:, 1]
