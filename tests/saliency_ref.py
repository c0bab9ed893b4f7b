"""Float64 numpy restatement of csrc/saliency.hip (igcn_saliency_maps, igcn_grad_cam) and of the midpoint-rule integrated
gradients the models' ``integrated_gradients`` runs.  Each kernel function also returns ``s``, the sum of the absolute
terms of every element's reduction — the scale of the per-element bound 1e-6 + 1e-4 s the GPU tests hold the kernels to
(an fp32 sum of n <= 512 terms errs by at most (n - 1) 2^-24 <= 3.1e-5 of s)."""
import numpy as np


def bound(s):
    return 1e-6 + 1e-4 * np.asarray(s, dtype=np.float64)


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)


def saliency_maps(x, dx, rois, base=None, norm=False):
    """x [B R, H0], dx [M, B R, H0] (or [B R, H0]), base None / [R, H0] / [B R, H0] -> (attr [B, R, H0], roi [B, R],
    s_attr [B, R, H0] = |x - base| * mean_m |dx|).  ``norm``: every subject divided by its largest roi (left as it is
    when that is 0)."""
    x, dx = _f64(x), _f64(dx)
    if dx.ndim == 2:
        dx = dx[None]
    n, h0 = x.shape
    b = n // rois
    d = x.copy()
    if base is not None:
        base = _f64(base)
        d = d - (base if base.shape[0] == n else np.tile(base, (b, 1)))
    attr = (d * dx.mean(0)).reshape(b, rois, h0)
    s = (np.abs(d) * np.abs(dx).mean(0)).reshape(b, rois, h0)
    roi = np.abs(attr).sum(2)
    if norm:
        attr, roi = normalise(attr, roi)
    return attr, roi, s


def normalise(attr, roi):
    """(attr, roi) divided, subject by subject, by the subject's largest roi; untouched where that is 0."""
    mx = roi.max(1)
    div = np.where(mx > 0, mx, 1.0)
    return attr / div.reshape(-1, *([1] * (attr.ndim - 1))), roi / div[:, None]


def grad_cam(acts, grads, rois, norm=False):
    """acts, grads [B R, K] -> (cam [B, R], alpha [B, K], s_cam [B, R] = sum_k |alpha_k acts_k|)."""
    acts, grads = _f64(acts), _f64(grads)
    k = acts.shape[1]
    a, g = acts.reshape(-1, rois, k), grads.reshape(-1, rois, k)
    alpha = g.mean(1)
    terms = alpha[:, None, :] * a
    cam = np.maximum(terms.sum(2), 0.0)
    if norm:
        cam = normalise(cam, cam)[1]
    return cam, alpha, np.abs(terms).sum(2)


def integrated_gradients(score_and_grad, x, rois, steps, base=None):
    """Midpoint rule at alpha_m = (m + 1/2) / steps from ``base`` (None: zeros, [R, H0] or [B R, H0]) to x [B R, H0].
    ``score_and_grad(x)`` -> (score [B], d score / d x [B R, H0]) in float64.  Returns (attr [B, R, H0], roi [B, R],
    delta [B] = sum attr - (score(x) - score(base)), dx [steps, B R, H0])."""
    x = _f64(x)
    n = x.shape[0]
    b = n // rois
    base_full = np.zeros_like(x) if base is None else (_f64(base) if _f64(base).shape[0] == n else np.tile(_f64(base), (b, 1)))
    dx = np.stack([_f64(score_and_grad(base_full + (m + 0.5) / steps * (x - base_full))[1]) for m in range(steps)])
    attr, roi, _ = saliency_maps(x, dx, rois, base)
    gap = _f64(score_and_grad(x)[0]) - _f64(score_and_grad(base_full)[0])
    return attr, roi, attr.sum((1, 2)) - gap, dx
