"""Per-subject ROI x modality saliency maps: gradient x input, integrated gradients and Grad-CAM.

Every reference forward sets ``data.x.requires_grad = True`` and keeps ``self.input`` (kernel/sgcn_img_snp.py:210-211,
kernel/sgcn.py:113,362, kernel/gcn_img_snp.py) so that ``data.x.grad`` can be read as an input-gradient saliency, and
``SGCN_Ori`` fills the Grad-CAM taps ``final_conv_acts`` / ``final_conv_grads`` (kernel/sgcn.py:16-17,72,124-126); the
reference forms no map from either.  The functions here are what the model classes' ``input_saliency``,
``integrated_gradients`` and ``grad_cam`` run: the class-targeted backward of an eval-mode forward (a one-hot cotangent
on the first output, the log-probabilities — subjects are independent in eval mode, so one backward serves the batch),
and the maps themselves as one launch of csrc/saliency.hip (ops.saliency_maps / ops.grad_cam).

The contract of the sibling passes (``attention_weights``, ``edge_importance``): the pass runs in eval mode and the
model is left as it was — ``training``, parameters, buffers, every parameter's ``.grad`` (the parameters do not require a
gradient for the duration, so no parameter-gradient reduction is formed or queued), ``data.x.grad``,
``data.snps_feat.requires_grad``, the random state; ``last_edge_prob`` and the hand-over to ``loss_probability`` are reset
as after an evaluation sweep.  Eager only: the calls refuse to run under stream capture."""
import torch

from . import ops

INPUTS = ("image", "snps", "both")


def _has_snps(model):
    return hasattr(model, "go_network")


def _check(name, model, data, isExplain, inputs):
    if inputs not in INPUTS:
        raise ValueError(f"{name}: inputs={inputs!r} (one of {INPUTS})")
    if inputs != "image" and not _has_snps(model):
        raise ValueError(f"{name}: {model.__class__.__name__} is an image-only model (inputs='image' only)")
    if isExplain and getattr(model, "single_pass", False):
        raise ValueError(f"{name}: {model.__class__.__name__} has one plain pass (no masked pass)")
    x = data.x
    if x.shape[0] % model.rois:
        raise ValueError(f"every graph must have exactly rois={model.rois} nodes (got {x.shape[0]} nodes)")
    if x.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{name}: runs eagerly only (the current stream is being captured)")


def _logp(model, data, temperature, device, isExplain):
    """The model's first output, the log-probabilities [B, C] (the diagnosis head of SGCN_GCN_CLUSTERLABEL)."""
    if _has_snps(model):
        if getattr(model, "single_pass", False):
            return model(data, temperature, device)[0]
        return model(data, temperature, device, isExplain=isExplain)[0]
    return model(data, isExplain=isExplain)


class _untouched:
    """The model in eval mode with frozen parameters for the duration; on exit the model, ``data.x`` / ``data.snps_feat``
    (the tensors themselves, their ``requires_grad``; ``.grad`` is never written: the gradients are taken with
    ``torch.autograd.grad``) and what a forward leaves on the model are as before."""

    _KEPT = ("input", "final_conv_acts", "final_conv_pair_acts", "_tap", "_fired", "_cut")

    def __init__(self, model, data):
        self.model, self.data = model, data

    def __enter__(self):
        model, data = self.model, self.data
        self.was = model.training
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.x, self.x_rg = data.x, data.x.requires_grad
        self.snps = getattr(data, "snps_feat", None)
        self.snps_rg = None if self.snps is None else self.snps.requires_grad
        self.kept = {k: getattr(model, k) for k in self._KEPT if k in model.__dict__}
        model.eval()
        for p in self.params:
            p.requires_grad_(False)
        return self

    def __exit__(self, *exc):
        model, data = self.model, self.data
        for p in self.params:
            p.requires_grad_(True)
        data.x = self.x
        if self.x.is_leaf:
            self.x.requires_grad_(self.x_rg)
        if self.snps is not None:
            data.snps_feat = self.snps
            if self.snps.is_leaf:
                self.snps.requires_grad_(self.snps_rg)
        for k, v in self.kept.items():
            setattr(model, k, v)
        model.last_edge_prob = None                     # no later loss_probability is served from this batch
        if hasattr(model, "_handoff"):
            model._handoff = type(model._handoff)()
        model.train(self.was)
        return False


def _target(target, logp):
    b, c = logp.shape
    if target is None:
        return logp.detach().argmax(dim=1)              # the predicted class, on the device (no host read)
    if torch.is_tensor(target):
        t = target.reshape(-1).to(device=logp.device, dtype=torch.int64)
        if t.numel() != b:
            raise ValueError(f"target: {t.numel()} classes for {b} subjects")
        return t
    t = int(target)
    if not 0 <= t < c:
        raise ValueError(f"target={t} lies outside the model's {c} classes")
    return torch.full((b,), t, dtype=torch.int64, device=logp.device)


def _one_hot(target, logp):
    """The cotangent [B, C] by comparison, not by indexing: a label outside the classes gives a zero row (and a zero
    map), never an out-of-range access on the device."""
    classes = torch.arange(logp.shape[1], device=logp.device)
    return (classes.view(1, -1) == target.view(-1, 1)).to(logp.dtype)


def _score(logp, target):
    return (logp.detach() * _one_hot(target, logp)).sum(dim=1)


def _grads(model, data, temperature, device, isExplain, x, snps, want_snps, target):
    """One forward on (x, snps) and the backward of the target class's log-probability -> (dx, dsnps or None, logp,
    target)."""
    data.x = x.detach().requires_grad_(True)
    leaves = [data.x]
    if snps is not None:
        data.snps_feat = snps.detach().requires_grad_(want_snps)
        if want_snps:
            leaves.append(data.snps_feat)
    logp = _logp(model, data, temperature, device, isExplain)
    target = _target(target, logp)
    g = torch.autograd.grad(logp, leaves, grad_outputs=_one_hot(target, logp), allow_unused=True)
    g = [torch.zeros_like(t) if d is None else d for t, d in zip(leaves, g)]
    return g[0], (g[1] if want_snps else None), logp.detach(), target


def _snps_map(snps, dsnps, normalize):
    b, s = snps.shape
    a, _ = ops.saliency_maps(snps.reshape(b * s, 1).float(), dsnps.reshape(-1, b * s, 1).float(), s, None, normalize)
    return a.view(b, s)


def input_saliency(model, data, temperature=None, device=None, target=None, isExplain=False, inputs="image",
                   normalize=False):
    _check("input_saliency", model, data, isExplain, inputs)
    want_snps = inputs != "image"
    with _untouched(model, data) as keep:
        dx, dsnps, _, tgt = _grads(model, data, temperature, device, isExplain, keep.x, keep.snps, want_snps, target)
        attr, roi = ops.saliency_maps(keep.x.detach().float(), dx.float(), model.rois, None, normalize)
        out = {"attr": attr, "roi": roi, "target": tgt}
        if want_snps:
            out["snps"] = _snps_map(keep.snps.detach(), dsnps, normalize)
    return out


def integrated_gradients(model, data, temperature=None, device=None, target=None, isExplain=False, inputs="image",
                         normalize=False, steps=16, baseline=None):
    _check("integrated_gradients", model, data, isExplain, inputs)
    steps = int(steps)
    if not 1 <= steps <= ops.SALIENCY_MAX_STEPS:
        raise ValueError(f"integrated_gradients: steps={steps} (1 .. {ops.SALIENCY_MAX_STEPS})")
    move_x, move_s = inputs != "snps", inputs != "image"
    with _untouched(model, data) as keep:
        x = keep.x.detach().float()
        n, h0 = x.shape
        base = None
        if baseline is not None:
            base = baseline.detach().to(device=x.device, dtype=torch.float32).contiguous()
            if tuple(base.shape) not in ((model.rois, h0), (n, h0)):
                raise ValueError(f"integrated_gradients: baseline {tuple(base.shape)} is neither [{model.rois}, {h0}] "
                                 f"nor [{n}, {h0}]")
        base_full = (torch.zeros_like(x) if base is None else
                     base if base.shape[0] == n else base.repeat(n // model.rois, 1))
        snps = None if keep.snps is None else keep.snps.detach()
        with torch.no_grad():                           # the two ends of the path: score(x), score(baseline)
            data.x = x
            logp_x = _logp(model, data, temperature, device, isExplain)
            tgt = _target(target, logp_x)               # None: the prediction at the unscaled input
            data.x = base_full if move_x else x
            if move_s:
                data.snps_feat = torch.zeros_like(snps)
            logp_0 = _logp(model, data, temperature, device, isExplain)
        gap = _score(logp_x, tgt).double() - _score(logp_0, tgt).double()
        dxs, dss = [], []
        for m in range(steps):                          # midpoint rule, one pass after another on the batch's one plan
            alpha = (m + 0.5) / steps
            x_m = torch.lerp(base_full, x, alpha) if move_x else x
            s_m = snps * alpha if move_s else snps
            dx, ds, _, _ = _grads(model, data, temperature, device, isExplain, x_m, s_m, move_s, tgt)
            dxs.append(dx.float())
            dss.append(ds)
        out = {"target": tgt}
        total = torch.zeros_like(gap)
        if move_x:                                      # (delta is the gap of the un-normalised attributions)
            dxs = torch.stack(dxs)
            attr, roi = ops.saliency_maps(x, dxs, model.rois, base, normalize=False)
            total = total + attr.double().sum(dim=(1, 2))
            out["attr"], out["roi"] = ops.saliency_maps(x, dxs, model.rois, base, True) if normalize else (attr, roi)
        if move_s:
            dss = torch.stack(dss)
            sm = _snps_map(snps, dss, False)
            total = total + sm.double().sum(dim=1)
            out["snps"] = _snps_map(snps, dss, True) if normalize else sm
        out["delta"] = (total - gap).float()
    return out


def grad_cam(model, data, target=None, isExplain=False, normalize=True):
    if not hasattr(model, "_tap_fired"):
        raise ValueError(f"grad_cam: {model.__class__.__name__}: the reference never fills final_conv_acts there "
                         "(kernel/sgcn.py:124-126 is SGCN_Ori's)")
    _check("grad_cam", model, data, isExplain, "image")
    with _untouched(model, data) as keep:
        data.x = keep.x.detach().requires_grad_(True)
        logp = model(data, isExplain=isExplain)
        tgt = _target(target, logp)
        acts, tap = model.final_conv_acts, model._tap   # the pre-ReLU conv3 activations of this eval pass
        # the tap's gradient leaves the stack's backward itself (ops.SgcnOriStack / the per-layer route's hook)
        torch.autograd.grad(logp, [data.x], grad_outputs=_one_hot(tgt, logp))
        if tap is None or tap.grads is None:
            raise RuntimeError("grad_cam: the backward did not reach the final_conv_acts tap")
        return ops.grad_cam(acts.detach().float(), tap.grads.detach().float(), model.rois, normalize)
