"""The genetics-only trainer: ``Gene_ontology_network`` alone as a binary classifier on the 54 SNPs
(kernel/train_eval_snps.py — the genetics-only arm of the paper's ablation, and the one consumer of the GO network's
``classification`` module).

Per batch the reference computes (train() :298-335)

    latent, x_hat, ... = model(data, T, device)
    y_hat = model.classification(cat(latent, data))
    loss  = sum BCELoss(y_hat, label) + lambda0 * sum (x_hat - data)^2            lambda0 = 1e-5 (:169)

and takes an Adam step; ``eval_loss`` / ``eval_acc`` / ``eval_scores`` (:338-425) report the loss, accuracy, AUC,
weighted F1, sensitivity and specificity.  As shipped, the reference trainer unpacks THREE values from ``forward``'s
four-tuple (:314; kernel/go_model.py:302 likewise) and raises; everything here takes the first two outputs (latent,
x_hat) and ignores the rest.

A batch of this trainer is a pair of tensors ``(data [B, 54], label [B])`` — the tuples of the reference's SnpsDataset
loader — not a graph ``Batch``: the step, the captured step and the epoch live here, not in ``train.GraphedTrainStep``.

What runs: the GO network's own kernels; behind them the head — BatchNorm1d over the batch, ReLU, dropout, Linear(-> 16),
ReLU, dropout, Linear(16 -> 1), sigmoid — the BCE and the reconstruction term are ONE launch per direction
(``ops.SnpsHeadLoss``, csrc/snps_head.hip) on the GPU with gradients enabled and a shape the launch takes (batch <= 1024);
anywhere else (no gradients, refused shapes, IGCN_NO_HEAD_LOSS_FUSED=1) the same terms from ``ops.BatchNorm1dGrouped``,
``ops.linear`` (the narrow layer: ``ops.small_linear``'s kernel) and torch's sigmoid / binary_cross_entropy — which is
also the independent cross-check of the fused launch on the device.  The head's two dropout sites are drawn by the GO
network's one mask launch (``extra_dropout``).  ``model.classification`` itself stays a plain ``nn.Sequential``: the
``state_dict`` is the reference's.
"""
import torch
import torch.nn.functional as F

from . import _lib, ops, switches
from . import train as T
from .capture import GradTable, ShapeCache, _capture, kept_trainer, rolled_back

SNPS_LAMBDA0 = 1e-5                      # kernel/train_eval_snps.py:169
SNPS_TERMS = ("class", "recon")
EVAL_MAX_ROWS = _lib.LIMITS["IGCN_EVAL_MAX_ROWS"]      # rows one igcn_eval_metrics call takes


def _head(model):
    """(BatchNorm1d(l_dim + 54), Dropout, Linear(-> 16, no bias), Dropout, Linear(16 -> 1)) of ``model.classification``."""
    c = model.classification
    return c[0], c[2], c[3], c[5], c[6]


def _head_unfused(model, latent, data, keep1, keep2):
    """``model.classification(cat(latent, data))`` [B] from the project's existing pieces (torch's own op where a piece
    does not take the tensors: the CPU), with the dropout factors ``keep1`` / ``keep2`` (None: no dropout)."""
    bn, _, lin1, _, lin2 = _head(model)
    x = torch.cat((latent, data), -1)
    training = model.training
    if x.is_cuda and x.dtype == torch.float32:
        a = ops.BatchNorm1dGrouped.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum,
                                         bn.eps, True, 1, keep1)
        h = ops.linear(a, lin1.weight, None, relu=True)
        z = ops.linear(h, lin2.weight, lin2.bias, keep=keep2)
    else:
        a = F.relu(F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, training, bn.momentum, bn.eps))
        if keep1 is not None:
            a = a * keep1
        h = F.relu(F.linear(a, lin1.weight))
        if keep2 is not None:
            h = h * keep2
        z = F.linear(h, lin2.weight, lin2.bias)
    return torch.sigmoid(z).view(-1)


def _fused(model, latent, data):
    return (data.is_cuda and torch.is_grad_enabled() and not switches.on("IGCN_NO_HEAD_LOSS_FUSED")
            and _head(model)[0].momentum is not None and ops.snps_head_supported(latent, data, _head(model)[2].weight))


def losses_snps(model, data, label, lambda0=SNPS_LAMBDA0, temperature=None, lazy_value=False):
    """The loss of train() kernel/train_eval_snps.py:314-320 for one batch ``(data [B, 54], label [B])`` in the model's
    current mode.  Returns (loss, {"class", "recon"}, (latent, x_hat, y_hat [B])).  ``forward`` returns a four-tuple; the
    reference unpacks three values from it and raises (:314) — the first two are taken here.  ``temperature`` is passed to
    the forward, which does not read it.  ``lazy_value``: as in ``train.losses`` (the fused launch writes the value
    itself: nothing is deferred)."""
    bn, d1, lin1, d2, lin2 = _head(model)
    b = int(data.shape[0])
    training = bool(model.training)
    if training and b == 1:
        raise ValueError("losses_snps: training mode needs more than one sample per batch (BatchNorm1d over the batch)")
    extra = [((b, bn.num_features), float(d1.p)), ((b, lin1.weight.shape[0]), float(d2.p))]
    latent, x_hat = model(data, temperature, data.device, extra_dropout=extra, tail_ride=False)[:2]
    keep1, keep2 = model.extra_masks
    y = label.reshape(-1).to(data.dtype)
    lam = float(lambda0)
    if training and bn.track_running_stats:
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
    if _fused(model, latent, data):
        loss, terms, y_hat = ops.SnpsHeadLoss.apply(latent, data, x_hat, y, bn.weight, bn.bias, bn.running_mean,
                                                    bn.running_var, bn.momentum, bn.eps, training, keep1, keep2,
                                                    lin1.weight, lin2.weight, lin2.bias, lam, bool(lazy_value))
        return loss, dict(zip(SNPS_TERMS, terms.unbind(0))), (latent, x_hat, y_hat)
    y_hat = _head_unfused(model, latent, data, keep1, keep2)
    t = {"class": F.binary_cross_entropy(y_hat, y, reduction="sum"),
         "recon": lam * torch.sum((x_hat - data) ** 2) if lam != 0.0 else torch.zeros((), dtype=data.dtype, device=data.device)}
    return t["class"] + t["recon"], t, (latent, x_hat, y_hat)


@torch.no_grad()
def classify(model, latent, data):
    """Eval-mode ``y_hat`` [B] = ``model.classification(cat(latent, data))`` with the running statistics: on the GPU the
    forward launch alone (igcn_snps_head_loss_fwd without labels, a grid over the rows, any batch size)."""
    bn, _, lin1, _, lin2 = _head(model)
    if (data.is_cuda and latent.dtype == data.dtype == torch.float32 and lin1.weight.shape[0] == 16
            and ops.snps_head_supported(latent[:1], data[:1], lin1.weight)):
        return ops.snps_head_predict(latent, data, bn, lin1.weight, lin2.weight, lin2.bias)
    was = model.training
    model.training = False
    try:
        return _head_unfused(model, latent, data, None, None)
    finally:
        model.training = was


def _check_optimizer(optimizer):
    if any(g.get("weight_decay", 0) for g in getattr(optimizer, "param_groups", ())):
        raise ValueError("train_step_snps: weight_decay must be 0 (FlatAdam has no coupled weight decay)")


def _fwd_bwd(model, optimizer, data, label, lambda0, temperature=None):
    """zero_grad, forward, loss, backward (:307-324).  Returns the device vector [loss, class, recon]."""
    optimizer.zero_grad()
    if data.is_cuda:
        T.forget_riders(model)
        T.ensure_unit_grad(data.device)
    loss, terms, _ = losses_snps(model, data, label, lambda0, temperature, lazy_value=True)
    # (no deferred reductions: train._single_use_parameters keeps the deferral to the models whose batched sweep was
    # built for it, and the bare GO network — whose attention read-out feeds nothing here — is not one of them)
    T.backward_to_grads(loss, optimizer, None, defer=T._single_use_parameters(model), tick=True)
    T.assert_nothing_pending("train_step_snps")
    return torch.stack((loss.detach(), terms["class"].detach(), terms["recon"].detach()))


def train_step_snps(model, optimizer, data, label, lambda0=SNPS_LAMBDA0, temperature=None):
    """One iteration of the loop body of train() kernel/train_eval_snps.py:305-330 on ``train.FlatAdam`` (whose
    ``weight_decay`` must be 0).  Returns the (device) loss tensor."""
    _check_optimizer(optimizer)
    vec = _fwd_bwd(model, optimizer, data, label, lambda0, temperature)
    optimizer.step()
    return vec[0]


class GraphedSnpsStep:
    """The whole genetics-only step — forward, loss, backward, Adam — captured ONCE into a hipGraph and replayed per step:
    the protocol of ``capture.py`` for a batch that is a pair of tensors.  ``load(data, label)`` copies a batch of the
    captured shape into the static inputs, ``step()`` replays and returns the loss (a device scalar that the next replay
    overwrites; ``terms`` = the device vector [loss, class, recon]).

    Construction runs ``warmup`` eager steps on the construction batch and rolls them back (``capture.rolled_back``:
    optimiser state, module buffers, the dropout generator's counter): N replays equal N eager steps.  Single process
    only (no gradient exchange)."""

    def __init__(self, model, optimizer, data, label, lambda0=SNPS_LAMBDA0, warmup=3, temperature=None):
        _check_optimizer(optimizer)
        if not data.is_cuda or not isinstance(optimizer, T.FlatAdam) or optimizer.flat_grads:
            raise ValueError("GraphedSnpsStep: needs device tensors and a table-mode train.FlatAdam")
        self.model, self.opt, self.lambda0, self.temperature = model, optimizer, float(lambda0), temperature
        self.data, self.label = data.detach().clone().contiguous(), label.detach().clone().contiguous()
        with rolled_back(model, optimizer):
            for _ in range(int(warmup)):
                self._fwd_bwd()
                optimizer.step()
        self.graph = torch.cuda.CUDAGraph()
        self._table = GradTable(optimizer)
        with _capture(self.graph):
            self.terms = self._fwd_bwd()
            optimizer.step(refresh=False, table=self._table.table)
        self.loss = self.terms[0]
        self._table.seal()
        torch.cuda.synchronize()

    def _fwd_bwd(self):
        return _fwd_bwd(self.model, self.opt, self.data, self.label, self.lambda0, self.temperature)

    def load(self, data, label):
        """Copy a batch of the captured shape into the static inputs; another shape is refused (ValueError)."""
        if tuple(data.shape) != tuple(self.data.shape) or label.numel() != self.label.numel():
            raise ValueError(f"graphed step needs fixed shapes; data {tuple(data.shape)} vs {tuple(self.data.shape)}, "
                             f"label {tuple(label.shape)} vs {tuple(self.label.shape)}")
        with torch.no_grad():
            _lib.copy_multi([(self.data, data), (self.label, label.reshape(self.label.shape))])

    def step(self):
        self._table.claim(self)
        self.graph.replay()
        self.opt.mark_stepped()
        return self.loss

    __call__ = step


class SnpsEpochTrainer(ShapeCache):
    """train() kernel/train_eval_snps.py:298-335 over a whole loader: one captured step per batch SHAPE (the full batches
    and the ragged tail of a loader without ``drop_last``) once the shape has been seen ``capture_after`` times, the eager
    ``train_step_snps`` until then (``capture.ShapeCache``)."""

    def __init__(self, model, optimizer, lambda0=SNPS_LAMBDA0, temperature=None, capture_after=1, max_graphs=4, warmup=2):
        _check_optimizer(optimizer)
        self.model, self.opt, self.lambda0, self.temperature = model, optimizer, float(lambda0), temperature
        self.warmup = int(warmup)
        super().__init__(capture_after, max_graphs)

    def step(self, data, label):
        """One optimisation step; returns the device vector [loss, class, recon] (valid until the next step of the
        same shape)."""
        graphable = data.is_cuda and isinstance(self.opt, T.FlatAdam) and not self.opt.flat_grads
        g = self.lookup((tuple(data.shape), int(label.numel())), graphable,
                        lambda: GraphedSnpsStep(self.model, self.opt, data, label, self.lambda0, self.warmup,
                                                self.temperature),
                        lambda g: g.load(data, label))
        if g is None:
            vec = _fwd_bwd(self.model, self.opt, data, label, self.lambda0, self.temperature)
            self.opt.step()
            return vec
        g.step()
        return g.terms

    def fit_epoch(self, loader, device=None):
        self.model.train()
        total, count = None, 0
        for data, label in _pairs(loader, device):
            vec = self.step(data, label)
            total = vec.clone() if total is None else total + vec       # (a new tensor: a replay overwrites ``vec``)
            count += int(data.shape[0])
        if total is None:
            return 0.0, 0.0, 0.0
        ll, ll_class, ll_reg = (float(v) / count for v in total.tolist())      # the epoch's one synchronisation
        return ll, ll_class, ll_reg


def _pairs(loader, device):
    for data, label in loader:
        if device is not None:
            data, label = data.to(device), label.to(device)
        yield data, label


def fit_epoch_snps(model, optimizer, loader, device=None, lambda0=SNPS_LAMBDA0, temperature=None):
    """``train(model, optimizer, loader, device, criterion_class, criterion_recon, temperature, lambda0)`` of the
    reference (:298-335): one pass over ``loader`` of ``(data, label)`` pairs.  Returns (ll, ll_class, ll_reg): the sums
    of the batches' loss, classification term and reconstruction term divided by the number of samples (:331-335),
    accumulated on the device and read once.  The trainer (and its captured steps) is kept on the optimiser, so calling
    this once per epoch re-uses them.  The learning rate is the caller's: ``optimizer.param_groups[0]['lr'] *= factor``
    (the reference's StepLR(50, 0.7) and its own decay are both such multiplications) is read by the captured steps from
    device memory."""
    key = (id(model), float(lambda0), temperature.data_ptr() if torch.is_tensor(temperature) else temperature)
    tr = kept_trainer(optimizer, "_igcn_snps_trainers", key,
                      lambda: SnpsEpochTrainer(model, optimizer, lambda0, temperature), model)
    return tr.fit_epoch(loader, device)


# ---- evaluation (:338-425) ------------------------------------------------------------------------------------------
@torch.no_grad()
def eval_loss_snps(model, loader, device=None, criterion_class=None, criterion_recon=None, temperature=None,
                   lambda0=SNPS_LAMBDA0):
    """eval_loss() :356-386 — the training loss in eval mode: (ll, ll_class, ll_reg), the three sums over the loader
    divided by the number of samples.  The unfused route (no gradients); accumulated on the device, read once.
    ``criterion_class`` / ``criterion_recon`` are accepted and unused (BCELoss and the squared error, both un-reduced and
    summed, are what the trainer passes)."""
    model.eval()
    total, count = None, 0
    for data, label in _pairs(loader, device):
        loss, t, _ = losses_snps(model, data, label, lambda0, temperature)
        vec = torch.stack((loss, t["class"], t["recon"]))
        total = vec if total is None else total + vec
        count += int(data.shape[0])
    if total is None:
        return 0.0, 0.0, 0.0
    return tuple(float(v) / count for v in total.tolist())


@torch.no_grad()
def _scores(model, loader, device, temperature):
    """(y_hat [n], label [n]) of the whole loader on the loader's device: the GO forward and ``classify`` per batch."""
    model.eval()
    ys, ls = [], []
    for data, label in _pairs(loader, device):
        latent = model(data, temperature, data.device)[0]
        ys.append(classify(model, latent, data))
        ls.append(label.reshape(-1).to(data.dtype))
    if not ys:
        raise ValueError("the loader is empty")
    return torch.cat(ys), torch.cat(ls)


def eval_acc_snps(model, loader, device=None, criterion_class=None, criterion_recon=None, temperature=None,
                  lambda0=SNPS_LAMBDA0):
    """eval_acc() :338-353 — the share of samples with (y_hat > 0.5) == (label > 0.5); counted on the device, read once."""
    y_hat, label = _scores(model, loader, device, temperature)
    return float(((y_hat > 0.5) == (label > 0.5)).sum()) / y_hat.numel()


def eval_scores_snps(model, loader, device=None, criterion_class=None, criterion_recon=None, temperature=None,
                     lambda0=SNPS_LAMBDA0):
    """eval_scores() :388-423 with its 7-tuple (true_label, pred_label, accuracy, auc, f1, sensitivity, specificity);
    the two label arrays are numpy bool, as the reference's.  The prediction is ``y_hat > 0.5`` (a score of exactly 0.5 is
    class 0).  Routes: on the GPU with at most 65536 (EVAL_MAX_ROWS) rows every metric comes from igcn_eval_metrics (C =
    2, scores [log(1 - y_hat), log y_hat], whose order is y_hat's: auc = the Mann-Whitney statistic with ties 1/2, which is what
    roc_curve + auc compute; weighted f1, sensitivity and specificity from its confusion counts) — the thresholding, the
    correct count and the two logarithms are torch launches in front of it; anywhere else (CPU, more rows) the same
    definitions on the host in numpy.  No sklearn.  As in the reference, a NaN score gives auc 0."""
    y_hat, label = _scores(model, loader, device, temperature)
    truth, pred = label > 0.5, y_hat > 0.5
    n = int(y_hat.numel())
    if y_hat.is_cuda and n <= EVAL_MAX_ROWS:
        logp = torch.stack((torch.log1p(-y_hat), torch.log(y_hat)), 1).contiguous()
        p64, t64 = pred.long(), truth.long()
        state = torch.stack((torch.tensor(n, device=y_hat.device), torch.tensor(0, device=y_hat.device),
                             (p64 == t64).sum())).long()
        loss_sum = torch.zeros(1, dtype=torch.float64, device=y_hat.device)
        parts = torch.zeros(2 * ((n + 255) // 256), dtype=torch.int64, device=y_hat.device)
        out = torch.zeros(8 + 4, dtype=torch.float64, device=y_hat.device)
        ops.call("igcn_eval_metrics", n, 2, 0, ops.ptr(logp), ops.ptr(p64), ops.ptr(t64), None, None, ops.ptr(state),
                 ops.ptr(loss_sum), ops.ptr(parts), ops.ptr(out), ops.stream_ptr())
        v = out.cpu().tolist()
        acc, auc, f1, sens, spec = v[3], v[4], v[5], v[6], v[7]
    else:
        acc, auc, f1, sens, spec = _host_metrics(y_hat.cpu().numpy(), truth.cpu().numpy(), pred.cpu().numpy())
    return truth.cpu().numpy(), pred.cpu().numpy(), acc, auc, f1, sens, spec


def _host_metrics(scores, truth, pred):
    """The metrics of eval_scores() on the host, as igcn_eval_metrics defines them."""
    import numpy as np
    n = len(truth)
    cm = np.zeros((2, 2), np.int64)
    for t, p in zip(truth.astype(int), pred.astype(int)):
        cm[t, p] += 1
    pos, neg = scores[truth], scores[~truth]
    if np.isnan(scores).any():
        auc = 0.0
    elif len(pos) == 0 or len(neg) == 0:
        auc = float("nan")
    else:
        auc = (2 * int((pos[:, None] > neg[None, :]).sum()) + int((pos[:, None] == neg[None, :]).sum())) \
            / (2.0 * len(pos) * len(neg))
    (tn, fp), (fn, tp) = cm.tolist()
    f1, wsum = 0.0, 0.0
    for lab in range(2):
        sup, prd, hit = int(cm[lab].sum()), int(cm[:, lab].sum()), float(cm[lab, lab])
        if sup + prd:
            f1 += (2.0 * hit / (sup + prd) if hit else 0.0) * sup
            wsum += sup
    return (float((truth == pred).sum()) / n, auc, f1 / wsum if wsum else 0.0,
            tp / (tp + fn) if tp + fn else float("nan"), tn / (tn + fp) if tn + fp else float("nan"))
