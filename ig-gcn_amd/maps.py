"""The cohort explanation passes — ``attention_maps``, ``association_maps``, ``connectivity_maps`` and ``saliency_maps``
— over one per-class accumulator (``ClassSums``).  Every pass runs a model method per batch, sums what it returns per
class of ``data.y`` on the device (igcn_attn_map_accumulate: fp64, sample order; one call per quantity and batch) and
reads the device once at the end.  ``group_difference`` is a pass of its own: it keeps every subject's map and hands the
table to the max-T permutation test of ``igcn_amd.stats``; ``network_difference`` hands the ROI x ROI tables to its
network-based statistic.  None of them trains; ``igcn_amd.train`` re-exports the six names.
"""
import torch

from . import _lib
from . import ops
from .data import _batches


class ClassSums:
    """fp64 sums [C, Lq, Lk] and int64 counts [C] of the quantities of one pass ``name``, and the one state word in which
    every launch counts the labels it skipped.  ``num_classes``: None reads the model's classification head."""

    def __init__(self, name, model, num_classes=None):
        if num_classes is None:
            head = (model.lin2_classify if getattr(model, "clusterlabel", False) else
                    model.lin2 if hasattr(model, "lin2") else model.fc3)
            num_classes = head.weight.shape[0]
        self.name, self.c = name, int(num_classes)
        if self.c <= 0:
            raise ValueError(f"{name}: num_classes={self.c}")
        self.acc = {}                                            # quantity -> (sums, counts, the shape of one subject's map)
        self.state, self.zero_y = None, {}
        self.n = self.labelled = 0

    def add(self, data, labelled, unlabelled=None):
        """One batch.  ``labelled`` (quantity -> [B, ...] fp32, in launch order) is summed per class of ``data.y``;
        ``unlabelled`` after it into one-class tables, for the quantities that are averaged over everybody."""
        dev = next(iter(labelled.values())).device
        if self.state is None:
            self.state = torch.zeros(1, dtype=torch.int64, device=dev)
        y = data.y.view(-1).to(device=dev, dtype=torch.int64).contiguous()
        for name, t in labelled.items():
            self._accumulate(name, t, y, True)
        if unlabelled:
            if y.numel() not in self.zero_y:
                self.zero_y[y.numel()] = torch.zeros_like(y)
            for name, t in unlabelled.items():
                self._accumulate(name, t, self.zero_y[y.numel()], False)     # (label 0 of 1 class: never skipped)
        self.n += int(data.num_graphs)

    def _accumulate(self, name, t, y, labelled):
        t = t.contiguous()
        w = t.unsqueeze(2) if t.dim() == 2 else t.view(t.shape[0], -1, t.shape[-1])
        if name not in self.acc:
            c = self.c if labelled else 1
            self.acc[name] = (torch.zeros(c, w.shape[1], w.shape[2], dtype=torch.float64, device=w.device),
                              torch.zeros(c, dtype=torch.int64, device=w.device), tuple(t.shape[1:]))
            self.labelled += labelled
        ops.attention_map_accumulate(w, y, *self.acc[name][:2], self.state)

    def finish(self):
        """The number of subjects, after the pass's one synchronisation."""
        if self.n == 0:
            raise ValueError(f"{self.name}: the loader is empty")
        skipped = int(self.state.item()) // self.labelled       # every labelled quantity counted the same bad labels
        if skipped:
            raise _lib.IgcnError(f"{self.name}: {skipped} of {self.n} labels lie outside [0, {self.c})")
        return self.n

    def count(self, name):
        return self.acc[name][1]

    def mean(self, name):
        """fp64 [C, ...]: the class means, zeros for a class without subjects."""
        sums, counts, shape = self.acc[name]
        return (sums / counts.clamp(min=1).view(-1, 1, 1).double()).view(-1, *shape)

    def overall(self, name):
        """fp64 [...]: the mean over all subjects."""
        return (self.acc[name][0].sum(0) / float(self.n)).view(self.acc[name][2])


def _go_rows(model, n_top, device):
    n_nodes = int(model.go_network.n_nodes)
    return torch.arange(n_nodes - n_top, n_nodes, dtype=torch.int64, device=device)


def attention_maps(model, loader, temperature=None, device=None, isExplain=False, num_classes=None, top_k=10):
    """The ROI x GO-term attention table of a cohort: ``model.attention_weights`` (the weights
    ``self.multihead_attn`` returns at kernel/sgcn_img_snp.py:240, which the reference discards) of every batch of
    ``loader``, summed per class of ``data.y`` on the device (igcn_attn_map_accumulate: fp64, sample order) and read
    once at the end.  Returns a dict: ``mean`` [C, rois, Ntop] (fp32; zeros for a class without subjects), ``count`` [C]
    (int64), ``overall`` [rois, Ntop] (the count-weighted mean over the classes), ``go_rows`` [Ntop] (int64: the GO node
    behind every key row — the encoder drops the two deepest levels, which lead the builder's node order, so the rows
    are nodes N - Ntop .. N - 1), ``top_terms`` [rois, top_k] (int64: the GO nodes of the ``top_k`` largest entries
    of every row of ``overall``) and ``n`` (subjects).  A label outside [0, C) raises IgcnError after the pass."""
    acc = ClassSums("attention_maps", model, num_classes)
    for data in _batches(loader, device):
        acc.add(data, {"w": model.attention_weights(data, temperature, device, isExplain)})
    n = acc.finish()
    overall = acc.overall("w").float()
    go_rows = _go_rows(model, overall.shape[1], overall.device)
    top = torch.topk(overall, min(int(top_k), overall.shape[1]), dim=1).indices
    return {"mean": acc.mean("w").float(), "count": acc.count("w"), "overall": overall, "go_rows": go_rows,
            "top_terms": go_rows[top], "n": n}


def association_maps(model, loader, temperature=None, device=None, isExplain=False, num_classes=None, top_k=10):
    """The ROI x SNP association table of a cohort: ``model.snp_association`` — the cross-attention weights of
    kernel/sgcn_img_snp.py:240 times the attention roll-out of the GO encoder (go_model.py:208-251) down to the 54
    SNPs — of every batch of ``loader``, summed per class of ``data.y`` on the device (igcn_attn_map_accumulate with
    Lk = 54: fp64, sample order) and read once at the end.  Returns a dict: ``mean`` [C, rois, 54] (fp32; zeros for a
    class without subjects), ``count`` [C] (int64), ``overall`` [rois, 54] (the mean over all subjects), ``go_to_snp``
    [Ntop, 54] (the cohort mean of the roll-out R_top itself), ``go_rows`` [Ntop] (int64: the GO node behind every row
    of ``go_to_snp``, as in ``attention_maps``), ``top_snps`` [rois, top_k] (int64: the SNP columns of the ``top_k``
    largest entries of every row of ``overall``) and ``n`` (subjects).  A label outside [0, C) raises IgcnError after
    the pass."""
    acc = ClassSums("association_maps", model, num_classes)
    for data in _batches(loader, device):
        a, r_top = model._snp_association(data, temperature, device, isExplain)
        acc.add(data, {"a": a}, {"r_top": r_top})
    n = acc.finish()
    overall, go_to_snp = acc.overall("a").float(), acc.overall("r_top").float()
    top = torch.topk(overall, min(int(top_k), overall.shape[1]), dim=1).indices
    return {"mean": acc.mean("a").float(), "count": acc.count("a"), "overall": overall, "go_to_snp": go_to_snp,
            "go_rows": _go_rows(model, go_to_snp.shape[0], overall.device), "top_snps": top, "n": n}


def connectivity_maps(model, loader, source="mask", weighted=False, isExplain=False, num_classes=None, top_k=10,
                      symmetric=False, temperature=None, device=None):
    """The ROI x ROI connectivity table of a cohort — the brain connections the model keeps.  ``source="mask"``:
    ``model.edge_importance`` (the connective-importance mask of cal_probability, kernel/sgcn_img_snp.py:133-151;
    ``weighted``: times the edge weight); ``source="gat"``: ``model.gat_attention`` (the per-edge GATConv attention of
    every layer, kernel/sgcn.py:235-267 / kernel/gcn_img_snp.py:217-221; ``isExplain``: of the masked pass).  Every
    batch's maps are summed per class of ``data.y`` on the device (igcn_attn_map_accumulate: fp64, sample order; one
    call per quantity) and read once at the end.  Maps are indexed [source region, target region], like ``data.A``.
    Returns a dict: ``mean`` [C, R, R] ([C, L, R, R] for "gat"; fp32, zeros for a class without subjects), ``count`` [C]
    (int64), ``overall`` [R, R] ([L, R, R]: the mean over all subjects), ``strength`` [R] ((row sum + column sum) / 2 of
    ``overall``; of its layer mean for "gat"), ``top_edges`` [top_k, 2] (int64: the (source, target) pairs of the largest
    entries of ``overall`` / its layer mean, largest first), ``n`` (subjects) and, for "mask" only, ``present`` [R, R]
    (the mean number of stored copies of the edge per subject) and ``mean_present`` [R, R] (``overall / present`` where
    ``present > 0``, else 0: the mean mask over the subjects that store the edge).  ``symmetric``: ``mean``, ``overall``,
    ``mean_present`` and ``present`` are returned as (M + M^T) / 2 (per layer for "gat"), applied once to the finished
    tables; ``strength`` and ``top_edges`` are taken from the ``overall`` that is returned.  ``temperature`` is accepted
    for the signature of the sibling passes (no GO network runs here).  A label outside [0, C) raises IgcnError after the
    pass."""
    if source not in ("mask", "gat"):
        raise ValueError(f"connectivity_maps: source={source!r} ('mask' or 'gat')")
    acc = ClassSums("connectivity_maps", model, num_classes)
    for data in _batches(loader, device):
        if source == "mask":
            m, cnt = model.edge_importance(data, weighted=weighted, return_count=True)
            acc.add(data, {"m": m}, {"present": cnt})
        else:
            acc.add(data, {"m": model.gat_attention(data, isExplain=isExplain)})
    n = acc.finish()
    sym = (lambda t: (t + t.transpose(-1, -2)) / 2) if symmetric else (lambda t: t)     # (in fp64, rounded once after)
    overall = acc.overall("m")
    out = {"mean": sym(acc.mean("m")).float(), "count": acc.count("m"), "overall": sym(overall).float(), "n": n}
    if source == "mask":
        present = acc.overall("present")
        mean_present = torch.where(present > 0, overall / present.clamp(min=1e-300), torch.zeros_like(overall))
        out["present"], out["mean_present"] = sym(present).float(), sym(mean_present).float()
    flat = out["overall"] if overall.dim() == 2 else out["overall"].double().mean(0).float()
    r = flat.shape[-1]
    out["strength"] = ((flat.double().sum(1) + flat.double().sum(0)) / 2).float()
    top = torch.topk(flat.reshape(-1), min(int(top_k), r * r)).indices
    out["top_edges"] = torch.stack((top // r, top % r), dim=1)
    return out


def saliency_maps(model, loader, method="gradxinput", target=None, inputs="image", isExplain=False, steps=16,
                  baseline=None, normalize=True, num_classes=None, top_k=10, temperature=None, device=None):
    """The ROI x modality saliency table of a cohort — which regions, in which imaging modality, drive the predicted
    class.  ``method``: "gradxinput" (``model.input_saliency``), "ig" (``model.integrated_gradients`` with ``steps`` and
    ``baseline``) or "gradcam" (``SGCN_Ori.grad_cam``).  ``target``: None (every subject's predicted class), "label"
    (``data.y``) or an int.  Every batch's maps are summed per class of ``data.y`` on the device
    (igcn_attn_map_accumulate: fp64, sample order; one call per quantity) and read once at the end.  Returns a dict:
    ``mean`` [C, R, H0] ([C, R] for "gradcam"; fp32, zeros for a class without subjects), ``roi_mean`` [C, R] (the
    class mean of the per-subject ``roi`` = sum_h |attr|; the map itself for "gradcam"), ``overall`` / ``roi_overall``
    [R] (the means over all subjects), ``count`` [C] (int64), ``n`` (subjects), ``top_regions`` [top_k] (int64: the
    regions of the largest ``roi_overall``, largest first); with ``inputs`` "snps" / "both" also ``snps_mean`` [C, 54]
    and ``top_snps`` [top_k] (by the magnitude of the mean over all subjects); for "ig" ``mean_abs_delta`` (a float:
    the mean quadrature gap).  "ig" with ``inputs="snps"`` moves the SNP vector alone: the image keys are absent.  A
    label outside [0, C) raises IgcnError after the pass."""
    if method not in ("gradxinput", "ig", "gradcam"):
        raise ValueError(f"saliency_maps: method={method!r} ('gradxinput', 'ig' or 'gradcam')")
    if not (target is None or target == "label" or (isinstance(target, int) and not isinstance(target, bool))):
        raise ValueError(f"saliency_maps: target={target!r} (None, 'label' or an int)")
    if method == "gradcam" and inputs != "image":
        raise ValueError("saliency_maps: 'gradcam' maps the image branch only (inputs='image')")
    acc = ClassSums("saliency_maps", model, num_classes)
    delta_sum = None
    for data in _batches(loader, device):
        tgt = data.y.view(-1) if isinstance(target, str) else target
        if method == "gradcam":
            r = {"roi": model.grad_cam(data, target=tgt, isExplain=isExplain, normalize=normalize)}
        elif method == "ig":
            r = model.integrated_gradients(data, temperature, device, target=tgt, isExplain=isExplain, inputs=inputs,
                                           normalize=normalize, steps=steps, baseline=baseline)
        else:
            r = model.input_saliency(data, temperature, device, target=tgt, isExplain=isExplain, inputs=inputs,
                                     normalize=normalize)
        acc.add(data, {k: r[k] for k in ("attr", "roi", "snps") if k in r})
        if "delta" in r:
            d = r["delta"].double().abs().sum()
            delta_sum = d if delta_sum is None else delta_sum + d
    out = {"n": acc.finish()}
    if "roi" in acc.acc:
        out.update({"count": acc.count("roi"), "roi_mean": acc.mean("roi").float(),
                    "roi_overall": acc.overall("roi").float()})
        if method == "gradcam":                                  # (the map is its own regional summary)
            out.update({"mean": out["roi_mean"], "overall": out["roi_overall"]})
        else:
            out.update({"mean": acc.mean("attr").float(), "overall": acc.overall("attr").float()})
        out["top_regions"] = torch.topk(out["roi_overall"], min(int(top_k), out["roi_overall"].numel())).indices
    if "snps" in acc.acc:
        out.setdefault("count", acc.count("snps"))
        out["snps_mean"] = acc.mean("snps").float()
        snps_overall = acc.overall("snps").float()
        out["top_snps"] = torch.topk(snps_overall.abs(), min(int(top_k), snps_overall.shape[0])).indices
    if delta_sum is not None:
        out["mean_abs_delta"] = float(delta_sum) / out["n"]
    return out


QUANTITIES = ("association", "attention", "connectivity", "saliency")


def _subject_maps(model, data, quantity, kw):
    """[B, ...] fp32: the per-subject maps of one batch, from the model method the corresponding cohort pass calls."""
    temperature, device, explain = kw.get("temperature"), kw.get("device"), kw.get("isExplain", False)
    if quantity == "attention":
        return model.attention_weights(data, temperature, device, explain)
    if quantity == "association":
        return model.snp_association(data, temperature, device, explain)
    if quantity == "connectivity":
        if kw.get("source", "mask") == "mask":
            return model.edge_importance(data, weighted=kw.get("weighted", False))
        return model.gat_attention(data, isExplain=explain)
    target = kw.get("target")
    tgt = data.y.view(-1) if isinstance(target, str) else target
    return model.input_saliency(data, temperature, device, target=tgt, isExplain=explain,
                                inputs=kw.get("inputs", "image"), normalize=kw.get("normalize", True))["attr"]


def _stack_subject_maps(who, loader, device, subject_maps):
    """(x [n, ...] fp32, labels [n] int64): the per-subject maps ``subject_maps(data)`` [B, ...] of every batch copied
    into one preallocated [S_all, E] device buffer, ``data.y`` beside it."""
    total = len(loader.dataset) if hasattr(loader, "dataset") else sum(int(d.num_graphs) for d in loader)
    buf = labels = None
    n = 0
    for data in _batches(loader, device):
        m = subject_maps(data).detach()
        b = int(m.shape[0])
        if buf is None:
            shape = tuple(m.shape[1:])
            buf = ops._buffer((total, m[0].numel()), torch.float32, m.device)
            labels = ops._buffer((total,), torch.int64, m.device)
        if n + b > total:
            raise ValueError(f"{who}: the loader yields more than its {total} subjects")
        buf[n:n + b] = m.reshape(b, -1)
        labels[n:n + b] = data.y.view(-1)
        n += b
    if n == 0:
        raise ValueError(f"{who}: the loader is empty")
    return buf[:n].view(n, *shape), labels[:n]


def group_difference(model, loader, quantity="association", groups=(0, 1), permutations=10000, seed=0, members=None,
                     top_k=10, **pass_kw):
    """Which entries of a cohort map differ between two diagnosis groups, corrected over the whole map: the two-sample
    max-T permutation test (``stats.permutation_test``) on the per-subject maps of ``quantity`` — "association"
    (``model.snp_association``), "attention" (``model.attention_weights``), "connectivity" (``model.edge_importance``,
    or ``model.gat_attention`` with ``source="gat"``) or "saliency" (``model.input_saliency``'s ``attr``).  ``pass_kw``
    are the keywords of the corresponding cohort pass (``temperature``, ``device``, ``isExplain``; ``source``,
    ``weighted``; ``target``, ``inputs``, ``normalize``).  A pass of its own: every batch's maps are copied into one
    preallocated [S_all, E] device buffer, the labels beside it, and nothing is summed per class.  Returns the dict of
    ``stats.permutation_test`` in the map's shape plus ``significant`` (int64: the flat indices of the entries with
    ``p_fwe <= 0.05``, largest |t| first, at most ``top_k``).  A group with fewer than 2 subjects raises ValueError.

    With three to five labels in ``groups`` (``groups=(0, 1, 2)``) the question is where the groups differ at all: the
    max-F permutation test ``stats.permutation_anova``, whose dict is returned instead; ``members`` then carries its
    label rows (uint8 [P, S], codes in the order of ``groups``) and ``significant`` lists the largest F first."""
    from . import stats
    if quantity not in QUANTITIES:
        raise ValueError(f"group_difference: quantity={quantity!r} (one of {QUANTITIES})")
    known = set(("temperature", "device", "isExplain") + {"connectivity": ("source", "weighted"),
                                                          "saliency": ("target", "inputs", "normalize")}.get(quantity, ()))
    if set(pass_kw) - known:
        raise TypeError(f"group_difference: {quantity!r} takes no {sorted(set(pass_kw) - known)}")
    if pass_kw.get("source", "mask") not in ("mask", "gat"):
        raise ValueError(f"group_difference: source={pass_kw['source']!r} ('mask' or 'gat')")
    x, labels = _stack_subject_maps("group_difference", loader, pass_kw.get("device"),
                                    lambda data: _subject_maps(model, data, quantity, pass_kw))
    if len(groups) > 2:
        out = stats.permutation_anova(x, labels, groups=groups, permutations=permutations, seed=seed, labels=members)
        t_abs = out["f"].reshape(-1)
    else:
        out = stats.permutation_test(x, labels, groups=groups, permutations=permutations, seed=seed, members=members)
        t_abs = out["t"].reshape(-1).abs()
    hit = torch.nonzero(out["p_fwe"].reshape(-1) <= 0.05).view(-1)
    order = torch.argsort(t_abs[hit], descending=True, stable=True)[:max(int(top_k), 0)]
    out["significant"] = hit[order]
    return out


def network_difference(model, loader, source="mask", groups=(0, 1), threshold=3.1, tail="both", permutations=5000,
                       seed=0, members=None, symmetric=False, weighted=False, layer=-1, isExplain=False, device=None):
    """Which connected sub-networks of the ROI x ROI connectivity maps differ between two diagnosis groups: the
    network-based statistic (``stats.network_based_statistic``) on the per-subject maps of ``source`` — "mask"
    (``model.edge_importance``, with ``weighted``) or "gat" (layer ``layer`` of ``model.gat_attention``, with
    ``isExplain``).  A pass of its own, like ``group_difference``: every subject's map is kept.  ``threshold``, ``tail``,
    ``permutations``, ``seed``, ``members`` and ``symmetric`` are those of the statistic.  Returns its dict plus
    ``significant`` (int64: the labels of the components with ``p_fwe <= 0.05``, largest extent first).  A group with fewer
    than 2 subjects raises ValueError."""
    from . import stats
    if source not in ("mask", "gat"):
        raise ValueError(f"network_difference: source={source!r} ('mask' or 'gat')")
    subject_maps = ((lambda data: model.edge_importance(data, weighted=weighted)) if source == "mask" else
                    (lambda data: model.gat_attention(data, isExplain=isExplain)[:, layer]))
    x, labels = _stack_subject_maps("network_difference", loader, device, subject_maps)
    out = stats.network_based_statistic(x, labels, groups=groups, threshold=threshold, tail=tail,
                                        permutations=permutations, seed=seed, members=members, symmetric=symmetric)
    comp, extent = out["component"], out["extent"]
    roots = torch.nonzero((comp == torch.arange(comp.numel(), device=comp.device)) & (out["p_fwe"] <= 0.05)).view(-1)
    out["significant"] = roots[torch.argsort(extent[roots], descending=True, stable=True)]
    return out
