"""Per-fold KNN imputation of the clinical scores on the device (csrc/knn_impute.hip).

The reference's fold loop (kernel/train_eval_sgcn_img_snps.py:85-99) calls ``KNNImputationVal`` (util/tool.py:22-73; the
two-split twin ``KNNImputation`` at :75-111) before it builds a fold's loaders: a ``KNNImputer(n_neighbors=3)`` fitted
on the TRAINING subjects' ``demographics`` (9 columns, NaN = not measured) imputes the three splits, ``scaler4score``
(a ``MinMaxScaler``, sgcn_data.py:127) rescales them, and columns [5, 7, 8] (tau, adas13, mmse) — or the single column
``clinical_score_index`` — overwrite every subject's ``clini_score``: the regression targets of the loss, different in
every fold.  Python loops over ``Data`` objects, two numpy round trips and sklearn; with the dataset resident in HBM
(``loader.UniformGraphStore``) it would also mean pulling the store to the host and rebuilding it per fold.

Here a fold is prepared by ``impute_store`` / ``impute_fold``: the column statistics of the training rows, then one
transform per split that reads ``demographics`` through the split's index vector and writes ``clini_score`` in place.

* ``KNNImputer``                    sklearn's names and meaning on float32 device tensors.
* ``affine_of``                     (scale, shift) of a fitted MinMaxScaler / StandardScaler, duck-typed.
* ``impute_fold`` / ``impute_store``  the fold preparation on tensors / on a device ``UniformGraphStore``.
* ``KNNImputationVal`` / ``KNNImputation``  the reference's signatures on lists of ``Data``: for a maintainer of the
  reference the change is the import of these two names.
* ``fold_indices``                  the tail of ``k_fold`` (:475-483): validation = the previous fold's test subjects.

Semantics are ``KNNImputer(weights="uniform", metric="nan_euclidean")`` with one addition — equal distances go to the
lower training row, where sklearn leaves the choice to ``argpartition`` — and one refusal: a column that no training row
observes raises ``ValueError`` at fit time (sklearn drops it from its output, which would silently shift [5, 7, 8]).
"""
import numpy as np
import torch

from . import ops

DEFAULT_SELECT = (5, 7, 8)          # tau, adas13, mmse (util/tool.py:52)


def _check_counts(counts):
    """The fit's one synchronisation: the per-column counts of observed training values."""
    c = counts.cpu()
    if bool((c < 0).any()):
        raise ValueError("KNN imputation: a training row index lies outside the matrix")
    empty = [int(i) for i in torch.nonzero(c == 0).view(-1)]
    if empty:
        raise ValueError(f"KNN imputation: no training row observes column(s) {empty}; sklearn would drop them from its "
                         "output and shift the selected columns — refusing instead")


class KNNImputer:
    """``sklearn.impute.KNNImputer(n_neighbors=k)`` (uniform weights, nan_euclidean metric, NaN = missing) on float32
    device tensors.  ``fit`` keeps a reference to X; ``transform`` returns a new tensor.  ``last_fallbacks``: device
    int64 [1], the number of entries of the last transform that no neighbour could fill (column mean instead)."""

    def __init__(self, n_neighbors=3):
        self.n_neighbors = int(n_neighbors)
        self.last_fallbacks = None
        self._fit = None

    def fit(self, X):
        counts, means = ops.knn_impute_stats(X)
        _check_counts(counts)
        self._fit, self._means = X.detach().contiguous(), means
        return self

    def _run(self, x, rows_fit, rows_q):
        full, _, _, status = ops.knn_impute(x, self._means, self.n_neighbors, rows_fit, rows_q)
        self.last_fallbacks = status
        return full

    def transform(self, X):
        if self._fit is None:
            raise RuntimeError("KNNImputer.transform before fit")
        if X.dim() != 2 or X.shape[1] != self._fit.shape[1]:
            raise ValueError(f"KNNImputer: X {tuple(X.shape)} does not have the {self._fit.shape[1]} columns of the fit")
        n_fit, n_q = self._fit.shape[0], X.shape[0]
        both = torch.cat([self._fit, X.detach().to(self._fit.device)])
        rows = torch.arange(n_fit + n_q, dtype=torch.int64, device=both.device)
        return self._run(both, rows[:n_fit], rows[n_fit:])

    def fit_transform(self, X):
        self.fit(X)
        return self._run(self._fit, None, None)


def affine_of(scaler, device=None):
    """(scale, shift) float32 tensors with ``scaler.transform(x) == x * scale + shift``: an object with ``scale_`` and
    ``min_`` (MinMaxScaler: x * scale_ + min_) or ``mean_`` and ``scale_`` (StandardScaler: (x - mean_) / scale_)."""
    if hasattr(scaler, "min_") and hasattr(scaler, "scale_"):
        scale = np.asarray(scaler.scale_, dtype=np.float64)
        shift = np.asarray(scaler.min_, dtype=np.float64)
    elif hasattr(scaler, "mean_") and hasattr(scaler, "scale_"):
        scale = 1.0 / np.asarray(scaler.scale_, dtype=np.float64)
        shift = -np.asarray(scaler.mean_, dtype=np.float64) * scale
    else:
        raise TypeError("affine_of: needs scale_ and min_ (MinMaxScaler) or mean_ and scale_ (StandardScaler)")
    return (torch.tensor(scale, dtype=torch.float32, device=device),
            torch.tensor(shift, dtype=torch.float32, device=device))


def impute_fold(demographics, clini_score, train_idx, val_idx, test_idx, scale, shift, select_index=DEFAULT_SELECT, k=3):
    """One fold's ``KNNImputationVal`` on device tensors: fit on ``demographics[train_idx]`` ([S, F] float32, NaN =
    missing), impute train / val / test, apply ``x * scale + shift`` (tensors [F], or None), select ``select_index`` and
    write ``clini_score[idx]`` ([S, len(select_index)] float32) IN PLACE — rows outside the index vectors are left
    untouched.  ``val_idx`` may be None.  Index vectors: int64 on the device, no subject twice.  Returns the fallback
    counts (device int64 [1] each) as (train, val or None, test)."""
    sel = [int(c) for c in select_index]
    if clini_score.dim() != 2 or clini_score.shape[1] != len(sel) or clini_score.shape[0] != demographics.shape[0]:
        raise ValueError(f"impute_fold: clini_score {tuple(clini_score.shape)} is not [{demographics.shape[0]}, {len(sel)}]"
                         f" for select_index {tuple(sel)}")
    if not sel or min(sel) < 0 or max(sel) >= demographics.shape[1]:
        raise ValueError(f"impute_fold: select_index {tuple(sel)} outside the {demographics.shape[1]} columns")
    counts, means = ops.knn_impute_stats(demographics, train_idx)
    _check_counts(counts)
    select = torch.tensor(sel, dtype=torch.int32, device=demographics.device)
    out = []
    for idx in (train_idx, val_idx, test_idx):
        if idx is None:
            out.append(None)
            continue
        out.append(ops.knn_impute(demographics, means, k, train_idx, idx, scale, shift, select, into=clini_score,
                                  want_full=False)[3])
    return tuple(out)


def impute_store(store, train_idx, val_idx, test_idx, scale, shift, select_index=DEFAULT_SELECT, k=3):
    """``impute_fold`` on ``store.cols["demographics"]`` / ``store.cols["clini_score"]`` of a device-resident
    ``UniformGraphStore``: the batches the store hands out afterwards carry the fold's targets."""
    if store.device.type != "cuda":
        raise ValueError("impute_store reads a device-resident store")
    for key in ("demographics", "clini_score"):
        if key not in store.cols:
            raise ValueError(f"impute_store: the store has no {key!r} column")
    return impute_fold(store.cols["demographics"], store.cols["clini_score"], train_idx, val_idx, test_idx, scale, shift,
                       select_index, k)


def _impute_lists(args, lists, scaler4score, k):
    sizes = [len(d) for d in lists]
    demo = torch.stack([d.demographics.reshape(-1) for ds in lists for d in ds]).to(torch.float32)
    dev = torch.device("cuda", torch.cuda.current_device())
    select = DEFAULT_SELECT if args.clinical_score_index == -1 else (int(args.clinical_score_index),)
    scale, shift = affine_of(scaler4score, dev)
    demo = demo.to(dev)
    score = torch.empty(demo.shape[0], len(select), dtype=torch.float32, device=dev)
    bounds = np.cumsum([0] + sizes)
    idx = [torch.arange(int(a), int(b), dtype=torch.int64, device=dev) for a, b in zip(bounds[:-1], bounds[1:])]
    train, rest = idx[0], idx[1:]
    val, test = (rest[0], rest[1]) if len(rest) == 2 else (None, rest[0])
    impute_fold(demo, score, train, val if val is not None and val.numel() else None, test, scale, shift, select, k)
    score = score.cpu()
    row = 0
    for ds in lists:
        for i in range(len(ds)):
            ds[i].clini_score = score[row].clone()
            row += 1


def KNNImputationVal(args, train_dataset, val_dataset, test_dataset, scaler4score, k=3):
    """util/tool.py:22-73 with the imputation, rescaling and selection on the device.  Lists of ``Data``; every item's
    ``clini_score`` becomes a float32 CPU tensor.  Returns (train, test, val) like the reference."""
    _impute_lists(args, [train_dataset, val_dataset, test_dataset], scaler4score, k)
    return train_dataset, test_dataset, val_dataset


def KNNImputation(args, train_dataset, test_dataset, scaler4score, k=3):
    """util/tool.py:75-111 (no validation split).  Returns (train, test)."""
    _impute_lists(args, [train_dataset, test_dataset], scaler4score, k)
    return train_dataset, test_dataset


def fold_indices(test_indices, n):
    """The tail of ``k_fold`` (kernel/train_eval_sgcn_img_snps.py:475-483) for the per-fold test index vectors of a
    split of ``n`` subjects: ``val[i] = test[i - 1]`` and train = every other subject in ascending order.  Returns
    (train_indices, test_indices, val_indices), lists of int64 tensors.  The stratified split itself stays with the
    caller."""
    test_indices = [torch.as_tensor(t, dtype=torch.int64) for t in test_indices]
    folds = len(test_indices)
    val_indices = [test_indices[i - 1] for i in range(folds)]
    train_indices = []
    for i in range(folds):
        mask = torch.ones(int(n), dtype=torch.bool)
        mask[test_indices[i]] = False
        mask[val_indices[i]] = False
        train_indices.append(mask.nonzero().view(-1))
    return train_indices, test_indices, val_indices
