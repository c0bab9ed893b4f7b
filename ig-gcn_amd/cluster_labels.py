"""Cluster labels on the device: exact t-SNE and KMeans (csrc/tsne.hip, csrc/kmeans.hip).

``SGCN_GCN_CLUSTERLABEL`` trains against two per-subject inputs: ``clust_y``, the cluster label its second head
predicts, and ``tsne_fdim``, the embedding behind the RBF Laplacian of the soft-similarity loss.  The reference makes both
in util/image_cluster.py:148-282 (``run_cluster_ADNI874``) with sklearn on the host — exact t-SNE of the normalised
image features, KMeans(2) on the embedding, ``calculate_WSS`` over k = 1..10 — saves them, and sgcn_data.py:145-157,
263-266 loads them back.  Here the same pipeline runs on float32 device tensors and writes a device-resident
``loader.UniformGraphStore`` in place.

* ``TSNE``            sklearn 1.7's ``TSNE(method="exact")`` for 2 components: names, defaults and stopping rules.
* ``KMeans``          sklearn's Lloyd ``KMeans`` (one run: ``n_init="auto"`` with k-means++ or an array).
* ``wss_curve``       the reference's ``calculate_WSS``: the inertia for k = 1..kmax.
* ``cluster_labels``  the reference's pipeline: features -> (clust_y, embedding, info).
* ``label_store``     ``clust_y`` / ``tsne_fdim`` of a device store, in place.

What is NOT sklearn's: ``init="pca"`` takes the exact top-2 principal components (sklearn runs a randomized PCA that is
not reproduced; the components agree to its accuracy and up to sign), with each component's sign fixed so that its
largest-magnitude loading is positive; equal distances go to the lower centre / point; the arithmetic is fp32 with the
perplexity search, the scans and the cluster sums in fp64.  The gradient descent is chaotic: a run agrees with sklearn's
in what it optimises (KL divergence, recovered clusters), not in coordinates.

Supported: 4 <= S <= 4096 subjects, 1 <= D <= 1024 features (ops.TSNE_MIN_S, TSNE_MAX_S, TSNE_MAX_D), 2 embedding
dimensions, 1 <= k <= 16 clusters (ops.KMEANS_MAX_K), KMeans input width 1 <= d <= 1024 (ops.KMEANS_MAX_D); anything else
raises ``ValueError``.
"""
import numpy as np
import torch

from . import ops
from .capture import _capture

N_ITER_CHECK = 50            # sklearn's _gradient_descent n_iter_check
EXPLORATION_ITERS = 250      # sklearn's _EXPLORATION_MAX_ITER (early exaggeration, momentum 0.5)


def auto_learning_rate(n_samples, early_exaggeration):
    """sklearn's ``learning_rate="auto"``: max(S / early_exaggeration / 4, 50)."""
    return max(float(n_samples) / float(early_exaggeration) / 4.0, 50.0)


def pca_sign_fix(components):
    """Each row (component) of ``components`` [c, D] with its sign chosen so that its largest-magnitude loading is
    positive (the first of equal magnitudes decides)."""
    components = torch.as_tensor(components)
    lead = components.abs().argmax(dim=1)
    sign = torch.sign(components.gather(1, lead.view(-1, 1)))
    sign[sign == 0] = 1
    return components * sign


def _points(x, what, lo, hi_rows, hi_cols):
    """``ops.cl_matrix`` — the one input check — and the shape: (x detached and contiguous, rows, columns)."""
    x = ops.cl_matrix(x, what, lo, hi_rows, hi_cols)
    return x, int(x.shape[0]), int(x.shape[1])


def pca_init(x):
    """sklearn's ``init="pca"`` start with an EXACT PCA: the top-2 principal components of x [S, D] (device), signs by
    ``pca_sign_fix``, scaled so that column 0 has standard deviation 1e-4.  Set-up, not hot path: the centred covariance
    [D, D] and the projection are exact-fp32 GEMMs on the device, the eigendecomposition runs once on the host in fp64."""
    if x.shape[1] < 2:
        raise ValueError("TSNE(init='pca'): two components need at least 2 features")
    xc = (x - x.mean(0, keepdim=True)).contiguous()
    cov = ops.gemm_tn(xc, xc)
    _, vec = torch.linalg.eigh(cov.double().cpu())                       # ascending eigenvalues
    comps = pca_sign_fix(vec[:, [-1, -2]].T.contiguous()).to(torch.float32).to(x.device)
    y = ops.gemm_nt(xc, comps.contiguous())
    return (y / y[:, 0].std(unbiased=False) * 1e-4).contiguous()


class TSNE:
    """``sklearn.manifold.TSNE(method="exact")`` for float32 device tensors and 2 components.

    ``fit_transform(X)`` -> float32 [S, 2] device tensor; afterwards ``embedding_``, ``kl_divergence_`` (of the embedding
    returned), ``n_iter_``, ``learning_rate_`` and ``betas_`` (device float64 [S]).  250 exploration iterations at
    momentum 0.5 under the early exaggeration, then momentum 0.8 with ``update`` and ``gains`` started afresh, as
    sklearn's second ``_gradient_descent`` call starts them; every 50 iterations the KL divergence and the gradient norm
    are read back — the descent's only synchronisation — and it stops on no progress for 250 /
    ``n_iter_without_progress`` iterations or on a gradient norm <= ``min_grad_norm``.  A block of 50 iterations is
    captured once per phase and replayed; ``captured=False``, or a ``max_iter`` that is no multiple of 50, runs the same
    launches eagerly (the same bits).
    ``init``: "pca" (``pca_init``: exact, not sklearn's randomized PCA) or a float32 [S, 2] tensor used as is.
    ``kl_at_exploration_end_``: the KL divergence (of the exaggerated P) at the last check of the first phase."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, init="pca", captured=True):
        if int(n_components) != 2:
            raise ValueError(f"TSNE: {n_components} embedding dimensions; only 2 are supported")
        if float(early_exaggeration) < 1.0:
            raise ValueError("TSNE: early_exaggeration must be at least 1")
        if not (learning_rate == "auto" or float(learning_rate) > 0):
            raise ValueError("TSNE: learning_rate must be 'auto' or positive")
        if int(max_iter) < EXPLORATION_ITERS:
            raise ValueError(f"TSNE: max_iter must be at least {EXPLORATION_ITERS}")
        if not (torch.is_tensor(init) or init == "pca"):
            raise ValueError("TSNE: init must be 'pca' or a float32 [S, 2] tensor")
        self.n_components, self.perplexity, self.early_exaggeration = 2, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.max_iter = learning_rate, int(max_iter)
        self.n_iter_without_progress, self.min_grad_norm = int(n_iter_without_progress), float(min_grad_norm)
        self.init, self.captured = init, bool(captured)

    # one _gradient_descent call of sklearn: iterations it .. max_iter - 1
    def _descend(self, st, it, max_iter, exaggeration, momentum, patience):
        lr = self.learning_rate_
        st.update.zero_()                                    # every call starts from update = 0, gains = 1 (_t_sne.py:
        st.gains.fill_(1.0)                                  # 387-389): momentum and gains do NOT survive the phase switch

        def run(i0, i1):                                     # the launches of iterations i0 .. i1 - 1
            for i in range(i0, i1):
                check = (i + 1) % N_ITER_CHECK == 0 or i == max_iter - 1
                ops.tsne_grad(st, want_kl=check)
                ops.tsne_update(st, exaggeration, momentum, lr, check=check)

        whole = self.captured and it % N_ITER_CHECK == 0 and max_iter % N_ITER_CHECK == 0 and max_iter > it
        graph = None
        if whole:                                            # every block of this call is the same chain of 101 launches
            graph = torch.cuda.CUDAGraph()
            with _capture(graph):
                run(it, it + N_ITER_CHECK)
        best, best_iter, error, i = float("inf"), it, float("nan"), it
        while i < max_iter:
            end = min(max_iter, (i // N_ITER_CHECK + 1) * N_ITER_CHECK)
            if graph is not None:
                graph.replay()
            else:
                run(i, end)
            i = end - 1
            status = st.status.cpu()                         # the block's one synchronisation
            error, grad_norm = float(status[0]), float(status[1])
            if end % N_ITER_CHECK == 0:
                if error < best:
                    best, best_iter = error, i
                elif i - best_iter > patience:
                    break
                if grad_norm <= self.min_grad_norm:
                    break
            i = end
        return error, min(i, max_iter - 1)

    def fit_transform(self, X):
        if torch.is_tensor(X) and X.dim() == 2 and 0 < X.shape[0] <= self.perplexity:     # sklearn's refusal, first
            raise ValueError(f"TSNE: perplexity ({self.perplexity}) must be less than n_samples ({X.shape[0]})")
        if self.perplexity <= 0:
            raise ValueError("TSNE: perplexity must be positive")
        x, s, _ = _points(X, "TSNE", ops.TSNE_MIN_S, ops.TSNE_MAX_S, ops.TSNE_MAX_D)
        if torch.is_tensor(self.init):
            y0 = _points(self.init, "TSNE init", s, s, 2)[0].to(x.device)
            if y0.shape[1] != 2:
                raise ValueError(f"TSNE: init {tuple(self.init.shape)} is not [{s}, 2]")
        else:
            y0 = pca_init(x)
        self.learning_rate_ = (auto_learning_rate(s, self.early_exaggeration) if self.learning_rate == "auto"
                               else float(self.learning_rate))
        p, self.betas_, pstats = ops.tsne_joint_p(ops.tsne_sqdist(x), self.perplexity)
        st = ops.TsneState(p, pstats, y0)
        if self.captured:                                    # every kernel of a block once, outside a capture, on a copy
            warm = ops.TsneState(p, pstats, y0)
            ops.tsne_grad(warm, want_kl=True)
            ops.tsne_update(warm, 1.0, 0.5, 0.0, check=True)
        error, it = self._descend(st, 0, EXPLORATION_ITERS, self.early_exaggeration, 0.5, EXPLORATION_ITERS)
        self.kl_at_exploration_end_ = error
        if it < EXPLORATION_ITERS or self.max_iter > EXPLORATION_ITERS:
            if self.max_iter > it + 1:
                error, it = self._descend(st, it + 1, self.max_iter, 1.0, 0.8, self.n_iter_without_progress)
        # sklearn reports the divergence one update before the embedding it returns; here it is that of the embedding
        # itself: one more pass over P on a copy of the state, with a step of length 0
        last = ops.TsneState(p, pstats, st.y)
        ops.tsne_grad(last, want_kl=True)
        ops.tsne_update(last, 1.0, 0.0, 0.0, check=True)
        self.kl_divergence_, self.n_iter_ = float(last.status[0]), it
        self.embedding_ = st.y
        return st.y

    def fit(self, X):
        self.fit_transform(X)
        return self


def _kmeanspp_draws(n, k, random_state):
    """The random numbers of sklearn's ``_kmeans_plusplus`` from ``numpy.random.RandomState(random_state)``, by the same
    calls in the same order: one ``choice(n, p=uniform)`` — the first centre — then one ``uniform(size=t)`` per further
    centre, t = 2 + floor(ln k)."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    t = 2 + int(np.log(k))
    weight = np.ones(n, dtype=np.float32)                    # sklearn's sample weights take the dtype of X
    first = int(rs.choice(n, p=weight / weight.sum()))
    return first, np.stack([rs.uniform(size=t) for _ in range(k - 1)]) if k > 1 else np.zeros((0, t))


def kmeans_plusplus(x, n_clusters, random_state=None):
    """sklearn's greedy k-means++ (``_kmeans_plusplus``) on x [N, d] (device): (centres [k, d], indices [k] int64 on the
    device).  The random numbers are drawn on the host (``_kmeanspp_draws``) and uploaded once."""
    x, n, _ = _points(x, "kmeans_plusplus", 1, ops.KMEANS_MAX_N, ops.KMEANS_MAX_D)
    k = int(n_clusters)
    if not 1 <= k <= ops.KMEANS_MAX_K or k > n:
        raise ValueError(f"kmeans_plusplus: {k} clusters outside 1..min({ops.KMEANS_MAX_K}, N={n})")
    first, draws = _kmeanspp_draws(n, k, random_state)
    dev = x.device
    u = torch.from_numpy(draws).to(dev)
    chosen = torch.empty(k, dtype=torch.int64, device=dev)
    chosen[0] = first
    _, closest, _, _, stats = ops.kmeans_assign(x, x[first:first + 1].contiguous(), want_sums=False)
    pot = stats[0:1].clone()
    for c in range(1, k):
        ops.kmeanspp_step(x, u[c - 1], closest, pot, chosen[c:c + 1])
    return x[chosen].contiguous(), chosen


class KMeans:
    """``sklearn.cluster.KMeans(algorithm="lloyd")`` on float32 device tensors, one run (sklearn's ``n_init="auto"`` for
    k-means++ or an array init).  ``fit`` / ``predict`` / ``fit_predict``; ``cluster_centers_`` [k, d] float32,
    ``labels_`` [N] int64, ``inertia_``, ``n_iter_``.  Lloyd's algorithm on the mean-centred data; ``tol`` is scaled by the
    mean column variance; it stops on unchanged labels or on a total squared centre shift <= tol, and after the latter
    assigns once more.  ``init``: "k-means++" (random numbers from ``numpy.random.RandomState(random_state)``, drawn as
    sklearn draws them) or a float32 [k, d] tensor used as is."""

    def __init__(self, n_clusters=2, init="k-means++", max_iter=300, tol=1e-4, random_state=None):
        if not 1 <= int(n_clusters) <= ops.KMEANS_MAX_K:
            raise ValueError(f"KMeans: {n_clusters} clusters outside 1..{ops.KMEANS_MAX_K}")
        if not (torch.is_tensor(init) or init == "k-means++"):
            raise ValueError("KMeans: init must be 'k-means++' or a float32 [k, d] tensor")
        if int(max_iter) < 1:
            raise ValueError("KMeans: max_iter must be at least 1")
        self.n_clusters, self.init, self.max_iter = int(n_clusters), init, int(max_iter)
        self.tol, self.random_state = float(tol), random_state

    def fit(self, X):
        k = self.n_clusters
        x, n, d = _points(X, "KMeans", k, ops.KMEANS_MAX_N, ops.KMEANS_MAX_D)     # (sklearn too: n_samples >= n_clusters)
        mean = x.mean(0, keepdim=True)
        xc = (x - mean).contiguous()
        tol = float(xc.double().var(0, unbiased=False).mean()) * self.tol
        if torch.is_tensor(self.init):
            if tuple(self.init.shape) != (k, d):
                raise ValueError(f"KMeans: init {tuple(self.init.shape)} is not [{k}, {d}]")
            centers = (_points(self.init, "KMeans init", k, k, d)[0].to(x.device) - mean).contiguous()
        else:
            centers, _ = kmeans_plusplus(xc, k, self.random_state)
        labels = torch.full((n,), -1, dtype=torch.int64, device=x.device)
        strict, inertia = False, None
        for it in range(self.max_iter):
            _, mind, counts, sums, stats = ops.kmeans_assign(xc, centers, labels)
            ops.kmeans_update(xc, centers, labels, mind, counts, sums, stats)
            inertia, _, shift, changed = (float(v) for v in stats.cpu())    # the iteration's one synchronisation
            if not changed:
                strict = True
                break
            if shift <= tol:
                break
        if not strict:
            _, _, _, _, stats = ops.kmeans_assign(xc, centers, labels, want_sums=False)
            inertia = float(stats[0])
        self._mean, self._centers = mean, centers
        self.cluster_centers_ = (centers + mean).contiguous()
        self.labels_, self.inertia_, self.n_iter_ = labels, inertia, it + 1
        return self

    def predict(self, X):
        if not hasattr(self, "_centers"):
            raise RuntimeError("KMeans.predict before fit")
        x, n, d = _points(X, "KMeans.predict", 1, ops.KMEANS_MAX_N, ops.KMEANS_MAX_D)
        if d != self._centers.shape[1]:
            raise ValueError(f"KMeans.predict: {d} columns, the fit had {self._centers.shape[1]}")
        return ops.kmeans_assign((x - self._mean).contiguous(), self._centers, want_sums=False)[0]

    def fit_predict(self, X):
        return self.fit(X).labels_


def wss_curve(points, kmax=10, random_state=None):
    """The reference's ``calculate_WSS``: the within-cluster sum of squares of ``KMeans(k)`` for k = 1..kmax (its
    hand-rolled sum is the inertia).  Returns a list of floats."""
    return [KMeans(n_clusters=k, random_state=random_state).fit(points).inertia_ for k in range(1, int(kmax) + 1)]


def cluster_labels(features, n_clusters=2, perplexity=40.0, random_state=1000, use_tsne=True, y=None, **tsne_kw):
    """The reference's ``run_cluster_ADNI874``: exact t-SNE of ``features`` [S, D] (float32, device), then
    ``KMeans(n_clusters, init="k-means++", random_state)`` on the embedding.  ``use_tsne=False``: KMeans on the features
    themselves (no embedding).  Returns (clust_y int64 [S], embedding [S, 2] or None, info): ``info`` holds ``kl``,
    ``n_iter``, ``inertia``, ``kmeans_n_iter``, ``sizes`` and, with class labels ``y`` [S], ``class_counts`` [k][classes]
    — the per-cluster class counts the reference prints."""
    info = {}
    emb = None
    if use_tsne:
        tsne = TSNE(perplexity=perplexity, **tsne_kw)
        emb = tsne.fit_transform(features)
        info.update(kl=tsne.kl_divergence_, n_iter=tsne.n_iter_, kl_exploration=tsne.kl_at_exploration_end_)
    km = KMeans(n_clusters=n_clusters, random_state=random_state).fit(emb if use_tsne else features)
    labels = km.labels_
    info.update(inertia=km.inertia_, kmeans_n_iter=km.n_iter_,
                sizes=torch.bincount(labels, minlength=n_clusters).tolist())
    if y is not None:
        yy = torch.as_tensor(y).view(-1).to(labels.device).long()
        classes = int(yy.max()) + 1
        info["class_counts"] = torch.bincount(labels * classes + yy, minlength=n_clusters * classes).view(
            n_clusters, classes).tolist()
    return labels, emb, info


def label_store(store, features=None, similarity="tsne", **kw):
    """Write ``store.cols["clust_y"]`` ([S, 1] int64) and ``store.cols["tsne_fdim"]`` ([S, 1, F] float32) of a
    device-resident ``UniformGraphStore`` in place: the batches it hands out afterwards carry them.  ``features`` [S, D]
    defaults to ``store.cols["x"]`` flattened per subject.  ``similarity="tsne"`` stores the embedding (F = 2);
    ``"features"`` stores the flattened features (the reference's pet_for_similarity / multimodal_for_similarity
    choice) and still clusters on the embedding unless ``use_tsne=False``.  ``kw`` goes to ``cluster_labels``.  Returns
    its ``info``."""
    if store.device.type != "cuda":
        raise ValueError("label_store writes a device-resident store")
    if similarity not in ("tsne", "features"):
        raise ValueError(f"label_store: similarity {similarity!r} is neither 'tsne' nor 'features'")
    if features is None:
        if "x" not in store.cols:
            raise ValueError("label_store: the store has no 'x' column and no features were given")
        features = store.cols["x"].reshape(store.size, -1)
    features = features.to(torch.float32).contiguous()
    if features.dim() != 2 or features.shape[0] != store.size:
        raise ValueError(f"label_store: features {tuple(features.shape)} are not [{store.size}, D]")
    if similarity == "tsne" and kw.get("use_tsne", True) is False:
        raise ValueError("label_store: similarity='tsne' needs the embedding (use_tsne=True)")
    labels, emb, info = cluster_labels(features, **kw)
    fdim = emb if similarity == "tsne" else features.clone()            # (never a view of store.cols["x"])
    store.cols["clust_y"] = labels.view(store.size, 1).contiguous()
    store.cols["tsne_fdim"] = fdim.view(store.size, 1, -1).contiguous()
    store.shapes["clust_y"], store.shapes["tsne_fdim"] = (1,), (1, int(fdim.shape[1]))
    for key in ("clust_y", "tsne_fdim"):
        if key not in store.keys:
            store.keys = list(store.keys) + [key]
    return info
