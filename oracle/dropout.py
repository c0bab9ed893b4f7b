"""oracle/dropout.py — TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

numpy restatement of libigcn's dropout-mask generator (``ig-gcn_amd/csrc/dropout.h``: ``dropout_masks_body``), the
replacement of the reference's ``F.dropout`` / ``nn.Dropout`` / ``nn.Dropout2d`` draws (kernel/go_model.py:124-128,246-251,
270-275; kernel/sgcn_img_snp.py:289-290,300-301).  The reference draws from torch's global generator, so there is nothing
of ITS numbers to pin; what this pins is the generator's contract — a factor is a pure function of (stream counter,
flat element index, the site's p): ``keep(i) = 0 if u(c, i) < p else 1 / (1 - p)`` with

    k0 = H(lo32(c) ^ 0x9E3779B9),  k1 = H(hi32(c) + 0x85EBCA6B + k0)
    h  = H((lo32(i) * 0x9E3779B1) ^ k0) + hi32(i) * 0x85EBCA77
    u  = (H(h ^ k1) >> 8) / 2^24                               H = lowbias32

so that a consumer may compute it instead of loading it and a test can rebuild any step's masks on the
host.  Sites are laid out back to back, each starting on a multiple of four elements.

``MaskFeed`` is the other half: the oracle's ``dropout`` argument may be a feed instead of True / False, and every dropout
site then multiplies by the factors the feed holds under the site's NAME (its module key: ``w_act.0``, ``B.1``, ``lin1`` ...)
instead of drawing its own — which is how a dropout-on HIP run is compared with the oracle: under the run's own masks.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def uniforms(counter, n):
    """u(c, i) for i in [0, n): float32 in [0, 1), exactly the kernel's."""
    c = np.uint64(counter)
    k0 = lowbias32((c & M32) ^ np.uint64(0x9E3779B9))
    k1 = lowbias32(((c >> np.uint64(32)) + np.uint64(0x85EBCA6B) + k0) & M32)
    i = np.arange(n, dtype=np.uint64)
    h = (lowbias32((((i & M32) * np.uint64(0x9E3779B1)) & M32) ^ k0) + (i >> np.uint64(32)) * np.uint64(0x85EBCA77)) & M32
    r = lowbias32(h ^ k1) >> np.uint64(8)
    return r.astype(np.float32) * np.float32(1.0 / 16777216.0)


def masks(sites, counter):
    """``sites``: [(shape, p), ...] -> the factor arrays one launch at stream counter ``counter`` writes (float32)."""
    sizes = [int(np.prod(shape)) for shape, _ in sites]
    starts, total = [], 0
    for n in sizes:
        starts.append(total)
        total += (n + 3) // 4 * 4
    u = uniforms(counter, total)
    out = []
    for (shape, p), s0, n in zip(sites, starts, sizes):
        p32 = np.float32(p)
        scale = np.float32(1.0) / (np.float32(1.0) - p32)
        out.append(np.where(u[s0:s0 + n] < p32, np.float32(0.0), scale).astype(np.float32).reshape(shape))
    return out


class MaskFeed:
    """Dropout factors for an oracle run, keyed by site name.  ``masks``: {name: (float32 array, p)} — node sites [B, N]
    (broadcast over features), element sites the activation's shape.  A site calls ``take(name, shape, p, like)`` and
    gets its factors as a tensor of ``like``'s dtype.  ``rows(lo, hi)`` is a view of rows [lo, hi) of every array that
    shares this feed's book-keeping: the plain pass of a train step reads rows [0, B) of a 2B-row draw and the masked pass
    rows [B, 2B).  Refused with a ``MaskFeedError`` that names the site: an unknown name, a shape or a p other than the
    site's own, factors outside {0, fp32(1 / (1 - p))} (``check_factors=False`` lifts that one — an all-ones feed is the
    identity), rows asked for twice, and — ``close()``, or leaving the ``with`` block without another exception — rows
    nobody consumed."""

    def __init__(self, masks, check_factors=True):
        self._m, self._used, self._lo, self._hi, self._root = {}, {}, 0, None, self
        for name, (arr, p) in masks.items():
            arr = np.asarray(arr)
            if arr.ndim < 1:
                raise MaskFeedError(f"dropout site {name}: factors need a leading row dimension")
            if check_factors:
                p32 = np.float32(p)
                scale = np.float32(1.0) / (np.float32(1.0) - p32)
                bad = (arr != 0) & (arr.astype(np.float32) != scale)
                if arr.dtype != np.float32 or bad.any():
                    raise MaskFeedError(f"dropout site {name}: factors outside {{0, {float(scale)!r}}} (p = {float(p32)!r}; "
                                        f"{int(bad.sum())} entries, dtype {arr.dtype})")
            self._m[name] = (arr, float(np.float32(p)))
            self._used[name] = np.zeros(arr.shape[0], dtype=np.int64)

    def rows(self, lo, hi):
        view = object.__new__(MaskFeed)
        view._root, view._lo, view._hi = self._root, self._lo + int(lo), self._lo + int(hi)
        return view

    def take(self, site, shape, p, like=None):
        import torch
        root = self._root
        if site not in root._m:
            raise MaskFeedError(f"dropout site {site}: the feed holds no factors of that name (has {sorted(root._m)})")
        arr, p_own = root._m[site]
        lo, hi = self._lo, arr.shape[0] if self._hi is None else self._hi
        if float(np.float32(p)) != p_own:
            raise MaskFeedError(f"dropout site {site}: drawn with p = {p_own!r}, the site drops with p = {float(p)!r}")
        shape = tuple(int(d) for d in shape)
        if not (0 <= lo <= hi <= arr.shape[0]) or (hi - lo,) + arr.shape[1:] != shape:
            raise MaskFeedError(f"dropout site {site}: rows [{lo}, {hi}) of factors {arr.shape} do not fit the site's "
                                f"shape {shape}")
        if root._used[site][lo:hi].any():
            raise MaskFeedError(f"dropout site {site}: rows [{lo}, {hi}) asked for twice")
        root._used[site][lo:hi] += 1
        t = torch.from_numpy(np.ascontiguousarray(arr[lo:hi]))
        return t if like is None else t.to(like.dtype)

    def close(self):
        left = {k: int((u == 0).sum()) for k, u in self._root._used.items() if (u == 0).any()}
        if left:
            raise MaskFeedError("dropout factors nobody consumed: " + ", ".join(f"{k} ({n} rows)" for k, n in left.items()))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        return False


class MaskFeedError(ValueError):
    pass


def is_feed(dropout):
    """The oracle's ``dropout`` argument: True / False (draw / do not drop) or a MaskFeed."""
    return isinstance(dropout, MaskFeed)


def go_site_names(n_l=2, extra=()):
    """Oracle site names in the order ``Gene_ontology_network._dropout_masks`` lays its sites out: the encoder LayerNorm
    sites, the decoder LayerNorm sites, ``inp``, ``out_d``, ``h``, then the caller's ``extra`` names."""
    return ([f"w_act.{j}" for j in range(n_l)] + [f"w_act_out.{j}" for j in range(n_l)] + ["B.1", "B_D.1", "latent.2"]
            + list(extra))


HEADS = ("lin1", "lin1_regr")                                   # SGCN_GCN_IMGSNP._head_dropout
CLUSTER_HEADS = ("lin1_classify", "lin1_cluster")               # SGCN_GCN_CLUSTERLABEL._head_dropout
GUIDE_EXTRA = ("encoder_i_N.1", "decoder_i_N.1", "decoder_i_N.5", "lin1", "lin1_regr")     # GUIDE_IMGSNP.forward's extra


def feed_of(sites, arrays, names, check_factors=True):
    """The feed of one launch: ``sites`` [(shape, p), ...] as the model recorded them, ``arrays`` their factors (numpy, or
    anything ``np.asarray`` takes), ``names`` the oracle's site names in the same order (``go_site_names``)."""
    if not (len(sites) == len(arrays) == len(names)) or len(set(names)) != len(names):
        raise MaskFeedError(f"{len(sites)} sites, {len(arrays)} arrays, {len(names)} names ({list(names)})")
    return MaskFeed({n: (np.asarray(a).reshape(tuple(shape)), p) for n, a, (shape, p) in zip(names, arrays, sites)},
                    check_factors)


def stack_rows(parts, names, check_factors=True):
    """One feed of several launches' factors, rows back to back: ``parts`` [(sites, arrays), ...] with the same site list
    up to the row count (two forward() calls of a train step: rows [0, B) drawn at counter c, [B, 2B) at c + 1)."""
    masks = {}
    for k, n in enumerate(names):
        ps = {float(np.float32(sites[k][1])) for sites, _ in parts}
        if len(ps) != 1:
            raise MaskFeedError(f"dropout site {n}: drawn with different p {sorted(ps)}")
        masks[n] = (np.concatenate([np.asarray(arrays[k]).reshape(tuple(sites[k][0])) for sites, arrays in parts], axis=0),
                    ps.pop())
    return MaskFeed(masks, check_factors)
