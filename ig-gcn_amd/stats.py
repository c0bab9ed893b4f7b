"""Two-sample permutation test of a group difference over the entries of a per-subject map table, with the max-statistic
(Westfall-Young "max-T") family-wise correction — the map-level counterpart of the reference's model-level
``--isPermutTest`` (sgcn_data.py:205-208, which shuffles the regression targets and retrains).

For S subjects of two groups (n_a + n_b = S) and E map entries the statistic of entry e under a relabelling with group A
``member`` is the pooled-variance Student t.  With z the column standardised over the S subjects (mean 0, population sd
1) and G = sum_{s in A} z[s], the point-biserial correlation of the labelling with the column is
``r = G / sqrt(n_a n_b)`` and ``t = r sqrt((S - 2) / (1 - r^2))``: |t| is ONE increasing function of |G| for every column
and every relabelling, so comparing |G| is comparing |t| and the kernel (csrc/perm_test.hip, igcn_perm_maxsum) never
forms t.  Two-sided only.

``permutation_anova`` below is the counterpart for three to five groups: the one-way ANOVA F with the same max-statistic
correction (igcn_perm_maxf).  ``network_based_statistic`` at the end is the cluster-level test for the ROI x ROI
connectivity maps: connected components of the suprathreshold graph, corrected by the largest component's extent
(igcn_perm_supra, igcn_nbs_components).
"""
import math
from types import SimpleNamespace

import torch

from . import ops

DEFAULT_CHUNK = 4096


def _padded_rows(p, n, device):
    """uint8 zeros [p, n] whose rows start 16-byte aligned (a view of [p, n rounded up to 16]): the staging of
    igcn_perm_maxsum then reads member 16 bytes at a time."""
    return ops._buffer((p, -(-n // 16) * 16), torch.uint8, device).zero_()[:, :n]


def draw_members(n, n_a, permutations, seed=0, device="cuda"):
    """uint8 [permutations, n]: row p marks the ``n_a`` smallest of n uniform draws of a ``torch.Generator`` on
    ``device`` seeded with ``seed`` — a uniformly drawn group A of every relabelling.  All rows come from one draw, so
    the rows do not depend on how a caller chunks them."""
    n, n_a, p = int(n), int(n_a), int(permutations)
    if not 0 < n_a < n or p < 1:
        raise ValueError(f"draw_members: n_a={n_a} of n={n}, {p} relabellings")
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    u = torch.rand(p, n, generator=gen, device=device)
    idx = torch.topk(u, n_a, dim=1, largest=False).indices
    members = _padded_rows(p, n, u.device)
    members.scatter_(1, idx, 1)
    return members


def _two_groups(who, x, y, groups, permutations, seed, members, chunk):
    """What the two-group tests share up to the observed labelling: the kept rows, the checked (or drawn) and aligned
    ``members``, the chunk, the statistics and planes of ``ops.perm_prepare`` and ``g_obs`` [E] (``ops.perm_maxsum`` on the
    observed labelling).  ``who`` names the caller in the messages."""
    x2 = x.reshape(x.shape[0], -1).contiguous()
    dev = x2.device
    y = torch.as_tensor(y).view(-1).to(device=dev, dtype=torch.int64)
    if y.numel() != x2.shape[0]:
        raise ValueError(f"{who}: {y.numel()} labels for {x2.shape[0]} subjects")
    ga, gb = int(groups[0]), int(groups[1])
    if ga == gb:
        raise ValueError(f"{who}: the two groups are the same label")
    rows = torch.nonzero((y == ga) | (y == gb)).view(-1)
    in_a = (y[rows] == ga)
    s = int(rows.numel())
    n_a = int(in_a.sum())
    n_b = s - n_a
    if n_a < 2 or n_b < 2:
        raise ValueError(f"{who}: groups {ga} / {gb} have {n_a} / {n_b} subjects (at least 2 each)")
    if not ops.PERM_MIN_S <= s <= ops.PERM_MAX_S:
        raise ValueError(f"{who}: S={s} subjects outside [{ops.PERM_MIN_S}, {ops.PERM_MAX_S}]")
    e = int(x2.shape[1])
    if members is None:
        members = draw_members(s, n_a, permutations, seed, dev)
    else:
        if (not torch.is_tensor(members) or members.dim() != 2 or members.shape[1] != s or members.shape[0] < 1
                or members.dtype != torch.uint8):
            raise ValueError(f"{who}: members must be uint8 [P, {s}]")
        members = members.to(dev)
        if bool((members > 1).any()) or bool((members.sum(1, dtype=torch.int64) != n_a).any()):
            raise ValueError(f"{who}: every row of members must hold {n_a} ones and {n_b} zeros")
        if members.stride(1) != 1 or members.stride(0) % 16 or members.data_ptr() % 16:
            padded = _padded_rows(members.shape[0], s, dev)
            padded.copy_(members)
            members = padded
    p_total = int(members.shape[0])
    chunk = DEFAULT_CHUNK if chunk is None else int(chunk)
    if not 1 <= chunk <= ops.PERM_MAX_P:
        raise ValueError(f"{who}: chunk={chunk} outside [1, {ops.PERM_MAX_P}]")

    mean, sd, constant, planes = ops.perm_prepare(x2, rows, standardize=True)
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(sd).all())):
        raise ValueError(f"{who}: x holds non-finite values in the rows under test")
    observed = _padded_rows(1, s, dev)
    observed.copy_(in_a.view(1, s))
    _, g = ops.perm_maxsum(observed, planes, e)
    return SimpleNamespace(dev=dev, s=s, n_a=n_a, n_b=n_b, e=e, members=members, p_total=p_total, chunk=chunk, sd=sd,
                           constant=constant, planes=planes, observed=observed, g_obs=g.view(-1).contiguous())


def _t_and_diff(c):
    """(t, diff) [E] fp64 of the observed labelling of ``_two_groups``: the pooled-variance Student t and the group-A
    mean minus the group-B mean in original units; 0 for a constant entry."""
    const = c.constant.bool()
    gd = c.g_obs.double()
    diff = (c.sd * gd * (c.s / (c.n_a * c.n_b))).masked_fill(const, 0.0)
    r = (gd / math.sqrt(c.n_a * c.n_b)).clamp(-1.0, 1.0)
    t = (r * torch.sqrt((c.s - 2) / (1 - r * r))).masked_fill(const, 0.0)
    return t, diff


def permutation_test(x, y, groups=(0, 1), permutations=10000, seed=0, members=None, chunk=None):
    """Max-T permutation test of ``groups[0]`` against ``groups[1]`` for every entry of the per-subject maps
    ``x`` [S_all, ...] (fp32, on the device) with labels ``y`` [S_all].  The rows with another label are left out.
    ``members`` (uint8 [P, S], S = n_a + n_b, every row with n_a ones, in the order of the kept rows) replaces the
    ``permutations`` relabellings drawn by ``draw_members(S, n_a, permutations, seed)``.  The relabellings run in chunks
    of ``chunk`` rows (4096); the result has the same bits for any chunking.

    Returns a dict, the per-entry tensors in the shape of one map: ``diff`` (group-A mean minus group-B mean, original
    units), ``t`` (pooled-variance Student t of the observed labelling), ``p_unc`` = (1 + #{p : |t_p[e]| >= |t_obs[e]|})
    / (1 + P), ``p_fwe`` = (1 + #{p : max_e' |t_p[e']| >= |t_obs[e]|}) / (1 + P) (all fp64), ``constant`` (bool: the
    entry has one value over the kept rows; p-values 1 and t 0 there); ``null_max`` [P] (fp32: max_e |G_p[e]|, the null
    distribution of the maximum in the units of G), ``n`` = (n_a, n_b) and ``permutations`` = P."""
    if not torch.is_tensor(x) or x.dim() < 2 or x.dtype != torch.float32:
        raise TypeError("permutation_test: x must be a float32 tensor [S_all, ...]")
    shape = tuple(x.shape[1:])
    c = _two_groups("permutation_test", x, y, groups, permutations, seed, members, chunk)
    dev, n_a, n_b, e, members, p_total, chunk = c.dev, c.n_a, c.n_b, c.e, c.members, c.p_total, c.chunk
    constant, planes, g_obs = c.constant, c.planes, c.g_obs
    null_max = ops._buffer((p_total,), torch.float32, dev)
    exceed = ops._buffer((e,), torch.int64, dev).zero_()
    for p0 in range(0, p_total, chunk):
        mx, ex = ops.perm_maxsum(members[p0:p0 + chunk], planes, e, g_obs)
        null_max[p0:p0 + mx.numel()] = mx
        exceed += ex
    const = constant.bool()
    thr = g_obs.abs()
    srt = torch.sort(null_max).values
    fwe = p_total - torch.searchsorted(srt, thr.contiguous(), right=False)        # #{p : null_max[p] >= |g_obs[e]|}
    den = torch.tensor(float(1 + p_total), dtype=torch.float64, device=dev)      # (a tensor divisor: a true division)
    p_unc = ((1 + exceed).double() / den).masked_fill(const, 1.0)
    p_fwe = ((1 + fwe).double() / den).masked_fill(const, 1.0)
    t, diff = _t_and_diff(c)
    return {"diff": diff.view(shape), "t": t.view(shape), "p_unc": p_unc.view(shape), "p_fwe": p_fwe.view(shape),
            "constant": const.view(shape), "null_max": null_max, "n": (n_a, n_b), "permutations": p_total}


# ---- more than two groups: the max-F test --------------------------------------------------------------------------------
# One-way ANOVA over K groups of sizes n_g on the same standardised column (sum z = 0, sum z^2 = S): the between-groups
# sum of squares is B = sum_g G_g^2 / n_g with G_g the group sums, the total is S, and
#   F = (B / (K - 1)) / ((S - B) / (S - K))
# is ONE increasing function of B for every column and every relabelling, so the kernel (igcn_perm_maxf) compares B and
# never forms F.  The LAST group's sum is DEFINED as minus the sum of the others: the column sum of the fp32 z is zero
# only to rounding, and the definition is the same in the kernel, here and in the tests' restatement.
def draw_labels(observed, permutations, seed=0, device="cuda"):
    """uint8 [permutations, S]: every row a uniformly drawn permutation of the group codes ``observed`` [S] (0..K-1), by
    the argsort of one ``torch.rand(permutations, S)`` of a ``torch.Generator`` on ``device`` seeded with ``seed`` — one
    draw for all rows, so the rows do not depend on how a caller chunks them.  Rows start 16-byte aligned."""
    observed = torch.as_tensor(observed).view(-1)
    n, p = int(observed.numel()), int(permutations)
    if n < 2 or p < 1:
        raise ValueError(f"draw_labels: {n} subjects, {p} relabellings")
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    u = torch.rand(p, n, generator=gen, device=device)
    codes = observed.to(device=u.device, dtype=torch.uint8)
    labels = _padded_rows(p, n, u.device)
    labels.copy_(codes[torch.argsort(u, dim=1)])
    return labels


def permutation_anova(x, y, groups=(0, 1, 2), permutations=10000, seed=0, labels=None, chunk=None):
    """Max-F permutation test of a difference between the K = 2..5 diagnosis groups ``groups`` for every entry of the
    per-subject maps ``x`` [S_all, ...] (fp32, on the device) with labels ``y`` [S_all].  The rows with another label are
    left out; a kept row's code is the position of its label in ``groups``.  ``labels`` (uint8 [P, S], every row a
    rearrangement of the kept rows' codes, in the order of the kept rows) replaces the ``permutations`` relabellings
    drawn by ``draw_labels(codes, permutations, seed)``.  The relabellings run in chunks of ``chunk`` rows (4096); the
    result has the same bits for any chunking.

    Returns a dict, the per-entry tensors in the shape of one map and fp64 unless noted: ``f`` (the one-way ANOVA F of
    the observed labelling), ``eta2`` = B / S (the share of the variance between the groups), ``means`` [K, ...] (the
    group means in original units, mean + sd G_g / n_g; the last group's G is minus the sum of the others),
    ``p_unc`` = (1 + #{p : F_p[e] >= F_obs[e]}) / (1 + P), ``p_fwe`` = (1 + #{p : max_e' F_p[e'] >= F_obs[e]}) / (1 + P),
    ``constant`` (bool: the entry has one value over the kept rows; f 0 and p-values 1 there); ``null_max`` [P] (fp32:
    max_e B_p[e], the null distribution of the maximum in the units of B), ``n`` (the K group sizes),
    ``df`` = (K - 1, S - K) and ``permutations`` = P."""
    if not torch.is_tensor(x) or x.dim() < 2 or x.dtype != torch.float32:
        raise TypeError("permutation_anova: x must be a float32 tensor [S_all, ...]")
    shape = tuple(x.shape[1:])
    x2 = x.reshape(x.shape[0], -1).contiguous()
    dev = x2.device
    y = torch.as_tensor(y).view(-1).to(device=dev, dtype=torch.int64)
    if y.numel() != x2.shape[0]:
        raise ValueError(f"permutation_anova: {y.numel()} labels for {x2.shape[0]} subjects")
    groups = tuple(int(v) for v in groups)
    k = len(groups)
    if not 2 <= k <= ops.PERM_MAX_GROUPS:
        raise ValueError(f"permutation_anova: {k} groups (2 to {ops.PERM_MAX_GROUPS})")
    if len(set(groups)) != k:
        raise ValueError(f"permutation_anova: a label is repeated in groups={groups}")
    code = torch.full_like(y, k)
    for c, label in enumerate(groups):
        code[y == label] = c
    rows = torch.nonzero(code < k).view(-1)
    codes = code[rows].to(torch.uint8)
    s = int(rows.numel())
    n = tuple(int(v) for v in torch.bincount(codes.long(), minlength=k).tolist())
    if min(n) < 2:
        raise ValueError(f"permutation_anova: groups {groups} have {n} subjects (at least 2 each)")
    if not ops.PERM_MIN_S <= s <= ops.PERM_MAX_S:
        raise ValueError(f"permutation_anova: S={s} subjects outside [{ops.PERM_MIN_S}, {ops.PERM_MAX_S}]")
    e = int(x2.shape[1])
    if labels is None:
        labels = draw_labels(codes, permutations, seed, dev)
    else:
        if (not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[1] != s or labels.shape[0] < 1
                or labels.dtype != torch.uint8):
            raise ValueError(f"permutation_anova: labels must be uint8 [P, {s}]")
        labels = labels.to(dev)
        if any(bool(((labels == c).sum(1, dtype=torch.int64) != n[c]).any()) for c in range(k)):
            raise ValueError(f"permutation_anova: every row of labels must hold the codes 0..{k - 1} {n} times")
        if labels.stride(1) != 1 or labels.stride(0) % 16 or labels.data_ptr() % 16:
            padded = _padded_rows(labels.shape[0], s, dev)
            padded.copy_(labels)
            labels = padded
    p_total = int(labels.shape[0])
    chunk = DEFAULT_CHUNK if chunk is None else int(chunk)
    if not 1 <= chunk <= ops.PERM_MAX_P:
        raise ValueError(f"permutation_anova: chunk={chunk} outside [1, {ops.PERM_MAX_P}]")

    mean, sd, constant, planes = ops.perm_prepare(x2, rows, standardize=True)
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(sd).all())):
        raise ValueError("permutation_anova: x holds non-finite values in the rows under test")
    weights = [1.0 / v for v in n]
    observed = _padded_rows(1, s, dev)
    observed.copy_(codes.view(1, s))
    _, b, g = ops.perm_maxf(observed, planes, e, weights, want_g=True)
    b_obs = b.view(-1).contiguous()
    null_max = ops._buffer((p_total,), torch.float32, dev)
    exceed = ops._buffer((e,), torch.int64, dev).zero_()
    for p0 in range(0, p_total, chunk):
        mx, ex = ops.perm_maxf(labels[p0:p0 + chunk], planes, e, weights, b_obs)
        null_max[p0:p0 + mx.numel()] = mx
        exceed += ex
    const = constant.bool()
    srt = torch.sort(null_max).values
    fwe = p_total - torch.searchsorted(srt, b_obs, right=False)                   # #{p : null_max[p] >= b_obs[e]}
    den = torch.tensor(float(1 + p_total), dtype=torch.float64, device=dev)      # (a tensor divisor: a true division)
    p_unc = ((1 + exceed).double() / den).masked_fill(const, 1.0)
    p_fwe = ((1 + fwe).double() / den).masked_fill(const, 1.0)
    eta2 = (b_obs.double() / s).clamp(0.0, 1.0).masked_fill(const, 0.0)
    f = ((eta2 / (k - 1)) / ((1 - eta2) / (s - k))).masked_fill(const, 0.0)
    gd = g.view(k - 1, e).double()
    gd = torch.cat([gd, -gd.sum(0, keepdim=True)])                                # the last group: minus the others
    means = mean + sd * gd / torch.tensor(n, dtype=torch.float64, device=dev).view(k, 1)
    return {"f": f.view(shape), "eta2": eta2.view(shape), "means": means.view(k, *shape), "p_unc": p_unc.view(shape),
            "p_fwe": p_fwe.view(shape), "constant": const.view(shape), "null_max": null_max, "n": n,
            "df": (k - 1, s - k), "permutations": p_total}


# ---- cluster level, on the one map that is a graph: the network-based statistic ---------------------------------------------
# Zalesky, Fornito & Bullmore 2010: threshold the edge-wise t map of the ROI x ROI connectivity maps at a primary
# threshold t0, take the connected components of the suprathreshold graph, measure each by its extent (its number of
# suprathreshold entries) and correct with the permutation distribution of the LARGEST extent.  |t| is one increasing
# function of |G|, so t0 is the one threshold  thr = sqrt(n_a n_b) t0 / sqrt(S - 2 + t0^2)  on G for every entry and
# every relabelling: igcn_perm_supra keeps one bit per (relabelling, entry) of the product igcn_perm_maxsum forms, and
# igcn_nbs_components labels the P graphs, one wave each.
TAILS = {"both": 0, "greater": 1, "less": -1}


def _unpack_bits(bits, e):
    """bool [P, e] from the int32 words of ``ops.perm_supra``."""
    shifts = torch.arange(32, dtype=torch.int32, device=bits.device)
    return ((bits.unsqueeze(-1) >> shifts) & 1).bool().view(bits.shape[0], -1)[:, :e]


def network_based_statistic(x, y, groups=(0, 1), threshold=3.1, tail="both", permutations=5000, seed=0, members=None,
                            chunk=None, tested=None, symmetric=False):
    """Network-based statistic of ``groups[0]`` against ``groups[1]`` on the per-subject ROI x ROI maps ``x``
    [S_all, R, R] (fp32, on the device; entry (i, j): source row i, target column j, like ``data.A``) with labels ``y``.
    Rows, ``members``, ``permutations`` / ``seed`` and ``chunk`` are those of ``permutation_test``.  ``threshold`` is the
    primary threshold t0 on the pooled-variance Student t; ``tail`` "both" (|t| >= t0), "greater" (t >= t0: group A above
    group B) or "less".  Tested are the entries of ``tested`` (bool [R, R], default all) off the diagonal that are not
    constant over the kept rows; ``symmetric=True`` also drops the entries with i >= j, so that a symmetric map counts
    every undirected edge once.  Regions i != j are joined when entry (i, j) or (j, i) is suprathreshold; a component's
    extent is the number of suprathreshold entries whose source row lies in it.  R <= 128 (``ops.NBS_MAX_ROIS``).

    Returns a dict: ``t``, ``diff`` [R, R] (fp64, as ``permutation_test`` forms them), ``supra`` (bool [R, R]: the
    suprathreshold entries of the observed labelling), ``component`` (int64 [R]: the smallest region index of the
    region's component, -1 where its extent is 0), ``extent`` (int64 [R]: of the region's component), ``p_fwe`` (fp64 [R]:
    (1 + #{p : null_max[p] >= extent}) / (1 + P), 1 where the extent is 0), ``edge_p_fwe`` (fp64 [R, R]: the component's
    p on the ``supra`` entries, 1 elsewhere), ``null_max`` (int32 [P]: the largest extent of every relabelling),
    ``tested`` (bool [R, R]), ``threshold`` = (t0, the fp32 threshold on G), ``n`` = (n_a, n_b), ``permutations`` = P.
    The result has the same bits for any chunking."""
    who = "network_based_statistic"
    if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != x.shape[2] or x.dtype != torch.float32:
        raise ValueError(f"{who}: x must be a float32 tensor [S_all, R, R]")
    r = int(x.shape[1])
    if not 2 <= r <= ops.NBS_MAX_ROIS:
        raise ValueError(f"{who}: R={r} regions outside [2, {ops.NBS_MAX_ROIS}]")
    t0 = float(threshold)
    if not 0 < t0 < float("inf"):
        raise ValueError(f"{who}: threshold={threshold} (finite and > 0)")
    if tail not in TAILS:
        raise ValueError(f"{who}: tail={tail!r} (one of {tuple(TAILS)})")
    if tested is not None and (not torch.is_tensor(tested) or tested.dtype != torch.bool or tuple(tested.shape) != (r, r)):
        raise ValueError(f"{who}: tested must be bool [{r}, {r}]")
    c = _two_groups(who, x, y, groups, permutations, seed, members, chunk)
    dev, e, p_total = c.dev, c.e, c.p_total
    # the threshold on G: fp64 on the host, rounded once to fp32
    thr = float(torch.tensor(math.sqrt(c.n_a * c.n_b) * t0 / math.sqrt(c.s - 2 + t0 * t0), dtype=torch.float64).float())
    if not 0 < thr < float("inf"):
        raise ValueError(f"{who}: threshold={threshold} gives the threshold {thr} on G")
    keep = torch.ones(r, r, dtype=torch.bool, device=dev) if tested is None else tested.to(dev).clone()
    keep &= ~torch.eye(r, dtype=torch.bool, device=dev)
    if symmetric:
        keep &= torch.ones(r, r, dtype=torch.bool, device=dev).triu(1)
    keep &= ~c.constant.bool().view(r, r)
    flags = keep.view(-1).to(torch.uint8)

    bits_obs = ops.perm_supra(c.observed, c.planes, e, thr, TAILS[tail], flags)
    _, label, extent = ops.nbs_components(bits_obs, r, want_labels=True)
    null_max = ops._buffer((p_total,), torch.int32, dev)
    for p0 in range(0, p_total, c.chunk):
        bits = ops.perm_supra(c.members[p0:p0 + c.chunk], c.planes, e, thr, TAILS[tail], flags)
        mx = ops.nbs_components(bits, r)
        null_max[p0:p0 + mx.numel()] = mx
    extent = extent.view(r).long()
    empty = extent == 0
    srt = torch.sort(null_max).values.long()
    fwe = p_total - torch.searchsorted(srt, extent.contiguous(), right=False)     # #{p : null_max[p] >= extent[i]}
    den = torch.tensor(float(1 + p_total), dtype=torch.float64, device=dev)      # (a tensor divisor: a true division)
    p_fwe = ((1 + fwe).double() / den).masked_fill(empty, 1.0)
    supra = _unpack_bits(bits_obs, e).view(r, r)
    edge_p = torch.where(supra, p_fwe.view(r, 1).expand(r, r), torch.ones((), dtype=torch.float64, device=dev))
    t, diff = _t_and_diff(c)
    return {"t": t.view(r, r), "diff": diff.view(r, r), "supra": supra,
            "component": label.view(r).long().masked_fill(empty, -1), "extent": extent, "p_fwe": p_fwe,
            "edge_p_fwe": edge_p, "null_max": null_max, "tested": keep, "threshold": (t0, thr), "n": (c.n_a, c.n_b),
            "permutations": p_total}
