"""Two-sample permutation test of a group difference over the entries of a per-subject map table, with the max-statistic
(Westfall-Young "max-T") family-wise correction — the map-level counterpart of the reference's model-level
``--isPermutTest`` (sgcn_data.py:205-208, which shuffles the regression targets and retrains).

For S subjects of two groups (n_a + n_b = S) and E map entries the statistic of entry e under a relabelling with group A
``member`` is the pooled-variance Student t.  With z the column standardised over the S subjects (mean 0, population sd
1) and G = sum_{s in A} z[s], the point-biserial correlation of the labelling with the column is
``r = G / sqrt(n_a n_b)`` and ``t = r sqrt((S - 2) / (1 - r^2))``: |t| is ONE increasing function of |G| for every column
and every relabelling, so comparing |G| is comparing |t| and the kernel (csrc/perm_test.hip, igcn_perm_maxsum) never
forms t.  Two-sided only.
"""
import math

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
    x2 = x.reshape(x.shape[0], -1).contiguous()
    dev = x2.device
    y = torch.as_tensor(y).view(-1).to(device=dev, dtype=torch.int64)
    if y.numel() != x2.shape[0]:
        raise ValueError(f"permutation_test: {y.numel()} labels for {x2.shape[0]} subjects")
    ga, gb = int(groups[0]), int(groups[1])
    if ga == gb:
        raise ValueError("permutation_test: the two groups are the same label")
    rows = torch.nonzero((y == ga) | (y == gb)).view(-1)
    in_a = (y[rows] == ga)
    s = int(rows.numel())
    n_a = int(in_a.sum())
    n_b = s - n_a
    if n_a < 2 or n_b < 2:
        raise ValueError(f"permutation_test: groups {ga} / {gb} have {n_a} / {n_b} subjects (at least 2 each)")
    if not ops.PERM_MIN_S <= s <= ops.PERM_MAX_S:
        raise ValueError(f"permutation_test: S={s} subjects outside [{ops.PERM_MIN_S}, {ops.PERM_MAX_S}]")
    e = int(x2.shape[1])
    if members is None:
        members = draw_members(s, n_a, permutations, seed, dev)
    else:
        if (not torch.is_tensor(members) or members.dim() != 2 or members.shape[1] != s or members.shape[0] < 1
                or members.dtype != torch.uint8):
            raise ValueError(f"permutation_test: members must be uint8 [P, {s}]")
        members = members.to(dev)
        if bool((members > 1).any()) or bool((members.sum(1, dtype=torch.int64) != n_a).any()):
            raise ValueError(f"permutation_test: every row of members must hold {n_a} ones and {n_b} zeros")
        if members.stride(1) != 1 or members.stride(0) % 16 or members.data_ptr() % 16:
            padded = _padded_rows(members.shape[0], s, dev)
            padded.copy_(members)
            members = padded
    p_total = int(members.shape[0])
    chunk = DEFAULT_CHUNK if chunk is None else int(chunk)
    if not 1 <= chunk <= ops.PERM_MAX_P:
        raise ValueError(f"permutation_test: chunk={chunk} outside [1, {ops.PERM_MAX_P}]")

    mean, sd, constant, planes = ops.perm_prepare(x2, rows, standardize=True)
    if not (bool(torch.isfinite(mean).all()) and bool(torch.isfinite(sd).all())):
        raise ValueError("permutation_test: x holds non-finite values in the rows under test")
    observed = _padded_rows(1, s, dev)
    observed.copy_(in_a.view(1, s))
    _, g = ops.perm_maxsum(observed, planes, e)
    g_obs = g.view(-1).contiguous()
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
    gd = g_obs.double()
    diff = (sd * gd * (s / (n_a * n_b))).masked_fill(const, 0.0)
    r = (gd / math.sqrt(n_a * n_b)).clamp(-1.0, 1.0)
    t = (r * torch.sqrt((s - 2) / (1 - r * r))).masked_fill(const, 0.0)
    return {"diff": diff.view(shape), "t": t.view(shape), "p_unc": p_unc.view(shape), "p_fwe": p_fwe.view(shape),
            "constant": const.view(shape), "null_max": null_max, "n": (n_a, n_b), "permutations": p_total}
