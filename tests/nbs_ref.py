"""numpy restatement of the network-based statistic (igcn_amd.stats.network_based_statistic, igcn_perm_supra in
csrc/perm_test.hip, igcn_nbs_components in csrc/nbs.hip), for the tests: the suprathreshold bits of an int64 or fp64 G,
the connected components by a union-find of its own, the extents and the p-values.

An entry set is bool [R, R] (source row i, target column j).  Nodes i != j are joined when entry (i, j) or (j, i) is set;
a diagonal entry joins nothing.  The extent of a component is the number of set entries whose source row lies in it.
"""
import numpy as np

TAILS = {"both": 0, "greater": 1, "less": -1}


def threshold_g(t0, n_a, n_b):
    """The threshold on G (fp64) that a primary threshold t0 on the pooled-variance Student t is."""
    s = n_a + n_b
    return np.sqrt(float(n_a * n_b)) * t0 / np.sqrt(s - 2 + t0 * t0)


def threshold_g32(t0, n_a, n_b):
    """``threshold_g`` rounded once to fp32, as a Python float: the number the kernel compares with."""
    return float(np.float32(threshold_g(t0, n_a, n_b)))


def supra(g, thr, tail, tested):
    """bool [P, E]: tested[e] and v >= thr, v = |G| (tail 0), G (+1) or -G (-1).  G int64 or fp64."""
    g = np.asarray(g)
    v = np.abs(g) if tail == 0 else g if tail > 0 else -g
    return (v >= thr) & np.asarray(tested, dtype=bool).reshape(1, -1)


def words_per_row(e):
    """Ep / 32 with Ep = e rounded up to the 64 entries of one tile."""
    return -(-e // 64) * 2


def pack(mask):
    """uint32 [P, Ep / 32] of bool [P, E]: entry e at bit e & 31 of word e >> 5, zeros behind E."""
    mask = np.asarray(mask, dtype=bool)
    p, e = mask.shape
    out = np.zeros((p, words_per_row(e)), dtype=np.uint32)
    for i in range(e):
        out[:, i >> 5] |= mask[:, i].astype(np.uint32) << np.uint32(i & 31)
    return out


def unpack(bits, e):
    """bool [P, e] of uint32 (or int32) words."""
    bits = np.ascontiguousarray(bits).view(np.uint32)
    idx = np.arange(e)
    return ((bits[:, idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool)


def components(entries):
    """(label [R], extent [R], max_extent) of one entry set bool [R, R]: label = the smallest node index of the node's
    component; extent = the extent of the node's component (0 for a node with no set entry in its row and no
    neighbour)."""
    a = np.asarray(entries, dtype=bool)
    r = a.shape[0]
    parent = list(range(r))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, j in zip(*np.nonzero(a)):
        if i != j:
            ri, rj = find(int(i)), find(int(j))
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)              # the smaller index stays the root
    label = np.array([find(i) for i in range(r)], dtype=np.int64)
    per_root = np.zeros(r, dtype=np.int64)
    np.add.at(per_root, label, a.sum(1))
    extent = per_root[label]
    return label, extent, int(extent.max())


def components_many(masks):
    """(label [P, R], extent [P, R], max_extent [P]) of bool [P, R, R]."""
    out = [components(m) for m in masks]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int64))


def p_values(extent, null_max):
    """fp64 [R]: (1 + #{p : null_max[p] >= extent[i]}) / (1 + P), and 1 where the extent is 0."""
    extent, null_max = np.asarray(extent, dtype=np.int64), np.asarray(null_max, dtype=np.int64)
    count = (null_max[:, None] >= extent[None, :]).sum(0)
    return np.where(extent == 0, 1.0, (1 + count) / (1.0 + null_max.size))


def from_bits(bits_obs, bits, r):
    """The statistic given the bits (uint32 words) of the observed labelling [1, W] and of the relabellings [P, W]: a
    dict of supra [R, R], component, extent [R] (component -1 where the extent is 0), null_max [P], p_fwe [R] and
    edge_p_fwe [R, R]."""
    obs = unpack(bits_obs, r * r)[0].reshape(r, r)
    label, extent, _ = components(obs)
    null_max = components_many(unpack(bits, r * r).reshape(-1, r, r))[2]
    p = p_values(extent, null_max)
    return {"supra": obs, "component": np.where(extent == 0, -1, label), "extent": extent, "null_max": null_max,
            "p_fwe": p, "edge_p_fwe": np.where(obs, p[:, None], 1.0)}


def restate(z, member, observed, t0, tail, tested):
    """The whole statistic in fp64: z [S, R R] standardised, member [P, S] 0/1, observed [S] 0/1, tested bool [R, R].
    Returns ``from_bits``'s dict plus G [P, E], g_obs [E] and thr (fp64)."""
    z = np.asarray(z, dtype=np.float64)
    r = int(round(np.sqrt(z.shape[1])))
    o = np.asarray(observed, dtype=np.float64)
    n_a = int(round(o.sum()))
    thr = threshold_g(t0, n_a, o.size - n_a)
    g = np.asarray(member, dtype=np.float64) @ z
    g_obs = o @ z
    flags = np.asarray(tested, dtype=bool).reshape(-1)
    code = TAILS[tail]
    out = from_bits(pack(supra(g_obs[None, :], thr, code, flags)), pack(supra(g, thr, code, flags)), r)
    out.update({"G": g, "g_obs": g_obs, "thr": thr})
    return out


# ---- the data of the tests ---------------------------------------------------------------------------------------------
def random_entries(p, r, degree, seed):
    """bool [p, r, r]: every entry set independently, ``degree`` of them a row on average (directed, diagonal included)."""
    rng = np.random.default_rng(seed)
    return rng.random((p, r, r)) < degree / r


def planted(seed=21, s=64, n_a=29, r=40, nodes=13, shift=1.5, symmetric=False):
    """The GPU test's planted case: (x [s, r, r] fp32, y [s], tree: the 12 (i, j) entries, i < j, of a random tree on 13
    regions).  Unit Gaussian entries; the tree's entries are shifted by ``shift`` sd in group 0.  ``symmetric``: the
    map is symmetrised, so (j, i) carries the shift too."""
    rng = np.random.default_rng(seed)
    y = np.ones(s, dtype=np.int64)
    y[rng.permutation(s)[:n_a]] = 0
    regions = rng.permutation(r)[:nodes]
    tree = []
    for k in range(1, nodes):
        a, b = int(regions[k]), int(regions[rng.integers(0, k)])
        tree.append((min(a, b), max(a, b)))
    x = rng.standard_normal((s, r, r))
    if symmetric:
        x = (x + x.transpose(0, 2, 1)) / np.sqrt(2.0)
    for i, j in tree:
        x[y == 0, i, j] += shift
        if symmetric:
            x[y == 0, j, i] += shift
    return x.astype(np.float32), y, tree
