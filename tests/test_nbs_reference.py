"""CPU checks of the network-based statistic's restatement (tests/nbs_ref.py), which the GPU tests hold the kernels to:
its components are scipy's weakly connected components, a hand-worked 6-node example, the bits layout (also
``ops.nbs_pack`` on the CPU), the t <-> G threshold conversion and the planted sub-network of the GPU test."""
import numpy as np
import pytest
import torch

import nbs_ref as N
import perm_test_ref as R


@pytest.mark.parametrize("r", [2, 9, 33, 90, 128])
def test_components_are_scipys_weakly_connected_components(r):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for k, degree in enumerate((0.5, 1, 2, 8)):
        for a in N.random_entries(3, r, degree, seed=100 * r + k):
            label, extent, max_extent = N.components(a)
            off = a & ~np.eye(r, dtype=bool)
            n, lab = connected_components(sparse.csr_matrix(off), directed=True, connection="weak")
            first = np.full(n, r)
            np.minimum.at(first, lab, np.arange(r))                     # scipy's label -> the smallest node index
            assert np.array_equal(label, first[lab])
            want = np.zeros(r, dtype=np.int64)
            np.add.at(want, label, a.sum(1))
            assert np.array_equal(extent, want[label]) and max_extent == want.max()
            assert extent.sum() >= a.sum() and want.sum() == a.sum()    # every set entry counts once


def test_hand_worked_six_node_example():
    """0 <-> 1 -> 2 is one component of 3 entries (node 2 has an empty row and a neighbour), 3 -> 4 with 4's diagonal
    entry one of 2, node 5 has nothing."""
    a = np.zeros((6, 6), dtype=bool)
    for i, j in ((0, 1), (1, 0), (1, 2), (3, 4), (4, 4)):
        a[i, j] = True
    label, extent, max_extent = N.components(a)
    assert label.tolist() == [0, 0, 0, 3, 3, 5]
    assert extent.tolist() == [3, 3, 3, 2, 2, 0] and max_extent == 3
    p = N.p_values(extent, [0, 1, 2, 3, 3, 5, 2])
    assert p.tolist() == [4 / 8, 4 / 8, 4 / 8, 6 / 8, 6 / 8, 1.0]
    out = N.from_bits(N.pack(a.reshape(1, -1)), N.pack(np.stack([a, a.T, np.eye(6, dtype=bool)]).reshape(3, -1)), 6)
    assert out["component"].tolist() == [0, 0, 0, 3, 3, -1]
    assert out["null_max"].tolist() == [3, 3, 1]                       # the transpose: the same graph, rows 0 1 2: 1 1 1
    assert out["p_fwe"].tolist() == [3 / 4, 3 / 4, 3 / 4, 3 / 4, 3 / 4, 1.0]
    assert np.array_equal(out["edge_p_fwe"], np.where(a, 0.75, 1.0))
    # a diagonal entry joins nothing and counts once; one direction is enough to join
    d = np.eye(6, dtype=bool)
    assert N.components(d)[0].tolist() == list(range(6)) and N.components(d)[1].tolist() == [1] * 6
    one = np.zeros((6, 6), dtype=bool)
    one[5, 0] = True
    assert N.components(one)[0].tolist() == [0, 1, 2, 3, 4, 0] and N.components(one)[1].tolist() == [1, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("r", [2, 8, 9, 33, 128])
def test_bits_layout_and_nbs_pack(r):
    from igcn_amd import ops
    e = r * r
    mask = N.random_entries(5, r, 3, seed=r)
    mask[0], mask[1] = False, True
    words = N.pack(mask.reshape(5, e))
    assert words.shape == (5, -(-e // 64) * 2) and words.dtype == np.uint32
    for p, i, j in ((2, 0, 0), (3, r - 1, r - 1), (4, r // 2, 1)):
        k = i * r + j
        assert bool((words[p, k >> 5] >> np.uint32(k & 31)) & 1) == bool(mask[p, i, j])
    assert np.array_equal(N.unpack(words, e), mask.reshape(5, e))
    full = N.unpack(words, words.shape[1] * 32)
    assert not full[:, e:].any() and not words[0].any()                # zeros behind E
    got = ops.nbs_pack(torch.from_numpy(mask))
    assert got.dtype == torch.int32 and np.array_equal(got.numpy().view(np.uint32), words)
    with pytest.raises(ValueError):
        ops.nbs_pack(torch.zeros(2, 3, 4, dtype=torch.bool))


@pytest.mark.parametrize("n", [(29, 35), (2, 2), (437, 437), (11, 22)])
def test_threshold_on_g_is_the_threshold_on_t(n):
    n_a, n_b = n
    for t0 in (0.5, 2.0, 3.1, 10.0):
        thr = N.threshold_g(t0, n_a, n_b)
        assert abs(R.student_t(thr, n_a, n_b) - t0) <= 1e-12 * t0
        assert 0 < thr < np.sqrt(n_a * n_b)
        t32 = R.student_t(N.threshold_g32(t0, n_a, n_b), n_a, n_b)     # one fp32 rounding of thr: a relative 2^-24 of G
        assert abs(t32 - t0) <= 1e-6 * t0 * (1 + t0 * t0 / (n_a + n_b - 2))
    g = np.array([[-3.0, 0.5, 2.0, 2.5]])
    tested = np.array([True, True, True, False])
    assert N.supra(g, 2.0, 0, tested).tolist() == [[True, False, True, False]]          # >=: a tie is in
    assert N.supra(g, 2.0, 1, tested).tolist() == [[False, False, True, False]]
    assert N.supra(g, 2.0, -1, tested).tolist() == [[True, False, False, False]]


def test_planted_tree_is_recovered_by_the_restatement():
    """The condition of the GPU test, on the restatement alone: the planted component is recovered, it has the largest
    observed extent and its p is 1 / (1 + P)."""
    x, y, tree = N.planted()
    s, r, p = 64, 40, 512
    z, _, _, _ = R.standardize(x.reshape(s, -1))
    member = R.draw(p, s, 29, seed=5)
    tested = ~np.eye(r, dtype=bool)
    ref = N.restate(z, member, y == 0, 3.1, "both", tested)
    nodes = sorted({v for edge in tree for v in edge})
    root = nodes[0]
    assert all(ref["supra"][i, j] for i, j in tree)
    assert all(ref["component"][v] == root for v in nodes)
    assert ref["extent"][root] == ref["extent"].max() >= 12
    assert ref["p_fwe"][root] == 1.0 / (1 + p) and ref["null_max"].max() < ref["extent"][root]
    assert len(set(ref["null_max"].tolist())) > 1
