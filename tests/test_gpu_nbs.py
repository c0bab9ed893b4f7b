"""GPU tests of the network-based statistic: igcn_perm_supra (csrc/perm_test.hip) against an int64 oracle where the
arithmetic is exact, against the g of igcn_perm_maxsum bit for bit and against the fp64 restatement inside the any-order
summation bound elsewhere; igcn_nbs_components (csrc/nbs.hip) against the union-find of tests/nbs_ref.py;
``stats.network_based_statistic`` and ``maps.network_difference`` on top of them.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nbs_ref as N
import perm_test_ref as R
from test_gpu_perm_test import _cohort, _imgsnp, _integer_case, _same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _words(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- (1) kernel 1, exact integers --------------------------------------------------------------------------------------
INT_SHAPES = [(5, 2, 1, 2), (33, 3, 63, 11), (64, 8, 64, 29), (64, 9, 129, 29), (127, 23, 130, 40), (257, 33, 65, 40),
              (64, 90, 130, 29), (64, 128, 129, 29)]                          # (S, R, P, n_a)


def _run_integer_supra(s, r, p, n_a, bits):
    """[(got, want)] for the three tails: the device's words and the oracle's, for a threshold that occurs in |G|."""
    from igcn_amd import ops
    e = r * r
    z, rows, member, _ = _integer_case(s, e, p, n_a, bits)
    rng = np.random.default_rng(s + r)
    tested = rng.random((r, r)) < 0.7
    tested[rng.permutation(r)[:max(1, r // 4)]] = False                   # whole rows cleared
    big = member.astype(np.int64) @ z[rows]
    assert np.abs(big).max() < 2 ** 24
    cand = np.abs(big)[:, tested.reshape(-1)]                               # a value of |G| at a tested entry: >= meets a tie
    cand = np.sort((cand if cand.size else np.abs(big)).ravel())
    thr = int(cand[int(0.6 * cand.size)])
    x = torch.from_numpy(z.astype(np.float32)).cuda()
    _, _, _, planes = ops.perm_prepare(x, torch.from_numpy(rows).cuda(), standardize=False)
    m, flags = torch.from_numpy(member).cuda(), torch.from_numpy(tested.reshape(-1)).cuda()
    out = []
    for tail in (0, 1, -1):
        got = ops.perm_supra(m, planes, e, float(thr), tail, flags)
        want = N.pack(N.supra(big, thr, tail, tested))
        assert (np.abs(big) == thr).any() and (tail != 0 or want.any() == tested.any())
        out.append((got, want))
    return out


@pytest.mark.parametrize("bits", [17, 18])
@pytest.mark.parametrize("shape", INT_SHAPES)
def test_integer_bits_equal_the_int64_oracle(shape, bits):
    s, r, p, n_a = shape
    for got, want in _run_integer_supra(s, r, p, n_a, bits):
        assert got.dtype == torch.int32 and tuple(got.shape) == (p, N.words_per_row(r * r))
        assert np.array_equal(_words(got), want)                             # the whole buffer, padding words zero


# ---- (2) kernel 1, any data --------------------------------------------------------------------------------------------
FLOAT_SHAPES = [(64, 16, 512, 29, 11), (130, 23, 320, 40, 12)]               # (S, R, P, n_a, seed)
FLOAT_TAILS = [(3.1, 0), (2.0, 1), (2.0, -1)]                                # (t0, tail)


@functools.lru_cache(maxsize=None)
def _float_case(shape):
    from igcn_amd import ops
    s, r, p, n_a, seed = shape
    e = r * r
    x, y = R.cohort(s, e, n_a, seed)
    rows = np.nonzero(y != 2)[0]
    member = R.draw(p, s, n_a, seed + 100)
    xd = torch.from_numpy(x).cuda()
    _, _, _, planes = ops.perm_prepare(xd, torch.from_numpy(rows).cuda())
    z = ops.perm_planes_to_z(planes, s, e).cpu().numpy().astype(np.float64)
    m = torch.from_numpy(member).cuda()
    g = torch.cat([ops.perm_maxsum(m[i:i + 8], planes, e)[1] for i in range(0, p, 8)]).cpu().numpy()
    mf = member.astype(np.float64)
    return SimpleNamespace(x=xd, y=torch.from_numpy(y).cuda(), member=member, m=m, planes=planes, g=g, G=mf @ z,
                           A=mf @ np.abs(z))


@pytest.mark.parametrize("shape", FLOAT_SHAPES)
def test_float_bits_are_the_thresholded_g_of_perm_maxsum(shape):
    from igcn_amd import ops
    s, r, p, n_a, _ = shape
    e = r * r
    c = _float_case(shape)
    tested = np.ones(e, dtype=bool)
    flags = torch.from_numpy(tested).cuda()
    for t0, tail in FLOAT_TAILS:
        thr = N.threshold_g32(t0, n_a, s - n_a)
        got = N.unpack(_words(ops.perm_supra(c.m, c.planes, e, thr, tail, flags)), e)
        assert np.array_equal(got, N.supra(c.g.astype(np.float64), thr, tail, tested))       # exact
        ref = N.supra(c.G, thr, tail, tested)
        v = np.abs(c.G) if tail == 0 else c.G * tail
        is_open = np.abs(v - thr) <= R.bound(c.A, s)
        print(f"{shape[:4]} t0={t0} tail={tail}: set {ref.mean():.3e}, differing {(got != ref).sum()}, "
              f"open share {is_open.mean():.3e}")
        assert is_open.mean() <= 1e-3                                      # the condition, on the restatement alone
        assert ref.any() and not np.any((got != ref) & ~is_open)


# ---- (3) kernel 2 alone ------------------------------------------------------------------------------------------------
def _graphs(r):
    """(masks bool [130, r, r], names): the structured cases first, then random directed graphs."""
    idx = np.arange(r)
    out, names = [], []

    def add(name, pairs=(), base=None):
        a = np.zeros((r, r), dtype=bool) if base is None else base.copy()
        for i, j in pairs:
            a[i, j] = True
        out.append(a)
        names.append(name)

    add("empty")
    add("complete", base=np.ones((r, r), dtype=bool))
    add("diagonal", base=np.eye(r, dtype=bool))
    add("path up", [(i, i + 1) for i in range(r - 1)])
    add("path down", [(i + 1, i) for i in range(r - 1)])
    order = np.random.default_rng(r).permutation(r)
    add("path shuffled", [(int(order[i]), int(order[i + 1])) for i in range(r - 1)])
    zig = np.concatenate([idx[::2], idx[1::2][::-1]])                       # labels descend towards node 0's far end
    add("path zigzag", [(int(zig[i + 1]), int(zig[i])) for i in range(r - 1)])
    add("star out", [(r - 1, j) for j in range(r - 1)])
    add("star in", [(j, 0) for j in range(1, r)])
    h = r // 2
    cl = np.zeros((r, r), dtype=bool)
    cl[:h, :h] = True
    cl[h:, h:] = True
    add("two cliques", base=cl)
    add("two cliques joined", [(r - 1, 0)], base=cl)
    add("ring", [(i, (i + 1) % r) for i in range(r)])
    add("two rings", [(i, (i + 2) % r) for i in range(r)])
    k = 0
    while len(out) < 130:
        degree = (0.5, 1, 2, 8)[k % 4]
        out.append(N.random_entries(1, r, degree, seed=1000 * r + k)[0])
        names.append(f"random {degree}")
        k += 1
    return np.stack(out), names


def _components_case(masks):
    from igcn_amd import ops
    r = masks.shape[1]
    bits = ops.nbs_pack(torch.from_numpy(masks).cuda())
    assert np.array_equal(_words(bits), N.pack(masks.reshape(len(masks), -1)))
    mx, label, extent = ops.nbs_components(bits, r, want_labels=True)
    only = ops.nbs_components(bits, r)
    return bits, mx, label, extent, only


@pytest.mark.parametrize("r", [2, 9, 33, 64, 65, 128])
def test_components_equal_the_union_find(r):
    masks, names = _graphs(r)
    want = N.components_many(masks)
    multi = [len({l for l, n in zip(*np.unique(lab, return_counts=True)) if n > 1}) for lab in want[0]]
    rand = [i for i, n in enumerate(names) if n.startswith("random")]
    if r >= 9:                                                              # the restatement alone: the cases bite
        assert max(multi[i] for i in rand) >= 2 and len({int(want[2][i]) for i in rand}) > 2
    assert multi[names.index("two cliques")] == (2 if r >= 4 else 0) and multi[names.index("two cliques joined")] == 1
    assert want[2][names.index("empty")] == 0 and want[2][names.index("diagonal")] == 1
    assert want[2][names.index("complete")] == r * r and want[2][names.index("path zigzag")] == r - 1
    for sel in (slice(0, 130), [names.index("path zigzag")], slice(0, 4), slice(20, 25)):       # P = 130, 1, 4, 5
        _, mx, label, extent, only = _components_case(masks[sel])
        assert mx.dtype == label.dtype == extent.dtype == torch.int32
        assert np.array_equal(label.cpu().numpy(), want[0][sel])
        assert np.array_equal(extent.cpu().numpy(), want[1][sel])
        assert np.array_equal(mx.cpu().numpy(), want[2][sel]) and torch.equal(mx, only)


# ---- (4) the statistic on a planted sub-network ------------------------------------------------------------------------
S4, R4, P4, NA4 = 64, 40, 512, 29


@functools.lru_cache(maxsize=None)
def _planted_case(symmetric=False):
    x, y, tree = N.planted(symmetric=symmetric)
    members = torch.from_numpy(R.draw(P4, S4, NA4, seed=5)).cuda()
    return SimpleNamespace(x=torch.from_numpy(x).cuda(), y=torch.from_numpy(y).cuda(), tree=tree, members=members,
                           nodes=sorted({v for edge in tree for v in edge}))


def _own_bits(c, out, tail):
    """The device's bits of the observed labelling and of every relabelling, from the ops the statistic calls."""
    from igcn_amd import ops
    rows = torch.arange(S4, device="cuda")
    _, _, _, planes = ops.perm_prepare(c.x.reshape(S4, -1), rows)
    flags = out["tested"].reshape(-1)
    observed = (c.y == 0).to(torch.uint8).view(1, S4)
    thr = out["threshold"][1]
    return (ops.perm_supra(observed, planes, R4 * R4, thr, N.TAILS[tail], flags),
            ops.perm_supra(c.members, planes, R4 * R4, thr, N.TAILS[tail], flags))


def _equals_restatement(out, ref):
    for key in ("supra", "component", "extent", "null_max", "p_fwe", "edge_p_fwe"):
        got = out[key].cpu().numpy()
        assert got.dtype == (np.int32 if key == "null_max" else ref[key].dtype), key
        assert np.array_equal(got, ref[key]), key


def test_planted_sub_network_is_found_and_equals_the_restatement_on_the_own_bits():
    from igcn_amd import stats
    c = _planted_case()
    out = stats.network_based_statistic(c.x, c.y, threshold=3.1, members=c.members)
    assert out["n"] == (NA4, S4 - NA4) and out["permutations"] == P4
    assert out["threshold"] == (3.1, N.threshold_g32(3.1, NA4, S4 - NA4))
    assert np.array_equal(out["tested"].cpu().numpy(), ~np.eye(R4, dtype=bool))
    bits_obs, bits = _own_bits(c, out, "both")
    _equals_restatement(out, N.from_bits(_words(bits_obs), _words(bits), R4))
    root = c.nodes[0]
    comp, extent, p = out["component"].cpu().numpy(), out["extent"].cpu().numpy(), out["p_fwe"].cpu().numpy()
    assert all(bool(out["supra"][i, j]) for i, j in c.tree) and all(comp[v] == root for v in c.nodes)
    assert extent[root] == extent.max() >= 12 and p[root] == 1.0 / (1 + P4)
    t, sup = np.abs(out["t"].cpu().numpy()), out["supra"].cpu().numpy()     # (t is formed from the same G, in fp64)
    assert t[sup].min() >= 3.1 * (1 - 1e-6) and t[~sup & ~np.eye(R4, dtype=bool)].max() <= 3.1 * (1 + 1e-6)
    # one tail
    up = stats.network_based_statistic(c.x, c.y, threshold=3.1, tail="greater", members=c.members)
    _equals_restatement(up, N.from_bits(*[_words(b) for b in _own_bits(c, up, "greater")], R4))
    assert all(up["component"][v] == root for v in c.nodes) and float(up["p_fwe"][root]) == 1.0 / (1 + P4)
    assert bool((up["t"][up["supra"]] > 0).all())
    down = stats.network_based_statistic(c.x, c.y, threshold=3.1, tail="less", members=c.members)
    _equals_restatement(down, N.from_bits(*[_words(b) for b in _own_bits(c, down, "less")], R4))
    assert not any(bool(down["supra"][i, j]) for i, j in c.tree) and int(down["extent"].max()) < 12
    assert float(down["p_fwe"].min()) > 0.05
    # groups the other way round: the tails swap
    swapped = stats.network_based_statistic(c.x, c.y, groups=(1, 0), threshold=3.1, tail="less", permutations=64)
    assert all(bool(swapped["supra"][i, j]) for i, j in c.tree)


def test_symmetric_counts_every_edge_once():
    from igcn_amd import stats
    c = _planted_case(symmetric=True)
    full = stats.network_based_statistic(c.x, c.y, threshold=3.1, members=c.members)
    half = stats.network_based_statistic(c.x, c.y, threshold=3.1, members=c.members, symmetric=True)
    sup = full["supra"].cpu().numpy()
    assert np.array_equal(sup, sup.T)
    assert np.array_equal(half["supra"].cpu().numpy(), np.triu(sup, 1))
    assert np.array_equal(half["tested"].cpu().numpy(), np.triu(np.ones((R4, R4), dtype=bool), 1))
    assert torch.equal(half["component"], full["component"]) and torch.equal(2 * half["extent"], full["extent"])
    root = c.nodes[0]
    assert int(half["extent"][root]) >= 12 and float(half["p_fwe"][root]) == 1.0 / (1 + P4)
    _equals_restatement(half, N.from_bits(*[_words(b) for b in _own_bits(c, half, "both")], R4))


# ---- (5) same bits ------------------------------------------------------------------------------------------------------
def test_same_bits_for_two_runs_any_chunking_and_any_row_of_members():
    from igcn_amd import ops, stats
    c = _planted_case()
    first = stats.network_based_statistic(c.x, c.y, threshold=3.1, members=c.members)
    _same_bits(first, stats.network_based_statistic(c.x, c.y, threshold=3.1, members=c.members))
    for chunk in (64, 100, P4):
        _same_bits(first, stats.network_based_statistic(c.x, c.y, threshold=3.1, members=c.members, chunk=chunk))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(P4)).cuda()
    moved = stats.network_based_statistic(c.x, c.y, threshold=3.1, members=c.members[perm])
    assert torch.equal(moved["null_max"], first["null_max"][perm])
    moved["null_max"] = first["null_max"]
    _same_bits(first, moved)
    # a relabelling equal to the observed labelling reproduces the observed bits and extents
    observed = (c.y == 0).to(torch.uint8).view(1, S4)
    again = c.members.clone()
    again[77] = observed[0]
    bits_obs, bits = _own_bits(SimpleNamespace(x=c.x, y=c.y, members=again), first, "both")
    assert torch.equal(bits[77], bits_obs[0])
    mx, label, extent = ops.nbs_components(bits[70:80], R4, want_labels=True)
    assert int(mx[7]) == int(first["extent"].max()) and torch.equal(extent[7].long(), first["extent"])
    assert torch.equal(label[7].long().masked_fill(extent[7] == 0, -1), first["component"])
    # drawn relabellings: the seed decides them, the chunking does not
    a = stats.network_based_statistic(c.x, c.y, permutations=200, seed=3)
    _same_bits(a, stats.network_based_statistic(c.x, c.y, permutations=200, seed=3, chunk=64))
    assert a["permutations"] == 200 and not torch.equal(
        a["null_max"], stats.network_based_statistic(c.x, c.y, permutations=200, seed=4)["null_max"])


def test_unaligned_and_aligned_member_rows_give_the_same_bits():
    from igcn_amd import ops
    shape = FLOAT_SHAPES[1]
    s, r, p, n_a, _ = shape
    c = _float_case(shape)
    assert c.m.stride(0) % 16                                               # rows at an odd stride: byte staging
    padded = torch.zeros(p, 144, dtype=torch.uint8, device="cuda")[:, :s]
    padded.copy_(c.m)
    flags = torch.ones(r * r, dtype=torch.bool, device="cuda")
    thr = N.threshold_g32(2.0, n_a, s - n_a)
    assert torch.equal(ops.perm_supra(c.m, c.planes, r * r, thr, 0, flags),
                       ops.perm_supra(padded, c.planes, r * r, thr, 0, flags))


# ---- (6) bad inputs -----------------------------------------------------------------------------------------------------
def test_bad_inputs_raise_value_error():
    from igcn_amd import ops, stats
    c = _planted_case()
    nbs = stats.network_based_statistic
    for kw in ({"threshold": 0.0}, {"threshold": -1.0}, {"threshold": float("nan")}, {"threshold": float("inf")},
               {"tail": "two"}, {"tested": torch.ones(R4, R4 + 1, dtype=torch.bool)},
               {"tested": torch.ones(R4 * R4, dtype=torch.bool)}, {"groups": (0, 5)}, {"groups": (1, 1)},
               {"chunk": 0}, {"members": c.members[:, :-1]}):
        with pytest.raises(ValueError):
            nbs(c.x, c.y, **{"members": c.members, **kw})
    bad = c.members.clone()
    bad[3, torch.nonzero(bad[3])[0]] = 0
    with pytest.raises(ValueError):
        nbs(c.x, c.y, members=bad)                                          # a row whose sum is not n_a
    with pytest.raises(ValueError):
        nbs(c.x.reshape(S4, -1), c.y, members=c.members)                    # not [*, R, R]
    with pytest.raises(ValueError):
        nbs(c.x[:, :, :-1], c.y, members=c.members)
    with pytest.raises(ValueError):
        nbs(torch.randn(8, 1, 1, device="cuda"), torch.arange(8).cuda() % 2, permutations=4)         # R below the limit
    with pytest.raises(ValueError, match=str(ops.NBS_MAX_ROIS)):
        nbs(torch.randn(8, 129, 129, device="cuda"), torch.arange(8).cuda() % 2, permutations=4)     # a larger atlas
    x = c.x.clone()
    x[0, 2, 3] = float("inf")
    with pytest.raises(ValueError):
        nbs(x, c.y, members=c.members)
    with pytest.raises(ValueError):
        nbs(c.x[:3], torch.tensor([0, 1, 0]).cuda(), permutations=4)        # one subject in group 1
    bits = ops.nbs_pack(torch.zeros(2, 9, 9, dtype=torch.bool, device="cuda"))
    for r in (1, 129, 12):                                                  # (12: more entries than the rows hold)
        with pytest.raises(ValueError):
            ops.nbs_components(bits, r)
    assert ops.NBS_MAX_ROIS == 128


# ---- (7) end to end -----------------------------------------------------------------------------------------------------
def _sgcn_gat():
    from igcn_amd.sgcn import SGCN_GAT
    torch.manual_seed(3)
    return SGCN_GAT(SimpleNamespace(num_features=3, num_classes=3), 2, 16, rois=90, H_0=3).cuda()


def _end_to_end(model, loader, members, method, **kw):
    from igcn_amd import maps, stats
    got = maps.network_difference(model, loader(), groups=(0, 1), threshold=1.5, members=members, device="cuda", **kw)
    per_batch, ys = [], []
    for data in loader():
        data = data.to("cuda")
        per_batch.append(method(data))
        ys.append(data.y.view(-1))
    want = stats.network_based_statistic(torch.cat(per_batch), torch.cat(ys), groups=(0, 1), threshold=1.5,
                                         members=members)
    return got, want


def _check_end_to_end(got, want):
    sig = got.pop("significant")
    _same_bits(want, got)
    assert tuple(got["t"].shape) == (90, 90) and sig.dtype == torch.int64
    assert bool((got["p_fwe"][sig] <= 0.05).all()) and bool((got["component"][sig] == sig).all())
    assert bool((got["extent"][sig][:-1] >= got["extent"][sig][1:]).all())


def test_network_difference_is_the_statistic_on_the_stacked_edge_importance_maps():
    from igcn_amd import maps
    model = _imgsnp()
    _, loader, members = _cohort()
    got, want = _end_to_end(model, loader, members, lambda d: model.edge_importance(d), source="mask")
    _check_end_to_end(got, want)
    with pytest.raises(ValueError):
        maps.network_difference(model, loader(), groups=(0, 4), members=members, device="cuda")
    with pytest.raises(ValueError):
        maps.network_difference(model, loader(), source="gcn", members=members, device="cuda")


@pytest.mark.parametrize("layer", [0, -1])
def test_network_difference_on_gat_attention(layer):
    model = _sgcn_gat()
    _, loader, members = _cohort()
    got, want = _end_to_end(model, loader, members, lambda d: model.gat_attention(d)[:, layer], source="gat", layer=layer)
    _check_end_to_end(got, want)


# ---- (8) fenced ---------------------------------------------------------------------------------------------------------
def test_fenced_runs_write_inside_their_buffers_and_leave_no_poison():
    from fenced import fenced, unwritten
    model = _imgsnp()
    _, loader, members = _cohort()
    masks, _ = _graphs(33)
    with fenced() as f:
        pairs = _run_integer_supra(*INT_SHAPES[3], 18)
        assert all(np.array_equal(_words(a), b) for a, b in pairs)
        outs = [a for a, _ in pairs] + list(_components_case(masks))
        got, _ = _end_to_end(model, loader, members, lambda d: model.edge_importance(d), source="mask")
        torch.cuda.synchronize()
        f.check()
        assert any(s.startswith("ig-gcn_amd/gdc.py") for s in f.sites)      # (the package's device-buffer helper)
        assert 129 * 4 * 4 in sorted(r[1] for r in f.records)               # the bits of (64, 9, 129, 29): 4 words a row
        for t in (*outs, *[v for v in got.values() if torch.is_tensor(v)]):
            assert unwritten(t) == 0
    assert int(outs[-2].sum()) > 0 and not bool(torch.isnan(got["t"]).any())
