"""GPU tests of the max-F permutation test: igcn_perm_maxf (csrc/perm_test.hip) against an int64 oracle where the
arithmetic is exact and against the fp64 restatement (tests/perm_anova_ref.py) inside its bound elsewhere;
``stats.permutation_anova`` and ``maps.group_difference`` with more than two groups on top of it.

Figures of the float-statistics test on an MI355X (printed by the test; the bound is perm_anova_ref.statistic's):
  (66, 270, 512, (20, 25, 21)): largest use of the bound b_obs 0.010, maxstat 0.014; near share 1.2e-04, max-F 1.4e-05
  (131, 513, 320, (40, 50, 41)): largest use of the bound b_obs 0.005, maxstat 0.007; near share 3.4e-04, max-F 4.9e-05
  (70, 130, 256, (15, 20, 17, 18)): largest use of the bound b_obs 0.006, maxstat 0.007; near share 9.0e-05, max-F 0
  (70, 130, 256, (12, 15, 13, 14, 16)): largest use of the bound b_obs 0.004, maxstat 0.006; near share 1.2e-04, max-F 0
  (33, 65, 129, (16, 17)): largest use of the bound b_obs 0.020, maxstat 0.021; near share 0, max-F 0
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import perm_anova_ref as A
import perm_test_ref as R
from test_gpu_perm_test import _bits, _imgsnp, _same_bits, ROIS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _codes(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.uint8)


def _group_sums(z, labels, k):
    """int64 [P, K-1, E]: the accumulated groups' sums of the integer table z [S, E]."""
    return np.stack([(labels == c).astype(np.int64) @ z for c in range(k - 1)], axis=1)


def _padded(labels):
    """The same rows at a 16-byte aligned stride (the 16-byte staging); the bytes behind S hold code 0."""
    p, s = labels.shape
    out = torch.zeros(p, -(-s // 16) * 16 + 16, dtype=torch.uint8, device="cuda")[:, :s]
    out.copy_(labels)
    return out


# ---- (1) exact group sums ----------------------------------------------------------------------------------------------
SUM_SHAPES = [(5, 1), (33, 17), (64, 270), (127, 513), (257, 129)]


@pytest.mark.parametrize("bits", [17, 18])
@pytest.mark.parametrize("shape", SUM_SHAPES)
def test_group_sums_equal_the_int64_oracle(shape, bits):
    """Odd integers of 17 and 18 significant bits (18: the lo plane carries too); the two accumulated groups hold at most
    40 subjects, so every partial sum stays below 2^24 in any order.  Rows at an odd stride (byte staging) and at an
    aligned one (16-byte staging) give the same bits."""
    from igcn_amd import ops
    s, e = shape
    p = min(8, s)
    rng = np.random.default_rng(1000 * s + e + bits)
    z = (rng.integers(2 ** (bits - 2), 2 ** (bits - 1), (s + 2, e)) * 2 + 1) * rng.choice([-1, 1], (s + 2, e))
    rows = np.sort(rng.permutation(s + 2)[:s])
    n = min(40, s // 3)
    labels = A.draw_labels(p, _codes((n, n, s - 2 * n)), seed=s + p)
    _, _, _, planes = ops.perm_prepare(torch.from_numpy(z.astype(np.float32)).cuda(), torch.from_numpy(rows).cuda(),
                                       standardize=False)
    lab = torch.from_numpy(labels).cuda()
    maxstat, b, g = ops.perm_maxf(lab, planes, e, (1.0, 1.0, 1.0), want_g=True)
    want = _group_sums(z[rows], labels, 3)
    assert np.abs(want).max() < 2 ** 24
    assert tuple(g.shape) == (p, 2, e) and np.array_equal(g.cpu().numpy().astype(np.int64), want)
    again = ops.perm_maxf(_padded(lab), planes, e, (1.0, 1.0, 1.0), want_g=True)
    for x, y in zip((maxstat, b, g), again):
        assert torch.equal(_bits(x), _bits(y))
    assert len(ops.perm_maxf(lab, planes, e, (1.0, 1.0, 1.0))) == 2              # (maxstat, b) without want_g


# ---- (2) exact statistic, maxima and counts ------------------------------------------------------------------------------
STAT_SHAPES = [(5, 1, 1, (2, 2, 1)), (33, 17, 63, (11, 12, 10)), (64, 270, 64, (20, 20, 24)),
               (127, 513, 130, (20, 20, 20, 67)), (257, 129, 65, (20, 20, 20, 20, 177)), (33, 17, 63, (16, 17))]
WEIGHTS = (1.0, 0.5, 0.25, 2.0, 1.0)


def _run_stat_case(s, e, p, sizes):
    """Odd integers |z| <= 15, accumulated groups of at most 20 subjects and weights that are powers of two: |G_g| <= 300,
    |sum G_g| <= 1200, and every square, product and sum of B is a multiple of 1/4 below 2^21 — exact in fp32 whatever
    the order or the contraction."""
    from igcn_amd import ops
    k = len(sizes)
    rng = np.random.default_rng(77 * s + e)
    z = (rng.integers(0, 8, (s, e)) * 2 + 1) * rng.choice([-1, 1], (s, e))
    labels = A.draw_labels(p, _codes(sizes), seed=s + p)
    observed = A.draw_labels(1, _codes(sizes), seed=7 * s)
    _, _, _, planes = ops.perm_prepare(torch.from_numpy(z.astype(np.float32)).cuda(), torch.arange(s).cuda(),
                                       standardize=False)
    w = WEIGHTS[:k]
    _, b, g = ops.perm_maxf(torch.from_numpy(observed).cuda(), planes, e, w, want_g=True)
    b_obs = b.view(-1).contiguous()
    maxstat, exceed = ops.perm_maxf(torch.from_numpy(labels).cuda(), planes, e, w, b_obs)

    def four_b(lab):
        gs = _group_sums(z, lab, k)
        w4 = [int(4 * v) for v in w]
        return sum(w4[c] * gs[:, c] ** 2 for c in range(k - 1)) + w4[k - 1] * gs.sum(1) ** 2
    return four_b(observed)[0], four_b(labels), planes, b_obs, g, maxstat, exceed


@pytest.mark.parametrize("shape", STAT_SHAPES)
def test_statistic_maxima_and_counts_equal_the_integer_oracle(shape):
    want_obs, want, _, b_obs, _, maxstat, exceed = _run_stat_case(*shape)
    assert want.max() < 2 ** 23 and want_obs.max() < 2 ** 23
    assert np.array_equal(4.0 * b_obs.cpu().numpy().astype(np.float64), want_obs.astype(np.float64))
    assert np.array_equal(4.0 * maxstat.cpu().numpy().astype(np.float64), want.max(1).astype(np.float64))
    assert np.array_equal(exceed.cpu().numpy().astype(np.int64), (want >= want_obs[None, :]).sum(0))


# ---- (3) float statistics ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float_case(shape):
    """Everything the float tests share, computed once: the data, the device's results and the restatement on the
    device's own reassembled planes, with the fp32 weights the launch was given."""
    from igcn_amd import ops
    s, e, p, sizes, seed = shape
    k = len(sizes)
    x, y = A.cohort_k(s, e, sizes, seed)
    rows = np.nonzero(y != k)[0]
    observed = y[rows].astype(np.uint8)
    labels = A.draw_labels(p, observed, seed + 100)
    w32 = [float(np.float32(1.0 / n)) for n in sizes]
    xd = torch.from_numpy(x).cuda()
    _, _, _, planes = ops.perm_prepare(xd, torch.from_numpy(rows).cuda())
    z = ops.perm_planes_to_z(planes, s, e).cpu().numpy()
    _, b, g = ops.perm_maxf(torch.from_numpy(observed[None, :]).cuda(), planes, e, w32, want_g=True)
    b_obs = b.view(-1).contiguous()
    maxstat, exceed = ops.perm_maxf(torch.from_numpy(labels).cuda(), planes, e, w32, b_obs)
    ref = A.restate(z, labels, observed, w32)
    return SimpleNamespace(x=xd, y=torch.from_numpy(y).cuda(), z=z, xk=x[rows].astype(np.float64), lab=y[rows],
                           labels=labels, ref=ref, near=A.near_counts(ref), b_obs=b_obs.cpu().numpy().astype(np.float64),
                           maxstat=maxstat.cpu().numpy().astype(np.float64),
                           exceed=exceed.cpu().numpy().astype(np.int64))


@pytest.mark.parametrize("shape", A.FLOAT_SHAPES)
def test_float_statistics_inside_the_bound(shape):
    from igcn_amd import stats
    s, e, p, sizes, _ = shape
    k = len(sizes)
    c = _float_case(shape)
    ref, (near, near_fwe) = c.ref, c.near
    # values
    use_b = np.abs(c.b_obs - ref["b_obs"]) / ref["bound_obs"]
    use_m = np.abs(c.maxstat - ref["maxstat"]) / ref["bound"].max(1)
    print(f"{shape[:4]}: largest use of the bound: b_obs {use_b.max():.3f}, maxstat {use_m.max():.3f}")
    assert use_b.max() <= 1.0 and use_m.max() <= 1.0
    # the condition, on the restatement
    print(f"{shape[:4]}: near share {near.sum() / (p * e):.3e}, max-F near share {near_fwe.sum() / (p * e):.3e}")
    assert near.sum() <= 1e-3 * p * e and near_fwe.sum() <= 1e-3 * p * e
    # counts
    fwe = (c.maxstat[:, None] >= c.b_obs[None, :]).sum(0)
    assert np.all(np.abs(c.exceed - ref["exceed"]) <= near)
    assert np.all(np.abs(fwe - ref["fwe"]) <= near_fwe)
    # the test on top of the kernel reports exactly these counts; its significant set is the restatement's
    out = stats.permutation_anova(c.x, c.y, groups=tuple(range(k)), labels=torch.from_numpy(c.labels).cuda())
    assert out["n"] == tuple(sizes) and out["df"] == (k - 1, s - k) and out["permutations"] == p
    for key, count in (("p_unc", c.exceed), ("p_fwe", fwe)):       # the counts behind the p-values, then the p-values
        got = out[key].cpu().numpy()
        assert np.array_equal(np.rint(got * (1 + p)).astype(np.int64) - 1, count), key
        np.testing.assert_allclose(got, (1 + count) / (1.0 + p), rtol=4e-16, atol=0)
    assert np.array_equal(out["null_max"].cpu().numpy().astype(np.float64), c.maxstat)
    sure = near_fwe == 0
    got, want = out["p_fwe"].cpu().numpy() <= 0.05, ref["p_fwe"] <= 0.05
    assert np.array_equal(got[sure], want[sure])
    assert np.any(np.nonzero(got)[0] % 7 == 0)                      # planted columns are found
    assert not bool(out["constant"].any())
    # f, eta2 and the group means against numpy on the raw data
    grand = c.xk.mean(0)
    means = np.stack([c.xk[c.lab == q].mean(0) for q in range(k)])
    ssb = sum(n * (means[q] - grand) ** 2 for q, n in enumerate(sizes))
    sst = ((c.xk - grand) ** 2).sum(0)
    np.testing.assert_allclose(out["eta2"].cpu().numpy(), ssb / sst, rtol=1e-4)
    np.testing.assert_allclose(out["f"].cpu().numpy(), (ssb / (k - 1)) / ((sst - ssb) / (s - k)), rtol=1e-4)
    np.testing.assert_allclose(out["means"].cpu().numpy(), means, rtol=1e-4)


# ---- (4) two groups ----------------------------------------------------------------------------------------------------
def test_two_groups_agree_with_the_two_sample_test():
    """F = t^2 for K = 2.  Both tests count relabellings against the same exact threshold (B = G^2 (1/n_a + 1/n_b) is one
    increasing function of |G|), each within the near count of its own restatement, so the two p_fwe differ by at most
    the two near counts together."""
    from igcn_amd import stats
    shape = A.FLOAT_SHAPES[4]
    s, e, p, sizes, _ = shape
    c = _float_case(shape)
    labels = torch.from_numpy(c.labels).cuda()
    members = (labels == 0).to(torch.uint8)
    f = stats.permutation_anova(c.x, c.y, groups=(0, 1), labels=labels)
    t = stats.permutation_test(c.x, c.y, groups=(0, 1), members=members)
    np.testing.assert_allclose(f["f"].cpu().numpy(), t["t"].cpu().numpy() ** 2, rtol=1e-6)
    assert f["n"] == t["n"] == tuple(sizes)
    _, near_t = R.near_counts(R.restate(c.z, members.cpu().numpy(), (c.lab == 0).astype(np.uint8)), s)
    count = lambda out: np.rint(out["p_fwe"].cpu().numpy() * (1 + p)).astype(np.int64)      # noqa: E731
    assert np.all(np.abs(count(f) - count(t)) <= c.near[1] + near_t)


# ---- (5) reproducibility -----------------------------------------------------------------------------------------------
def test_same_bits_for_two_runs_any_chunking_and_any_row_order():
    from igcn_amd import stats
    shape = A.FLOAT_SHAPES[1]
    p = shape[2]
    c = _float_case(shape)
    labels = torch.from_numpy(c.labels).cuda()
    first = stats.permutation_anova(c.x, c.y, labels=labels)
    _same_bits(first, stats.permutation_anova(c.x, c.y, labels=labels))
    for chunk in (64, 100, p):
        _same_bits(first, stats.permutation_anova(c.x, c.y, labels=labels, chunk=chunk))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(p)).cuda()
    moved = stats.permutation_anova(c.x, c.y, labels=labels[perm])
    assert torch.equal(_bits(moved["null_max"]), _bits(first["null_max"][perm]))
    assert torch.equal(_bits(moved["p_unc"]), _bits(first["p_unc"]))
    # drawn relabellings: the seed decides them, the chunking does not
    a = stats.permutation_anova(c.x, c.y, permutations=200, seed=3)
    _same_bits(a, stats.permutation_anova(c.x, c.y, permutations=200, seed=3, chunk=64))
    assert a["permutations"] == 200 and not torch.equal(
        a["null_max"], stats.permutation_anova(c.x, c.y, permutations=200, seed=4)["null_max"])
    drawn = stats.draw_labels(torch.from_numpy(c.lab), 50, seed=3)
    assert drawn.is_cuda and bool((drawn.sort(1).values == torch.from_numpy(np.sort(c.lab)).cuda()).all())


# ---- (6) bad inputs ----------------------------------------------------------------------------------------------------
def test_bad_inputs_raise_value_error():
    from igcn_amd import stats
    c = _float_case(A.FLOAT_SHAPES[0])
    labels = torch.from_numpy(c.labels).cuda()
    with pytest.raises(ValueError):
        stats.permutation_anova(c.x, c.y, groups=(0, 1, 7), labels=labels)        # a group without subjects
    with pytest.raises(ValueError):
        stats.permutation_anova(c.x, c.y, groups=(0, 1, 1), labels=labels)        # a repeated label
    with pytest.raises(ValueError):
        stats.permutation_anova(c.x, c.y, groups=(0, 1, 2, 3, 4, 5), permutations=4)          # six groups
    bad = labels.clone()
    bad[3, int(torch.nonzero(bad[3] == 0)[0])] = 1
    with pytest.raises(ValueError):
        stats.permutation_anova(c.x, c.y, labels=bad)                             # a row with wrong counts
    bad = labels.clone()
    bad[5, 0] = 3
    with pytest.raises(ValueError):
        stats.permutation_anova(c.x, c.y, labels=bad)                             # a row holding a code >= K
    x = c.x.clone()
    x[int(torch.nonzero(c.y != 3)[0]), 2] = float("inf")
    with pytest.raises(ValueError):
        stats.permutation_anova(x, c.y, labels=labels)                            # inf in a kept row
    with pytest.raises(ValueError):                                               # group 2 has one subject
        stats.permutation_anova(c.x[:5], torch.tensor([0, 1, 0, 1, 2]).cuda(), permutations=4)
    with pytest.raises(ValueError):                                               # S above the limit
        stats.permutation_anova(torch.randn(4100, 2, device="cuda"), torch.arange(4100).cuda() % 3, permutations=4)


# ---- (7) end to end ----------------------------------------------------------------------------------------------------
def _cohort3():
    """Eight synthetic subjects in three classes of 4 / 2 / 2 and all 420 distinct label rows."""
    from igcn_amd import synth
    from igcn_amd.data import DataLoader
    graphs = synth.brain_graph_list(8, seed=6, rois=ROIS, h0=3, top_k=3, tsne_dim=16, num_classes=3)
    lab = [int(g.y) for g in graphs]
    assert min(lab.count(q) for q in range(3)) >= 2, lab
    rows = torch.tensor(sorted(set(itertools.permutations(lab))), dtype=torch.uint8).cuda()
    assert 210 <= rows.shape[0] <= 4000
    return graphs, (lambda: DataLoader(graphs, batch_size=3)), rows


def _stacked(model, loader, method):
    per_batch, ys = [], []
    for data in loader():
        data = data.to("cuda")
        per_batch.append(method(data))
        ys.append(data.y.view(-1))
    return torch.cat(per_batch), torch.cat(ys)


def _methods(model, quantity):
    if quantity == "association":
        return (lambda d: model.snp_association(d, None, "cuda")), {}
    return (lambda d: model.edge_importance(d)), {"source": "mask"}


@pytest.mark.parametrize("quantity", ["association", "connectivity"])
def test_group_difference_of_three_groups_is_the_anova_on_the_stacked_maps(quantity):
    from igcn_amd import maps, stats
    model = _imgsnp()
    graphs, loader, rows = _cohort3()
    method, kw = _methods(model, quantity)
    got = maps.group_difference(model, loader(), quantity=quantity, groups=(0, 1, 2), members=rows, device="cuda", **kw)
    x, y = _stacked(model, loader, method)
    want = stats.permutation_anova(x, y, groups=(0, 1, 2), labels=rows)
    shape = (ROIS, 54) if quantity == "association" else (ROIS, ROIS)
    assert tuple(got["f"].shape) == shape and tuple(got["means"].shape) == (3,) + shape
    sig = got.pop("significant")
    _same_bits(want, got)
    assert sig.dtype == torch.int64 and sig.numel() <= 10
    assert bool((got["p_fwe"].reshape(-1)[sig] <= 0.05).all())
    assert bool((got["f"].reshape(-1)[sig][:-1] >= got["f"].reshape(-1)[sig][1:]).all())
    # two labels: what the call returned before
    s2 = int(((y == 0) | (y == 1)).sum())
    n_a = int((y == 0).sum())
    members = torch.stack([torch.zeros(s2, dtype=torch.uint8).index_fill_(0, torch.tensor(q), 1)
                           for q in itertools.combinations(range(s2), n_a)]).cuda()
    two = maps.group_difference(model, loader(), quantity=quantity, groups=(0, 1), members=members, device="cuda", **kw)
    want2 = stats.permutation_test(x, y, groups=(0, 1), members=members)
    sig2 = two.pop("significant")
    _same_bits(want2, two)
    hit = torch.nonzero(two["p_fwe"].reshape(-1) <= 0.05).view(-1)
    order = torch.argsort(two["t"].reshape(-1).abs()[hit], descending=True, stable=True)[:10]
    assert torch.equal(sig2, hit[order])


# ---- (8) fenced --------------------------------------------------------------------------------------------------------
def test_fenced_runs_write_inside_their_buffers_and_leave_no_poison():
    from fenced import fenced, unwritten
    from igcn_amd import maps
    model = _imgsnp()
    graphs, loader, rows = _cohort3()
    with fenced() as f:
        _, _, planes, b_obs, g, maxstat, exceed = _run_stat_case(*STAT_SHAPES[3])
        got = maps.group_difference(model, loader(), quantity="association", groups=(0, 1, 2), members=rows,
                                    device="cuda")
        torch.cuda.synchronize()
        f.check()
        for t in (planes, b_obs, g, maxstat, exceed, *[v for v in got.values() if torch.is_tensor(v)]):
            assert unwritten(t) == 0
    assert int(exceed.sum()) > 0 and not bool(torch.isnan(got["f"]).any())
