"""GPU tests of the max-T permutation test: igcn_perm_prepare / igcn_perm_maxsum (csrc/perm_test.hip) against an int64
oracle where the arithmetic is exact and against the fp64 restatement (tests/perm_test_ref.py) inside the any-order fp32
summation bound elsewhere; ``stats.permutation_test`` and ``maps.group_difference`` on top of them.

Figures of the float-statistics test on an MI355X (printed by the test; the bound is 2 (S + 8) 2^-24 A):
  (64, 270, 512, 29):  largest use of the bound 0.014 (g_obs 0.014, maxabs 0.012), near share 8.0e-05, max-T 1.4e-05
  (130, 513, 320, 40): largest use of the bound 0.012 (g_obs 0.012, maxabs 0.006), near share 1.9e-04, max-T 1.2e-05
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import perm_test_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.uint8) if t.dtype != torch.bool else t.to(torch.uint8)


def _same_bits(a, b):
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
        else:
            assert a[k] == b[k], k


# ---- (1) exact integers ------------------------------------------------------------------------------------------------
INT_SHAPES = [(5, 1, 1, 2), (33, 17, 63, 11), (64, 270, 64, 29), (127, 513, 130, 40), (257, 129, 65, 40)]


def _integer_case(s, e, p, n_a, bits=17):
    """z: odd integers of ``bits`` significant bits, either sign; n_a <= 40 keeps every partial sum below 2^24 in any
    order at 17 and at 18 bits.  hi takes 8 bits and the SIGNED residual of 17 bits fits mid's 8, so at 17 bits hi and
    mid carry everything and lo is zero; one bit more and about half the values leave a lo of +-1.  Two rows more than
    S in the table, which the row list skips."""
    rng = np.random.default_rng(1000 * s + e)
    z = (rng.integers(2 ** (bits - 2), 2 ** (bits - 1), (s + 2, e)) * 2 + 1) * rng.choice([-1, 1], (s + 2, e))
    rows = np.sort(rng.permutation(s + 2)[:s])
    member = R.draw(p, s, n_a, seed=s + p)
    observed = R.draw(1, s, n_a, seed=7 * s)[0]
    return z.astype(np.int64), rows, member, observed


def _run_integer_case(s, e, p, n_a, bits=17):
    from igcn_amd import ops
    z, rows, member, observed = _integer_case(s, e, p, n_a, bits)
    x = torch.from_numpy(z.astype(np.float32)).cuda()
    _, _, _, planes = ops.perm_prepare(x, torch.from_numpy(rows).cuda(), standardize=False)
    _, g = ops.perm_maxsum(torch.from_numpy(observed[None, :]).cuda(), planes, e)
    g_obs = g.view(-1).contiguous()
    maxabs, exceed = ops.perm_maxsum(torch.from_numpy(member).cuda(), planes, e, g_obs)
    return z[rows], member, observed, planes, g_obs, maxabs, exceed


@pytest.mark.parametrize("bits", [17, 18])
@pytest.mark.parametrize("shape", INT_SHAPES)
def test_integer_sums_equal_the_int64_oracle(shape, bits):
    from igcn_amd import ops
    s, e, p, n_a = shape
    z, member, observed, planes, g_obs, maxabs, exceed = _run_integer_case(*shape, bits)
    back = ops.perm_planes_to_z(planes, s, e).cpu().numpy()
    assert np.array_equal(back.view(np.uint32), z.astype(np.float32).view(np.uint32))
    pl = planes.float().cpu().numpy()
    assert all(np.any(pl[q, :e, :s] != 0) for q in range(3 if bits == 18 else 2))
    assert not np.any(pl[:, e:, :]) and not np.any(pl[:, :, s:])                 # zeros in the padding
    g_want = observed.astype(np.int64) @ z
    big = member.astype(np.int64) @ z
    assert np.abs(big).max() < 2 ** 24
    assert np.array_equal(g_obs.cpu().numpy().astype(np.int64), g_want)
    assert np.array_equal(maxabs.cpu().numpy().astype(np.int64), np.abs(big).max(1))
    assert np.array_equal(exceed.cpu().numpy().astype(np.int64), (np.abs(big) >= np.abs(g_want)[None, :]).sum(0))


def test_unaligned_and_aligned_member_rows_give_the_same_bits():
    """member with rows 16-byte aligned (the 16-byte staging) and at an odd stride (byte staging): one LDS image."""
    from igcn_amd import ops
    s, e, p, n_a = INT_SHAPES[3]
    z, rows, member, observed = _integer_case(s, e, p, n_a)
    x = torch.from_numpy(z.astype(np.float32)).cuda()
    _, _, _, planes = ops.perm_prepare(x, torch.from_numpy(rows).cuda(), standardize=False)
    _, g = ops.perm_maxsum(torch.from_numpy(observed[None, :]).cuda(), planes, e)
    g_obs = g.view(-1).contiguous()
    m = torch.from_numpy(member).cuda()
    padded = torch.zeros(p, 128, dtype=torch.uint8, device="cuda")[:, :s]
    padded.copy_(m)
    a, b = ops.perm_maxsum(m, planes, e, g_obs), ops.perm_maxsum(padded, planes, e, g_obs)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])


# ---- (2) prepare -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 270), (131, 77)])
def test_prepare_statistics_and_standardised_values(shape):
    from igcn_amd import ops
    s, e = shape
    x, y = R.cohort(s, e, s // 2, seed=s, extra=5)
    rows = np.nonzero(y != 2)[0]
    x[:, 3] = 1.25                                                  # constant everywhere
    x[:, 5] = np.where(y == 2, 7.0, -0.5)                           # constant over the listed rows only
    x[y == 2, 9] = 2.0                                              # constant only outside the listed rows: not constant
    mean, sd, constant, planes = ops.perm_prepare(torch.from_numpy(x).cuda(), torch.from_numpy(rows).cuda())
    z_ref, mean_ref, sd_ref, const_ref = R.standardize(x[rows])
    assert const_ref[3] and const_ref[5] and not const_ref[9] and const_ref.sum() == 2
    assert np.array_equal(constant.cpu().numpy().astype(bool), const_ref)
    mean, sd = mean.cpu().numpy(), sd.cpu().numpy()
    assert np.all(np.abs(mean - mean_ref) <= 1e-13 * np.abs(mean_ref))
    assert np.all(np.abs(sd - sd_ref) <= 1e-13 * np.abs(sd_ref))
    z = ops.perm_planes_to_z(planes, s, e).cpu().numpy()
    z32 = z_ref.astype(np.float32)
    assert np.all(np.abs(z.astype(np.float64) - z32.astype(np.float64)) <= np.spacing(np.abs(z32)).astype(np.float64))
    assert not np.any(z[:, const_ref])


# ---- (3) float statistics ----------------------------------------------------------------------------------------------
FLOAT_SHAPES = [(64, 270, 512, 29, 11), (130, 513, 320, 40, 12)]       # (S, E, P, n_a, seed): the CPU test's condition


@functools.lru_cache(maxsize=None)
def _float_case(shape):
    """Everything the float tests share, computed once: the data, the device's results and the restatement on the
    device's own reassembled planes."""
    from igcn_amd import ops
    s, e, p, n_a, seed = shape
    x, y = R.cohort(s, e, n_a, seed)
    rows = np.nonzero(y != 2)[0]
    member = R.draw(p, s, n_a, seed + 100)
    observed = (y[rows] == 0).astype(np.uint8)
    xd = torch.from_numpy(x).cuda()
    _, _, _, planes = ops.perm_prepare(xd, torch.from_numpy(rows).cuda())
    z = ops.perm_planes_to_z(planes, s, e).cpu().numpy()
    _, g = ops.perm_maxsum(torch.from_numpy(observed[None, :]).cuda(), planes, e)
    g_obs = g.view(-1).contiguous()
    maxabs, exceed = ops.perm_maxsum(torch.from_numpy(member).cuda(), planes, e, g_obs)
    ref = R.restate(z, member, observed)
    return SimpleNamespace(x=xd, y=torch.from_numpy(y).cuda(), member=member, ref=ref, near=R.near_counts(ref, s),
                           g_obs=g_obs.cpu().numpy().astype(np.float64), maxabs=maxabs.cpu().numpy().astype(np.float64),
                           exceed=exceed.cpu().numpy().astype(np.int64))


@pytest.mark.parametrize("shape", FLOAT_SHAPES)
def test_float_statistics_inside_the_summation_bound(shape):
    from igcn_amd import stats
    s, e, p, n_a, _ = shape
    c = _float_case(shape)
    ref, (near, near_fwe) = c.ref, c.near
    # values
    b_obs, b_max = R.bound(ref["a_obs"], s), R.bound(ref["A"], s).max(1)
    use_g = np.abs(c.g_obs - ref["g_obs"]) / b_obs
    use_m = np.abs(c.maxabs - ref["maxabs"]) / b_max
    print(f"{shape[:4]}: largest use of the bound: g_obs {use_g.max():.3f}, maxabs {use_m.max():.3f}")
    assert use_g.max() <= 1.0 and use_m.max() <= 1.0
    # the condition, on the restatement
    print(f"{shape[:4]}: near share {near.sum() / (p * e):.3e}, max-T near share {near_fwe.sum() / (p * e):.3e}")
    assert near.sum() <= 1e-3 * p * e and near_fwe.sum() <= 1e-3 * p * e
    # counts
    thr = np.abs(c.g_obs)
    fwe = (c.maxabs[:, None] >= thr[None, :]).sum(0)
    assert np.all(np.abs(c.exceed - ref["exceed"]) <= near)
    assert np.all(np.abs(fwe - ref["fwe"]) <= near_fwe)
    # the test on top of the kernels reports exactly these counts; its significant set is the restatement's
    out = stats.permutation_test(c.x, c.y, groups=(0, 1), members=torch.from_numpy(c.member).cuda())
    assert out["n"] == (n_a, s - n_a) and out["permutations"] == p
    for key, count in (("p_unc", c.exceed), ("p_fwe", fwe)):       # the counts behind the p-values, then the p-values
        got = out[key].cpu().numpy()
        assert np.array_equal(np.rint(got * (1 + p)).astype(np.int64) - 1, count), key
        np.testing.assert_allclose(got, (1 + count) / (1.0 + p), rtol=4e-16, atol=0)
    assert np.array_equal(out["null_max"].cpu().numpy().astype(np.float64), c.maxabs)
    sure = near_fwe == 0
    got, want = out["p_fwe"].cpu().numpy() <= 0.05, ref["p_fwe"] <= 0.05
    assert np.array_equal(got[sure], want[sure])
    assert np.any(np.nonzero(got)[0] % 7 == 0)                      # planted columns are found
    np.testing.assert_allclose(out["t"].cpu().numpy(), R.student_t(c.g_obs, n_a, s - n_a), rtol=1e-12)
    xk = c.x.cpu().numpy().astype(np.float64)[c.y.cpu().numpy() != 2]
    lab = c.y.cpu().numpy()[c.y.cpu().numpy() != 2]
    np.testing.assert_allclose(out["diff"].cpu().numpy(), xk[lab == 0].mean(0) - xk[lab == 1].mean(0), rtol=1e-4,
                               atol=1e-5)


# ---- (4) reproducibility -----------------------------------------------------------------------------------------------
def test_same_bits_for_two_runs_any_chunking_and_any_row_of_members():
    from igcn_amd import stats
    shape = FLOAT_SHAPES[1]
    p = shape[2]
    c = _float_case(shape)
    members = torch.from_numpy(c.member).cuda()
    first = stats.permutation_test(c.x, c.y, members=members)
    _same_bits(first, stats.permutation_test(c.x, c.y, members=members))
    for chunk in (64, 100, p):
        _same_bits(first, stats.permutation_test(c.x, c.y, members=members, chunk=chunk))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(p)).cuda()
    moved = stats.permutation_test(c.x, c.y, members=members[perm])
    assert torch.equal(_bits(moved["null_max"]), _bits(first["null_max"][perm]))
    assert torch.equal(_bits(moved["p_unc"]), _bits(first["p_unc"]))
    # drawn relabellings: the seed decides them, the chunking does not
    a = stats.permutation_test(c.x, c.y, permutations=200, seed=3)
    _same_bits(a, stats.permutation_test(c.x, c.y, permutations=200, seed=3, chunk=64))
    assert a["permutations"] == 200 and not torch.equal(
        a["null_max"], stats.permutation_test(c.x, c.y, permutations=200, seed=4)["null_max"])


def test_bad_inputs_raise_value_error():
    from igcn_amd import stats
    c = _float_case(FLOAT_SHAPES[0])
    members = torch.from_numpy(c.member).cuda()
    with pytest.raises(ValueError):
        stats.permutation_test(c.x, c.y, groups=(0, 5), members=members)          # a group without subjects
    bad = members.clone()
    bad[3, torch.nonzero(bad[3])[0]] = 0
    with pytest.raises(ValueError):
        stats.permutation_test(c.x, c.y, members=bad)                             # a row whose sum is not n_a
    x = c.x.clone()
    x[int(torch.nonzero(c.y != 2)[0]), 2] = float("inf")
    with pytest.raises(ValueError):
        stats.permutation_test(x, c.y, members=members)
    with pytest.raises(ValueError):
        stats.permutation_test(c.x[:3], torch.tensor([0, 1, 0]).cuda(), permutations=4)          # one subject in group 1
    with pytest.raises(ValueError):                                                                # S above the limit
        stats.permutation_test(torch.randn(4100, 2, device="cuda"), torch.arange(4100).cuda() % 2, permutations=4)


# ---- (5) end to end ----------------------------------------------------------------------------------------------------
ROIS, C = 90, 3
POOL = (37, 18, 9, 3, 1)                        # the cohort of tests/test_gpu_maps.py: same models, same DAG


def _imgsnp():
    from igcn_amd import synth
    from igcn_amd.sgcn_img_snp import SGCN_GCN_IMGSNP
    go_snps, adj, pool_dim = synth.go_hierarchy(POOL, seed=2)
    a_g, a = synth.go_sparse_inputs(go_snps, adj, "cuda")
    torch.manual_seed(11)
    return SGCN_GCN_IMGSNP(2, 16, a_g, a, pool_dim, 32, "cuda", rois=ROIS, H_0=3, num_classes=C, isSoftSimilarity=True,
                           rbf_gamma=0.01, isCrossAtten=True, num_regr=3, isuseProb4Regr=True, isImageOnly=False,
                           isSNPsOnly=False).cuda()


def _cohort():
    from igcn_amd import synth
    from igcn_amd.data import DataLoader
    graphs = synth.brain_graph_list(7, seed=6, rois=ROIS, h0=3, top_k=3, tsne_dim=16, num_classes=C)
    labels = [int(g.y) for g in graphs]
    n_a, n_b = labels.count(0), labels.count(1)
    assert n_a >= 2 and n_b >= 2, labels
    s = n_a + n_b
    rows = [torch.zeros(s, dtype=torch.uint8).index_fill_(0, torch.tensor(c), 1)
            for c in itertools.combinations(range(s), n_a)]
    members = torch.stack(rows).cuda()
    return graphs, (lambda: DataLoader(graphs, batch_size=3)), members


def _end_to_end(model, loader, members, quantity, method, kw):
    from igcn_amd import maps, stats
    got = maps.group_difference(model, loader(), quantity=quantity, groups=(0, 1), members=members, device="cuda", **kw)
    per_batch, ys = [], []
    for data in loader():
        data = data.to("cuda")
        per_batch.append(method(data))
        ys.append(data.y.view(-1))
    want = stats.permutation_test(torch.cat(per_batch), torch.cat(ys), groups=(0, 1), members=members)
    return got, want


@pytest.mark.parametrize("quantity", ["association", "connectivity"])
def test_group_difference_is_the_permutation_test_on_the_stacked_maps(quantity):
    from igcn_amd import maps
    model = _imgsnp()
    graphs, loader, members = _cohort()
    method = ((lambda d: model.snp_association(d, None, "cuda")) if quantity == "association" else
              (lambda d: model.edge_importance(d)))
    kw = {} if quantity == "association" else {"source": "mask"}
    got, want = _end_to_end(model, loader, members, quantity, method, kw)
    assert tuple(got["t"].shape) == ((ROIS, 54) if quantity == "association" else (ROIS, ROIS))
    sig = got.pop("significant")
    _same_bits(want, got)
    assert sig.dtype == torch.int64 and sig.numel() <= 10
    assert bool((got["p_fwe"].reshape(-1)[sig] <= 0.05).all())
    with pytest.raises(ValueError):
        maps.group_difference(model, loader(), quantity=quantity, groups=(0, 4), members=members, device="cuda", **kw)


# ---- (6) fenced --------------------------------------------------------------------------------------------------------
def test_fenced_runs_write_inside_their_buffers_and_leave_no_poison():
    from fenced import fenced, unwritten
    model = _imgsnp()
    graphs, loader, members = _cohort()
    with fenced() as f:
        _, _, _, planes, g_obs, maxabs, exceed = _run_integer_case(*INT_SHAPES[2])
        got, _ = _end_to_end(model, loader, members, "association", lambda d: model.snp_association(d, None, "cuda"), {})
        torch.cuda.synchronize()
        f.check()
        assert any(s.startswith("ig-gcn_amd/gdc.py") for s in f.sites)      # (the package's device-buffer helper)
        fenced_bytes = sorted(r[1] for r in f.records)
        assert 3 * 320 * 64 * 2 in fenced_bytes and 4 * 64 in fenced_bytes        # the planes and maxabs of (64, 270, 64, 29)
        for t in (planes, g_obs, maxabs, exceed, *[v for v in got.values() if torch.is_tensor(v)]):
            assert unwritten(t) == 0
    assert int(exceed.sum()) > 0 and not bool(torch.isnan(got["t"]).any())
