"""oracle/dropout.py (the numpy restatement of libigcn's dropout-mask generator) on the CPU: known answers — values that
``tests/test_gpu_ops.py::test_dropout_masks_are_a_pure_function_of_counter_and_index`` found equal to the kernel's, bit for
bit, on an MI355X (round 5) — and the statistics a mask needs.  Then ``MaskFeed``, through which the oracle takes the masks
of a HIP run instead of drawing its own: the identity feed, every refusal, and the negative control of the GPU tests that
use it."""
import numpy as np
import pytest
import torch

import dropout_cases as DC
from igcn_amd.data import Batch
from oracle import dropout as OD
from oracle import go_network as OG
from oracle import sgcn_img_snp as OS


def test_known_answers():
    u = OD.uniforms(5, 8)
    assert u.dtype == np.float32
    assert u.tolist() == [0.9984018802642822, 0.5936101078987122, 0.8251862525939941, 0.6147086024284363,
                          0.2441442608833313, 0.6102808117866516, 0.6006595492362976, 0.809348464012146]
    assert OD.uniforms((1 << 40) + 12345, 4).tolist() == [0.7643221616744995, 0.006993472576141357, 0.2771338224411011,
                                                          0.6378827691078186]
    m = OD.masks([((3, 5), 0.4), ((6,), 0.5)], 7)
    k = np.float32(1.0) / (np.float32(1.0) - np.float32(0.4))
    assert m[0].tolist() == [[k, k, 0.0, 0.0, k], [k, k, 0.0, k, k], [k, k, 0.0, 0.0, 0.0]]
    assert m[1].tolist() == [0.0, 2.0, 0.0, 0.0, 2.0, 0.0]        # (the second site starts at element 16, not 15)


def test_statistics_and_independence_of_counters():
    u = OD.uniforms(123, 1 << 18)
    assert 0.0 <= float(u.min()) and float(u.max()) < 1.0
    assert abs(float(u.mean()) - 0.5) < 3e-3 and abs(float((u < 0.3).mean()) - 0.3) < 3e-3
    v = OD.uniforms(124, 1 << 18)
    assert abs(float(np.corrcoef(u, v)[0, 1])) < 0.01              # consecutive steps draw unrelated masks
    assert abs(float(np.corrcoef(u[:-1], u[1:])[0, 1])) < 0.01     # neighbours are unrelated
    a, b = OD.masks([((64, 300), 0.4)], 9)[0], OD.masks([((64, 300), 0.4)], 9)[0]
    assert np.array_equal(a, b)                                    # a pure function of (counter, index, p)
    assert set(np.unique(a).tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.4)))}


# ---- the mask feed: the oracle's ``dropout`` argument as the masks of a HIP run --------------------------------------
def _go_tiny(golden):
    from test_oracle_golden import _go_setup
    store = golden("go_tiny")
    idx, sd = _go_setup(store)
    return store, idx, sd


def _ones_feed(sites, names):
    return OD.feed_of(sites, [np.ones(s, dtype=np.float32) for s, _ in sites], names, check_factors=False)


def _grads(sd, extra=()):
    return {k: v.grad.clone() for k, v in sd.items() if v.requires_grad and v.grad is not None} | \
        {f"input{i}": t.grad.clone() for i, t in enumerate(extra)}


def test_all_ones_feed_is_dropout_off_bit_for_bit_go_forward(golden):
    store, idx, sd0 = _go_tiny(golden)
    snps0 = torch.from_numpy(store["snps"])
    got = []
    for use_feed in (False, True):
        sd = OS.make_leaf_state(sd0)
        snps = snps0.clone().requires_grad_(True)
        feed = _ones_feed(DC.go_sites(idx["pool"], snps.shape[0]), OD.go_site_names(2)) if use_feed else False
        outs = OG.go_forward(sd, idx, snps, training=True, dropout=feed)
        if use_feed:
            feed.close()
        sum((o * o).sum() + o.sum() for o in outs).backward()
        got.append(([o.detach() for o in outs], _grads(sd, [snps])))
    for a, b in zip(got[0][0], got[1][0]):
        assert torch.equal(a, b)
    assert got[0][1].keys() == got[1][1].keys() and len(got[0][1]) > 10
    for k in got[0][1]:
        assert torch.equal(got[0][1][k], got[1][1][k]), k


def test_all_ones_feed_is_dropout_off_bit_for_bit_train_losses(golden):
    from test_oracle_golden import _full_setup
    cfg, idx, sd0, graphs, _ = _full_setup(golden("full_tiny"))
    got = []
    for use_feed in (False, True):
        sd = OS.make_leaf_state(sd0)
        data = Batch.from_data_list(graphs)
        data.x.requires_grad_(True)
        b, hl = len(graphs), sd["lin1.weight"].shape[0]
        sites = DC.go_sites(idx["pool"], 2 * b, [((2 * b, hl), 0.5), ((2 * b, hl), 0.3)])
        feed = _ones_feed(sites, OD.go_site_names(2, OD.HEADS)) if use_feed else False
        loss, terms, _ = OS.train_losses(sd, cfg, idx, data, DC.LAM, dropout=feed)     # (closes the feed itself)
        loss.backward()
        got.append((loss.detach(), {k: torch.as_tensor(v).detach() for k, v in terms.items()}, _grads(sd, [data.x])))
    assert torch.equal(got[0][0], got[1][0])
    for k in got[0][1]:
        assert torch.equal(got[0][1][k], got[1][1][k]), k
    assert got[0][2].keys() == got[1][2].keys() and len(got[0][2]) > 20
    for k in got[0][2]:
        assert torch.equal(got[0][2][k], got[1][2][k]), k


def test_the_feed_applies_the_factors_it_holds():
    """take() returns the named rows; a node site broadcasts its [B, N] factors over the features."""
    sites = [((4, 3), 0.4), ((4, 5), 0.5)]
    m = OD.masks(sites, 11)
    feed = OD.feed_of(sites, m, ["w_act.0", "B.1"])
    x = torch.arange(4 * 3 * 2, dtype=torch.float64).reshape(4, 3, 2) + 1
    lo = OG._node_dropout(x[:2], 0.4, True, feed.rows(0, 2), "w_act.0")
    hi = OG._node_dropout(x[2:], 0.4, True, feed.rows(2, 4), "w_act.0")
    assert torch.equal(torch.cat([lo, hi]), x * torch.from_numpy(m[0]).double().unsqueeze(2))
    y = torch.ones(4, 5, dtype=torch.float64)
    assert torch.equal(OG._dropout(y, 0.5, True, feed, "B.1"), torch.from_numpy(m[1]).double())
    assert OG._dropout(y, 0.5, False, feed, "B.1") is y            # eval mode: no site asks
    feed.close()


def _small_feed(**kw):
    sites = [((4, 3), 0.4), ((4, 5), 0.5), ((4, 5), 0.5)]
    return OD.feed_of(sites, OD.masks(sites, 3), ["w_act.0", "lin1_classify", "lin1_cluster"], **kw)


@pytest.mark.parametrize("why", ["shape", "rows", "p", "values", "scale", "dtype", "twice", "twice_rows", "unknown",
                                 "left", "left_rows", "left_with"])
def test_the_feed_refuses(why):
    x = torch.ones(4, 5, dtype=torch.float64)
    feed = _small_feed()
    with pytest.raises(OD.MaskFeedError) as err:
        if why == "shape":
            feed.take("lin1_classify", (4, 6), 0.5, x)
        elif why == "rows":                                          # a pass asks for more rows than its range holds
            feed.rows(2, 4).take("lin1_classify", (4, 5), 0.5, x)
        elif why == "p":
            feed.take("lin1_classify", (4, 5), 0.3, x)
        elif why == "values":
            OD.MaskFeed({"lin1_classify": (np.full((4, 5), 1.0, dtype=np.float32), 0.5)})
        elif why == "scale":                                         # the factors of another p
            OD.MaskFeed({"lin1_classify": (OD.masks([((4, 5), 0.3)], 1)[0], 0.5)})
        elif why == "dtype":
            OD.MaskFeed({"lin1_classify": (OD.masks([((4, 5), 0.5)], 1)[0].astype(np.float64), 0.5)})
        elif why == "twice":
            feed.take("lin1_classify", (4, 5), 0.5, x)
            feed.take("lin1_classify", (4, 5), 0.5, x)
        elif why == "twice_rows":                                    # the masked pass handed the plain pass's rows
            feed.rows(0, 2).take("lin1_classify", (2, 5), 0.5, x)
            feed.rows(0, 2).take("lin1_classify", (2, 5), 0.5, x)
        elif why == "unknown":
            feed.take("lin1", (4, 5), 0.5, x)
        elif why == "left":
            feed.take("w_act.0", (4, 3), 0.4, x)
            feed.take("lin1_cluster", (4, 5), 0.5, x)
            feed.close()
        elif why == "left_rows":                                     # half of a site's rows
            for name, shape, p in (("w_act.0", (4, 3), 0.4), ("lin1_cluster", (4, 5), 0.5)):
                feed.take(name, shape, p, x)
            feed.rows(0, 2).take("lin1_classify", (2, 5), 0.5, x)
            feed.close()
        elif why == "left_with":
            with feed:
                feed.take("w_act.0", (4, 3), 0.4, x)
                feed.take("lin1_cluster", (4, 5), 0.5, x)
    site = {"unknown": "lin1", "left": "lin1_classify", "left_rows": "lin1_classify", "left_with": "lin1_classify"}
    assert site.get(why, "lin1_classify") in str(err.value), str(err.value)        # the exception names the site


def test_a_site_given_another_sites_mask_is_not_refused_but_differs():
    """Two sites of one shape and p (the CLUSTERLABEL heads) cannot be told apart by the feed's checks: only values do —
    which is why the GPU tests compare losses under the masks by NAME."""
    feed = _small_feed()
    a = feed.take("lin1_classify", (4, 5), 0.5)
    b = feed.take("lin1_cluster", (4, 5), 0.5)
    assert not torch.equal(a, b)


# ---- negative control: other masks give another loss -----------------------------------------------------------------
# dropout_cases.gap between the float64 oracle under the masks of COUNTER and under other masks, at the configurations of
# the GPU tests (tests/dropout_cases.py), as measured here.  The GPU tests hold the HIP loss and terms to LOSS_TOL = 1e-4 of
# the first and require them MARGIN = 100 LOSS_TOL away from the others.  A seed that does not give the margin is replaced
# (headline: graph seeds 78 and 80 gave 0.0052 and 0.0004 on the loss — its ``orth`` term, 9.1 of 12.1, hardly sees the masks
# — 79 gives what is below; GUIDE: seed 83 gave 0.0057, 97 what is below), the margin stays.  The two swap controls read
# the terms (dropout_cases.gap says why), the row swap against dropout_cases.ROWS_MARGIN.
MEASURED = {"headline": 0.011160, "headline_rows_swapped": 0.007375, "guide": 0.016756, "h0_3": 0.020792,
            "h0_3_heads_swapped": 0.024979, "nopredict": 0.029761}


def _gap(name, own, other, what="loss", margin=DC.MARGIN):
    gap = DC.gap(own, other, what)
    print(f"\n[{name}] loss {float(own[0]):.6f} under the step's masks, {float(other[0]):.6f} under the others: "
          f"gap of the {what} {gap:.6f}")
    assert gap >= margin, (name, gap)
    want = MEASURED[name]
    assert want is not None and abs(gap - want) <= 1e-3 * want, (name, gap, want)   # (as recorded)


def swap_rows(arrays, b):
    return [np.concatenate([a[b:], a[:b]], axis=0) for a in arrays]


def test_masks_matter_headline():
    cfg, idx, sd, graphs = DC.headline_cpu(DC.SMALL_POOL)
    b = len(graphs)
    sites = DC.headline_sites(DC.SMALL_POOL, 2 * b)
    names = OD.go_site_names(2, OD.HEADS)

    def loss(feed):
        with torch.no_grad():
            return OS.train_losses(OS.make_leaf_state(sd, torch.float64), cfg, idx, DC.cpu_batch(graphs), DC.LAM,
                                   dropout=feed)[:2]
    own = loss(DC.feed(sites, DC.COUNTER, OD.HEADS))
    _gap("headline", own, loss(DC.feed(sites, DC.COUNTER + 1, OD.HEADS)))
    _gap("headline_rows_swapped", own, loss(OD.feed_of(sites, swap_rows(OD.masks(sites, DC.COUNTER), b), names)), "terms",
         DC.ROWS_MARGIN)


def test_masks_matter_guide():
    from oracle import guide as OGD
    c = DC.GUIDE
    _, sd, idx, graphs, noise = DC.guide_setup(c["hidden"], c["bsz"], c["seed"], "cpu")
    sites = DC.guide_sites(c["bsz"])

    def loss(counter):
        with torch.no_grad():
            return OGD.train_losses(OS.make_leaf_state(sd, torch.float64), OGD.SimpleNamespace(rois=c["rois"]), idx,
                                    OGD.batch_data(Batch.from_data_list(graphs)), c["tau"],
                                    torch.from_numpy(noise).double(),
                                    dropout=DC.feed(sites, counter, OD.GUIDE_EXTRA))[:2]
    _gap("guide", loss(DC.COUNTER), loss(DC.COUNTER + 1))


@pytest.mark.parametrize("tag", DC.CLUSTER_TAGS)
def test_masks_matter_clusterlabel(golden, tag):
    import clusterlabel_ref as REF
    cfg, idx, sd, graphs = REF.fixture_setup(golden("clusterlabel"), tag)
    b = DC.CLUSTER_B
    sites = DC.cluster_sites(cfg.pool, 2 * b)
    names = OD.go_site_names(2, OD.CLUSTER_HEADS)

    def loss(feed):
        with torch.no_grad():
            return REF.train_losses(OS.make_leaf_state(sd, torch.float64), cfg.rois, idx,
                                    DC.cpu_batch(graphs["train"][:b]), cfg.lambda0, cfg.predict, dropout=feed)[:2]
    own = loss(DC.feed(sites, DC.COUNTER, OD.CLUSTER_HEADS))
    _gap(tag, own, loss(DC.feed(sites, DC.COUNTER + 1, OD.CLUSTER_HEADS)))
    if cfg.predict:                     # (a cluster head that predicts nothing enters no term: its mask cannot show)
        m = OD.masks(sites, DC.COUNTER)
        m[-2], m[-1] = m[-1], m[-2]
        _gap(tag + "_heads_swapped", own, loss(OD.feed_of(sites, m, names)), "terms")
