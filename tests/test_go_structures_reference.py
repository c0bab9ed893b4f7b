"""CPU checks of tests/go_structures.py, run before any GPU test uses it: the generator hands out valid structures (a
kernel is never given an index the CPU has not checked), the fp64 references agree with a dense-matrix evaluation, and
— through the host-side route probes igcn_spmm_route / igcn_go_route, the functions the launch wrappers themselves read
(csrc/go.hip) — every row of every case table lands on the route it names and the tables together reach every route
the probes can answer in default mode.  Coverage is a condition: a threshold that moves fails here, and the table gets
a new shape.  No GPU, no compute calls."""
import ctypes
import os

import numpy as np
import pytest
import torch

import go_structures as gs
from igcn_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def spmm_route(lib, pass_, b, c, i, j, nnz):
    out = (ctypes.c_int64 * 4)()
    assert lib.igcn_spmm_route(pass_, b, c, i, j, nnz, out) == 0, lib.igcn_last_error()
    return dict(zip(("route", "tile", "lds", "wgs"), (int(v) for v in out)))


def go_route(lib, op, b, nin, nout, fin, fout, with_ln=0):
    out = (ctypes.c_int64 * 4)()
    assert lib.igcn_go_route(op, b, nin, nout, fin, fout, with_ln, out) == 0, lib.igcn_last_error()
    return dict(zip(("route", "threads", "passes", "lds"), (int(v) for v in out)))


# ------------------------------------------------------------------------------------------------ generator validity
def _all_structures():
    for c in gs.MAP_CASES:
        yield "map " + c.name, c.build(), (c.I, c.J)
    for k, e in enumerate(gs.ENC_CASES):
        yield f"enc {e.fin} {e.n}", gs.square_planted(e.n, 200 + k), (e.n, e.n)
    for n, _, _ in gs.ENC_LN_CASES:
        yield f"enc-ln {n}", gs.square_planted(n, 300 + n), (n, n)
    for k, d in enumerate(gs.DEC_CASES):
        yield f"dec {d.nin} {d.nout} {d.head}", gs.decoder(d.nout, d.nin, d.head, 400 + k), (d.nout, d.nin)
    yield "square short", gs.square_short(700, 1), (700, 700)


def _check(name, s, shape):
    from igcn_amd import ops
    n_rows, n_cols = shape
    assert (s.n_rows, s.n_cols) == shape, name
    r, c = s.rows.numpy(), s.cols.numpy()
    assert r.dtype == np.int64 and c.dtype == np.int64 and r.shape == c.shape, name
    if r.size:
        assert r.min() >= 0 and r.max() < n_rows and c.min() >= 0 and c.max() < n_cols, name
        key = r * n_cols + c
        assert (key[1:] > key[:-1]).all(), name                        # row-major and unique
    rl, cl = np.bincount(r, minlength=n_rows), np.bincount(c, minlength=n_cols)
    for row, want in s.planted_rows.items():
        assert rl[row] == want, (name, "row", row, want, rl[row])
    for col, want in s.planted_cols.items():
        assert cl[col] == want, (name, "col", col, want, cl[col])
    if s.empty_row is not None:
        assert rl[s.empty_row] == 0 and cl[s.empty_col] == 0, name
    csr = ops.Csr(s.rows, s.cols, n_rows, n_cols, "cpu")              # what the kernels are handed
    for ptr, idx, n_lists, bound in ((csr.row_ptr, csr.col, n_rows, n_cols), (csr.t_ptr, csr.t_row, n_cols, n_rows)):
        p = ptr.numpy().astype(np.int64)
        assert p.shape == (n_lists + 1,) and p[0] == 0 and (np.diff(p) >= 0).all() and p[-1] == r.size, name
        if r.size:
            assert idx.min() >= 0 and idx.max() < bound, name
    if r.size:
        tk = csr.t_k.numpy()
        assert sorted(tk.tolist()) == list(range(r.size)), name
    return rl, cl


def test_every_table_structure_is_valid():
    for name, s, shape in _all_structures():
        _check(name, s, shape)


def test_planted_recipe_places_its_lists_where_it_says():
    s = gs.planted(600, 1024, 104)
    rl, cl = _check("planted", s, (600, 1024))
    for lens, planted_, n in ((rl, s.planted_rows, 600), (cl, s.planted_cols, 1024)):
        assert sorted(planted_.values()) == sorted(gs.PLANTED)
        heavy = [i for i, v in planted_.items() if v > 12]
        groups = np.bincount(np.asarray(heavy) // 64)
        assert groups.max() >= 2                                       # two heavy lists inside one wave's 64 lists
        assert planted_.get(n - 1, 0) > 12                             # a heavy list on the last row / column
        assert (lens == 0).any()
    # the short recipe: 0-4 entries, about a third empty
    rl, _ = _check("short", gs.short(3000, 500, 3), (3000, 500))
    assert rl.max() <= 4 and 0.25 < (rl == 0).mean() < 0.42 and 1.3 < rl.mean() < 1.7
    # long: nnz > 8 rows, every row at least 9
    s = gs.long(57, 3001, 110, (192, 193, 230, 700))
    rl, _ = _check("long", s, (57, 3001))
    assert rl.min() >= 9 and s.rows.numel() > 8 * 57 and sorted(rl[-4:].tolist()) == [192, 193, 230, 700]
    assert gs.exact(100, 300, 801, 1).rows.numel() == 801
    # the same seed gives the same structure
    a, b = gs.planted(300, 54, 7), gs.planted(300, 54, 7)
    assert torch.equal(a.rows, b.rows) and torch.equal(a.cols, b.cols)


def test_decoder_variants_sit_on_both_sides_of_the_column_cap():
    """GO_DEC_COLCAP (4096 column indices of a workgroup's rows in LDS) with a margin of 2x on either side, for the
    first workgroup's GO_DEC_ROWS = 3072 rows."""
    for k, d in enumerate(gs.DEC_CASES):
        s = gs.decoder(d.nout, d.nin, d.head, 400 + k)
        if d.nout > gs.GO_DEC_ROWS:
            if d.head == "dense":
                assert gs.head_entries(s) > 2 * gs.GO_DEC_COLCAP, (d, gs.head_entries(s))
            else:
                assert gs.head_entries(s) < gs.GO_DEC_COLCAP // 2, (d, gs.head_entries(s))
                assert min(s.planted_rows) >= gs.GO_DEC_ROWS           # heavy rows in a workgroup with r_base != 0
    assert {d.head for d in gs.DEC_CASES if d.nout > gs.GO_DEC_ROWS and d.fout == 5 and d.nin >= 600} == {"dense", "sparse"}


# ------------------------------------------------------------------------------------------------ oracle cross-check
def test_references_agree_with_a_dense_evaluation():
    """The fp64 references against dense-matrix fp64 on a 30-node structure, to 1e-12."""
    rng = np.random.default_rng(0)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s))             # noqa: E731
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))   # noqa: E731
    n, b = 30, 3
    # map: y[b, c, :] = (A * val_c) x
    s = gs.make(n, 17, gs._short_lengths(n), 5, planted_rows=(13, 5), planted_cols=(14,))
    a = gs.dense_of(s.rows, s.cols, n, 17)
    x, val = t(b, 17), t(2, s.rows.numel())
    dense = torch.stack([torch.einsum("ij,bj->bi", torch.zeros(n, 17, dtype=torch.float64).index_put(
        (s.rows, s.cols), val[c]), x) for c in range(2)], 1)
    assert close(gs.map_ref(s.rows, s.cols, n, x, val), dense)
    # encoder layer: softmax over a row's entries of exp(tanh(.)), as a masked dense matrix
    s = gs.make(n, n, gs._short_lengths(n), 6, planted_rows=(13,), planted_cols=(14,))
    a = gs.dense_of(s.rows, s.cols, n, n)
    for fin in (2, 5):
        xd, w_inc, w_s, a_in, a_s = t(b, n, fin), t(5, fin), t(5, fin), t(1, 10), t(1, 5)
        x_in, x_s = xd @ w_inc.t(), xd @ w_s.t()
        e = torch.exp(torch.tanh((x_in @ a_in[0, :5]).unsqueeze(2) + (x_in @ a_in[0, 5:]).unsqueeze(1))) * a
        den = e.sum(2, keepdim=True)
        alpha = torch.where(den > 0, e / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(e))
        dense = alpha @ x_in + x_s * torch.sigmoid(x_s @ a_s.t())
        y = gs.attn_ref(s.rows, s.cols, xd, w_inc, w_s, a_in, a_s)
        assert close(y, dense)
        # + LayerNorm block, written out
        gamma, beta = 1 + 0.2 * t(n), 0.1 * t(n)
        keep = torch.from_numpy((rng.random((b, n)) > 0.3) / 0.7)
        yt = dense.transpose(1, 2)
        mu, var = yt.mean(2, keepdim=True), yt.var(2, unbiased=False, keepdim=True)
        z = torch.relu((yt - mu) / torch.sqrt(var + 1e-5) * gamma + beta) * keep.unsqueeze(1)
        assert close(gs.attn_ln_ref(s.rows, s.cols, keep, 8, xd, w_inc, w_s, a_in, a_s, gamma, beta), z[:, :, 8:])
    # decoder layer: row-normalised adjacency + the self term on the last n_cols rows
    s = gs.make(n, 11, gs._short_lengths(n), 7, planted_rows=(9,), planted_cols=(13,))
    a = gs.dense_of(s.rows, s.cols, n, 11)
    for fout in (5, 2):
        xd, w_out, w_sout = t(b, 11, 5), t(fout, 5), t(fout, 5)
        deg = a.sum(1, keepdim=True)
        dense = (a / torch.where(deg > 0, deg, torch.ones_like(deg))) @ (xd @ w_out.t())
        dense[:, n - 11:] += xd @ w_sout.t()
        assert close(gs.decode_ref(s.rows, s.cols, n, 11, xd, w_out, w_sout), dense)
        gamma, beta = 1 + 0.2 * t(n), 0.1 * t(n)
        yt = dense.transpose(1, 2)
        mu, var = yt.mean(2, keepdim=True), yt.var(2, unbiased=False, keepdim=True)
        z = torch.relu((yt - mu) / torch.sqrt(var + 1e-5) * gamma + beta)
        assert close(gs.decode_ln_ref(s.rows, s.cols, n, 11, None, xd, w_out, w_sout, gamma, beta), z)


# ------------------------------------------------------------------------------------------------ coverage
def test_every_map_case_takes_the_route_it_names(lib):
    for c in gs.MAP_CASES:
        nnz = c.build().rows.numel()
        f = spmm_route(lib, gs.PASS_FWD, c.B, c.C, c.I, c.J, nnz)
        d = spmm_route(lib, gs.PASS_DX, c.B, c.C, c.I, c.J, nnz)
        v = spmm_route(lib, gs.PASS_DVAL, c.B, c.C, c.I, c.J, nnz)
        assert f["route"] == c.fwd, (c.name, "forward", f)
        assert d["route"] == c.dx, (c.name, "dx", d)
        assert (v["route"], v["tile"]) == c.dval, (c.name, "dval", v)
        assert 2 <= c.B <= 11 and c.B % 8, c.name                       # off the sample tile of k_spmm_rows_tiled
    c = gs.MAP_BY_NAME["1"]
    assert c.B % c.dval[1] and c.B > 2 * c.dval[1]                      # full value-gradient tiles and a ragged last one
    for name, pass_ in gs.MAP_BIG_LDS:
        c = gs.MAP_BY_NAME[name]
        r = spmm_route(lib, pass_, c.B, c.C, c.I, c.J, c.build().rows.numel())
        assert gs.BIG_LDS < r["lds"] <= 160 * 1024, (name, pass_, r)
    # scalar staging of k_spmm_long_lds: an operand vector whose length is no multiple of 4
    assert all(c.J % 4 for c in gs.MAP_CASES if c.name.startswith("6-"))
    # the two-map value-gradient launch: lds + global, and two lds maps of different LDS size
    v1, v2, v10 = (spmm_route(lib, gs.PASS_DVAL, c.B, c.C, c.I, c.J, 1) for c in
                   (gs.MAP_BY_NAME["1"], gs.MAP_BY_NAME["2"], gs.MAP_BY_NAME["10"]))
    assert (v1["route"], v2["route"], v10["route"]) == (gs.DVAL_LDS, gs.DVAL_GLOBAL, gs.DVAL_LDS)
    assert v1["lds"] != v10["lds"] and v1["tile"] != v10["tile"]


def test_map_table_reaches_every_route(lib):
    for pass_, attr in ((gs.PASS_FWD, "fwd"), (gs.PASS_DX, "dx")):
        assert {getattr(c, attr) for c in gs.MAP_CASES} == {gs.LONG_LDS, gs.TILED, gs.WAVE, gs.THREAD}, attr
    assert {c.dval for c in gs.MAP_CASES} == {(gs.DVAL_LDS, 4), (gs.DVAL_LDS, 3), (gs.DVAL_LDS, 2), (gs.DVAL_LDS, 1),
                                              (gs.DVAL_GLOBAL, 0)}
    # nothing else can come back: a sweep of sizes around the thresholds answers inside the same sets
    seen_l, seen_v = set(), set()
    for c in (1, 2, 3):
        for i in (1, 100, 7000, 1024, 1025, 10000, 38400, 38401):
            for j in (1, 8, 54, 1024, 1025, 30000, 38400, 38401):
                for nnz in (0, 8 * min(i, j), 8 * i + 1, 8 * j + 1):
                    seen_l.add(spmm_route(lib, gs.PASS_FWD, 3, c, i, j, nnz)["route"])
                    seen_l.add(spmm_route(lib, gs.PASS_DX, 3, c, i, j, nnz)["route"])
                    v = spmm_route(lib, gs.PASS_DVAL, 3, c, i, j, nnz)
                    seen_v.add((v["route"], v["tile"]))
    assert seen_l == {gs.LONG_LDS, gs.TILED, gs.WAVE, gs.THREAD}
    assert seen_v == {c.dval for c in gs.MAP_CASES}


def test_every_encoder_case_takes_the_route_it_names(lib):
    got = set()
    for e in gs.ENC_CASES:
        r = go_route(lib, gs.OP_ATTN_BWD, 2, e.n, e.n, e.fin, 5)
        assert (r["route"], r["threads"], r["passes"]) == e.route, (e, r)
        if r["route"] == gs.LDS:
            got.add((e.fin, r["threads"], r["passes"]))
            assert r["threads"] == lib.igcn_go_attn_bwd_threads(e.n, e.fin, 5) and r["lds"] <= 160 * 1024
    assert got == gs.ENC_REACHABLE
    assert {e.fin for e in gs.ENC_CASES if e.route[0] == gs.GLOBAL} == {2, 5}
    # the reachable set is the whole of what the probe answers: every N up to beyond the LDS limit
    swept = set()
    for fin in (2, 5):
        for n in range(1, 4200):
            r = go_route(lib, gs.OP_ATTN_BWD, 2, n, n, fin, 5)
            if r["route"] == gs.LDS:
                swept.add((fin, r["threads"], r["passes"]))
    assert swept == gs.ENC_REACHABLE
    # both sides of every switch point: the case after a boundary case differs from it
    for fin in (2, 5):
        ns = sorted(e.n for e in gs.ENC_CASES if e.fin == fin)
        routes = {e.n: e.route for e in gs.ENC_CASES if e.fin == fin}
        for a, b in zip(ns[0::2], ns[1::2]):
            assert b == a + 1 and routes[a] != routes[b], (fin, a, b)
    for fin, n in gs.ENC_WALK_ORDER:
        assert any(e.fin == fin and e.n == n for e in gs.ENC_CASES)
    assert {lib.igcn_go_attn_bwd_threads(n, fin, 5) for fin, n in gs.ENC_WALK_ORDER} == {512, 1024}
    for n, pool, ok in gs.ENC_LN_CASES:
        assert lib.igcn_go_attn_ln_fused_ok(n, 2, 5, pool) == ok and pool % 4 == 0, (n, pool)
    assert go_route(lib, gs.OP_ATTN_BWD, 2, 3724, 3724, 2, 5)["route"] == gs.GLOBAL


def test_every_decoder_case_takes_the_route_it_names(lib):
    fwd, bwd = set(), set()
    for d in gs.DEC_CASES:
        f = go_route(lib, gs.OP_DECODE_FWD, 3, d.nin, d.nout, 5, d.fout)
        assert (f["route"], f["passes"]) == d.fwd, (d, f)
        fwd.add(f["route"])
        for b in gs.DEC_BATCHES:
            r = go_route(lib, gs.OP_DECODE_BWD, b, d.nin, d.nout, 5, d.fout)
            want = d.bwd if b >= 128 else (gs.GLOBAL, 256)             # few samples: thread per node
            assert (r["route"], r["threads"]) == want, (d, b, r)
            bwd.add((r["route"], r["threads"] if r["route"] == gs.LDS else 0))
        assert lib.igcn_go_decode_ln_fused_ok(d.nin, d.nout, 5, d.fout) == d.ln_ok, d
        if d.ln_ok:                                                    # the LayerNorm rides along: LDS at any B
            assert go_route(lib, gs.OP_DECODE_BWD, 3, d.nin, d.nout, 5, d.fout, 1)["route"] == gs.LDS
    assert fwd == {gs.LDS, gs.GLOBAL}
    assert bwd == {(gs.LDS, 512), (gs.LDS, 1024), (gs.GLOBAL, 0)}
    assert max(d.fwd[1] for d in gs.DEC_CASES) == 3 and any(d.fwd[1] == 2 for d in gs.DEC_CASES)     # bx >= 1
    assert {d.ln_ok for d in gs.DEC_CASES} == {0, 1}


def test_probes_refuse_bad_arguments(lib):
    out = (ctypes.c_int64 * 4)()
    assert lib.igcn_spmm_route(3, 2, 1, 4, 4, 4, out) != 0
    assert lib.igcn_spmm_route(0, 2, 1, 0, 4, 4, out) != 0
    assert lib.igcn_spmm_route(0, 2, 1, 4, 4, 4, None) != 0
    assert lib.igcn_go_route(7, 2, 10, 10, 2, 5, 0, out) != 0
    assert lib.igcn_go_route(gs.OP_ATTN_BWD, 2, 10, 12, 2, 5, 0, out) != 0
    assert lib.igcn_go_route(gs.OP_DECODE_FWD, 2, 12, 10, 5, 5, 0, out) != 0
    assert lib.igcn_go_route(gs.OP_DECODE_FWD, 2, 10, 12, 5, 5, 0, None) != 0
