"""The GO sparse kernels (csrc/go.hip, csrc/spmm_long.h) against fp64 on every route and list shape: the SNP <-> GO maps,
the attention encoder layer and the decoder layer on the adversarial structures and the case tables of
tests/go_structures.py.  tests/test_go_structures_reference.py proves on the CPU that every case takes the route it
names and that the tables reach every route; each case here asserts its route again through the same probes, then runs
fp32 through ``ops.*`` inside ``fenced()`` (an output word nobody wrote comes back as the poison NaN, an overrun breaks a
fence) and compares with the fp64 references.  Bounds are those of the sibling tests in tests/test_gpu_ops.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import go_structures as gs
from calltrace import record_calls
from conftest import assert_matches
from fenced import fenced

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib, ops as o
    _lib.load()          # raises if libigcn.so is missing: no fallback
    return o


def _lib_():
    from igcn_amd import _lib
    return _lib.load()


def spmm_route(pass_, b, c, i, j, nnz):
    out = (ctypes.c_int64 * 4)()
    assert _lib_().igcn_spmm_route(pass_, b, c, i, j, nnz, out) == 0
    return int(out[0]), int(out[1])


def go_route(op, b, nin, nout, fin, fout, with_ln=0):
    out = (ctypes.c_int64 * 4)()
    assert _lib_().igcn_go_route(op, b, nin, nout, fin, fout, with_ln, out) == 0
    return int(out[0]), int(out[1]), int(out[2])


def _t(rng, *shape, scale=1.0, shift=0.0):
    return torch.from_numpy(rng.standard_normal(shape) * scale + shift).float()


# ------------------------------------------------------------------------------------------------ maps
@functools.lru_cache(maxsize=None)
def _map_problem(name):
    """Structure, inputs and the fp64 outputs / gradients of one map case: computed once, shared, never modified."""
    c = gs.MAP_BY_NAME[name]
    s = c.build()
    rng = np.random.default_rng(1000 + gs.MAP_CASES.index(c))
    nnz = s.rows.numel()
    x, val, cot = _t(rng, c.B, c.J), _t(rng, c.C, nnz, scale=0.1, shift=1.0), _t(rng, c.B, c.C, c.I)
    ref_in = [x.double().requires_grad_(True), val.double().requires_grad_(True)]
    y_ref = gs.map_ref(s.rows, s.cols, c.I, *ref_in)
    g_ref = torch.autograd.grad((y_ref * cot.double()).sum(), ref_in)
    return s, x, val, cot, y_ref.detach().numpy(), g_ref[0].numpy(), g_ref[1].numpy()


def _force_csr(ops, monkeypatch):
    monkeypatch.setattr(ops.SparseMap, "DENSE_LIMIT", 0)              # never the dense image + GEMM formulation
    monkeypatch.setattr(ops.SparseMap, "SPARSE_MIN_BATCH", 0)


def _assert_map_routes(c, nnz):
    assert spmm_route(gs.PASS_FWD, c.B, c.C, c.I, c.J, nnz)[0] == c.fwd, c.name
    assert spmm_route(gs.PASS_DX, c.B, c.C, c.I, c.J, nnz)[0] == c.dx, c.name
    assert spmm_route(gs.PASS_DVAL, c.B, c.C, c.I, c.J, nnz) == c.dval, c.name


@pytest.mark.parametrize("name", [c.name for c in gs.MAP_CASES])
def test_sparse_map_routes(ops, monkeypatch, name):
    c = gs.MAP_BY_NAME[name]
    s, x, val, cot, y_ref, dx_ref, dval_ref = _map_problem(name)
    _assert_map_routes(c, s.rows.numel())
    _force_csr(ops, monkeypatch)
    seen = record_calls(monkeypatch)
    csr = ops.Csr(s.rows, s.cols, c.I, c.J, "cuda")
    with fenced() as f:
        dev = [x.cuda().requires_grad_(True), val.cuda().requires_grad_(True)]
        y = ops.SparseMap.apply(dev[0], csr, dev[1])
        g = torch.autograd.grad((y * cot.cuda()).sum(), dev)
    assert f.records and f.passed["other"] == 0, f.other_sites
    assert [n[0] for n in seen if n[0].startswith("igcn_spmm")] == ["igcn_spmm_fwd", "igcn_spmm_bwd"]
    assert_matches(y, y_ref, TOL, "y")
    assert_matches(g[0], dx_ref, TOL, "dx")
    assert_matches(g[1], dval_ref, TOL, "dval")


@pytest.mark.parametrize("name", ["1", "10"])
def test_sparse_map_routes_with_strided_value_vectors(ops, monkeypatch, name):
    """The C value vectors as views at stride nnz + 5 of one buffer (igcn_spmm_{fwd,bwd}_strided): rows that start at
    addresses of every alignment."""
    c = gs.MAP_BY_NAME[name]
    s, x, val, cot, y_ref, dx_ref, dval_ref = _map_problem(name)
    nnz = s.rows.numel()
    _assert_map_routes(c, nnz)
    _force_csr(ops, monkeypatch)
    seen = record_calls(monkeypatch)
    csr = ops.Csr(s.rows, s.cols, c.I, c.J, "cuda")
    stride = nnz + 5
    flat = torch.full((c.C * stride + 3,), 1e30)                       # the gaps hold a value that would show
    for ch in range(c.C):
        flat[ch * stride:ch * stride + nnz] = val[ch]
    flat = flat.cuda()
    with fenced() as f:
        xs = x.cuda().requires_grad_(True)
        vals = [flat[ch * stride:ch * stride + nnz].detach().requires_grad_(True) for ch in range(c.C)]
        assert ops.SparseMap._row_stride(vals, nnz) == stride
        y = ops.SparseMap.apply(xs, csr, *vals)
        g = torch.autograd.grad((y * cot.cuda()).sum(), [xs] + vals)
    assert f.records and f.passed["other"] == 0, f.other_sites
    assert [n[0] for n in seen if n[0].startswith("igcn_spmm")] == ["igcn_spmm_fwd_strided", "igcn_spmm_bwd_strided"]
    assert_matches(y, y_ref, TOL, "y")
    assert_matches(g[0], dx_ref, TOL, "dx")
    assert_matches(torch.stack(g[1:]), dval_ref, TOL, "dval")


@pytest.mark.parametrize("names", [("1", "2"), ("1", "10"), ("1",)])
def test_two_map_value_gradient_launch(ops, names):
    """igcn_spmm_bwd_dval_multi (a direct ABI call): (1, 2) an LDS map and a global-memory one, (1, 10) two LDS maps of
    different tile and LDS size, (1) one map — against fp64, and the same bits as igcn_spmm_bwd gives for each map."""
    from igcn_amd._lib import call, ptr, stream_ptr
    lib = _lib_()
    want_routes = {"1": gs.DVAL_LDS, "2": gs.DVAL_GLOBAL, "10": gs.DVAL_LDS}
    maps = []
    for name in names:
        c = gs.MAP_BY_NAME[name]
        s, x, val, cot, _, _, dval_ref = _map_problem(name)
        assert spmm_route(gs.PASS_DVAL, c.B, c.C, c.I, c.J, s.rows.numel())[0] == want_routes[name]
        maps.append((c, s.rows.numel(), ops.Csr(s.rows, s.cols, c.I, c.J, "cuda"), x.cuda(), val.cuda(), cot.cuda(),
                     dval_ref))
    with fenced() as f:
        table = (ctypes.c_int64 * (12 * len(maps)))()
        outs, alone, hold = [], [], []
        for k, (c, nnz, csr, x, val, dy, _) in enumerate(maps):
            n_scr = int(lib.igcn_spmm_bwd_scratch_floats(c.B, c.C, c.I, c.J, nnz))
            dval, scratch = torch.empty(c.C, nnz, device="cuda"), torch.empty(n_scr, device="cuda")
            table[12 * k:12 * k + 11] = [c.B, c.C, c.I, c.J, nnz, ptr(csr.col), ptr(csr.row_of), ptr(x), ptr(dy),
                                         ptr(dval), ptr(scratch)]
            outs.append(dval)
            hold.append(scratch)
        call("igcn_spmm_bwd_dval_multi", len(maps), ctypes.addressof(table), stream_ptr())
        for c, nnz, csr, x, val, dy, _ in maps:
            n_scr = int(lib.igcn_spmm_bwd_scratch_floats(c.B, c.C, c.I, c.J, nnz))
            dval, scratch = torch.empty(c.C, nnz, device="cuda"), torch.empty(n_scr, device="cuda")
            call("igcn_spmm_bwd", c.B, c.C, c.I, c.J, nnz, ptr(csr.row_ptr), ptr(csr.col), ptr(csr.row_of), ptr(csr.t_ptr),
                 ptr(csr.t_row), ptr(csr.t_k), ptr(val), ptr(x), ptr(dy), None, ptr(dval), ptr(scratch), stream_ptr())
            alone.append(dval)
            hold.append(scratch)
        torch.cuda.synchronize()
    assert f.records
    for (c, _, _, _, _, _, dval_ref), got, one in zip(maps, outs, alone):
        assert_matches(got, dval_ref, TOL, f"dval of case {c.name}")
        assert torch.equal(got, one), c.name


def test_sparse_map_computes_the_gradient_rows_somebody_reads(ops, monkeypatch):
    """ADVICE.md's contract of ``x._igcn_grad_rows = (lo, hi)``, unchanged here: the producer of x promises that only
    rows [lo, hi) of dx are ever read, and the backward computes those only — the other rows of dx are unspecified
    (they stay unwritten), so nothing is asserted about them."""
    c = gs.MAP_BY_NAME["1"]
    s = _map_problem("1")[0]
    nnz, b, lo, hi = s.rows.numel(), 21, 5, 16
    _force_csr(ops, monkeypatch)
    rng = np.random.default_rng(77)
    x, val, cot = _t(rng, b, c.J), _t(rng, c.C, nnz, scale=0.1, shift=1.0), _t(rng, b, c.C, c.I)
    xr = x.double().requires_grad_(True)
    y_ref = gs.map_ref(s.rows, s.cols, c.I, xr, val.double())
    dx_ref = torch.autograd.grad((y_ref * cot.double()).sum(), xr)[0].numpy()
    csr = ops.Csr(s.rows, s.cols, c.I, c.J, "cuda")
    seen = record_calls(monkeypatch)
    with fenced() as f:
        xd = x.cuda().requires_grad_(True)
        xd._igcn_grad_rows = (lo, hi)
        y = ops.SparseMap.apply(xd, csr, val.cuda())
        dx, = torch.autograd.grad((y * cot.cuda()).sum(), [xd])
    assert f.records
    bwd = [n for n in seen if n[0] == "igcn_spmm_bwd"]
    assert len(bwd) == 1 and bwd[0][1] == hi - lo                      # the launch covers the promised rows only
    assert_matches(y, y_ref.detach().numpy(), TOL, "y")
    assert_matches(dx[lo:hi], dx_ref[lo:hi], TOL, "dx rows [5, 16)")


# ------------------------------------------------------------------------------------------------ encoder layer
def _enc_inputs(fin, n, seed, bsz=2):
    s = gs.square_planted(n, seed)
    rng = np.random.default_rng(seed)
    x = _t(rng, bsz, n, fin)
    par = [_t(rng, *shape, scale=0.5) for shape in ((5, fin), (5, fin), (1, 10), (1, 5))]
    return s, rng, x, par


@pytest.mark.parametrize("fin,n", [(e.fin, e.n) for e in gs.ENC_CASES])
def test_go_attention_layer_routes(ops, fin, n):
    e = next(c for c in gs.ENC_CASES if (c.fin, c.n) == (fin, n))
    assert go_route(gs.OP_ATTN_BWD, 2, n, n, fin, 5) == e.route
    s, rng, x, par = _enc_inputs(fin, n, 200 + gs.ENC_CASES.index(e))
    cot = _t(rng, 2, n, 5)
    ref_in = [t.double().requires_grad_(True) for t in [x] + par]
    y_ref = gs.attn_ref(s.rows, s.cols, *ref_in)
    g_ref = torch.autograd.grad((y_ref * cot.double()).sum(), ref_in)
    csr = ops.Csr(s.rows, s.cols, n, n, "cuda")
    cot_d = cot.transpose(1, 2).contiguous().cuda()
    with fenced() as f:
        dev = [x.transpose(1, 2).contiguous().cuda().requires_grad_(True)] + [p.cuda().requires_grad_(True) for p in par]
        y = ops.GoAttention.apply(dev[0], dev[1], dev[2], dev[3].view(-1), dev[4].view(-1), csr)
        g = torch.autograd.grad((y * cot_d).sum(), dev, retain_graph=True)
    assert f.records and f.passed["other"] == 0, f.other_sites
    assert_matches(y.transpose(1, 2), y_ref.detach().numpy(), TOL, "y")
    assert_matches(g[0].transpose(1, 2), g_ref[0].numpy(), TOL, "dx")
    for got, want, nm in zip(g[1:], g_ref[1:], ("dW_inc", "dW_s", "da_in", "da_s")):
        assert_matches(got, want.numpy(), TOL, nm)
    if (fin, n) in gs.ENC_WALK_ORDER:
        # the balanced thread -> node map of the column walks only moves work between waves: in plain node order the
        # per-node results are the same bits, the parameter sums the same up to summation order
        wo = csr.walk_order(fin, 5)
        assert wo is not None and int((wo >= 0).sum()) == n
        ident = torch.arange(wo.numel(), dtype=torch.int32, device="cuda")
        ident[n:] = -1
        csr._walk_order[(fin, 5)] = ident
        g2 = torch.autograd.grad((y * cot_d).sum(), dev)
        assert torch.equal(g2[0], g[0])
        for a, c2, nm in zip(g2[1:], g[1:], ("dW_inc", "dW_s", "da_in", "da_s")):
            assert_matches(a, c2.cpu().numpy(), 1e-5, nm)


@pytest.mark.parametrize("n,pool,fused", gs.ENC_LN_CASES)
def test_go_attention_with_layernorm_routes(ops, monkeypatch, n, pool, fused):
    """ops.GoAttentionLN (2 -> 5) with dropout factors: one backward launch where igcn_go_attn_ln_fused_ok answers 1,
    the two-pass fallback where it answers 0 (beyond LDS; N no multiple of 4)."""
    assert _lib_().igcn_go_attn_ln_fused_ok(n, 2, 5, pool) == fused
    s, rng, x, par = _enc_inputs(2, n, 300 + n)
    gamma, beta = _t(rng, n, scale=0.2, shift=1.0), _t(rng, n, scale=0.1)
    keep = torch.from_numpy((rng.random((2, n)) > 0.3) / 0.7).float()
    cot = _t(rng, 2, 5, n - pool)
    ref_in = [t.double().requires_grad_(True) for t in [x] + par + [gamma, beta]]
    z_ref = gs.attn_ln_ref(s.rows, s.cols, keep, pool, *ref_in)
    g_ref = torch.autograd.grad((z_ref * cot.double()).sum(), ref_in)
    csr = ops.Csr(s.rows, s.cols, n, n, "cuda")
    seen = record_calls(monkeypatch)
    with fenced() as f:
        dev = [x.transpose(1, 2).contiguous().cuda().requires_grad_(True)] + \
              [p.cuda().requires_grad_(True) for p in par + [gamma, beta]]
        z = ops.GoAttentionLN.apply(dev[0], dev[1], dev[2], dev[3], dev[4], csr, dev[5], dev[6], keep.cuda(), pool, 1e-5)
        g = torch.autograd.grad((z * cot.cuda()).sum(), dev)
    assert f.records and f.passed["other"] == 0, f.other_sites
    assert any(c[0] == "igcn_go_attn_ln_bwd" for c in seen) == bool(fused)
    assert any(c[0] == "igcn_go_attn_bwd" for c in seen) != bool(fused)
    assert_matches(z, z_ref.detach().numpy(), TOL, "z")
    assert_matches(g[0].transpose(1, 2), g_ref[0].numpy(), TOL, "dx")
    for got, want, nm in zip(g[1:], g_ref[1:], ("dW_inc", "dW_s", "da_in", "da_s", "dgamma", "dbeta")):
        assert_matches(got, want.numpy(), TOL, nm)


# ------------------------------------------------------------------------------------------------ decoder layer
@functools.lru_cache(maxsize=None)
def _dec_structure(k):
    d = gs.DEC_CASES[k]
    return gs.decoder(d.nout, d.nin, d.head, 400 + k)


def _dec_id(d):
    return f"{d.nin}-{d.nout}-{d.fout}-{d.head}"


@pytest.mark.parametrize("bsz", gs.DEC_BATCHES)
@pytest.mark.parametrize("k", range(len(gs.DEC_CASES)), ids=[_dec_id(d) for d in gs.DEC_CASES])
def test_go_decoder_layer_routes(ops, k, bsz):
    d = gs.DEC_CASES[k]
    s = _dec_structure(k)
    fin, fout = 5, d.fout
    assert go_route(gs.OP_DECODE_FWD, bsz, d.nin, d.nout, fin, fout)[::2] == d.fwd
    assert go_route(gs.OP_DECODE_BWD, bsz, d.nin, d.nout, fin, fout)[:2] == (d.bwd if bsz >= 128 else (gs.GLOBAL, 256))
    rng = np.random.default_rng(500 + 2 * k + (bsz > 100))
    x = _t(rng, bsz, d.nin, fin)
    par = [_t(rng, fout, fin, scale=0.5) for _ in range(2)]
    cot = _t(rng, bsz, d.nout, fout)
    ref_in = [t.double().requires_grad_(True) for t in [x] + par]
    y_ref = gs.decode_ref(s.rows, s.cols, d.nout, d.nin, *ref_in)
    g_ref = torch.autograd.grad((y_ref * cot.double()).sum(), ref_in)
    csr = ops.Csr(s.rows, s.cols, d.nout, d.nin, "cuda")
    with fenced() as f:
        dev = [x.transpose(1, 2).contiguous().cuda().requires_grad_(True)] + [p.cuda().requires_grad_(True) for p in par]
        assert dev[0].data_ptr() % 16 == 0                             # the forward's one condition the probe does not see
        y = ops.GoDecode.apply(dev[0], dev[1], dev[2], csr)
        g = torch.autograd.grad((y * cot.transpose(1, 2).contiguous().cuda()).sum(), dev)
    assert f.records and f.passed["other"] == 0, f.other_sites
    assert_matches(y.transpose(1, 2), y_ref.detach().numpy(), TOL, "y")
    assert_matches(g[0].transpose(1, 2), g_ref[0].numpy(), TOL, "dx")
    assert_matches(g[1], g_ref[1].numpy(), TOL, "dW_out")
    assert_matches(g[2], g_ref[2].numpy(), TOL, "dW_sout")


_DEC_LN = [k for k, d in enumerate(gs.DEC_CASES) if d.ln_ok] + \
          [next(k for k, d in enumerate(gs.DEC_CASES) if not d.ln_ok and d.nout % 4 == 0)]


@pytest.mark.parametrize("k", _DEC_LN, ids=[_dec_id(gs.DEC_CASES[k]) for k in _DEC_LN])
def test_go_decoder_with_layernorm_routes(ops, monkeypatch, k):
    """ops.GoDecodeLN at B = 3: the LDS-resident backward with the LayerNorm riding along where
    igcn_go_decode_ln_fused_ok answers 1, the two passes where it answers 0."""
    d = gs.DEC_CASES[k]
    s = _dec_structure(k)
    fin, fout, bsz = 5, d.fout, 3
    assert _lib_().igcn_go_decode_ln_fused_ok(d.nin, d.nout, fin, fout) == d.ln_ok
    if d.ln_ok:
        assert go_route(gs.OP_DECODE_BWD, bsz, d.nin, d.nout, fin, fout, 1)[:2] == d.bwd
    rng = np.random.default_rng(600 + k)
    x = _t(rng, bsz, d.nin, fin)
    par = [_t(rng, fout, fin, scale=0.5) for _ in range(2)]
    gamma, beta = _t(rng, d.nout, scale=0.2, shift=1.0), _t(rng, d.nout, scale=0.1)
    keep = torch.from_numpy((rng.random((bsz, d.nout)) > 0.3) / 0.7).float()
    cot = _t(rng, bsz, fout, d.nout)
    ref_in = [t.double().requires_grad_(True) for t in [x] + par + [gamma, beta]]
    z_ref = gs.decode_ln_ref(s.rows, s.cols, d.nout, d.nin, keep, *ref_in)
    g_ref = torch.autograd.grad((z_ref * cot.double()).sum(), ref_in)
    csr = ops.Csr(s.rows, s.cols, d.nout, d.nin, "cuda")
    seen = record_calls(monkeypatch)
    with fenced() as f:
        dev = [x.transpose(1, 2).contiguous().cuda().requires_grad_(True)] + \
              [p.cuda().requires_grad_(True) for p in par + [gamma, beta]]
        z = ops.GoDecodeLN.apply(dev[0], dev[1], dev[2], csr, dev[3], dev[4], keep.cuda(), 1e-5)
        g = torch.autograd.grad((z * cot.cuda()).sum(), dev)
    assert f.records and f.passed["other"] == 0, f.other_sites
    assert any(c[0] == "igcn_go_decode_ln_bwd" for c in seen) == bool(d.ln_ok)
    assert_matches(z, z_ref.detach().numpy(), TOL, "z")
    assert_matches(g[0].transpose(1, 2), g_ref[0].numpy(), TOL, "dx")
    for got, want, nm in zip(g[1:], g_ref[1:], ("dW_out", "dW_sout", "dgamma", "dbeta")):
        assert_matches(got, want.numpy(), TOL, nm)
