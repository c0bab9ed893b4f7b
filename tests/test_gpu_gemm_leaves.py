"""Every template instantiation of the product kernels (csrc/gemm.hip) against an EXACT oracle.

Operands and bias are integers in [-8, 8] stored as fp32: every product is <= 64 in magnitude and every partial sum, in any
order, is an integer below 2^24 (K <= 1100 x batch 40 x 64 = 2.8e6), so fp32 accumulation in any order — and bf16 operands,
which hold these integers exactly — must reproduce the float64 CPU product bit for bit.  The assertion is torch.equal.
Outputs and split-K scratch live inside larger buffers pre-filled with a sentinel bit pattern: every word a call does not
own must come back untouched (compared as int32).  The case table (tests/gemm_cases.py) is the one tests/test_gemm_plan.py
proves to reach all 72 + 9 + 12 + 6 leaves; here each case first checks, with its real pointers, that the launch plan is
the leaf it was built for.  A rounding pass (seeded normal operands, one case per leaf) holds the worst-case bound of fp32
summation element by element."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_cases as gc
from conftest import assert_matches

pytestmark = pytest.mark.gpu

SENT = 0x7FA5A5A5                       # a NaN with a payload no computation produces
SLACK = 64                              # floats of sentinel in front of / behind scratch and grouped outputs


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib
    _lib.load()
    return _lib


def sentinel(n):
    t = torch.full((n,), SENT, dtype=torch.int32, device="cuda").view(torch.float32)
    assert t.data_ptr() % 16 == 0
    return t


def place(values, off):
    """A device buffer holding `values` (flattened) at float offset `off` from its 16-byte-aligned base; (buffer, address)."""
    flat = values.reshape(-1)
    buf = torch.zeros(flat.numel() + off + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + flat.numel()] = flat
    return buf, buf.data_ptr() + 4 * off


def lay(x, rowfast, off):
    """Logical operand x [rows, K] on the device: k-contiguous ([rows, K] storage) or row-contiguous ([K, rows])."""
    return place(x.t().contiguous() if rowfast else x.contiguous(), off)


def region(off, m, n, ld):
    return (off + torch.arange(m, device="cuda")[:, None] * ld + torch.arange(n, device="cuda")[None, :]).reshape(-1)


def check_buffer(buf, idx, want, what):
    """buf[idx] == want exactly (want: device fp32, flattened like idx) and every other word of buf is the sentinel."""
    got = buf[idx]
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        first = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} wrong elements, first at flat index {first}: "
                             f"got {float(got[first])}, want {float(want[first])}")
    mask = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    mask[idx] = False
    stray = torch.nonzero(mask & (buf.view(torch.int32) != SENT))
    assert stray.numel() == 0, f"{what}: {stray.numel()} words outside the output were written, first at {int(stray[0])}"


def untouched(buf, lo, hi, what):
    v = buf.view(torch.int32)
    assert bool((v[:lo] == SENT).all()) and bool((v[hi:] == SENT).all()), f"{what}: scratch written outside its slabs"


def test_the_checker_notices_one_wrong_element_and_one_stray_word(L):
    """check_buffer / untouched themselves (plain tensor work, no product): an output that differs in its last bit, a
    word written next to the output, a word written in front of the scratch."""
    m, n, ld = 5, 7, 10
    want = torch.arange(m * n, dtype=torch.float32, device="cuda")
    idx = region(ld, m, n, ld)

    def fresh():
        buf = sentinel((m + 2) * ld)
        buf[idx] = want
        return buf
    check_buffer(fresh(), idx, want, "clean")
    buf = fresh()
    buf.view(torch.int32)[ld + 3 * ld + 2] += 1                       # one ulp in element (3, 2)
    with pytest.raises(AssertionError, match="1 wrong elements"):
        check_buffer(buf, idx, want, "ulp")
    for stray in (ld + n, ld - 1, ld + m * ld, 0, (m + 2) * ld - 1):  # right of row 0, in front, behind, both ends
        buf = fresh()
        buf[stray] = 0.0
        with pytest.raises(AssertionError, match="outside the output"):
            check_buffer(buf, idx, want, "stray")
    s = sentinel(2 * SLACK + 8)
    untouched(s, SLACK, SLACK + 8, "clean")
    s[SLACK - 1] = 1.0
    with pytest.raises(AssertionError, match="outside its slabs"):
        untouched(s, SLACK, SLACK + 8, "front")


def plan_of(L, c, a_ptr, b_ptr):
    sam, sak, sbn, sbk = gc.strides(c)
    out = (ctypes.c_int64 * 8)()
    L.call("igcn_gemm_plan", c.bf16, c.M, c.N, c.K, a_ptr, sam, sak, b_ptr, sbn, sbk, gc.ldc(c), c.bias, c.act, c.split, out)
    return [int(v) for v in out]


def run_case(L, c, a, b, bias, want, what):
    """One call of igcn_gemm_f32 / igcn_gemm_bf16 as the case lays it out; a, b, bias: device fp32 [M,K], [N,K], [N];
    want: device fp32 [M,N] or None (then the output region is returned unchecked).  Runs the call twice."""
    sam, sak, sbn, sbk = gc.strides(c)
    a_buf, a_ptr = lay(a, c.arf, c.offa)
    b_buf, b_ptr = lay(b, c.brf, c.offb)
    bias_buf, bias_ptr = place(bias, c.offc) if c.bias else (None, None)
    bn, vw, pf, arf, brf, eff, kps, form = plan_of(L, c, a_ptr, b_ptr)
    leaf = (bn, vw) if c.bf16 else (bn, vw, pf, arf, brf)
    assert leaf == c.leaf, f"{what}: plan {leaf}, the case was built for {c.leaf}"
    what = f"{what} plan(bn {bn} vw {vw} pf {pf} arf {arf} brf {brf} split {eff} kps {kps} sum {form})"
    ld = gc.ldc(c)
    off0 = c.offc + ld                                               # a row of slack before, one behind
    idx = region(off0, c.M, c.N, ld)
    name = "igcn_gemm_bf16" if c.bf16 else "igcn_gemm_f32"
    outs = []
    for _ in range(2):
        cbuf = sentinel(c.offc + (c.M + 2) * ld + 4)
        sbuf = sentinel(2 * SLACK + eff * c.M * c.N)
        L.call(name, c.M, c.N, c.K, a_ptr, sam, sak, b_ptr, sbn, sbk, bias_ptr, cbuf.data_ptr() + 4 * off0, ld, c.act,
               c.split, sbuf.data_ptr() + 4 * SLACK, L.stream_ptr())
        torch.cuda.synchronize()
        outs.append((cbuf, sbuf))
    (cbuf, sbuf), (cbuf2, sbuf2) = outs
    assert torch.equal(cbuf.view(torch.int32), cbuf2.view(torch.int32)), f"{what}: two runs differ"
    assert torch.equal(sbuf.view(torch.int32), sbuf2.view(torch.int32)), f"{what}: two runs differ in the slabs"
    untouched(sbuf, SLACK, SLACK + (eff * c.M * c.N if eff > 1 else 0), what)
    if form == gc.SUM_LEFT:                                          # C untouched; the slabs sum to the product
        assert bool((cbuf.view(torch.int32) == SENT).all()), f"{what}: C written although the slabs were left"
        slabs = sbuf[SLACK:SLACK + eff * c.M * c.N].view(eff, c.M, c.N)
        got = slabs.double().sum(0).float()
        if want is not None:
            assert torch.equal(got, want), f"{what}: the float64 sum of the {eff} slabs is not the product"
        return got
    if want is None:
        check_buffer(cbuf, idx, cbuf[idx], what)                     # canaries only
    else:
        try:
            check_buffer(cbuf, idx, want.reshape(-1), what)
        except AssertionError as e:
            bad = torch.nonzero(cbuf[idx].view(c.M, c.N) != want)
            at = tuple(int(v) for v in bad[0]) if bad.numel() else None
            raise AssertionError(f"{e}; first wrong (i, j) = {at}") from None
    return cbuf[idx].view(c.M, c.N)


def reference(a, b, bias, act):
    w = a.double() @ b.double().t()
    if bias is not None:
        w = w + bias.double()
    return torch.relu(w) if act & 1 else w


@pytest.mark.parametrize("dtype,bn", [("f32", 16), ("f32", 32), ("f32", 64), ("bf16", 16), ("bf16", 32), ("bf16", 64)])
def test_every_leaf_is_exact_and_stays_inside_its_output(L, dtype, bn):
    cases = [c for c in gc.CASES if bool(c.bf16) == (dtype == "bf16") and gc.bn_of(c) == bn]
    assert cases
    rng = np.random.default_rng(bn + (100 if dtype == "bf16" else 0))
    mmax, nmax, kmax = max(c.M for c in cases), max(c.N for c in cases), max(c.K for c in cases)
    # the operands of the whole id, once: integer pools (exact pass) and normal pools (rounding pass); a case takes the
    # leading [M, K] / [N, K] block.  A and B are independent draws of different shapes: nothing is symmetric.
    pool = {}
    for kind in ("int", "normal"):
        draw = (lambda *s: rng.integers(-8, 9, s).astype(np.float32)) if kind == "int" else \
               (lambda *s: rng.standard_normal(s).astype(np.float32))
        pool[kind] = tuple(torch.from_numpy(draw(*s)) for s in ((mmax, kmax), (nmax, kmax), (nmax,)))
    dev = {k: tuple(t.cuda() for t in v) for k, v in pool.items()}

    def operands(kind, c, where):
        a, b, bias = where[kind]
        return a[:c.M, :c.K], b[:c.N, :c.K], (bias[:c.N] if c.bias else None)

    seen = set()
    for c in cases:
        # ---- exact pass
        a, b, bias = operands("int", c, pool)
        want = reference(a, b, bias, c.act).float().cuda()
        da, db, dbias = operands("int", c, dev)
        run_case(L, c, da, db, dbias, want, f"{c.name} exact")
        # ---- rounding pass, one case per leaf
        if c.leaf in seen or c.act & gc.ACT_LEAVE:
            continue
        seen.add(c.leaf)
        a, b, bias = operands("normal", c, pool)
        da, db, dbias = operands("normal", c, dev)
        got = run_case(L, c, da, db, dbias, None, f"{c.name} rounding").cpu().double()
        if c.bf16:
            r = lambda t: t.bfloat16().double()                                  # noqa: E731 (round-to-nearest-even)
            want = r(a) @ r(b).t() + (bias.double() if c.bias else 0.0)
            want = torch.relu(want) if c.act & 1 else want
            assert_matches(got, want.numpy(), 2e-5, f"{c.name} bf16 rounding")
        else:
            want = reference(a, b, bias, c.act)
            mag = a.double().abs() @ b.double().abs().t() + (bias.double().abs() if c.bias else 0.0)
            eff = int(L.load().igcn_gemm_effective_split(c.K, c.split))
            bound = (c.K + eff + 2) * 2.0 ** -23 * mag
            err = (got - want).abs()
            worst = float((err - bound).max())
            print(f"{c.name}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert worst <= 0.0, f"{c.name}: |got - want| exceeds (K + S + 2) 2^-23 sum|a b| by {worst:.3e}"
    want_leaves = {c.leaf for c in cases}
    assert {c.leaf for c in cases if not c.act & gc.ACT_LEAVE} == want_leaves == seen


# ------------------------------------------------------------------------------------------------------- flags
def _small(L, m, n, k, split, act, bias=None, pad=0, scratch=True, seed=0):
    rng = np.random.default_rng(seed)
    a = torch.from_numpy(rng.integers(-8, 9, (max(m, 1), k)).astype(np.float32)).cuda()      # (live tensors also where
    b = torch.from_numpy(rng.integers(-8, 9, (n, k)).astype(np.float32)).cuda()              # the call is to be refused)
    c = sentinel(max(m, 1) * (n + pad))
    s = sentinel(max(split, 1) * max(m, 1) * n) if scratch else None
    L.call("igcn_gemm_f32", m, n, k, L.ptr(a), k, 1, L.ptr(b), k, 1, L.ptr(bias), L.ptr(c), n + pad, act, split, L.ptr(s),
           L.stream_ptr())
    torch.cuda.synchronize()
    return a, b, c, s


def test_flags_and_refusals(L):
    # act | 0x100 outside deferred_reductions(): the plain result, bit for bit (split and unsplit)
    for m, n, k, split in ((132, 16, 128, 2), (66, 30, 64, 1), (5, 7, 1088, 34)):
        a, b, c0, _ = _small(L, m, n, k, split, 0)
        _, _, c1, _ = _small(L, m, n, k, split, gc.ACT_FINAL)
        assert torch.equal(c0.view(torch.int32), c1.view(torch.int32))
        assert torch.equal(c0.view(m, n).cpu(), (a.cpu().double() @ b.cpu().double().t()).float())
    assert L.load().igcn_stream_pending(L.stream_ptr()) == 0
    # act | 0x200 takes no bias, no activation and a dense C — refused on the host, before any launch
    bias = torch.ones(30, device="cuda")
    with pytest.raises(L.IgcnError):
        _small(L, 66, 30, 128, 2, gc.ACT_LEAVE, bias=bias)
    with pytest.raises(L.IgcnError):
        _small(L, 66, 30, 128, 2, gc.ACT_LEAVE | 1)
    with pytest.raises(L.IgcnError):
        _small(L, 66, 30, 128, 2, gc.ACT_LEAVE, pad=2)
    with pytest.raises(L.IgcnError):
        _small(L, 66, 30, 128, 2, gc.ACT_LEAVE | gc.ACT_FINAL)
    with pytest.raises(L.IgcnError):                                  # split_k > 1 and no scratch
        _small(L, 66, 30, 128, 2, 0, scratch=False)
    with pytest.raises(L.IgcnError):                                  # M = 0
        _small(L, 0, 30, 128, 1, 0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- batched
BATCHED = [
    # m, n, k, batch, split, brf, a_extra, b_extra, c_extra, pad     (x_batch = dense size + extra)
    (3, 4, 64, 3, 1, 0, 0, 0, 1, 0),           # c_batch 13, ldc 4: C_0 16-byte aligned, C_1 not — both epilogues in one launch
    (3, 4, 64, 3, 2, 0, 0, 0, 1, 0),
    (3, 4, 64, 3, 1, 1, 1, 2, 1, 0),           # a_batch odd, b_batch = 2 mod 4: scalar loads
    (3, 4, 64, 3, 2, 0, 2, 2, 1, 0),           # both = 2 mod 4: 8-byte loads
    (70, 33, 131, 3, 2, 0, 0, 0, 0, 0), (70, 33, 131, 1, 1, 1, 0, 0, 5, 3),
    (132, 32, 160, 3, 2, 1, 0, 4, 0, 4), (132, 32, 96, 1, 3, 0, 4, 0, 7, 0),
    (5, 7, 1088, 3, 34, 0, 0, 0, 0, 0),        # > 32 slabs over few outputs: the batched tree
    (5, 7, 1088, 3, 34, 1, 0, 0, 3, 1),        # ... and the column walk (ldc > N)
]


@pytest.mark.parametrize("m,n,k,batch,split,brf,ax,bx,cx,pad", BATCHED)
def test_batched_products_exact_with_canaries(L, m, n, k, batch, split, brf, ax, bx, cx, pad):
    rng = np.random.default_rng(m + n + k + batch + split)
    a_batch, b_batch, ld = m * k + ax, n * k + bx, n + pad
    c_batch = m * ld + cx
    a = torch.from_numpy(rng.integers(-8, 9, (batch, m, k)).astype(np.float32))
    b = torch.from_numpy(rng.integers(-8, 9, (batch, n, k)).astype(np.float32))
    want = torch.bmm(a.double(), b.double().transpose(1, 2)).float().cuda()
    abuf = torch.zeros(batch * a_batch + 4, device="cuda")
    bbuf = torch.zeros(batch * b_batch + 4, device="cuda")
    for z in range(batch):
        abuf[z * a_batch:z * a_batch + m * k] = a[z].reshape(-1).cuda()
        bbuf[z * b_batch:z * b_batch + n * k] = (b[z].t().contiguous() if brf else b[z]).reshape(-1).cuda()
    sbn, sbk = (1, n) if brf else (k, 1)
    eff = int(L.load().igcn_gemm_effective_split(k, split))
    off0 = ld
    idx = torch.cat([region(off0 + z * c_batch, m, n, ld) for z in range(batch)])
    runs = []
    for _ in range(2):
        cbuf = sentinel(batch * c_batch + 2 * ld + 4)
        sbuf = sentinel(2 * SLACK + batch * eff * m * n)
        L.call("igcn_gemm_f32_batched", m, n, k, batch, L.ptr(abuf), k, 1, a_batch, L.ptr(bbuf), sbn, sbk, b_batch,
               cbuf.data_ptr() + 4 * off0, c_batch, ld, split, sbuf.data_ptr() + 4 * SLACK, L.stream_ptr())
        torch.cuda.synchronize()
        runs.append(cbuf)
        check_buffer(cbuf, idx, want.reshape(-1), "batched")
        untouched(sbuf, SLACK, SLACK + (batch * eff * m * n if eff > 1 else 0), "batched")
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))


def test_batched_entry_points_refuse_k0_and_m0(L):
    t = torch.zeros(64, device="cuda")
    for m, k in ((4, 0), (0, 4)):
        with pytest.raises(L.IgcnError):
            L.call("igcn_gemm_f32_batched", m, 4, k, 2, L.ptr(t), max(k, 1), 1, 16, L.ptr(t), max(k, 1), 1, 16, L.ptr(t), 16, 4,
                   1, L.ptr(t), L.stream_ptr())
        with pytest.raises(L.IgcnError):
            L.call("igcn_gemm_f32_batched_sum", m, 4, k, 2, L.ptr(t), max(k, 1), 1, 16, L.ptr(t), max(k, 1), 1, 16, L.ptr(t), 4,
                   L.ptr(t), L.stream_ptr())
    with pytest.raises(L.IgcnError):                                   # neither operand moves with the batch
        L.call("igcn_gemm_f32_batched_sum", 4, 4, 4, 2, L.ptr(t), 4, 1, 0, L.ptr(t), 4, 1, 0, L.ptr(t), 4, L.ptr(t),
               L.stream_ptr())
    torch.cuda.synchronize()


BATCHED_SUM = [
    # m, n, k, batch, arf, brf, share (0: both move, 1: a_batch == 0, 2: b_batch == 0), pad
    (5, 7, 64, 2, 0, 0, 0, 0), (5, 7, 64, 40, 0, 0, 0, 0),             # column walk over 2 slabs; tree over 40
    (5, 7, 300, 40, 1, 1, 0, 0), (5, 7, 300, 40, 0, 0, 0, 2),          # 80 slabs: tree; ldc > N: column walk over 80
    (5, 7, 1100, 2, 0, 1, 1, 0), (5, 7, 1100, 40, 1, 0, 2, 0),         # K sliced 8 ways by the entry point's own loop
    (70, 33, 300, 2, 0, 0, 2, 3), (70, 65, 64, 40, 1, 1, 1, 0),        # M N > 4096: column walk over 40 slabs, bn 64
    (132, 32, 1100, 2, 1, 1, 0, 0), (63, 16, 300, 2, 1, 0, 0, 0),
]


@pytest.mark.parametrize("m,n,k,batch,arf,brf,share,pad", BATCHED_SUM)
def test_batched_sum_exact_with_canaries(L, m, n, k, batch, arf, brf, share, pad):
    rng = np.random.default_rng(m + n + k + batch + share)
    na, nb = (1 if share == 1 else batch), (1 if share == 2 else batch)
    a = torch.from_numpy(rng.integers(-8, 9, (na, m, k)).astype(np.float32))
    b = torch.from_numpy(rng.integers(-8, 9, (nb, n, k)).astype(np.float32))
    want = sum(a[z % na].double() @ b[z % nb].double().t() for z in range(batch)).float().cuda()
    abuf = (a.transpose(1, 2) if arf else a).contiguous().cuda()
    bbuf = (b.transpose(1, 2) if brf else b).contiguous().cuda()
    sam, sak = (1, m) if arf else (k, 1)
    sbn, sbk = (1, n) if brf else (k, 1)
    ld = n + pad
    idx = region(ld, m, n, ld)
    room = 16 * batch * m * n                                          # the scratch the header asks for
    runs = []
    for _ in range(2):
        cbuf = sentinel((m + 2) * ld + 4)
        sbuf = sentinel(2 * SLACK + room)
        L.call("igcn_gemm_f32_batched_sum", m, n, k, batch, L.ptr(abuf), sam, sak, 0 if share == 1 else m * k, L.ptr(bbuf),
               sbn, sbk, 0 if share == 2 else n * k, cbuf.data_ptr() + 4 * ld, ld, sbuf.data_ptr() + 4 * SLACK,
               L.stream_ptr())
        torch.cuda.synchronize()
        runs.append(cbuf)
        check_buffer(cbuf, idx, want.reshape(-1), "batched_sum")
        untouched(sbuf, SLACK, SLACK + room, "batched_sum")
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------------- grouped
def _group_run(L, members, bf16, rng_seed, single=False):
    """Run a group (or, `single`, its members one igcn_gemm_f32 / igcn_gemm_bf16 call each) on fresh sentinel buffers;
    returns (table, per-member output buffers, per-member scratch buffers, per-member references)."""
    rng = np.random.default_rng(rng_seed)
    bufs, wants = {}, []
    for i, (m, n, k, arf, brf, off, bias, act, split) in enumerate(members):
        a = torch.from_numpy(rng.integers(-8, 9, (m, k)).astype(np.float32))
        b = torch.from_numpy(rng.integers(-8, 9, (n, k)).astype(np.float32))
        bv = torch.from_numpy(rng.integers(-8, 9, (n,)).astype(np.float32))
        wants.append(reference(a, b, bv if bias else None, act).float().cuda())
        bufs[i, "a"] = lay(a.cuda(), arf, off)[0]
        bufs[i, "b"] = lay(b.cuda(), brf, off)[0]
        bufs[i, "bias"] = place(bv.cuda(), off)[0]
        bufs[i, "c"] = sentinel(2 * SLACK + m * n + 4)
        bufs[i, "scratch"] = sentinel(2 * SLACK + max(1, split) * m * n)

    def addr(i, what, floats):
        t = bufs[i, what]                                              # (group_table adds the member's own offset)
        return t.data_ptr() if what in ("a", "b", "bias") else t.data_ptr() + 4 * SLACK
    table = gc.group_table(members, bf16, addr)
    arr = (ctypes.c_int64 * len(table))(*table)
    if single:
        for i in range(len(members)):
            t = table[16 * i:16 * i + 16]
            L.call("igcn_gemm_bf16" if bf16 else "igcn_gemm_f32", t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8],
                   t[9] or None, t[10], t[11], t[12], t[13], t[14] or None, L.stream_ptr())
    else:
        assert L.load().igcn_stream_pending(L.stream_ptr()) == 0       # no riders queued
        L.call("igcn_gemm_f32_grouped", len(members), arr, L.stream_ptr())
    torch.cuda.synchronize()
    return arr, bufs, wants


@pytest.mark.parametrize("name,bf16,members,want_plan", gc.GROUPS, ids=[g[0] for g in gc.GROUPS])
def test_grouped_launch_exact_with_canaries(L, name, bf16, members, want_plan):
    arr, bufs, wants = _group_run(L, members, bf16, len(name))
    out = (ctypes.c_int64 * 4)()
    L.call("igcn_gemm_group_plan", len(members), arr, out)
    bn, vw, pf, grouped = (int(v) for v in out)
    assert (grouped == 0) if want_plan is None else (grouped == 1 and (bn, vw, pf) == want_plan), (bn, vw, pf, grouped)
    _, bufs2, _ = _group_run(L, members, bf16, len(name))
    _, bufs1, _ = _group_run(L, members, bf16, len(name), single=True)
    for i, (m, n, k, arf, brf, off, bias, act, split) in enumerate(members):
        what = f"{name} member {i} (group plan bn {bn} vw {vw} pf {pf} grouped {grouped})"
        o = SLACK + off
        idx = torch.arange(o, o + m * n, device="cuda")
        check_buffer(bufs[i, "c"], idx, wants[i].reshape(-1), what)
        eff = int(L.load().igcn_gemm_effective_split(k, split))
        untouched(bufs[i, "scratch"], SLACK, SLACK + (eff * m * n if eff > 1 else 0), what)
        assert torch.equal(bufs[i, "c"].view(torch.int32), bufs2[i, "c"].view(torch.int32)), what + ": two runs differ"
        # the same bits as the one-product launches (for the fallbacks these ARE the launches the entry point makes)
        assert torch.equal(bufs[i, "c"].view(torch.int32), bufs1[i, "c"].view(torch.int32)), what + ": group != single"


def test_grouped_launch_refuses_five_members_and_k0(L):
    five = [gc._m(132, 16, 64)] * 5
    with pytest.raises(L.IgcnError):
        _group_run(L, five, 0, 0)
    with pytest.raises(L.IgcnError):
        _group_run(L, [gc._m(132, 16, 64), gc._m(132, 16, 0)], 0, 0)
    torch.cuda.synchronize()
