"""The exact-fp32 attention core (csrc/attn_mfma.hip) at head_dim 33..96 — the widths of the reference's hidden-32
sweep (main.py:142-145: layers 2..5 at hidden 32 under nn.MultiheadAttention(layers * hidden, 2) = head_dim 32, 48, 64,
80) — padded in LDS to 48 / 64 / 80 / 96 columns: forward and backward, LDS-resident and streamed, against fp64.
(SGCN_GCN_IMGSNP itself does not reach the attention at those widths yet: the GO read-out igcn_node_linear_bn_* is
instantiated for attention widths up to 48 and refuses 64 / 96 / 128 / 160 — DESIGN.md, known issues.)"""
import numpy as np
import pytest
import torch

from conftest import assert_matches

pytestmark = pytest.mark.gpu

CHUNKED = 96 * 1024                      # igcn_attn_core_lds_bytes of the streamed form
# (D, H): head_dim 33 (neither 16-byte rows nor a multiple of 4), 36, 40, 48 -> 48 columns; 64; 80; 96; and four heads
WIDTHS = [(66, 2), (72, 2), (80, 2), (96, 2), (128, 2), (160, 2), (192, 2), (192, 4)]
# one ragged tile each way | resident at every width | forward-sized for residency up to 64 columns, streamed above |
# several key chunks (400 keys: 240-row chunks at 48 columns, 112-row at 96) and two query chunks at 96 columns
SHAPES = [(2, 7, 5), (2, 40, 70), (3, 90, 130), (2, 130, 400)]


def _hdp(hd):
    return (hd + 3) & ~3 if hd <= 32 else (hd + 15) & ~15


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from igcn_amd import _lib, ops as o
    _lib.load()          # raises if libigcn.so is missing: no fallback
    return o


def _case(bsz, lq, lk, d, seed=0):
    rng = np.random.default_rng(lq * lk + d + seed)
    return tuple(torch.from_numpy(rng.standard_normal(s)).float()
                 for s in ((bsz, lq, d), (bsz, lk, 2 * d), (bsz, lq, d)))


def _reference(q, kv, cot, h):
    """softmax(q k^T / sqrt(hd)) v per head and its gradients under ``cot`` in fp64 (the construction of
    test_attention_core)."""
    bsz, lq, d = q.shape
    lk = kv.shape[1]
    rq, rkv = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    qh = rq.view(bsz, lq, h, d // h).transpose(1, 2)
    kvh = rkv.view(bsz, lk, 2, h, d // h)
    k_, v_ = kvh[:, :, 0].transpose(1, 2), kvh[:, :, 1].transpose(1, 2)
    att = torch.softmax(qh @ k_.transpose(-1, -2) / (d // h) ** 0.5, dim=-1)
    o_ref = (att @ v_).transpose(1, 2).reshape(bsz, lq, d)
    g_ref = torch.autograd.grad((o_ref * cot.double()).sum(), [rq, rkv])
    return o_ref.detach(), g_ref[0], g_ref[1]


def _rel(got, want, floor=0.0):
    return float((got.detach().cpu().double() - want).abs().max()) / max(float(want.abs().max()), floor)


def _check(tag, got, want):
    print("ATTN_WIDE %s o %.3e dq %.3e dkv %.3e" % (tag, _rel(got[0], want[0]), _rel(got[1], want[1], 1e-6),
                                                    _rel(got[2], want[2], 1e-6)))
    assert_matches(got[0], want[0].numpy(), 1e-4, "o")
    assert_matches(got[1], want[1].numpy(), 2e-4, "dq", floor=1e-6)
    assert_matches(got[2], want[2].numpy(), 2e-4, "dkv", floor=1e-6)


@pytest.mark.parametrize("bsz,lq,lk", SHAPES)
@pytest.mark.parametrize("d,h", WIDTHS)
def test_attention_core_wide_vs_fp64(ops, d, h, bsz, lq, lk):
    """o within 1e-4, dq / dkv within 2e-4 (floor 1e-6) of the fp64 attention: the bounds of test_attention_core.  They
    rest on exact-fp32 products with fp32 accumulation; a reduction over 96 instead of 32 columns stays far inside."""
    q, kv, cot = _case(bsz, lq, lk, d)
    want = _reference(q, kv, cot, h)
    assert ops.attn_core_supported(d, h, lq, lk)
    q_, kv_ = q.cuda().requires_grad_(True), kv.cuda().requires_grad_(True)
    o = ops.AttentionCore.apply(q_, kv_, h)
    g = torch.autograd.grad((o * cot.cuda()).sum(), [q_, kv_])
    _check("hd=%d hdp=%d h=%d shape=%dx%dx%d" % (d // h, _hdp(d // h), h, bsz, lq, lk), (o, g[0], g[1]), want)


@pytest.mark.parametrize("bsz,lq,lk", [(2, 40, 70), (2, 130, 400)])
def test_attention_core_wide_unaligned_rows(ops, bsz, lq, lk):
    """head_dim 40 (a multiple of 4, padded to 48) on tensors that start one float past a 16-byte boundary: the
    scalar staging / store path at a width where the row length alone would allow 16-byte accesses."""
    d, h = 80, 2
    q, kv, cot = _case(bsz, lq, lk, d, seed=1)
    want = _reference(q, kv, cot, h)

    def shifted(t):
        flat = torch.zeros(t.numel() + 1, dtype=torch.float32, device="cuda")
        flat[1:] = t.reshape(-1).cuda()
        return flat.requires_grad_(True)
    fq, fkv, fcot = shifted(q), shifted(kv), shifted(cot)
    q_, kv_ = fq[1:].view(q.shape), fkv[1:].view(kv.shape)
    assert q_.data_ptr() % 16 == 4 and kv_.data_ptr() % 16 == 4 and q_.is_contiguous() and kv_.is_contiguous()
    o = ops.AttentionCore.apply(q_, kv_, h)
    g = torch.autograd.grad((o * fcot[1:].view(cot.shape).detach()).sum(), [fq, fkv])
    assert float(g[0][0]) == 0.0 and float(g[1][0]) == 0.0
    _check("unaligned hd=40 shape=%dx%dx%d" % (bsz, lq, lk), (o, g[0][1:].view(q.shape), g[1][1:].view(kv.shape)), want)


def test_both_forms_are_reached_at_every_new_width(ops):
    """Over the parametrisation above, every dispatch width (48, 64, 80, 96 columns) has a case whose backward keeps
    K, V, Q, dO resident and a case that is streamed — the two reported by igcn_attn_core_lds_bytes, the size the
    launches ask for."""
    from igcn_amd import _lib
    lib = _lib.load()
    seen = {}
    for d, h in WIDTHS:
        for _, lq, lk in SHAPES:
            n = int(lib.igcn_attn_core_lds_bytes(d, h, lq, lk, 1))
            assert 0 < n <= 150 * 1024
            seen.setdefault(_hdp(d // h), set()).add("chunked" if n == CHUNKED else "resident")
    assert seen == {w: {"resident", "chunked"} for w in (48, 64, 80, 96)}, seen


def test_attention_core_wide_is_deterministic(ops):
    """head_dim 80, 130 x 400 (streamed both ways): two runs give the same bits — one writer per output element, sums
    in a fixed order."""
    d, h = 160, 2
    q, kv, cot = (t.cuda() for t in _case(2, 130, 400, d, seed=2))
    runs = []
    for _ in range(2):
        q_, kv_ = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        o = ops.AttentionCore.apply(q_, kv_, h)
        lse = o.grad_fn.saved_tensors[3]
        g = torch.autograd.grad((o * cot).sum(), [q_, kv_])
        runs.append((o.detach().clone(), lse.detach().clone(), g[0], g[1]))
    for name, a, b in zip(("o", "lse", "dq", "dkv"), *runs):
        assert torch.equal(a, b), name
    assert runs[0][1].shape == (2, h, 130) and bool(torch.isfinite(runs[0][1]).all())


@pytest.mark.parametrize("bsz,lq,lk", [(2, 40, 70), (2, 130, 400)])
def test_padding_columns_are_inert(ops, bsz, lq, lk):
    """head_dim 40 is staged in 48-column LDS rows.  The ABI takes whole contiguous [.., H * head_dim] rows (no strides),
    so the eight columns behind a head ARE its neighbours': the next head's, or — behind the last head — the next row's
    first head / the value half of the same key.  With every element of the OTHER head (q, k, v and the cotangent) at
    1e30, a head's o, lse, dq, dk, dv equal the clean run bit for bit and stay finite: nothing past head_dim is read into
    a product.  And with H = 1 on buffers that continue past their last row, nothing past head_dim is written."""
    d, h, hd = 80, 2, 40
    q, kv, cot = (t.cuda() for t in _case(bsz, lq, lk, d, seed=3))

    def run(q, kv, cot, h=h):
        q_, kv_ = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        o = ops.AttentionCore.apply(q_, kv_, h)
        lse = o.grad_fn.saved_tensors[3].clone()
        g = torch.autograd.grad((o * cot).sum(), [q_, kv_])
        return o.detach(), lse, g[0], g[1]

    def head(res, i):
        o, lse, dq, dkv = res
        sl = slice(i * hd, (i + 1) * hd)
        return o[..., sl], lse[:, i], dq[..., sl], dkv.view(bsz, lk, 2, d)[..., sl]
    clean = run(q, kv, cot)
    for poisoned in (0, 1):
        sl = slice(poisoned * hd, (poisoned + 1) * hd)
        pq, pkv, pcot = q.clone(), kv.clone(), cot.clone()
        pq[..., sl] = 1e30
        pcot[..., sl] = 1e30
        pkv.view(bsz, lk, 2, d)[..., sl] = 1e30
        got = run(pq, pkv, pcot)
        for name, a, b in zip(("o", "lse", "dq", "dkv"), head(got, 1 - poisoned), head(clean, 1 - poisoned)):
            assert bool(torch.isfinite(a).all()), (poisoned, name)
            assert torch.equal(a, b), (poisoned, name)
    # writes: one head of 40 columns, outputs followed by a sentinel tail that the padded columns of the last row (and
    # every row's, shifted into the next) would land in
    from igcn_amd import _lib
    q1, kv1, cot1 = (t[..., :hd].contiguous() for t in (q, kv.view(bsz, lk, 2, d), cot))
    ref = run(q1, kv1.view(bsz, lk, 2 * hd), cot1, h=1)
    tail, mark = 64, 12345.0
    bufs = {n: torch.full((numel + tail,), mark, dtype=torch.float32, device="cuda")
            for n, numel in (("o", q1.numel()), ("dq", q1.numel()), ("dkv", kv1.numel()))}
    lse = torch.empty(bsz, 1, lq, dtype=torch.float32, device="cuda")
    scratch = torch.empty(int(_lib.load().igcn_attn_core_bwd_scratch_floats(bsz, 1, lq)), dtype=torch.float32, device="cuda")
    ops.call("igcn_attn_core_fwd", bsz, hd, 1, lq, lk, ops.ptr(q1), ops.ptr(kv1), ops.ptr(bufs["o"]), ops.ptr(lse),
             ops.stream_ptr())
    o1 = bufs["o"][:q1.numel()].view(q1.shape)
    ops.call("igcn_attn_core_bwd", bsz, hd, 1, lq, lk, ops.ptr(q1), ops.ptr(kv1), ops.ptr(o1), ops.ptr(lse), ops.ptr(cot1),
             ops.ptr(bufs["dq"]), ops.ptr(bufs["dkv"]), ops.ptr(scratch), ops.stream_ptr())
    torch.cuda.synchronize()
    for n, want in (("o", ref[0]), ("dq", ref[2]), ("dkv", ref[3])):
        assert bool((bufs[n][-tail:] == mark).all()), n + ": written past the last row"
        assert torch.equal(bufs[n][:-tail], want.reshape(-1)), n


@pytest.mark.parametrize("b,lq,lk", [(3, 90, 130), (2, 130, 400)])
@pytest.mark.parametrize("d", [96, 128, 160])
def test_projected_attention_wide_vs_fp64(ops, monkeypatch, d, b, lq, lk):
    """The route SGCN_GCN_IMGSNP._cross_attention takes at these widths: ops.ProjectedAttention (packed in-projection on
    the grouped GEMM — the streaming pair kernels are depth 32 / 48 only — + the attention core as one autograd node), at
    the widths of the hidden-32 sweep (H = 2, head_dim 48 / 64 / 80), the model's 90 queries and a streamed shape: output
    and all four gradients against nn.MultiheadAttention's in-projection + attention in fp64 at the bound of
    test_projected_attention_matches_multihead_attention (1e-4 of each tensor's scale), d b_k exactly zero; and the
    forward launches igcn_attn_core_fwd, the backward igcn_attn_core_bwd."""
    from calltrace import record_calls
    h = 2
    rng = np.random.default_rng(b + lq + lk + d)
    mk = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))     # noqa: E731
    query, memory, w, bias, cot = mk(b, lq, d), mk(b, lk, d), mk(3 * d, d) * 0.3, mk(3 * d), mk(b, lq, d)
    ref = [t.double().requires_grad_(True) for t in (query, memory, w, bias)]
    q = torch.nn.functional.linear(ref[0], ref[2][:d], ref[3][:d]).view(b, lq, h, d // h).transpose(1, 2)
    k = torch.nn.functional.linear(ref[1], ref[2][d:2 * d], ref[3][d:2 * d]).view(b, lk, h, d // h).transpose(1, 2)
    v = torch.nn.functional.linear(ref[1], ref[2][2 * d:], ref[3][2 * d:]).view(b, lk, h, d // h).transpose(1, 2)
    att = torch.softmax(q @ k.transpose(2, 3) / (d // h) ** 0.5, dim=-1)
    o_ref = (att @ v).transpose(1, 2).reshape(b, lq, d)
    g_ref = torch.autograd.grad((o_ref * cot.double()).sum(), ref)
    assert ops.attn_core_supported(d, h, lq, lk)
    dev = [t.cuda().requires_grad_(True) for t in (query, memory, w, bias)]
    seen = record_calls(monkeypatch)
    o = ops.ProjectedAttention.apply(*dev, h)
    fwd_calls = [c[0] for c in seen]
    del seen[:]
    g = torch.autograd.grad((o * cot.cuda()).sum(), dev)
    bwd_calls = [c[0] for c in seen]
    monkeypatch.undo()
    assert "igcn_attn_core_fwd" in fwd_calls and "igcn_proj_fwd_pair" not in fwd_calls, fwd_calls
    assert "igcn_attn_core_bwd" in bwd_calls, bwd_calls
    print("PROJ_WIDE d=%d shape=%dx%dx%d o %.3e " % (d, b, lq, lk, _rel(o, o_ref.detach()))
          + " ".join("%s %.3e" % (nm, _rel(a, c)) for a, c, nm in zip(g, g_ref, ("dquery", "dmemory", "dW", "dbias"))))
    assert_matches(o, o_ref.detach().numpy(), 1e-4, "o")
    for got, want, nm in zip(g, g_ref, ("dquery", "dmemory", "dW", "dbias")):
        assert_matches(got, want.numpy(), 1e-4, nm)
    assert float(g[3][d:2 * d].abs().max()) == 0.0


def test_head_dim_above_96_is_refused(ops, monkeypatch):
    """head_dim 100: not covered, and AttentionCore says so from the library's shape check — the one entry point it
    calls returns the error before any launch."""
    from calltrace import record_calls
    from igcn_amd import _lib
    assert not ops.attn_core_supported(200, 2, 90, 130)
    q = torch.randn(2, 90, 200, device="cuda")
    kv = torch.randn(2, 130, 400, device="cuda")
    seen = record_calls(monkeypatch)
    with pytest.raises(_lib.IgcnError, match="head_dim <= 96"):
        ops.AttentionCore.apply(q, kv, 2)
    assert [c[0] for c in seen] == ["igcn_attn_core_fwd"]
    torch.cuda.synchronize()
