"""The gene read-out whose launches carry the latent MLP (igcn_gene_tail_*): ``ops.GeneTail``.

Between the paired read-outs and the heads a step runs two independent chains: decoder -> gene read-out -> map, and
the latent MLP (Linear -> BatchNorm1d -> ReLU, twice).  The MLP's BatchNorm stages are 32-workgroup launches that cost
a dependent launch each; here they run in the first workgroups of the gene read-out's chip-wide launches.  Same kernel
bodies and operands as ``ops.NodeLinearBN`` (with its map rider), ``ops.LinearBN1d`` / ``ops.linear`` +
``ops.BatchNorm1dGrouped``: the same bits.
"""
import ctypes
import struct

import torch

from . import _lib, ops, switches
from ._lib import call, ptr, stream_ptr
from .gdc import _empty as _buffer

_REC = 40                                            # int64 words per record of the entry points' table


def _f64_word(v):
    return struct.unpack("<q", struct.pack("<d", float(v)))[0]


def _bn(kind, b, c, groups, relu, n_slabs=0, momentum=0.0, eps=0.0, x=None, gamma=None, beta=None, keep=None, dy=None,
        running_mean=None, running_var=None, y=None, mean=None, rstd=None, x_out=None, dgamma=None, dbeta=None):
    """A BatchNorm1d stage as a table record (include/igcn.h, igcn_gene_tail_fwd): kind 1 = igcn_bn1d_fwd,
    2 = igcn_bn1d_fwd_slabs, 3 = igcn_bn1d_bwd."""
    tens = (x, gamma, beta, keep, dy, running_mean, running_var, y, mean, rstd, x_out, dgamma, dbeta)
    return [kind, b, c, groups, int(relu), n_slabs, _f64_word(momentum), _f64_word(eps)] + [ptr(t) or 0 for t in tens]


def _product(form, a, b, out=None, final=False):
    """One fp32 product as igcn_gemm_f32_grouped's 16-word record (``ops.gemm_group``'s): "nt" a [M,K] b [N,K],
    "nn" a [M,K] b [K,N], "tn" a [K,M] b [K,N].  Returns (words, out, tensors the record points at)."""
    if form == "nt":
        (m, k), n = a.shape, b.shape[0]
        st = (k, 1, k, 1)
    elif form == "nn":
        (m, k), n = a.shape, b.shape[1]
        st = (k, 1, 1, n)
    else:
        (k, m), n = a.shape, b.shape[1]
        st = (1, m, 1, n)
    if out is None:
        out = _buffer((m, n), torch.float32, a.device)
    sk = ops._split_k(m, n, k)
    scratch = _buffer((sk * m * n,), torch.float32, a.device) if sk > 1 else None
    if final:
        ops._keep(scratch)
    words = [m, n, k, ptr(a), st[0], st[1], ptr(b), st[2], st[3], 0, ptr(out), n, 0x100 if final else 0, sk,
             ptr(scratch) or 0, 0]
    return words, out, (a, b, out, scratch)


def _table(*records):
    table = (ctypes.c_int64 * (_REC * len(records)))()
    for i, rec in enumerate(records):
        table[_REC * i:_REC * i + len(rec)] = rec
    return table


class GeneTail(torch.autograd.Function):
    """The gene read-out with its map rider (``ops.NodeLinearBN`` with ``rider``) and the two Linear -> BatchNorm1d ->
    ReLU stages of the latent MLP (``ops.LinearBN1d``, or ``ops.linear`` + ``ops.BatchNorm1dGrouped``, each) as ONE op:
    the read-out's launches carry the BatchNorm stages in their first workgroups (igcn_gene_tail_fwd / _bwd), four
    launches fewer per step.  Returns (out [B,N,1], latent); the map's output is left in ``out._igcn_map_y`` as
    NodeLinearBN leaves it.  Only for ``gene_tail_supported`` arguments."""

    @staticmethod
    def forward(ctx, x, inp, w_ro, g_ro, b_ro, rm_ro, rv_ro, mom_ro, eps_ro, keep_ro, csr, val,
                w1, g1, b1, rm1, rv1, mom1, eps1, keep1, w2, g2, b2, rm2, rv2, mom2, eps2, training, groups):
        f32 = ops._f32
        x, inp, w_ro, g_ro, b_ro, w1, g1, b1, w2, g2, b2 = (f32(t) for t in (x, inp, w_ro, g_ro, b_ro, w1, g1, b1, w2, g2,
                                                                            b2))
        keep_ro = f32(keep_ro) if keep_ro is not None else None
        keep1 = f32(keep1) if keep1 is not None else None
        b, f, n = x.shape
        bl, k1 = inp.shape
        c1, c2 = w1.shape[0], w2.shape[0]
        lib = _lib.load()
        e = lambda *shape: _buffer(shape, torch.float32, x.device)          # noqa: E731
        # product 1: its split-K slabs left un-summed (LinearBN1d.forward), or whole where that op does not apply (Linear)
        xl, h, mean1, rstd1 = e(bl, c1), e(bl, c1), e(groups, c1), e(groups, c1)
        slabs, eff = None, 1
        if ops.linear_bn1d_supported(inp, w1, groups):
            sk = ops._split_k(bl, c1, k1)
            slabs = e(sk * bl * c1)
            call("igcn_gemm_f32", bl, c1, k1, ptr(inp), k1, 1, ptr(w1), k1, 1, None, ptr(xl), c1, 0x200, sk, ptr(slabs),
                 stream_ptr())
            eff = int(lib.igcn_gemm_effective_split(k1, sk))
        else:
            ops.gemm_nt(inp, w1, out=xl)
        bn1 = _bn(2 if eff > 1 else 1, bl, c1, groups, 1, eff if eff > 1 else 0, mom1, eps1,
                  x=slabs if eff > 1 else xl, gamma=g1, beta=b1, keep=keep1, running_mean=rm1, running_var=rv1, y=h,
                  mean=mean1, rstd=rstd1, x_out=xl if eff > 1 else None)
        # product 2 (ops.linear: the narrow-output kernel or the unsplit GEMM) and its BatchNorm (BatchNorm1dGrouped)
        l2, latent, mean2, rstd2 = e(bl, c2), e(bl, c2), e(groups, c2), e(groups, c2)
        ctx.small2 = ops._small_linear_ok(h, w2, False)
        prod2 = [3, bl, c1, c2, ptr(h), 0, ptr(w2), 0, ptr(l2)] if ctx.small2 else [1] + _product("nt", h, w2, l2)[0]
        bn2 = _bn(1, bl, c2, groups, 1, 0, mom2, eps2, x=l2, gamma=g2, beta=b2, running_mean=rm2, running_var=rv2,
                  y=latent, mean=mean2, rstd=rstd2)
        # the read-out and its map (NodeLinearBN.forward with a rider)
        out, mean, rstd = e(b, n, 1), e(groups, n), e(groups, n)
        scratch = e(int(lib.igcn_node_linear_bn_scratch_floats(b, n, groups)))
        y = e(b, 1, csr.n_rows)
        table = _table(bn1, prod2, bn2)
        call("igcn_gene_tail_fwd", b, f, n, groups, ptr(x), ptr(w_ro), ptr(g_ro), ptr(b_ro), ptr(rm_ro), ptr(rv_ro),
             int(training), float(mom_ro), float(eps_ro), ptr(keep_ro), ptr(out), ptr(mean), ptr(rstd), ptr(scratch),
             csr.n_rows, csr.nnz, ptr(csr.row_ptr), ptr(csr.col), ptr(f32(val)), csr.nnz, ptr(y),
             ctypes.addressof(table), stream_ptr())
        out._igcn_map_y = y
        ctx.save_for_backward(x, w_ro, g_ro, b_ro, mean, rstd, keep_ro, inp, w1, xl, g1, b1, mean1, rstd1, keep1,
                              h, w2, l2, g2, b2, mean2, rstd2)
        ctx.training, ctx.groups = int(training), groups
        return out, latent

    @staticmethod
    def backward(ctx, dout, dlatent):
        (x, w_ro, g_ro, b_ro, mean, rstd, keep_ro, inp, w1, xl, g1, b1, mean1, rstd1, keep1,
         h, w2, l2, g2, b2, mean2, rstd2) = ctx.saved_tensors
        training, groups = ctx.training, ctx.groups
        dout, dlatent = ops._f32(dout), ops._f32(dlatent)
        b, f, n = x.shape
        bl, c1 = xl.shape
        c2 = l2.shape[1]
        lib = _lib.load()
        e = lambda *shape: _buffer(shape, torch.float32, x.device)          # noqa: E731
        # layer 2: BatchNorm1dGrouped.backward, then SmallLinear.backward or Linear.backward (dX | dW in one launch)
        dl2, dg2, db2 = e(bl, c2), e(c2), e(c2)
        bn2 = _bn(3, bl, c2, groups, 1, x=l2, gamma=g2, beta=b2, dy=dlatent, y=dl2, mean=mean2, rstd=rstd2, dgamma=dg2,
                  dbeta=db2)
        if ctx.small2:
            dh, dwb = e(bl, c1), e(c2 * c1 + c2)
            hold = ops._keep(e(int(lib.igcn_small_linear_bwd_scratch_floats(bl, c1, c2))))
            prod2 = [4, bl, c1, c2, ptr(h), 0, ptr(w2), ptr(dl2), ptr(dh), ptr(dwb), ptr(hold)]
            dw2 = dwb[:c2 * c1].view(c2, c1)
        else:
            (wx, dh, hx), (ww, dw2, hw) = _product("nn", dl2, w2), _product("tn", dl2, h, final=True)
            prod2, hold = [2, 2] + wx + ww, (hx, hw)
        # layer 1: LinearBN1d.backward
        dxl, dg1, db1 = e(bl, c1), e(c1), e(c1)
        bn1 = _bn(3, bl, c1, groups, 1, x=xl, gamma=g1, beta=b1, keep=keep1, dy=dh, y=dxl, mean=mean1, rstd=rstd1,
                  dgamma=dg1, dbeta=db1)
        (wx, dinp, hx), (ww, dw1, hw) = _product("nn", dxl, w1), _product("tn", dxl, inp, final=True)
        prod1, hold = [2, 2] + wx + ww, (hold, hx, hw)
        # the read-out: NodeLinearBN.backward
        dx, dw, dgb = e(b, f, n), e(*w_ro.shape), e(2, n)
        scratch = ops._keep(e(int(lib.igcn_node_linear_bn_bwd_scratch_floats(b, f, n, 1, groups))))
        table = _table(bn2, prod2, bn1, prod1)
        call("igcn_gene_tail_bwd", b, f, n, groups, training, ptr(x), ptr(w_ro), ptr(g_ro), ptr(b_ro), ptr(mean), ptr(rstd),
             ptr(dout), ptr(keep_ro), ptr(dx), ptr(dw), ptr(dgb), ptr(scratch), ctypes.addressof(table), stream_ptr())
        del hold
        return (dx, dinp, dw, dgb[0], dgb[1], None, None, None, None, None, None, None,
                dw1, dg1, db1, None, None, None, None, None, dw2, dg2, db2, None, None, None, None, None, None)


def gene_tail_supported(x, inp, w_ro, bn_ro, csr, val, lin1, bn1, lin2, bn2, groups):
    """``GeneTail`` computes what the separate ops compute, kernel for kernel: the read-out takes its map as a rider, the
    first latent layer is a ``LinearBN1d`` or a GEMM ``Linear`` and the second an unsplit product (``SmallLinear`` or
    ``Linear``), the BatchNorm stages fit the register kernels, the backward's products come in grouped launches and
    every gradient is wanted (so every parameter-gradient sum is final: ``ops._leaves``)."""
    if not (torch.is_grad_enabled() and x.is_cuda and x.requires_grad and inp.requires_grad and inp.dim() == 2
            and inp.dtype == torch.float32 and inp.is_contiguous() and lin1.bias is None and lin2.bias is None
            and not switches.on("IGCN_NO_GEMM_GROUPS")):
        return False
    params = (w_ro, bn_ro.weight, bn_ro.bias, lin1.weight, bn1.weight, bn1.bias, lin2.weight, bn2.weight, bn2.bias)
    if not (ops._leaves(*params) and all(p is not None and p.is_contiguous() and p.dtype == torch.float32 for p in params)):
        return False
    if any(bn.running_mean is None or bn.running_var is None or bn.momentum is None for bn in (bn_ro, bn1, bn2)):
        return False
    if not ops.node_linear_bn_map_supported(x, w_ro, csr, val) or ops._small_linear_ok(inp, lin1.weight, False):
        return False
    c1 = lin1.weight.shape[0]
    if lin2.weight.shape[1] != c1 or ops._split_k(inp.shape[0], lin2.weight.shape[0], c1) > 1:
        return False
    return bool(_lib.load().igcn_gene_tail_supported(int(x.shape[1]), int(w_ro.shape[0]), int(x.shape[2]), csr.n_rows,
                                                     csr.nnz, int(inp.shape[0]), groups))
