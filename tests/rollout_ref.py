"""fp64 restatement of the attention roll-out through the GO encoder (go_model.py:208-251), in plain torch on sparse
lists, independent of the kernels: what tests/test_gpu_rollout.py compares igcn_go_attn_coeffs, igcn_go_rollout_layer
and the ROI x SNP association with.

Node-major here (relevance [B, N, S], rows = GO nodes) — the library keeps it channel-major [B, S, N].
  1. E[n, s] = sum_c |t_c[k]| at the non-zeros k = (n, s) of the SNP -> GO encoding; R_0 = E with rows scaled to sum 1
  2. x_in = W_inc x, x_s = W_s x; s_e = exp(tanh(a_in[:f].x_in[row_e] + a_in[f:].x_in[col_e]));
     alpha_e = s_e / sum_{e' in row} s_e'; beta_r = sigmoid(a_s.x_s[r])
  3. R_{l+1}[r - pool] = (sum_e alpha_e R_l[col_e] + beta_r R_l[r]) / (sum_e alpha_e + beta_r) for r >= pool
     (an empty list: R_l[r])
  4. assoc = W . R_top
"""
import torch

RTOL, ATOL = 1e-4, 1e-6        # the bound tests/test_gpu_attn_weights.py holds the sibling weights kernel to


def row_of(row_ptr):
    row_ptr = row_ptr.long()
    return torch.repeat_interleave(torch.arange(row_ptr.numel() - 1), row_ptr[1:] - row_ptr[:-1])


def encoding_relevance(rows, cols, ts, n, s=54):
    """R_0 [n, s] from the non-zeros (rows[k], cols[k]) and the per-channel values ts = [t_c [nnz]]."""
    e = torch.zeros(n, s, dtype=torch.float64)
    e[rows.long(), cols.long()] = sum(t.detach().double().cpu().abs() for t in ts)
    tot = e.sum(1, keepdim=True)
    return torch.where(tot > 0, e / tot.clamp(min=1e-300), torch.zeros_like(e))


def layer_coeffs(x, w_inc, w_s, a_in, a_s, row_ptr, col):
    """(alpha [B, nnz], beta [B, N]) of one layer from its input x [B, fin, N] (any float dtype; computed in fp64)."""
    x, w_inc, w_s = x.detach().double().cpu(), w_inc.detach().double().cpu(), w_s.detach().double().cpu()
    a_in, a_s = a_in.detach().double().cpu().reshape(-1), a_s.detach().double().cpu().reshape(-1)
    f = w_inc.shape[0]
    rows, col = row_of(row_ptr.cpu()), col.cpu().long()[:int(row_ptr[-1])]
    x_in = torch.einsum("cd,bdn->bnc", w_inc, x)
    x_s = torch.einsum("cd,bdn->bnc", w_s, x)
    p, q = x_in @ a_in[:f], x_in @ a_in[f:]
    s = torch.exp(torch.tanh(p[:, rows] + q[:, col]))
    z = torch.zeros_like(p).index_add_(1, rows, s)
    return s / z[:, rows], torch.sigmoid(x_s @ a_s)


def rollout_layer(r, alpha, beta, row_ptr, col, pool):
    """R_{l+1} [B, N - pool, S] from R_l [B, N, S] (or [N, S], shared by all samples)."""
    alpha, beta = alpha.detach().double().cpu(), beta.detach().double().cpu()
    b, n = beta.shape
    r = r.detach().double().cpu()
    if r.dim() == 2:
        r = r.expand(b, *r.shape)
    rows, col = row_of(row_ptr.cpu()), col.cpu().long()[:int(row_ptr[-1])]
    num = torch.zeros_like(r).index_add_(1, rows, alpha[:, :, None] * r[:, col])
    den = torch.zeros_like(beta).index_add_(1, rows, alpha)
    out = (num + beta[:, :, None] * r) / (den + beta)[:, :, None]
    empty = (row_ptr[1:] == row_ptr[:-1]).cpu()
    out[:, empty] = r[:, empty]
    return out[:, pool:]


def rollout(r0, layers):
    """R_top and every intermediate: layers = [(alpha, beta, row_ptr, col, pool)]."""
    rs = [r0]
    for alpha, beta, row_ptr, col, pool in layers:
        rs.append(rollout_layer(rs[-1], alpha, beta, row_ptr, col, pool))
    return rs


def association(w, r_top):
    return w.detach().double().cpu() @ r_top.detach().double().cpu()


def err_ratio(got, want):
    """max over elements of |got - want| / (ATOL + RTOL * want): at most 1 inside the bound (``want`` is >= 0)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(((got - want).abs() / (ATOL + RTOL * want.abs())).max()) if want.numel() else 0.0


def assert_close(got, want, what):
    ratio = err_ratio(got, want)
    print(f"{what}: error / bound = {ratio:.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert ratio <= 1.0, f"{what}: error is {ratio:.3f} of the bound {ATOL} + {RTOL} v"
