// The genetics-only trainer's head and loss (kernel/train_eval_snps.py:314-320 on kernel/go_model.py:148-157) as ONE
// launch per direction:
//   x = cat(latent [B, L], snps [B, S])          (two pointers: the concatenation is never materialised, K1 = L + S)
//   a = relu(BatchNorm1d(K1)(x)) * keep1         (batch statistics in training mode, running ones in eval mode)
//   h = relu(a W1^T)          W1 [H, K1]         hk = h * keep2
//   z = hk W2^T + b2          W2 [1, H]          y_hat = sigmoid(z)
//   class = sum BCELoss(y_hat, label)   recon = lambda0 sum (x_hat - snps)^2   loss = class + recon
// BCELoss is torch's on the PROBABILITY: -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)), with the gradient
// (p - y) / max(p (1 - p), 1e-12) times sigmoid's p (1 - p) — not the logits form, from which it differs once fp32 sigmoid
// saturates.  lambda0 == 0 switches the reconstruction term off exactly.
//
// Shape of the launch.  The training-mode batch statistics couple all rows, and so do the loss sums and the parameter
// gradients: both directions are ONE workgroup that loops over passes of SH_ROWS rows (phase 1: column statistics in two
// sweeps, mean first, then centred squares; phase 2: the rows).  Without labels (eval mode, y_hat alone) the rows are
// independent and the grid is one workgroup per pass.  A pass stages a [rows, K1] in LDS; the first layer is computed with
// thread = (row, quad of H), which is the narrow-layer geometry (narrow_head.h) of the last layer K = H = 16, C = 1, whose
// arithmetic is that header's.  Every sum runs in a fixed order: no atomics.
// Supported (igcn_snps_head_supported): H == 16, L, S >= 1, L + S <= SH_MAXK, 1 <= B <= SH_MAXB (training: B >= 2).
#include "narrow_head.h"

#define SH_H 16
#define SH_MAXK 96
#define SH_ROWS 64          /* narrow_head_rows_per_pass(SH_H) */
#define SH_MAXB 1024
#define SH_DW (SH_H * SH_MAXK / 256)      /* dW1 elements per thread */
#define SH_EPT (SH_ROWS * SH_MAXK / 256)  /* elements of a pass per thread */
#define SH_BATCH 32                       /* independent loads a thread keeps in flight */

static_assert(SH_H * SH_MAXK % 256 == 0, "dW1 slots");

struct SnpsHeadFwdArgs {
  int B, L, S, training;
  const float *latent, *snps, *gamma, *beta;
  float *rmean, *rvar;
  float momentum, eps;
  const float *keep1, *keep2, *W1, *W2, *b2, *label, *x_hat;
  float lambda0;
  float *y_hat, *out, *ws;
};

struct SnpsHeadBwdArgs {
  int B, L, S, training;
  const float *latent, *snps, *gamma, *beta, *keep1, *keep2, *W1, *W2, *label, *y_hat, *x_hat;
  float lambda0;
  const float *up, *ws;
  float *dlatent, *dxhat, *dgamma, *dbeta, *dW1, *dW2, *db2;
};

// workspace: mean [K1] | rstd [K1] | (padding to a multiple of four floats) | h [B, H] = relu(a W1^T) before its dropout
__host__ __device__ static inline int sh_hid_offset(int K1) { return (2 * K1 + 3) / 4 * 4; }

// (one load from a selected address, 32-bit element indices: B (L + S) stays far below 2^31 — a branch per element or
// 64-bit index arithmetic made the compiler wait for every other load of a batch)
__device__ __forceinline__ float sh_x(const float* __restrict__ latent, const float* __restrict__ snps, int L, int S,
                                      int r, int k) {
  const float* p = k < L ? latent + (r * L + k) : snps + (r * S + (k - L));
  return *p;
}

// dst[k] = sum over rows r < B of term(r, k), k < K1: thread (g, k) adds rows g, g + G, ... in that order (G = 256 / KP
// row groups, KP = 64 or 128 column slots), then thread k adds the G partials in order.  One workgroup is latency-bound:
// the terms are fetched SH_BATCH at a time (independent loads in flight together; a row past the end counts 0) and then
// added in row order.  red: 256 floats.  Ends with a barrier.
template <class F>
__device__ __forceinline__ void sh_col_sums(int B, int K1, float* red, float* dst, F term) {
  const int KP = K1 <= 64 ? 64 : 128, G = 256 / KP, k = threadIdx.x % KP, g = threadIdx.x / KP;
  float t = 0.f;
  if (k < K1) {
    for (int r = g; r < B; r += SH_BATCH * G) {
      float v[SH_BATCH];
#pragma unroll
      for (int i = 0; i < SH_BATCH; ++i) v[i] = term(min(r + i * G, B - 1), k);      // (unconditional: clamped row)
#pragma unroll
      for (int i = 0; i < SH_BATCH; ++i) t += r + i * G < B ? v[i] : 0.f;
    }
  }
  red[threadIdx.x] = t;
  __syncthreads();
  if ((int)threadIdx.x < K1) {
    float s = red[threadIdx.x];
    for (int j = 1; j < G; ++j) s += red[j * KP + threadIdx.x];
    dst[threadIdx.x] = s;
  }
  __syncthreads();
}

// sum over i < n of term(i), this thread's share (i = tid, tid + 256, ...), fetched SH_BATCH at a time
template <class F>
__device__ __forceinline__ float sh_strided_sum(int n, F term) {
  float t = 0.f;
  for (int base = threadIdx.x; base < n; base += 256 * SH_BATCH) {
    float v[SH_BATCH];
#pragma unroll
    for (int i = 0; i < SH_BATCH; ++i) v[i] = term(min(base + 256 * i, n - 1));
#pragma unroll
    for (int i = 0; i < SH_BATCH; ++i) t += base + 256 * i < n ? v[i] : 0.f;
  }
  return t;
}

// a [nr, K1] of the pass that starts at row r0, into LDS (row stride K1), element e = tid + 256 i by this thread: every
// load of the pass is issued before the first use.  kv: the elements' dropout factors (ones without keep1), left to the
// caller; s_xn (or NULL): the normalised inputs (x - mean) rstd as well.  No barrier.
__device__ __forceinline__ void sh_stage(const float* __restrict__ latent, const float* __restrict__ snps,
                                         const float* __restrict__ keep1, int L, int S, int r0, int nr,
                                         const float* s_mean, const float* s_rstd, const float* s_g, const float* s_b,
                                         float* s_a, float* s_xn, float (&kv)[SH_EPT]) {
  const int K1 = L + S, n = nr * K1;
  // (row, column) of element e = tid + 256 i without a division per element: one for the first, then steps of 256
  const int step_r = 256 / K1, step_k = 256 - step_r * K1, rl0 = (int)threadIdx.x / K1, k0 = (int)threadIdx.x - rl0 * K1;
  float xv[SH_EPT];
  int rl = rl0, k = k0;
#pragma unroll
  for (int i = 0; i < SH_EPT; ++i) {      // (unconditional loads; an element past the end reads the pass's last row)
    const int rc = min(rl, nr - 1);
    xv[i] = sh_x(latent, snps, L, S, r0 + rc, k);
    kv[i] = keep1 ? keep1[(r0 + rc) * K1 + k] : 1.f;
    rl += step_r;
    k += step_k;
    if (k >= K1) { k -= K1; ++rl; }
  }
  k = k0;
#pragma unroll
  for (int i = 0; i < SH_EPT; ++i) {
    const int e = threadIdx.x + 256 * i;
    if (e < n) {
      const float xn = (xv[i] - s_mean[k]) * s_rstd[k];
      s_a[e] = fmaxf(xn * s_g[k] + s_b[k], 0.f) * kv[i];
      if (s_xn) s_xn[e] = xn;
    }
    k += step_k;
    if (k >= K1) k -= K1;
  }
}

__global__ void __launch_bounds__(256) k_snps_head_fwd(const SnpsHeadFwdArgs a) {
  __shared__ float red[NH_RED_FLOATS];
  __shared__ float s_a[SH_ROWS * SH_MAXK];
  __shared__ __attribute__((aligned(16))) float s_w1[SH_MAXK * SH_H];      // transposed: [k][j]
  __shared__ float s_mean[SH_MAXK], s_rstd[SH_MAXK], s_g[SH_MAXK], s_b[SH_MAXK];
  __shared__ float s_fin[2];
  const int B = a.B, L = a.L, S = a.S, K1 = L + S, tid = threadIdx.x;
  float* hid = a.ws ? a.ws + sh_hid_offset(K1) : nullptr;
  for (int i = tid; i < SH_H * K1; i += 256) {
    const int j = i / K1, k = i - j * K1;
    s_w1[k * SH_H + j] = a.W1[i];
  }
  if (tid < K1) {
    s_g[tid] = a.gamma[tid];
    s_b[tid] = a.beta[tid];
  }
  if (a.training) {
    // phase 1: the batch statistics, mean first, then the variance from centred values
    sh_col_sums(B, K1, red, s_mean, [&](int r, int k) { return sh_x(a.latent, a.snps, L, S, r, k); });
    if (tid < K1) s_mean[tid] = s_mean[tid] / (float)B;
    __syncthreads();
    sh_col_sums(B, K1, red, s_rstd, [&](int r, int k) {
      const float d = sh_x(a.latent, a.snps, L, S, r, k) - s_mean[k];
      return d * d;
    });
    if (tid < K1) {
      const float var = s_rstd[tid] / (float)B;
      s_rstd[tid] = 1.f / sqrtf(var + a.eps);
      a.rmean[tid] = (1.f - a.momentum) * a.rmean[tid] + a.momentum * s_mean[tid];
      a.rvar[tid] = (1.f - a.momentum) * a.rvar[tid] + a.momentum * (var * ((float)B / (float)(B - 1)));
    }
  } else if (tid < K1) {
    s_mean[tid] = a.rmean[tid];
    s_rstd[tid] = 1.f / sqrtf(a.rvar[tid] + a.eps);
  }
  __syncthreads();
  if (a.ws && blockIdx.x == 0 && tid < K1) {
    a.ws[tid] = s_mean[tid];
    a.ws[K1 + tid] = s_rstd[tid];
  }
  // phase 2: the rows
  const int q = tid % (SH_H / 4);
  float4 w2[NH_MAXC];
  nh_load_w(a.W2, SH_H, q, 1, w2);
  float sums[2] = {0.f, 0.f};      // BCE, sum (x_hat - snps)^2
  const unsigned npass = (unsigned)((B + SH_ROWS - 1) / SH_ROWS);
  for (unsigned pass = blockIdx.x; pass < npass; pass += gridDim.x) {
    const int r0 = (int)pass * SH_ROWS, nr = min(SH_ROWS, B - r0);
    const NhGeom g = nh_geom(SH_H, pass);
    float4 k2 = make_float4(1.f, 1.f, 1.f, 1.f);
    float y = 0.f;
    if (g.row < B) {      // (the row's own loads: in flight with the tile's)
      if (a.keep2) k2 = *reinterpret_cast<const float4*>(a.keep2 + (int)g.row * SH_H + 4 * q);
      if (a.label) y = a.label[g.row];
    }
    float kv[SH_EPT];
    sh_stage(a.latent, a.snps, a.keep1, L, S, r0, nr, s_mean, s_rstd, s_g, s_b, s_a, nullptr, kv);
    __syncthreads();
    if (g.row < B) {
      const float* ar = s_a + g.rl * K1;
      float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
      for (int k = 0; k < K1; ++k) {      // (one wave per SIMD: unrolled, so that the LDS reads of several steps are in flight)
        const float av = ar[k];
        const float4 w = *reinterpret_cast<const float4*>(&s_w1[k * SH_H + 4 * q]);
        hv.x = fmaf(av, w.x, hv.x); hv.y = fmaf(av, w.y, hv.y); hv.z = fmaf(av, w.z, hv.z); hv.w = fmaf(av, w.w, hv.w);
      }
      hv.x = fmaxf(hv.x, 0.f); hv.y = fmaxf(hv.y, 0.f); hv.z = fmaxf(hv.z, 0.f); hv.w = fmaxf(hv.w, 0.f);
      if (hid) *reinterpret_cast<float4*>(hid + g.row * SH_H + 4 * q) = hv;
      nh_keep(hv, k2);
      float s[NH_MAXC];
      nh_scores<false, false>(hv, w2, a.b2, 1, g.kq, s);
      const float p = 1.f / (1.f + expf(-s[0]));
      if (q == 0) {
        a.y_hat[g.row] = p;
        if (a.label) sums[0] -= y * fmaxf(logf(p), -100.f) + (1.f - y) * fmaxf(log1pf(-p), -100.f);
      }
    }
    __syncthreads();
  }
  if (!a.label) return;      // (y_hat alone: a grid over the passes; with labels the grid is one workgroup)
  if (a.lambda0 != 0.f)
    sums[1] = sh_strided_sum(B * S, [&](int i) {
      const float d = a.x_hat[i] - a.snps[i];
      return d * d;
    });
  nh_block_sums<2>(sums, red, s_fin, 0);
  if (tid == 0) {
    const float cls = s_fin[0], rec = a.lambda0 != 0.f ? a.lambda0 * s_fin[1] : 0.f;
    a.out[0] = cls + rec;
    a.out[1] = cls;
    a.out[2] = rec;
  }
}

__global__ void __launch_bounds__(256) k_snps_head_bwd(const SnpsHeadBwdArgs a) {
  __shared__ float s_a[SH_ROWS * SH_MAXK];      // a of the pass, then d loss / d (BatchNorm output) of the pass
  __shared__ float s_xn[SH_ROWS * SH_MAXK];     // (x - mean) rstd of the pass
  __shared__ float s_w1[SH_H * SH_MAXK];        // [j][k]
  __shared__ __attribute__((aligned(16))) float s_dp[SH_ROWS * SH_H];      // d loss / d (a W1^T) of the pass
  __shared__ float s_mean[SH_MAXK], s_rstd[SH_MAXK], s_g[SH_MAXK], s_b[SH_MAXK];
  __shared__ float s_tail[SH_H + 1];
  static_assert(SH_ROWS * SH_MAXK >= NH_RED_FLOATS, "the reductions behind the passes reuse the tile");
  float* red = s_a;                             // (free once the passes are done)
  const int B = a.B, L = a.L, S = a.S, K1 = L + S, tid = threadIdx.x;
  const float* hid = a.ws + sh_hid_offset(K1);
  const float up = a.up ? a.up[0] : 1.f;
  for (int i = tid; i < SH_H * K1; i += 256) s_w1[i] = a.W1[i];
  if (tid < K1) {
    s_mean[tid] = a.ws[tid];
    s_rstd[tid] = a.ws[K1 + tid];
    s_g[tid] = a.gamma[tid];
    s_b[tid] = a.beta[tid];
  }
  __syncthreads();
  const int KP = K1 <= 64 ? 64 : 128, G = 256 / KP, ck = tid % KP, cg = tid / KP;
  const NhGeom g0 = nh_geom(SH_H, 0);
  const int q = g0.q;
  float4 w2[NH_MAXC], gwa[NH_MAXC];
  float gba[NH_MAXC];
  nh_load_w(a.W2, SH_H, q, 1, w2);
  nh_zero(gwa, gba);
  float dw[SH_DW];
  int wj[SH_DW], wk[SH_DW];                     // this thread's elements (j, k) of dW1: i = tid + 256 s
#pragma unroll
  for (int s = 0; s < SH_DW; ++s) {
    const int i = tid + 256 * s < SH_H * K1 ? tid + 256 * s : 0;
    dw[s] = 0.f;
    wj[s] = i / K1;
    wk[s] = i - wj[s] * K1;
  }
  float dbeta = 0.f, dgamma = 0.f;
  const int npass = (B + SH_ROWS - 1) / SH_ROWS;
  for (int pass = 0; pass < npass; ++pass) {
    const int r0 = pass * SH_ROWS, nr = min(SH_ROWS, B - r0);
    // the row's own loads first: in flight with the tile's
    const int64_t row = r0 + g0.rl;
    float4 hv = make_float4(0.f, 0.f, 0.f, 0.f), k2 = make_float4(1.f, 1.f, 1.f, 1.f);
    float p = 0.5f, y = 0.5f;
    if (row < B) {
      hv = *reinterpret_cast<const float4*>(hid + row * SH_H + 4 * q);
      if (a.keep2) k2 = *reinterpret_cast<const float4*>(a.keep2 + row * SH_H + 4 * q);
      p = a.y_hat[row];
      y = a.label[row];
    }
    float kv[SH_EPT];      // the tile's dropout factors stay in registers: the dy step below maps elements the same way
    sh_stage(a.latent, a.snps, a.keep1, L, S, r0, nr, s_mean, s_rstd, s_g, s_b, s_a, s_xn, kv);
    // the last layer and the sigmoid + BCE, backwards: the row's d loss / d z, its share of dW2 | db2, d loss / d h
    if (row < B) {
      float4 hk = hv;
      nh_keep(hk, k2);
      const float pq = p * (1.f - p);
      const float d[NH_MAXC] = {(p - y) / fmaxf(pq, 1e-12f) * pq * up, 0.f, 0.f, 0.f};
      float4 dh, gw[NH_MAXC];
      float gb[NH_MAXC];
      nh_back(d, w2, hk, k2, reinterpret_cast<float*>(&dh), gw, gb);
      gwa[0].x += gw[0].x; gwa[0].y += gw[0].y; gwa[0].z += gw[0].z; gwa[0].w += gw[0].w;
      gba[0] += gb[0];
      *reinterpret_cast<float4*>(&s_dp[g0.rl * SH_H + 4 * q]) =
          make_float4(hv.x > 0.f ? dh.x : 0.f, hv.y > 0.f ? dh.y : 0.f, hv.z > 0.f ? dh.z : 0.f, hv.w > 0.f ? dh.w : 0.f);
    }
    __syncthreads();
    // dW1[j][k] += sum over the pass's rows, in order, of dpre[r][j] a[r][k]: this thread's SH_DW elements side by side
    // (independent LDS reads in flight together; a slot past the end reads element 0 and is never stored)
#pragma unroll 4
    for (int rl = 0; rl < nr; ++rl) {
#pragma unroll
      for (int s = 0; s < SH_DW; ++s) dw[s] = fmaf(s_dp[rl * SH_H + wj[s]], s_a[rl * K1 + wk[s]], dw[s]);
    }
    __syncthreads();
    // d loss / d (BatchNorm output) in place of a: through W1, the dropout and the ReLU (a > 0 iff both let it through)
    {
      const int step_r = 256 / K1, step_k = 256 - step_r * K1;
      int rl = tid / K1, k = tid - rl * K1;
#pragma unroll
      for (int i = 0; i < SH_EPT; ++i) {
        const int e = tid + 256 * i;
        if (e < nr * K1) {
          float da = 0.f;
#pragma unroll
          for (int j = 0; j < SH_H; ++j) da = fmaf(s_dp[rl * SH_H + j], s_w1[j * K1 + k], da);
          s_a[e] = s_a[e] > 0.f ? da * kv[i] : 0.f;
        }
        rl += step_r;
        k += step_k;
        if (k >= K1) { k -= K1; ++rl; }
      }
    }
    __syncthreads();
    // the columns' sums for dbeta | dgamma; the latent columns' dy is parked in dlatent for the last sweep
    if (ck < K1)
#pragma unroll 8
      for (int rl = cg; rl < nr; rl += G) {
        const float dy = s_a[rl * K1 + ck];
        dbeta += dy;
        dgamma = fmaf(dy, s_xn[rl * K1 + ck], dgamma);
        if (ck < L) a.dlatent[(r0 + rl) * L + ck] = dy;
      }
    __syncthreads();
  }
  red[tid] = dbeta;
  red[256 + tid] = dgamma;
  __syncthreads();
  if (tid < K1) {
    float sb = red[tid], sg = red[256 + tid];
    for (int j = 1; j < G; ++j) {
      sb += red[j * KP + tid];
      sg += red[256 + j * KP + tid];
    }
    a.dbeta[tid] = sb;
    a.dgamma[tid] = sg;
    s_b[tid] = sb;                                        // (beta is not needed any more)
    s_mean[tid] = sg;                                     // (nor is the mean in LDS: the last sweep reads it from ws)
  }
#pragma unroll
  for (int s = 0; s < SH_DW; ++s) {
    const int i = tid + 256 * s;
    if (i < SH_H * K1) a.dW1[i] = dw[s];
  }
  __syncthreads();
  nh_wpart(g0, 1, SH_H, gwa, gba, red, s_tail);
  if (tid < SH_H) a.dW2[tid] = s_tail[tid];
  if (tid == SH_H) a.db2[0] = s_tail[SH_H];
  // BatchNorm backwards for the latent columns (the SNP columns are data); loads SH_BATCH at a time
  const float inv_b = 1.f / (float)B;
  for (int base = tid; base < B * L; base += 256 * SH_BATCH) {
    float dy[SH_BATCH], xl[SH_BATCH];
#pragma unroll
    for (int i = 0; i < SH_BATCH; ++i) {
      const int e = min(base + 256 * i, B * L - 1);
      dy[i] = a.dlatent[e];
      xl[i] = a.latent[e];
    }
#pragma unroll
    for (int i = 0; i < SH_BATCH; ++i) {
      const int e = base + 256 * i;
      if (e < B * L) {
        const int k = e % L;
        float dx = dy[i];
        if (a.training) dx = dy[i] - s_b[k] * inv_b - (xl[i] - a.ws[k]) * s_rstd[k] * (s_mean[k] * inv_b);
        a.dlatent[e] = s_g[k] * s_rstd[k] * dx;
      }
    }
  }
  for (int base = tid; base < B * S; base += 256 * SH_BATCH) {
    float d[SH_BATCH];
#pragma unroll
    for (int i = 0; i < SH_BATCH; ++i) {
      const int e = min(base + 256 * i, B * S - 1);
      d[i] = a.x_hat[e] - a.snps[e];
    }
#pragma unroll
    for (int i = 0; i < SH_BATCH; ++i) {
      const int e = base + 256 * i;
      if (e < B * S) a.dxhat[e] = a.lambda0 != 0.f ? 2.f * a.lambda0 * d[i] * up : 0.f;
    }
  }
}

extern "C" int igcn_snps_head_supported(int B, int L, int S, int H) {
  return H == SH_H && narrow_head_ok(H, 1) && L >= 1 && S >= 1 && L + S <= SH_MAXK && B >= 1 && B <= SH_MAXB;
}
extern "C" size_t igcn_snps_head_workspace_bytes(int B, int L, int S, int H) {
  if (B < 1 || L < 1 || S < 1 || H < 1) return 0;
  return ((size_t)sh_hid_offset(L + S) + (size_t)B * H) * sizeof(float);
}

static int snps_head_refuse(const char* nm, int B, int L, int S, int H) {
  igcn_set_error("%s: needs H == %d, L, S >= 1, L + S <= %d and 1 <= B <= %d (B=%d L=%d S=%d H=%d)", nm, SH_H, SH_MAXK,
                 SH_MAXB, B, L, S, H);
  return IGCN_ERR_UNSUPPORTED;
}

// latent [B, L], snps [B, S]; bn_weight / bn_bias / running_mean / running_var [L + S]; keep1 [B, L + S], keep2 [B, H]
// ({0, 1/(1-p)} factors or NULL; training mode only); W1 [H, L + S], W2 [1, H], b2 [1]; label [B] floats in [0, 1]; x_hat
// [B, S].  Outputs: y_hat [B], out [3] = {loss, class, recon}, ws [igcn_snps_head_workspace_bytes] for the backward, and in
// training mode the running statistics (momentum m: (1 - m) running + m batch, the variance unbiased).
// label == NULL (eval mode only): y_hat alone, any B >= 1, a grid over the rows; x_hat, out and ws may be NULL.
extern "C" int igcn_snps_head_loss_fwd(int B, int L, int S, int H, const float* latent, const float* snps,
                                       const float* bn_weight, const float* bn_bias, float* running_mean,
                                       float* running_var, float momentum, float eps, int training, const float* keep1,
                                       const float* keep2, const float* W1, const float* W2, const float* b2,
                                       const float* label, const float* x_hat, float lambda0, float* y_hat, float* out,
                                       void* ws, void* stream) {
  const bool infer = label == nullptr;
  if (!igcn_snps_head_supported(infer && B > SH_MAXB ? SH_MAXB : B, L, S, H))
    return snps_head_refuse("snps_head_loss_fwd", B, L, S, H);
  IGCN_REQUIRE(!training || B >= 2, "snps_head_loss_fwd: training mode needs more than one row (B=%d)", B);
  IGCN_REQUIRE(!infer || !training, "snps_head_loss_fwd: training mode needs labels");
  IGCN_REQUIRE(B <= (1 << 24), "snps_head_loss_fwd: at most 2^24 rows per call (B=%d)", B);
  IGCN_REQUIRE(training || (!keep1 && !keep2), "snps_head_loss_fwd: eval mode takes no dropout factors");
  IGCN_REQUIRE(latent && snps && bn_weight && bn_bias && running_mean && running_var && W1 && W2 && b2 && y_hat &&
                   (infer || (x_hat && out && ws)),
               "snps_head_loss_fwd: null argument");
  IGCN_REQUIRE((((uintptr_t)keep2 | (uintptr_t)W2 | (uintptr_t)ws) & 15) == 0,
               "snps_head_loss_fwd: keep2, W2 and the workspace must be 16-byte aligned");
  const SnpsHeadFwdArgs a = {B, L, S, training != 0, latent, snps, bn_weight, bn_bias, running_mean, running_var, momentum,
                             eps, keep1, keep2, W1, W2, b2, label, x_hat, lambda0, y_hat, out, (float*)ws};
  const unsigned blocks = infer ? (unsigned)igcn_cdiv(B, SH_ROWS) : 1u;
  hipLaunchKernelGGL(k_snps_head_fwd, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  IGCN_CHECK_LAUNCH("snps_head_loss_fwd");
  return IGCN_OK;
}

// The backward of igcn_snps_head_loss_fwd (same inputs, its y_hat and ws) for the upstream gradient upstream[0] (DEVICE
// scalar; NULL: one).  Writes dlatent [B, L], dx_hat [B, S] = 2 lambda0 (x_hat - snps) upstream, dgamma / dbeta [L + S],
// dW1 [H, L + S], dW2 [H], db2 [1]; the SNP columns are data and get no gradient.
extern "C" int igcn_snps_head_loss_bwd(int B, int L, int S, int H, int training, const float* latent, const float* snps,
                                       const float* bn_weight, const float* bn_bias, const float* keep1,
                                       const float* keep2, const float* W1, const float* W2, const float* label,
                                       const float* y_hat, const float* x_hat, float lambda0, const float* upstream,
                                       const void* ws, float* dlatent, float* dx_hat, float* dgamma, float* dbeta,
                                       float* dW1, float* dW2, float* db2, void* stream) {
  if (!igcn_snps_head_supported(B, L, S, H)) return snps_head_refuse("snps_head_loss_bwd", B, L, S, H);
  IGCN_REQUIRE(!training || B >= 2, "snps_head_loss_bwd: training mode needs more than one row (B=%d)", B);
  IGCN_REQUIRE(training || (!keep1 && !keep2), "snps_head_loss_bwd: eval mode takes no dropout factors");
  IGCN_REQUIRE(latent && snps && bn_weight && bn_bias && W1 && W2 && label && y_hat && x_hat && ws && dlatent && dx_hat &&
                   dgamma && dbeta && dW1 && dW2 && db2,
               "snps_head_loss_bwd: null argument");
  IGCN_REQUIRE((((uintptr_t)keep2 | (uintptr_t)W2 | (uintptr_t)ws) & 15) == 0,
               "snps_head_loss_bwd: keep2, W2 and the workspace must be 16-byte aligned");
  const SnpsHeadBwdArgs a = {B, L, S, training != 0, latent, snps, bn_weight, bn_bias, keep1, keep2, W1, W2, label, y_hat,
                             x_hat, lambda0, upstream, (const float*)ws, dlatent, dx_hat, dgamma, dbeta, dW1, dW2, db2};
  hipLaunchKernelGGL(k_snps_head_bwd, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  IGCN_CHECK_LAUNCH("snps_head_loss_bwd");
  return IGCN_OK;
}
