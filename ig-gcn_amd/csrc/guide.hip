// GUIDE_IMGSNP (kernel/guide_img_snp.py + kernel/guide_go_model.py): the BatchNorm + PReLU blocks of the GO network's
// GUIDE form, and the image gate + encoder_i_N in one launch per direction.  (Its LayerNorm-over-nodes + PReLU block is
// csrc/nodes_ln.hip's kernels under the LnPrelu policy.)
//
// nn.PReLU() has ONE slope a (shape [1]): y = u > 0 ? u : a u; du = u > 0 ? dy : a dy; da = sum (u > 0 ? 0 : u dy), dy
// carrying the dropout factor behind the activation.  The slope is read from device memory (a captured step follows
// the optimiser), and da is a FINAL reduction of per-row / per-column partials summed in a fixed order
// (igcn_launch_reduce_rows_final: queued while the stream defers), so two identical steps give the same bits.
#include "common.h"
#include "dropout.h"

#define GD_T 256

__device__ __forceinline__ float gd_prelu(float u, float a) { return u > 0.f ? u : a * u; }

// =================================================================================================
// BatchNorm1d(C) + PReLU (+ dropout) on [B, C], optionally behind a per-node linear (guide_go_model.py:117-136 conc /
// B, conc_D / B_D, conc_for_attention; :138-144 the latent MLP; guide_img_snp.py:57-66 the image decoder).
// F == 0: the column is x[b, c] ([B, C]).  F > 0: x [B, F, C] channel-major, W [D, F], and the column holds
// pre[b, c, d] = sum_f W[d, f] x[b, f, c]: BatchNorm1d(C) on [B, C, D] normalises each c over (batch, d).
// One workgroup per column; y [B, C, D]; groups = 1.
// =================================================================================================
#define GD_FMAX 8
__device__ __forceinline__ float gd_col(int F, int C, int D, int c, int b, int d, const float* __restrict__ x,
                                        const float* __restrict__ W) {
  if (F == 0) return x[(int64_t)b * C + c];
  float s = 0.f;
  for (int k = 0; k < F; ++k) s += W[d * F + k] * x[((int64_t)b * F + k) * C + c];
  return s;
}

__global__ void __launch_bounds__(GD_T)
k_bn_prelu_fwd(int B, int C, int F, int D, int training, float momentum, float eps, const float* __restrict__ x,
               const float* __restrict__ W, const float* __restrict__ gamma, const float* __restrict__ beta,
               const float* __restrict__ keep, const float* __restrict__ slope, float* __restrict__ running_mean,
               float* __restrict__ running_var, float* __restrict__ y, float* __restrict__ save_mean,
               float* __restrict__ save_rstd) {
  __shared__ float red[16];
  const int c = blockIdx.x, n = B * D;
  float mean, var;
  if (training) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += GD_T) s += gd_col(F, C, D, c, i / D, i % D, x, W);
    mean = block_sum_all(s, red) / (float)n;
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += GD_T) {
      const float d = gd_col(F, C, D, c, i / D, i % D, x, W) - mean;
      v += d * d;
    }
    var = block_sum_all(v, red) / (float)n;
    if (threadIdx.x == 0) {
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * var * ((float)n / (float)(n - 1));
    }
  } else {
    mean = running_mean[c];
    var = running_var[c];
  }
  const float rstd = 1.0f / sqrtf(var + eps);
  if (threadIdx.x == 0) {
    save_mean[c] = mean;
    save_rstd[c] = rstd;
  }
  const float ga = gamma[c], be = beta[c], a = slope[0];
  for (int i = threadIdx.x; i < n; i += GD_T) {
    const int b = i / D, d = i % D;
    float t = gd_prelu((gd_col(F, C, D, c, b, d, x, W) - mean) * rstd * ga + be, a);
    if (keep) t *= keep[(int64_t)b * C + c];
    y[((int64_t)b * C + c) * D + d] = t;
  }
}

// D == 1.  dgamma / dbeta are whole columns (written directly); part [C][F + 1] = (d W of the column, d a share)
__global__ void __launch_bounds__(GD_T)
k_bn_prelu_bwd(int B, int C, int F, int training, const float* __restrict__ x, const float* __restrict__ W,
               const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ slope,
               const float* __restrict__ save_mean, const float* __restrict__ save_rstd, const float* __restrict__ dy,
               const float* __restrict__ keep, float* __restrict__ dx, float* __restrict__ dgamma,
               float* __restrict__ dbeta, float* __restrict__ part) {
  __shared__ float red[16];
  const int c = blockIdx.x;
  const float mean = save_mean[c], rstd = save_rstd[c], ga = gamma[c], be = beta[c], a = slope[0];
  float s1 = 0.f, s2 = 0.f, sa = 0.f;
  for (int b = threadIdx.x; b < B; b += GD_T) {
    const float xh = (gd_col(F, C, 1, c, b, 0, x, W) - mean) * rstd;
    const float up = keep ? dy[(int64_t)b * C + c] * keep[(int64_t)b * C + c] : dy[(int64_t)b * C + c];
    const float u = xh * ga + be;
    const float e = u > 0.f ? up : a * up;
    s1 += e;
    s2 += e * xh;
    sa += u > 0.f ? 0.f : u * up;
  }
  s1 = block_sum_all(s1, red);
  s2 = block_sum_all(s2, red);
  sa = block_sum_all(sa, red);
  const float m1 = training ? s1 / (float)B : 0.f, m2 = training ? s2 / (float)B : 0.f;
  float dw[GD_FMAX];
#pragma unroll
  for (int k = 0; k < GD_FMAX; ++k) dw[k] = 0.f;
  for (int b = threadIdx.x; b < B; b += GD_T) {
    const float xh = (gd_col(F, C, 1, c, b, 0, x, W) - mean) * rstd;
    const float up = keep ? dy[(int64_t)b * C + c] * keep[(int64_t)b * C + c] : dy[(int64_t)b * C + c];
    const float e = xh * ga + be > 0.f ? up : a * up;
    const float dv = ga * rstd * (e - m1 - xh * m2);
    if (F == 0) {
      dx[(int64_t)b * C + c] = dv;
    } else {
#pragma unroll
      for (int k = 0; k < GD_FMAX; ++k) {
        if (k < F) {
          const int64_t o = ((int64_t)b * F + k) * C + c;
          dx[o] = W[k] * dv;
          dw[k] += dv * x[o];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < GD_FMAX; ++k) {
    if (k < F) {
      const float t = block_sum_all(dw[k], red);
      if (threadIdx.x == 0) part[(int64_t)c * (F + 1) + k] = t;
    }
  }
  if (threadIdx.x == 0) {
    dgamma[c] = s2;
    dbeta[c] = s1;
    part[(int64_t)c * (F + 1) + F] = sa;
  }
}

extern "C" int igcn_bn_prelu_fwd(int B, int C, int F, int D, const float* x, const float* W, const float* gamma,
                                 const float* beta, float* running_mean, float* running_var, int training,
                                 float momentum, float eps, const float* keep, const float* slope, float* y,
                                 float* save_mean, float* save_rstd, void* stream) {
  IGCN_REQUIRE(B > 0 && C > 0 && F >= 0 && F <= GD_FMAX && D >= 1 && (F > 0 || D == 1) && (keep == nullptr || D == 1)
                   && (!training || (int64_t)B * D > 1) && slope && (F == 0 || W),
               "bn_prelu_fwd: bad sizes (F <= %d, D == 1 unless F > 0, keep only with D == 1)", GD_FMAX);
  hipLaunchKernelGGL(k_bn_prelu_fwd, dim3(C), dim3(GD_T), 0, (hipStream_t)stream, B, C, F, D, training, momentum, eps, x,
                     W, gamma, beta, keep, slope, running_mean, running_var, y, save_mean, save_rstd);
  IGCN_CHECK_LAUNCH("bn_prelu_fwd");
  return IGCN_OK;
}

extern "C" size_t igcn_bn_prelu_bwd_scratch_floats(int C, int F) { return (size_t)C * (F + 1) + 64; }

extern "C" int igcn_bn_prelu_bwd(int B, int C, int F, int training, const float* x, const float* W, const float* gamma,
                                 const float* beta, const float* slope, const float* save_mean, const float* save_rstd,
                                 const float* dy, const float* keep, float* dx, float* dW, float* dgamma, float* dbeta,
                                 float* dslope, float* scratch, void* stream) {
  IGCN_REQUIRE(B > 0 && C > 0 && F >= 0 && F <= GD_FMAX && slope && dslope && (F == 0 || (W && dW)),
               "bn_prelu_bwd: bad sizes (F <= %d)", GD_FMAX);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_bn_prelu_bwd, dim3(C), dim3(GD_T), 0, st, B, C, F, training, x, W, gamma, beta, slope, save_mean,
                     save_rstd, dy, keep, dx, dgamma, dbeta, scratch);
  IGCN_CHECK_LAUNCH("bn_prelu_bwd");
  if (F > 0) {
    const int rc = igcn_launch_reduce_rows_final(scratch, C, F + 1, F, dW, st);
    if (rc) return rc;
  }
  return igcn_launch_reduce_rows_final(scratch + F, C, F + 1, 1, dslope, st);
}

// =================================================================================================
// Image gate + encoder_i_N (guide_img_snp.py:88-100,112): one workgroup per sample.
// =================================================================================================
#define GG_KMAX 1024
#define GG_HMAX 64
#define GG_LMAX 64

// u = (r + 1/2) 2^-24 from the 24-bit draw r of element i at stream counter c (dropout.h's hash), g = -log(-log u).
// r + 1/2 needs 25 bits above 2^23 (r = 2^24 - 1 would round to u = 1, g = inf): there log u = log1p(-(1 - u)) with
// 1 - u = (2^24 - r - 1/2) 2^-24, exact in fp32.
__device__ __forceinline__ float gg_gumbel(uint32_t k0, uint32_t k1, int64_t i) {
  const uint32_t h = dm_hash(((uint32_t)i * 0x9E3779B1u) ^ k0) + (uint32_t)(i >> 32) * 0x85EBCA77u;
  const uint32_t r = dm_hash(h ^ k1) >> 8;
  const float lu = r < (1u << 23) ? logf(((float)r + 0.5f) * (1.0f / 16777216.0f))
                                  : log1pf(-((float)(16777216u - r) - 0.5f) * (1.0f / 16777216.0f));
  return -logf(-lu);
}

__device__ __forceinline__ void gg_imp(const float* __restrict__ bias, int k, float& p0, float& p1) {
  const float b0 = bias[2 * k], b1 = bias[2 * k + 1], m = fmaxf(b0, b1);
  const float e0 = expf(b0 - m), e1 = expf(b1 - m), s = e0 + e1;
  p0 = e0 / s;
  p1 = e1 / s;
}

__global__ void __launch_bounds__(GD_T)
k_guide_gate_fwd(int K, int H, int L, int training, const float* __restrict__ img, const float* __restrict__ bias,
                 const float* __restrict__ tau_p, float tau_v, const float* __restrict__ noise,
                 unsigned long long* __restrict__ state, const float* __restrict__ W1, const float* __restrict__ slope,
                 const float* __restrict__ keep, const float* __restrict__ W2, float* __restrict__ lat,
                 float* __restrict__ gate, float* __restrict__ imp1) {
  __shared__ float xin[GG_KMAX], hs[GG_HMAX];
  const int b = blockIdx.x;
  const bool draw = training && noise == nullptr;
  const unsigned long long c = draw ? state[0] : 0ull;
  const uint32_t k0 = dm_hash((uint32_t)c ^ 0x9E3779B9u), k1 = dm_hash((uint32_t)(c >> 32) + 0x85EBCA6Bu + k0);
  const float tau = tau_p ? tau_p[0] : tau_v;
  for (int k = threadIdx.x; k < K; k += GD_T) {
    float p0, p1;
    gg_imp(bias, k, p0, p1);
    if (b == 0) imp1[k] = p1;
    const int64_t e = (int64_t)b * K + k;
    float z1 = 1.f;
    if (training) {
      const float g0 = noise ? noise[2 * e] : gg_gumbel(k0, k1, 2 * e);
      const float g1 = noise ? noise[2 * e + 1] : gg_gumbel(k0, k1, 2 * e + 1);
      const float l0 = (logf(p0) + g0) / tau, l1 = (logf(p1) + g1) / tau, m = fmaxf(l0, l1);
      const float q0 = expf(l0 - m), q1 = expf(l1 - m), q = q0 + q1;
      const float s0 = q0 / q, s1 = q1 / q;
      // hard one-hot minus the detached soft value plus the soft value; ties go to class 0 (torch's max)
      z1 = s1 > s0 ? (1.f - s1) + s1 : (0.f - s1) + s1;
      gate[2 * e] = z1;
      gate[2 * e + 1] = s0 * s1;
    }
    xin[k] = img[e] * z1;
  }
  __syncthreads();
  const float a = slope[0];
  for (int j = threadIdx.x; j < H; j += GD_T) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += W1[(int64_t)j * K + k] * xin[k];
    float h = gd_prelu(s, a);
    if (keep) h *= keep[(int64_t)b * H + j];
    hs[j] = h;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < L; o += GD_T) {
    float s = 0.f;
    for (int j = 0; j < H; ++j) s += W2[o * H + j] * hs[j];
    lat[(int64_t)b * L + o] = s;
  }
  if (draw) {                              // every workgroup has read the counter: the last one to arrive advances it
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();
      if (atomicAdd(&state[1], 1ull) == (unsigned long long)gridDim.x - 1) {
        state[1] = 0;
        state[0] = c + 1;
      }
    }
  }
}

// part row of sample b: [H K d W1 | L H d W2 | 2 K d bias_n | 1 d a], ld floats apart
__global__ void __launch_bounds__(GD_T)
k_guide_gate_bwd(int K, int H, int L, int training, const float* __restrict__ img, const float* __restrict__ gate,
                 const float* __restrict__ bias, const float* __restrict__ tau_p, float tau_v,
                 const float* __restrict__ dimp1, const float* __restrict__ W1, const float* __restrict__ slope,
                 const float* __restrict__ keep, const float* __restrict__ W2, const float* __restrict__ dlat,
                 float* __restrict__ dimg, float* __restrict__ part, int64_t ld) {
  __shared__ float xin[GG_KMAX], hs[GG_HMAX], dpre[GG_HMAX], dl[GG_LMAX];
  __shared__ float red[16];
  const int b = blockIdx.x;
  const float a = slope[0], tau = tau_p ? tau_p[0] : tau_v;
  for (int k = threadIdx.x; k < K; k += GD_T) {
    const int64_t e = (int64_t)b * K + k;
    xin[k] = img[e] * (training ? gate[2 * e] : 1.f);
  }
  for (int o = threadIdx.x; o < L; o += GD_T) dl[o] = dlat[(int64_t)b * L + o];
  __syncthreads();
  float sa = 0.f;
  for (int j = threadIdx.x; j < H; j += GD_T) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += W1[(int64_t)j * K + k] * xin[k];
    const float kp = keep ? keep[(int64_t)b * H + j] : 1.f;
    hs[j] = gd_prelu(s, a) * kp;
    float dh = 0.f;
    for (int o = 0; o < L; ++o) dh += W2[o * H + j] * dl[o];
    const float up = dh * kp;
    dpre[j] = s > 0.f ? up : a * up;
    sa += s > 0.f ? 0.f : s * up;
  }
  sa = block_sum_all(sa, red);                 // (its barriers also publish hs / dpre)
  float* pr = part + (int64_t)b * ld;
  const int hk = H * K, lh = L * H;
  for (int i = threadIdx.x; i < hk; i += GD_T) pr[i] = dpre[i / K] * xin[i % K];
  for (int i = threadIdx.x; i < lh; i += GD_T) pr[hk + i] = dl[i / H] * hs[i % H];
  float* pb = pr + hk + lh;
  for (int k = threadIdx.x; k < K; k += GD_T) {
    float dx = 0.f;
    for (int j = 0; j < H; ++j) dx += W1[(int64_t)j * K + k] * dpre[j];
    const int64_t e = (int64_t)b * K + k;
    const float x = img[e];
    float db0 = 0.f, db1 = 0.f;
    if (training) {
      dimg[e] = dx * gate[2 * e];
      // straight-through: d z1 reaches the soft sample; softmax, 1/tau, log and softmax(bias_n) backward give
      // d bias_n[k] = (-1, +1) s0 s1 d z1 / tau (the two logit gradients sum to zero)
      const float dl1 = gate[2 * e + 1] * (dx * x) / tau;
      db0 = -dl1;
      db1 = dl1;
    } else {
      dimg[e] = dx;
    }
    if (b == 0 && dimp1) {                     // the gradient that reaches imp_N[:, 1] directly (the sparsity term)
      float p0, p1;
      gg_imp(bias, k, p0, p1);
      const float q = p0 * p1 * dimp1[k];
      db0 -= q;
      db1 += q;
    }
    pb[2 * k] = db0;
    pb[2 * k + 1] = db1;
  }
  if (threadIdx.x == 0) pb[2 * K] = sa;
}

extern "C" int igcn_guide_gate_supported(int K, int H, int L) {
  return K >= 1 && K <= GG_KMAX && H >= 1 && H <= GG_HMAX && L >= 1 && L <= GG_LMAX;
}

extern "C" int igcn_guide_gate_fwd(int B, int K, int H, int L, int training, const float* img, const float* bias,
                                   const float* tau, float tau_value, const float* noise, void* state, const float* W1,
                                   const float* slope, const float* keep, const float* W2, float* latent, float* gate,
                                   float* imp1, void* stream) {
  IGCN_REQUIRE(B >= 1 && igcn_guide_gate_supported(K, H, L), "guide_gate_fwd: K <= %d, H <= %d, latent <= %d",
               GG_KMAX, GG_HMAX, GG_LMAX);
  IGCN_REQUIRE(!training || gate != nullptr, "guide_gate_fwd: training needs the gate buffer");
  IGCN_REQUIRE(!training || noise != nullptr || state != nullptr, "guide_gate_fwd: training needs noise or a state");
  hipLaunchKernelGGL(k_guide_gate_fwd, dim3(B), dim3(GD_T), 0, (hipStream_t)stream, K, H, L, training, img, bias, tau,
                     tau_value, noise, (unsigned long long*)state, W1, slope, keep, W2, latent, gate, imp1);
  IGCN_CHECK_LAUNCH("guide_gate_fwd");
  return IGCN_OK;
}

extern "C" size_t igcn_guide_gate_bwd_scratch_floats(int B, int K, int H, int L) {
  return (size_t)B * (size_t)igcn_cdiv((int64_t)H * K + (int64_t)L * H + 2 * K + 1, 4) * 4 + 64;
}

extern "C" int igcn_guide_gate_bwd(int B, int K, int H, int L, int training, const float* img, const float* gate,
                                   const float* bias, const float* tau, float tau_value, const float* dimp1,
                                   const float* W1, const float* slope, const float* keep, const float* W2,
                                   const float* dlatent, float* dimg, float* dparams, float* scratch, void* stream) {
  IGCN_REQUIRE(B >= 1 && igcn_guide_gate_supported(K, H, L), "guide_gate_bwd: K <= %d, H <= %d, latent <= %d",
               GG_KMAX, GG_HMAX, GG_LMAX);
  IGCN_REQUIRE(!training || gate != nullptr, "guide_gate_bwd: training needs the gate buffer");
  hipStream_t st = (hipStream_t)stream;
  const int n = H * K + L * H + 2 * K + 1;
  const int64_t ld = igcn_cdiv(n, 4) * 4;
  hipLaunchKernelGGL(k_guide_gate_bwd, dim3(B), dim3(GD_T), 0, st, K, H, L, training, img, gate, bias, tau, tau_value,
                     dimp1, W1, slope, keep, W2, dlatent, dimg, scratch, ld);
  IGCN_CHECK_LAUNCH("guide_gate_bwd");
  return igcn_launch_reduce_rows_final(scratch, B, ld, n, dparams, st);
}
