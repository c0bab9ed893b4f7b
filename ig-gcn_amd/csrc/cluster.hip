// The cluster-label trainer's heads and loss (kernel/sgcn_img_snp_clusterlabel.py:217-228 and train() of
// kernel/train_eval_sgcn_clusterlabel.py:375-393) as ONE multi-workgroup launch — the sibling of k_head_loss_fwd
// (loss.hip) for TWO classification heads on the stacked sweep (rows [0,B): plain pass, rows [B,2B): isExplain pass):
//   lin2_classify (K -> C1) and lin2_cluster (K -> C2) with the dropout factors applied on load, both log_softmaxes,
//   ce = nll(logp1[:B], y)   ce_cluster = nll(logp2[:B], clust_y)   mi = nll(logp1[B:], y)   mi_cluster = nll(logp2[B:], clust_y)
//   recon = lambda0 (sum (x_hat[:B]-snps)^2 + sum (x_hat[B:]-snps)^2) / 2
//   loss = hp_ce (ce + ce_cluster)/2 + hp_mi (mi + mi_cluster)/2 + prob + recon            (predict_cluster, :391)
//   loss = hp_ce ce + hp_mi mi + prob + recon                                              (otherwise, :393)
// and the backward of all of it for an upstream gradient of one: a workgroup owns 256 / (K / 4) rows, computes their
// scores, the softmaxes, its share of the five row-wise sums, d loss / d scores and from those — they are in registers —
// the gradients of the two layers' inputs and its rows' share of the weight / bias gradients (partial rows for the
// deferred reduction).  No atomics; every sum in a fixed order.  The loss VALUE (igcn_cluster_loss_final) is only read by
// the host: it rides in the backward's flush as the headline's does (loss_final.h).
#include "loss_final.h"

#define CL_MAXC 4
struct ClusterHeadLossArgs {
  int B, K, C1, C2, S, predict;
  const float *x1, *keep1, *W1, *b1;      // diagnosis head: features [2B, K] (dropout factors or NULL), lin2_classify
  const float *x2, *keep2, *W2, *b2;      // cluster-label head: features [2B, K], lin2_cluster
  const int64_t *y, *cy;                   // [B] each
  const float *x_hat, *snps;               // [2B, S], [B, S]
  float hp_ce, hp_mi, lambda0;
  float *logp1, *logp2;                    // [2B, C1], [2B, C2] log_softmax
  float *dx1, *dx2, *dxhat;                // d loss / d (features, x_hat) for an upstream gradient of one
  float *parts;                            // [blocks][5]: sums of -logp1[y] | -logp2[cy] (plain), the same (masked), (x_hat - snps)^2
  float *wpart;                            // [blocks][C1 K + C1 + C2 K + C2]: the layers' weight | bias gradient partials
  float *dprob;                            // [1]: d loss / d regulariser
};

#define CL_RED_FLOATS (256 * 4 * CL_MAXC + 256 * CL_MAXC)
__global__ void __launch_bounds__(256) k_cluster_head_loss_fwd(const ClusterHeadLossArgs a) {
  __shared__ float red[CL_RED_FLOATS];
  const unsigned blk = blockIdx.x;
  const int K = a.K, kq = K / 4, q = threadIdx.x % kq, rl = threadIdx.x / kq, rpb = 256 / kq;
  const int rows = 2 * a.B;
  const int r = (int)blk * rpb + rl;
  const bool live = r < rows;
  const int b = r < a.B ? r : r - a.B;
  float ce = 0.f, cec = 0.f, mi = 0.f, mic = 0.f, rec = 0.f;
  float4 gw1[CL_MAXC], gw2[CL_MAXC];
  float gb1[CL_MAXC], gb2[CL_MAXC];
#pragma unroll
  for (int c = 0; c < CL_MAXC; ++c) {
    gw1[c] = gw2[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    gb1[c] = gb2[c] = 0.f;
  }
  if (live) {
    // every load of the row up front: features, dropout factors, both layers' weight quads, the two labels
    float4 x1 = *reinterpret_cast<const float4*>(a.x1 + (int64_t)r * K + 4 * q);
    float4 x2 = *reinterpret_cast<const float4*>(a.x2 + (int64_t)r * K + 4 * q);
    float4 k1 = make_float4(1.f, 1.f, 1.f, 1.f), k2 = k1;
    if (a.keep1) k1 = *reinterpret_cast<const float4*>(a.keep1 + (int64_t)r * K + 4 * q);
    if (a.keep2) k2 = *reinterpret_cast<const float4*>(a.keep2 + (int64_t)r * K + 4 * q);
    float4 w1[CL_MAXC], w2[CL_MAXC];
#pragma unroll
    for (int c = 0; c < CL_MAXC; ++c) {
      w1[c] = c < a.C1 ? *reinterpret_cast<const float4*>(a.W1 + c * K + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
      w2[c] = c < a.C2 ? *reinterpret_cast<const float4*>(a.W2 + c * K + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int64_t yc = a.y[b], cc = a.cy[b];
    x1.x *= k1.x; x1.y *= k1.y; x1.z *= k1.z; x1.w *= k1.w;           // dropout of the input, fused: x * keep
    x2.x *= k2.x; x2.y *= k2.y; x2.z *= k2.z; x2.w *= k2.w;
    float s1[CL_MAXC], s2[CL_MAXC];
#pragma unroll
    for (int c = 0; c < CL_MAXC; ++c) {
      s1[c] = (x1.x * w1[c].x + x1.y * w1[c].y) + (x1.z * w1[c].z + x1.w * w1[c].w);      // (k_small_linear_fwd's order)
      s2[c] = (x2.x * w2[c].x + x2.y * w2[c].y) + (x2.z * w2[c].z + x2.w * w2[c].w);
      for (int o = 1; o < kq; o <<= 1) {
        s1[c] += __shfl_xor(s1[c], o, 64);
        s2[c] += __shfl_xor(s2[c], o, 64);
      }
      s1[c] += (c < a.C1 && a.b1) ? a.b1[c] : 0.f;
      s2[c] += (c < a.C2 && a.b2) ? a.b2[c] : 0.f;
    }
    float m1 = -INFINITY, m2 = -INFINITY;
#pragma unroll
    for (int c = 0; c < CL_MAXC; ++c) {
      if (c < a.C1) m1 = fmaxf(m1, s1[c]);
      if (c < a.C2) m2 = fmaxf(m2, s2[c]);
    }
    float se1 = 0.f, se2 = 0.f;
#pragma unroll
    for (int c = 0; c < CL_MAXC; ++c) {
      if (c < a.C1) se1 += expf(s1[c] - m1);
      if (c < a.C2) se2 += expf(s2[c] - m2);
    }
    const float lse1 = logf(se1), lse2 = logf(se2);
    // d loss / d nll of this row's pass: hp/2 for both heads (:391), or hp for the diagnosis head alone (:393)
    const float hp = r < a.B ? a.hp_ce : a.hp_mi;
    const float wt1 = a.predict ? hp * 0.5f : hp, wt2 = a.predict ? hp * 0.5f : 0.f;
    float d1[CL_MAXC], d2[CL_MAXC];
#pragma unroll
    for (int c = 0; c < CL_MAXC; ++c) {
      const float lp1 = (s1[c] - m1) - lse1, lp2 = (s2[c] - m2) - lse2;
      d1[c] = (c < a.C1 && wt1 != 0.f) ? wt1 / (float)a.B * (expf(lp1) - (yc == c ? 1.f : 0.f)) : 0.f;
      d2[c] = (c < a.C2 && wt2 != 0.f) ? wt2 / (float)a.B * (expf(lp2) - (cc == c ? 1.f : 0.f)) : 0.f;
      if (q == 0) {
        if (c < a.C1) {
          a.logp1[(int64_t)r * a.C1 + c] = lp1;
          if (yc == c) { if (r < a.B) ce -= lp1; else mi -= lp1; }
        }
        if (c < a.C2) {
          a.logp2[(int64_t)r * a.C2 + c] = lp2;
          if (cc == c) { if (r < a.B) cec -= lp2; else mic -= lp2; }
        }
      }
    }
    if (q == 0) {                                                      // a label outside the classes: as k_head_loss_fwd,
      if (yc < 0 || yc >= a.C1) ce = __builtin_nanf("");              // poison the term instead of reading out of bounds
      if (cc < 0 || cc >= a.C2) cec = __builtin_nanf("");
    }
    // backward of the two layers for exactly those upstream gradients: dx = (d W) * keep, dW += d x^T, db += d
    float4 e1 = make_float4(0.f, 0.f, 0.f, 0.f), e2 = e1;
#pragma unroll
    for (int c = 0; c < CL_MAXC; ++c) {
      e1.x += d1[c] * w1[c].x; e1.y += d1[c] * w1[c].y; e1.z += d1[c] * w1[c].z; e1.w += d1[c] * w1[c].w;
      gw1[c] = make_float4(d1[c] * x1.x, d1[c] * x1.y, d1[c] * x1.z, d1[c] * x1.w);
      gb1[c] = d1[c];
      if (a.predict) {                                                 // (else: dx2, dW2, db2 stay EXACT zeros)
        e2.x += d2[c] * w2[c].x; e2.y += d2[c] * w2[c].y; e2.z += d2[c] * w2[c].z; e2.w += d2[c] * w2[c].w;
        gw2[c] = make_float4(d2[c] * x2.x, d2[c] * x2.y, d2[c] * x2.z, d2[c] * x2.w);
        gb2[c] = d2[c];
      }
    }
    *reinterpret_cast<float4*>(a.dx1 + (int64_t)r * K + 4 * q) = make_float4(e1.x * k1.x, e1.y * k1.y, e1.z * k1.z, e1.w * k1.w);
    *reinterpret_cast<float4*>(a.dx2 + (int64_t)r * K + 4 * q) =
        a.predict ? make_float4(e2.x * k2.x, e2.y * k2.y, e2.z * k2.z, e2.w * k2.w) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // reconstruction term of the block's rows (:385) and its gradient
  {
    const int64_t e0 = (int64_t)blk * rpb * a.S, e1 = min((int64_t)rows, (int64_t)(blk + 1) * rpb) * a.S;
    const int64_t half = (int64_t)a.B * a.S;
    for (int64_t i = e0 + threadIdx.x; i < e1; i += 256) {
      const float d = a.x_hat[i] - a.snps[i < half ? i : i - half];
      rec += d * d;
      a.dxhat[i] = a.lambda0 * d;
    }
  }
  // the block's five loss sums
  {
    ce = wave_sum(ce); cec = wave_sum(cec); mi = wave_sum(mi); mic = wave_sum(mic); rec = wave_sum(rec);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { red[wv] = ce; red[4 + wv] = cec; red[8 + wv] = mi; red[12 + wv] = mic; red[16 + wv] = rec; }
    __syncthreads();
    if (threadIdx.x < 5) {
      const float* p = red + 4 * threadIdx.x;
      a.parts[(int64_t)blk * 5 + threadIdx.x] = (p[0] + p[1]) + (p[2] + p[3]);
    }
    __syncthreads();
  }
  // weight / bias gradient partials: the block's row lanes summed in order through LDS, layer after layer
  float* prow = a.wpart + (int64_t)blk * (a.C1 * K + a.C1 + a.C2 * K + a.C2);
  float* redb = red + 256 * 4 * CL_MAXC;
#pragma unroll
  for (int layer = 0; layer < 2; ++layer) {
    const int CC = layer ? a.C2 : a.C1;
#pragma unroll
    for (int c = 0; c < CL_MAXC; ++c) {
      const float4 g4 = layer ? gw2[c] : gw1[c];
      float* rc = red + c * 1024;
      rc[threadIdx.x * 4 + 0] = g4.x; rc[threadIdx.x * 4 + 1] = g4.y; rc[threadIdx.x * 4 + 2] = g4.z; rc[threadIdx.x * 4 + 3] = g4.w;
      redb[c * 256 + threadIdx.x] = q == 0 ? (layer ? gb2[c] : gb1[c]) : 0.f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < CC * K; idx += 256) {
      const int c = idx / K, k = idx - c * K, qq = k / 4, j = k % 4;
      float t = 0.f;
      for (int l = 0; l < rpb; ++l) t += red[c * 1024 + (l * kq + qq) * 4 + j];
      prow[c * K + k] = t;
    }
    if (threadIdx.x < CC) {
      float t = 0.f;
      for (int l = 0; l < rpb; ++l) t += redb[threadIdx.x * 256 + l * kq];
      prow[CC * K + threadIdx.x] = t;
    }
    prow += CC * K + CC;
    __syncthreads();
  }
  if (blk == 0 && threadIdx.x == 0) a.dprob[0] = 1.f;
}

static bool cluster_head_loss_ok(int K, int C1, int C2) {
  const int kq = K / 4;
  return K > 0 && K % 4 == 0 && kq <= 64 && (kq & (kq - 1)) == 0 && C1 >= 1 && C1 <= CL_MAXC && C2 >= 1 && C2 <= CL_MAXC;
}
extern "C" int igcn_cluster_head_loss_supported(int K, int C1, int C2) { return cluster_head_loss_ok(K, C1, C2); }
extern "C" int igcn_cluster_head_loss_blocks(int B, int K) {
  return B > 0 && K >= 4 && K <= 256 ? (int)igcn_cdiv((int64_t)2 * B, 256 / (K / 4)) : 0;
}

// x1 / x2 [2B, K] (keep* [2B, K] or NULL), W1 [C1, K] + b1, W2 [C2, K] + b2, y / clust_y [B] int64, x_hat [2B, S], snps
// [B, S].  Outputs: logp1 [2B, C1], logp2 [2B, C2], dx1 / dx2 [2B, K], dxhat [2B, S], parts [blocks, 5], wpart [blocks,
// C1 K + C1 + C2 K + C2], dprob [1]  (blocks = igcn_cluster_head_loss_blocks(B, K)).
extern "C" int igcn_cluster_head_loss_fwd(int B, int K, int C1, int C2, int S, const float* x1, const float* keep1,
                                          const float* W1, const float* b1, const float* x2, const float* keep2,
                                          const float* W2, const float* b2, const int64_t* y, const int64_t* clust_y,
                                          const float* x_hat, const float* snps, float hp_ce, float hp_mi, float lambda0,
                                          int predict_cluster, float* logp1, float* logp2, float* dx1, float* dx2,
                                          float* dxhat, float* parts, float* wpart, float* dprob, void* stream) {
  IGCN_REQUIRE(B > 0 && S > 0 && cluster_head_loss_ok(K, C1, C2),
               "cluster_head_loss_fwd: K/4 a power of two <= 64, 1 <= C1, C2 <= 4 (K=%d C1=%d C2=%d)", K, C1, C2);
  IGCN_REQUIRE(x1 && W1 && x2 && W2 && y && clust_y && x_hat && snps && logp1 && logp2 && dx1 && dx2 && dxhat && parts &&
                   wpart && dprob,
               "cluster_head_loss_fwd: null argument");
  IGCN_REQUIRE((((uintptr_t)x1 | (uintptr_t)x2 | (uintptr_t)keep1 | (uintptr_t)keep2 | (uintptr_t)W1 | (uintptr_t)W2 |
                 (uintptr_t)dx1 | (uintptr_t)dx2) & 15) == 0,
               "cluster_head_loss_fwd: features, factors, weights and their gradients must be 16-byte aligned");
  const ClusterHeadLossArgs a = {B, K, C1, C2, S, predict_cluster != 0, x1, keep1, W1, b1, x2, keep2, W2, b2, y, clust_y,
                                 x_hat, snps, hp_ce, hp_mi, lambda0, logp1, logp2, dx1, dx2, dxhat, parts, wpart, dprob};
  hipLaunchKernelGGL(k_cluster_head_loss_fwd, dim3((unsigned)igcn_cluster_head_loss_blocks(B, K)), dim3(256), 0,
                     (hipStream_t)stream, a);
  IGCN_CHECK_LAUNCH("cluster_head_loss_fwd");
  return IGCN_OK;
}

__global__ void __launch_bounds__(256)
k_cluster_loss_final(const float* __restrict__ parts, int nparts, const float* __restrict__ prob, int prob_rows,
                     const float* __restrict__ wts, float* __restrict__ out) {
  __shared__ float lds[40];
  cluster_loss_final_body(parts, nparts, prob, prob_rows, wts, out, lds);
}

// The loss value from its partial sums (loss_final.h): parts [nparts, 5] of igcn_cluster_head_loss_fwd, prob [prob_rows] =
// the regulariser or its un-reduced partials, wts [5] DEVICE = {hp_ce, hp_mi, lambda0, B, predict_cluster}; out [8] = loss,
// ce, ce_cluster, mi, mi_cluster, prob, recon, 0.  While the stream defers its reductions the job joins the flush as
// igcn_loss_final's does (the same queue entry, told apart by its missing Gram partials); else a launch of its own.
int igcn_queue_loss_final(const float* parts, int nparts, const float* gram, int gram_rows, const float* prob,
                          int prob_rows, const float* wts, float* out, hipStream_t st);      // plan.hip
extern "C" int igcn_cluster_loss_final(const float* parts, int nparts, const float* prob, int prob_rows, const float* wts,
                                       float* out, void* stream) {
  IGCN_REQUIRE(parts && nparts >= 1 && prob && prob_rows >= 1 && wts && out, "cluster_loss_final: bad arguments");
  if (igcn_queue_loss_final(parts, nparts, nullptr, 0, prob, prob_rows, wts, out, (hipStream_t)stream)) return IGCN_OK;
  hipLaunchKernelGGL(k_cluster_loss_final, dim3(1), dim3(256), 0, (hipStream_t)stream, parts, nparts, prob, prob_rows, wts,
                     out);
  IGCN_CHECK_LAUNCH("cluster_loss_final");
  return IGCN_OK;
}
