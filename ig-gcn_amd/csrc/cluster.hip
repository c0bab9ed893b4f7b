// The cluster-label trainer's heads and loss (kernel/sgcn_img_snp_clusterlabel.py:217-228 and train() of
// kernel/train_eval_sgcn_clusterlabel.py:375-393) as ONE multi-workgroup launch on the narrow-layer core (narrow_head.h) —
// the sibling of k_head_loss_fwd (loss.hip) for TWO classification heads on the stacked sweep (rows [0,B): plain pass,
// rows [B,2B): isExplain pass): lin2_classify (K -> C1) and lin2_cluster (K -> C2), both log_softmaxes,
//   ce = nll(logp1[:B], y)   ce_cluster = nll(logp2[:B], clust_y)   mi = nll(logp1[B:], y)   mi_cluster = nll(logp2[B:], clust_y)
//   recon = lambda0 (sum (x_hat[:B]-snps)^2 + sum (x_hat[B:]-snps)^2) / 2
//   loss = hp_ce (ce + ce_cluster)/2 + hp_mi (mi + mi_cluster)/2 + prob + recon            (predict_cluster, :391)
//   loss = hp_ce ce + hp_mi mi + prob + recon                                              (otherwise, :393)
// and the backward of all of it for an upstream gradient of one.  What is this trainer's own:
//   - d loss / d nll of a row is hp/2 for both heads (:391), or hp for the diagnosis head alone (:393);
//   - without predict_cluster dx2, dW2, db2 are EXACT zeros;
//   - a label outside the classes poisons its plain-pass term with NaN instead of reading out of bounds;
//   - parts [blocks][5] = ce, ce_cluster, mi, mi_cluster, sum (x_hat - snps)^2; dprob = 1.
// The loss VALUE (igcn_cluster_loss_final) is only read by the host: it rides in the backward's flush as the headline's
// does (loss_final.h).
#include "loss_final.h"
#include "narrow_head.h"

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

__global__ void __launch_bounds__(256) k_cluster_head_loss_fwd(const ClusterHeadLossArgs a) {
  __shared__ float red[NH_RED_FLOATS];
  const unsigned blk = blockIdx.x;
  const int K = a.K, rows = 2 * a.B;
  const NhGeom g = nh_geom(K, blk);
  const int r = (int)g.row, q = g.q;
  const int b = r < a.B ? r : r - a.B;
  float sums[5] = {0.f, 0.f, 0.f, 0.f, 0.f};      // ce, ce_cluster, mi, mi_cluster, rec
  float4 gw1[NH_MAXC], gw2[NH_MAXC];
  float gb1[NH_MAXC], gb2[NH_MAXC];
  nh_zero(gw1, gb1);
  nh_zero(gw2, gb2);
  if (r < rows) {
    float4 x1, x2, k1, k2, w1[NH_MAXC], w2[NH_MAXC];
    nh_load_x(a.x1, a.keep1, r, K, q, x1, k1);
    nh_load_x(a.x2, a.keep2, r, K, q, x2, k2);
    nh_load_w(a.W1, K, q, a.C1, w1);
    nh_load_w(a.W2, K, q, a.C2, w2);
    const int64_t yc = a.y[b], cc = a.cy[b];
    nh_keep(x1, k1);
    nh_keep(x2, k2);
    float s1[NH_MAXC], s2[NH_MAXC], lp1[NH_MAXC], lp2[NH_MAXC], d1[NH_MAXC], d2[NH_MAXC];
    nh_scores2<false, false, false, false>(x1, w1, a.b1, a.C1, s1, x2, w2, a.b2, a.C2, s2, g.kq);
    nh_log_softmax(s1, a.C1, lp1);
    nh_log_softmax(s2, a.C2, lp2);
    const float hp = r < a.B ? a.hp_ce : a.hp_mi;
    const float wt1 = a.predict ? hp * 0.5f : hp, wt2 = a.predict ? hp * 0.5f : 0.f;
#pragma unroll
    for (int c = 0; c < NH_MAXC; ++c) {
      d1[c] = (c < a.C1 && wt1 != 0.f) ? wt1 / (float)a.B * (expf(lp1[c]) - (yc == c ? 1.f : 0.f)) : 0.f;
      d2[c] = (c < a.C2 && wt2 != 0.f) ? wt2 / (float)a.B * (expf(lp2[c]) - (cc == c ? 1.f : 0.f)) : 0.f;
      if (q == 0) {
        if (c < a.C1) {
          a.logp1[(int64_t)r * a.C1 + c] = lp1[c];
          if (yc == c) { if (r < a.B) sums[0] -= lp1[c]; else sums[2] -= lp1[c]; }
        }
        if (c < a.C2) {
          a.logp2[(int64_t)r * a.C2 + c] = lp2[c];
          if (cc == c) { if (r < a.B) sums[1] -= lp2[c]; else sums[3] -= lp2[c]; }
        }
      }
    }
    if (q == 0) {
      if (yc < 0 || yc >= a.C1) sums[0] = __builtin_nanf("");
      if (cc < 0 || cc >= a.C2) sums[1] = __builtin_nanf("");
    }
    nh_back(d1, w1, x1, k1, a.dx1 + (int64_t)r * K + 4 * q, gw1, gb1);
    if (a.predict) nh_back(d2, w2, x2, k2, a.dx2 + (int64_t)r * K + 4 * q, gw2, gb2);
    else *reinterpret_cast<float4*>(a.dx2 + (int64_t)r * K + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  sums[4] = nh_recon(blk, g.rpb, rows, a.S, a.x_hat, a.snps, a.lambda0, a.dxhat);      // (:385)
  nh_block_sums<5>(sums, red, a.parts, blk);
  float* prow = a.wpart + (int64_t)blk * (a.C1 * K + a.C1 + a.C2 * K + a.C2);
  nh_wpart(g, a.C1, K, gw1, gb1, red, prow);
  nh_wpart(g, a.C2, K, gw2, gb2, red, prow + a.C1 * K + a.C1);
  if (blk == 0 && threadIdx.x == 0) a.dprob[0] = 1.f;
}

static bool cluster_head_loss_ok(int K, int C1, int C2) { return narrow_head_ok(K, C1) && narrow_head_ok(K, C2); }
extern "C" int igcn_cluster_head_loss_supported(int K, int C1, int C2) { return cluster_head_loss_ok(K, C1, C2); }
// (0 for a K outside [4, 256]: ops sizes the launch's buffers with this before the launch refuses such a K)
extern "C" int igcn_cluster_head_loss_blocks(int B, int K) {
  return B > 0 && K >= 4 && K <= 256 ? (int)igcn_cdiv((int64_t)2 * B, narrow_head_rows_per_pass(K)) : 0;
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
               "cluster_head_loss_fwd: " NH_OK_TEXT " (K=%d C1=%d C2=%d)", K, C1, C2);
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
extern "C" int igcn_cluster_loss_final(const float* parts, int nparts, const float* prob, int prob_rows, const float* wts,
                                       float* out, void* stream) {
  IGCN_REQUIRE(parts && nparts >= 1 && prob && prob_rows >= 1 && wts && out, "cluster_loss_final: bad arguments");
  if (igcn_queue_loss_final(parts, nparts, nullptr, 0, prob, prob_rows, wts, out, (hipStream_t)stream)) return IGCN_OK;
  hipLaunchKernelGGL(k_cluster_loss_final, dim3(1), dim3(256), 0, (hipStream_t)stream, parts, nparts, prob, prob_rows, wts,
                     out);
  IGCN_CHECK_LAUNCH("cluster_loss_final");
  return IGCN_OK;
}
