// Epoch evaluation on the device: eval_loss / eval_acc / eval_scores of kernel/train_eval_sgcn_img_snps.py:551-671 without
// a host pass per batch.  igcn_eval_collect appends one batch's results to epoch buffers at a row cursor held in device
// memory (so ONE captured graph serves every batch of its shape); igcn_eval_metrics computes the epoch's metrics from
// those buffers into a small fp64 vector.  Every sum is in a fixed order or over integers: bitwise reproducible.
#include <math.h>

#include "common.h"

#define EVAL_THREADS 256
#define EVAL_MAX_CLASSES 16             // confusion matrix in LDS

// =================================================================================================
// igcn_eval_collect: one workgroup.  Every thread reads the cursor before the barrier; thread 0 advances it after the
// second one, so no thread sees a half-advanced cursor.
// =================================================================================================
__global__ void __launch_bounds__(EVAL_THREADS)
k_eval_collect(int B, int C, int NR, int F, int H, const float* __restrict__ loss, const float* __restrict__ logp,
               const float* __restrict__ reg, const float* __restrict__ out_lin, const float* __restrict__ lin_f,
               const int64_t* __restrict__ y, const float* __restrict__ clin, const int64_t* __restrict__ sbj,
               int64_t capacity, int64_t* __restrict__ state, double* __restrict__ loss_sum,
               float* __restrict__ rows_logp, int64_t* __restrict__ rows_pred, int64_t* __restrict__ rows_y,
               float* __restrict__ rows_reg, float* __restrict__ rows_clin, float* __restrict__ rows_out_lin,
               float* __restrict__ rows_lin_f, int64_t* __restrict__ rows_sbj) {
  __shared__ int s_correct;
  const int64_t c0 = state[0];
  // an earlier overflow stops every later batch too: the rows already written stay aligned with the batches
  const bool skip = state[1] != 0 || c0 < 0 || c0 + B > capacity;
  if (threadIdx.x == 0) s_correct = 0;
  __syncthreads();
  if (!skip) {
    // plain-pass rows [0, B) of the stacked [2B, *] outputs are their first B * width entries
    for (int64_t i = threadIdx.x; i < (int64_t)B * C; i += blockDim.x) rows_logp[c0 * C + i] = logp[i];
    for (int64_t i = threadIdx.x; i < (int64_t)B * NR; i += blockDim.x) {
      rows_reg[c0 * NR + i] = reg[i];
      rows_clin[c0 * NR + i] = clin[i];
    }
    for (int64_t i = threadIdx.x; i < (int64_t)B * F; i += blockDim.x) rows_out_lin[c0 * F + i] = out_lin[i];
    for (int64_t i = threadIdx.x; i < (int64_t)B * H; i += blockDim.x) rows_lin_f[c0 * H + i] = lin_f[i];
    int hits = 0;
    for (int r = threadIdx.x; r < B; r += blockDim.x) {
      // out.max(1)[1] (:557, :617): the first maximum; a NaN wins like torch's max
      const float* row = logp + (int64_t)r * C;
      int best = 0;
      float bv = row[0];
      for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (!isnan(bv) && (v > bv || isnan(v))) {
          bv = v;
          best = c;
        }
      }
      const int64_t yr = y[r];
      rows_pred[c0 + r] = best;
      rows_y[c0 + r] = yr;
      rows_sbj[c0 + r] = sbj[r];
      hits += (yr == best);
    }
    if (hits) atomicAdd(&s_correct, hits);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (skip) {
      state[1] = 1;
    } else {
      state[0] = c0 + B;
      state[2] += s_correct;
      loss_sum[0] += (double)loss[0] * (double)B;     // batches arrive in stream order: a fixed-order sum
    }
  }
}

extern "C" int igcn_eval_collect(int B, int C, int NR, int F, int H, const float* loss, const float* logp,
                                 const float* reg, const float* out_lin, const float* lin_f, const int64_t* y,
                                 const float* clin, const int64_t* sbj, int64_t capacity, int64_t* state,
                                 double* loss_sum, float* rows_logp, int64_t* rows_pred, int64_t* rows_y,
                                 float* rows_reg, float* rows_clin, float* rows_out_lin, float* rows_lin_f,
                                 int64_t* rows_sbj, void* stream) {
  IGCN_REQUIRE(B >= 1 && C >= 1 && NR >= 0 && F >= 0 && H >= 0 && capacity >= 0,
               "eval_collect: bad sizes B=%d C=%d NR=%d F=%d H=%d capacity=%lld", B, C, NR, F, H, (long long)capacity);
  IGCN_REQUIRE(loss && logp && y && sbj && state && loss_sum && rows_logp && rows_pred && rows_y && rows_sbj,
               "eval_collect: null pointer");
  IGCN_REQUIRE(NR == 0 || (reg && clin && rows_reg && rows_clin), "eval_collect: null regression pointer");
  IGCN_REQUIRE((F == 0 || (out_lin && rows_out_lin)) && (H == 0 || (lin_f && rows_lin_f)),
               "eval_collect: null feature pointer");
  hipLaunchKernelGGL(k_eval_collect, dim3(1), dim3(EVAL_THREADS), 0, (hipStream_t)stream, B, C, NR, F, H, loss, logp,
                     reg, out_lin, lin_f, y, clin, sbj, capacity, state, loss_sum, rows_logp, rows_pred, rows_y,
                     rows_reg, rows_clin, rows_out_lin, rows_lin_f, rows_sbj);
  IGCN_CHECK_LAUNCH("eval_collect");
  return IGCN_OK;
}

// =================================================================================================
// igcn_eval_metrics, part 1 (C = 2): the Mann-Whitney count of roc_curve + auc (:633-638).  Workgroup b owns rows
// [256 b, 256 b + 256) as the positive side and walks every row as the negative side in 256-row LDS tiles; a pair with
// the positive scored higher counts 2, a tie 1.  parts[b] = {that count, NaN scores among its rows}: integers, so the
// order of the final sum does not matter.
// =================================================================================================
__global__ void __launch_bounds__(EVAL_THREADS)
k_eval_auc(int64_t n, int C, const float* __restrict__ logp, const int64_t* __restrict__ y,
           int64_t* __restrict__ parts) {
  __shared__ float s_score[EVAL_THREADS];
  __shared__ int s_pos[EVAL_THREADS];
  __shared__ unsigned long long s_sum[2];
  const int64_t i = (int64_t)blockIdx.x * EVAL_THREADS + threadIdx.x;
  const bool mine = i < n;
  const float si = mine ? logp[i * C + 1] : 0.f;
  const bool pos = mine && y[i] == 1;
  unsigned long long cnt = 0;
  if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
  for (int64_t j0 = 0; j0 < n; j0 += EVAL_THREADS) {
    __syncthreads();                                   // the previous tile has been read
    const int64_t j = j0 + threadIdx.x;
    if (j < n) {
      s_score[threadIdx.x] = logp[j * C + 1];
      s_pos[threadIdx.x] = y[j] == 1;
    }
    __syncthreads();
    if (pos) {
      const int m = (int)(n - j0 < EVAL_THREADS ? n - j0 : EVAL_THREADS);
      for (int k = 0; k < m; ++k) {
        const float sj = s_score[k];
        cnt += s_pos[k] ? 0u : (si > sj ? 2u : (si == sj ? 1u : 0u));
      }
    }
  }
  if (cnt) atomicAdd(&s_sum[0], cnt);
  if (mine && isnan(si)) atomicAdd(&s_sum[1], 1ull);
  __syncthreads();
  if (threadIdx.x < 2) parts[2 * blockIdx.x + threadIdx.x] = (int64_t)s_sum[threadIdx.x];
}

// Block-wide fp64 sum in a fixed order (wave tree, then the waves in index order); result in every thread.
// `red` >= EVAL_THREADS / 64 doubles of LDS.
__device__ __forceinline__ double eval_block_sum(double v, double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();                                     // `red` is free again
  if (lane == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = 0; k < EVAL_THREADS / 64; ++k) t += red[k];
  return t;
}

// =================================================================================================
// igcn_eval_metrics, part 2: one workgroup.  Confusion counts (integer LDS atomics), accuracy, weighted F1,
// sensitivity / specificity, the AUC from part 1, and per regression target pearsonr / r2_score / RMSE (:646-655) as
// two fixed-order passes (means, then centred sums).  out layout: see include/igcn.h.
// =================================================================================================
__global__ void __launch_bounds__(EVAL_THREADS)
k_eval_final(int64_t n, int C, int NR, const int64_t* __restrict__ pred, const int64_t* __restrict__ y,
             const float* __restrict__ reg, const float* __restrict__ clin, const int64_t* __restrict__ state,
             const double* __restrict__ loss_sum, const int64_t* __restrict__ parts, int nparts,
             double* __restrict__ out) {
  __shared__ unsigned long long s_cm[EVAL_MAX_CLASSES * EVAL_MAX_CLASSES];
  __shared__ unsigned long long s_npos;
  __shared__ double red[EVAL_THREADS / 64];
  const double nan = __builtin_nan("");
  const double dn = (double)n;
  for (int k = threadIdx.x; k < C * C; k += blockDim.x) s_cm[k] = 0;
  if (threadIdx.x == 0) s_npos = 0;
  __syncthreads();
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const int64_t t = y[i], p = pred[i];
    if (t >= 0 && t < C && p >= 0 && p < C) atomicAdd(&s_cm[t * C + p], 1ull);   // labels outside [0, C) are left out
    if (t == 1) atomicAdd(&s_npos, 1ull);
  }
  __syncthreads();
  double* res = out + 8;
  for (int k = threadIdx.x; k < C * C; k += blockDim.x) res[3 * NR + k] = (double)s_cm[k];
  if (threadIdx.x == 0) {
    out[0] = (double)state[0];
    out[1] = (double)state[1];
    out[2] = loss_sum[0] / dn;
    out[3] = (double)state[2] / dn;
    double auc = 0.0, sens = 0.0, spec = 0.0;
    if (C == 2) {
      int64_t cnt = 0, nans = 0;
      for (int b = 0; b < nparts; ++b) {
        cnt += parts[2 * b];
        nans += parts[2 * b + 1];
      }
      const double np_ = (double)s_npos, nn_ = dn - np_;
      // sklearn rejects NaN scores (ValueError) and the reference's `except` makes that 0
      auc = nans ? 0.0 : (np_ == 0.0 || nn_ == 0.0 ? nan : (double)cnt / (2.0 * np_ * nn_));
      const double tn = (double)s_cm[0], fp = (double)s_cm[1], fn = (double)s_cm[2], tp = (double)s_cm[3];
      sens = tp + fn == 0.0 ? nan : tp / (tp + fn);
      spec = tn + fp == 0.0 ? nan : tn / (tn + fp);
    }
    // f1_score(average='weighted'): per label of the union of true and predicted labels, 2 tp / (support + predicted)
    // (0 where precision or recall is 0 / 0), weighted by the true support
    double f1 = 0.0, wsum = 0.0;
    for (int l = 0; l < C; ++l) {
      unsigned long long sup = 0, prd = 0;
      for (int m = 0; m < C; ++m) {
        sup += s_cm[l * C + m];
        prd += s_cm[m * C + l];
      }
      if (sup + prd == 0) continue;
      const double tp = (double)s_cm[l * C + l];
      f1 += (tp == 0.0 ? 0.0 : 2.0 * tp / (double)(sup + prd)) * (double)sup;
      wsum += (double)sup;
    }
    out[4] = auc;
    out[5] = wsum > 0.0 ? f1 / wsum : 0.0;
    out[6] = sens;
    out[7] = spec;
  }
  for (int k = 0; k < NR; ++k) {
    // predictions' NaN -> 0 first (:646)
    double st = 0.0, sp = 0.0, dt = 0.0, dp = 0.0;
    const float t0 = n ? clin[k] : 0.f, p0f = n ? reg[k] : 0.f;
    const float p0 = isnan(p0f) ? 0.f : p0f;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const float t = clin[i * NR + k], pf = reg[i * NR + k], p = isnan(pf) ? 0.f : pf;
      st += (double)t;
      sp += (double)p;
      dt += (double)(t != t0);
      dp += (double)(p != p0);
    }
    st = eval_block_sum(st, red);
    sp = eval_block_sum(sp, red);
    dt = eval_block_sum(dt, red);
    dp = eval_block_sum(dp, red);
    const double mt = st / dn, mp = sp / dn;
    double sxy = 0.0, sxx = 0.0, syy = 0.0, ssr = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      const float pf = reg[i * NR + k];
      const double t = (double)clin[i * NR + k], p = (double)(isnan(pf) ? 0.f : pf);
      const double a = t - mt, b = p - mp, e = t - p;
      sxy += a * b;
      sxx += a * a;
      syy += b * b;
      ssr += e * e;
    }
    sxy = eval_block_sum(sxy, red);
    sxx = eval_block_sum(sxx, red);
    syy = eval_block_sum(syy, red);
    ssr = eval_block_sum(ssr, red);
    if (threadIdx.x == 0) {
      // pearsonr: NaN for a constant input (scipy's check is exact equality, so is this one); clipped to [-1, 1]
      double r = nan;
      if (n >= 2 && dt != 0.0 && dp != 0.0) {
        r = sxy / sqrt(sxx * syy);
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
      }
      // r2_score (force_finite): a constant target has SS_tot = 0 -> 1.0 if SS_res = 0, else 0.0
      const double sstot = dt != 0.0 ? sxx : 0.0;
      res[k] = r;
      res[NR + k] = sstot == 0.0 ? (ssr == 0.0 ? 1.0 : 0.0) : 1.0 - ssr / sstot;
      res[2 * NR + k] = sqrt(ssr / dn);
    }
  }
}

extern "C" int igcn_eval_metrics(int64_t n, int C, int NR, const float* logp, const int64_t* pred, const int64_t* y,
                                 const float* reg, const float* clin, const int64_t* state, const double* loss_sum,
                                 int64_t* parts, double* out, void* stream) {
  // (pairwise AUC: n_pos * n_neg comparisons, one workgroup per 256 rows)
  IGCN_REQUIRE(n >= 1 && n <= IGCN_EVAL_MAX_ROWS, "eval_metrics: %lld rows outside [1, %d]", (long long)n,
               IGCN_EVAL_MAX_ROWS);
  IGCN_REQUIRE(C >= 1 && C <= EVAL_MAX_CLASSES && NR >= 0, "eval_metrics: C=%d (1..%d), NR=%d", C, EVAL_MAX_CLASSES, NR);
  IGCN_REQUIRE(logp && pred && y && state && loss_sum && parts && out && (NR == 0 || (reg && clin)),
               "eval_metrics: null pointer");
  const int nparts = (int)igcn_cdiv(n, EVAL_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (C == 2) {
    hipLaunchKernelGGL(k_eval_auc, dim3(nparts), dim3(EVAL_THREADS), 0, st, n, C, logp, y, parts);
    IGCN_CHECK_LAUNCH("eval_auc");
  }
  hipLaunchKernelGGL(k_eval_final, dim3(1), dim3(EVAL_THREADS), 0, st, n, C, NR, pred, y, reg, clin, state, loss_sum,
                     parts, C == 2 ? nparts : 0, out);
  IGCN_CHECK_LAUNCH("eval_metrics");
  return IGCN_OK;
}
