// Per-fold KNN imputation of the clinical scores, on the device:
//   util/tool.py:44-47, :90-92   KNNImputer(n_neighbors=k).fit_transform(train) / .transform(val, test)
//                                (sklearn: weights="uniform", metric="nan_euclidean"; NaN = not measured)
//   util/tool.py:48-50, :93-94   scaler4score.transform                    -> x * scale + shift
//   util/tool.py:51-72, :95-110  [:, select_index] and the clini_score overwrite -> out_sel, dense or scattered in place
//
// For a receiver row q and a training row t (F columns), P = the columns observed in both:
//   dist(q, t) = sqrt(sum_{c in P} (q_c - t_c)^2 / |P| * F), undefined when P is empty.
// A missing entry (q, c) takes the plain mean of column c over the min(k, #candidates) nearest candidates — the training
// rows that observe c and have a defined distance to q — or, with no candidate, the mean of column c over all training
// rows that observe it.  Candidates are ordered by (distance, training row position): equal distances go to the lower
// position; the donors' values are added in that order in fp32 and divided once.  Observed entries pass through.
//
// Exact fp32, no atomics, one writer per element — the same bits every run.  Three kernels per transform:
//   k_knn_dist    training rows through LDS in tiles of 256 (column-major: lane = row, no bank conflict); thread = training
//                 row, a block serves KNN_QC receivers.  Writes the [n_q, n_fit] distances as ORDERED KEYS (the bit
//                 pattern of a non-negative float orders like the float; an undefined distance is 0xffffffff, which
//                 orders last and is no float the kernel produces) and the presence mask of every training row.
//   k_knn_select  one wave per (receiver, column).  An observed entry is copied.  A missing one runs up to k rounds of a
//                 lexicographic (distance, position) arg-min over the candidates — key = dist bits << 32 | position, each
//                 round takes the smallest key strictly above the previous pick, so nothing is mutated — then writes the
//                 value, its selected/scaled copy, the donors and a fallback flag.
//   k_knn_status  one workgroup adds the flags into the int64 status word.
// Receivers with nothing missing skip the distance pass (their keys are never read).
//
// A row index outside [0, S) is never dereferenced: such a row counts as all-missing (as a receiver it is imputed by the
// column means, its scattered row is not written) and is reported — igcn_knn_impute_stats sets every count to -1,
// igcn_knn_impute sets status to minus the number of such receivers.
#include "common.h"

#define KNN_T 256            /* threads of k_knn_dist = training rows of an LDS tile */
#define KNN_QC 8             /* receivers per block of k_knn_dist */
#define KNN_MAXF 32          /* a row's presence fits one 32-bit mask */
#define KNN_MAXK 32
#define KNN_UNDEF 0xffffffffu
#define KNN_FLAG_BAD_ROW (1 << 20)

__device__ __forceinline__ int64_t knn_row(const int64_t* __restrict__ rows, int64_t i, int64_t S) {
  const int64_t r = rows ? rows[i] : i;
  return (r >= 0 && r < S) ? r : -1;
}

// ---- per column: count of observed training values and their mean (fp64 sum in a fixed order, rounded once) ----
__global__ void __launch_bounds__(KNN_T)
k_knn_stats(int64_t S, int F, const float* __restrict__ X, const int64_t* __restrict__ rows_fit, int64_t n_fit,
            int64_t* __restrict__ counts, float* __restrict__ means) {
  __shared__ double s_sum[KNN_T];
  __shared__ long long s_cnt[KNN_T];
  __shared__ int s_bad[KNN_T];
  const int c = blockIdx.x, tid = threadIdx.x;
  double sum = 0.0;
  long long cnt = 0;
  int bad = 0;
  for (int64_t t = tid; t < n_fit; t += KNN_T) {
    const int64_t r = knn_row(rows_fit, t, S);
    if (r < 0) {
      bad = 1;
      continue;
    }
    const float v = X[r * F + c];
    if (v == v) {
      sum += (double)v;
      ++cnt;
    }
  }
  s_sum[tid] = sum;
  s_cnt[tid] = cnt;
  s_bad[tid] = bad;
  __syncthreads();
  for (int o = KNN_T / 2; o > 0; o >>= 1) {             // fixed tree
    if (tid < o) {
      s_sum[tid] += s_sum[tid + o];
      s_cnt[tid] += s_cnt[tid + o];
      s_bad[tid] |= s_bad[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const long long n = s_cnt[0];
    counts[c] = s_bad[0] ? -1 : (int64_t)n;
    means[c] = n > 0 ? (float)(s_sum[0] / (double)n) : 0.f;
  }
}

// ---- pass 1: distance keys [n_q, n_fit] and training presence masks [n_fit] ----
__global__ void __launch_bounds__(KNN_T)
k_knn_dist(int64_t S, int F, const float* __restrict__ X, const int64_t* __restrict__ rows_fit, int64_t n_fit,
           const int64_t* __restrict__ rows_q, int64_t n_q, uint32_t* __restrict__ keys, uint32_t* __restrict__ fit_mask) {
  __shared__ float s_fit[KNN_MAXF * KNN_T];             // [F][KNN_T]: missing entries hold 0
  __shared__ uint32_t s_fmask[KNN_T];
  __shared__ float s_q[KNN_QC * KNN_MAXF];              // [KNN_QC][F]
  __shared__ uint32_t s_qmask[KNN_QC];
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * KNN_T, q0 = (int64_t)blockIdx.y * KNN_QC;
  const int nt = (int)min((int64_t)KNN_T, n_fit - t0), nq = (int)min((int64_t)KNN_QC, n_q - q0);

  for (int e = tid; e < nt * F; e += KNN_T) {           // consecutive lanes: consecutive floats of the tile's rows
    const int r = e / F, c = e - r * F;
    const int64_t g = knn_row(rows_fit, t0 + r, S);
    s_fit[c * KNN_T + r] = g < 0 ? __int_as_float(0x7fc00000) : X[g * F + c];
  }
  for (int e = tid; e < nq * F; e += KNN_T) {
    const int r = e / F, c = e - r * F;
    const int64_t g = knn_row(rows_q, q0 + r, S);
    s_q[r * F + c] = g < 0 ? __int_as_float(0x7fc00000) : X[g * F + c];
  }
  __syncthreads();
  if (tid < nt) {                                       // own row: presence mask, NaN -> 0
    uint32_t m = 0;
    for (int c = 0; c < F; ++c) {
      const float v = s_fit[c * KNN_T + tid];
      if (v == v) m |= 1u << c; else s_fit[c * KNN_T + tid] = 0.f;
    }
    s_fmask[tid] = m;
    if (blockIdx.y == 0) fit_mask[t0 + tid] = m;
  }
  if (tid < nq) {
    uint32_t m = 0;
    for (int c = 0; c < F; ++c) {
      const float v = s_q[tid * F + c];
      if (v == v) m |= 1u << c; else s_q[tid * F + c] = 0.f;
    }
    s_qmask[tid] = m;
  }
  __syncthreads();
  if (tid >= nt) return;                                // (no barrier below)
  const uint32_t full = F == 32 ? 0xffffffffu : (1u << F) - 1u, mt = s_fmask[tid];
  for (int qq = 0; qq < nq; ++qq) {
    const uint32_t mq = s_qmask[qq];                    // block-uniform
    if (mq == full) continue;                           // nothing missing: the row's keys are never read
    const uint32_t both = mq & mt;
    float s = 0.f;
    for (int c = 0; c < F; ++c) {
      const float d = s_q[qq * F + c] - s_fit[c * KNN_T + tid];
      if ((both >> c) & 1u) s = fmaf(d, d, s);
    }
    const int np = __popc(both);
    const float dist = sqrtf(s / (float)np * (float)F);
    // dist >= 0 or +inf: its bits order like the value; NaN (np == 0, or inf - inf from overflowed squares) is undefined
    keys[(q0 + qq) * n_fit + t0 + tid] = (np > 0 && dist == dist) ? __float_as_uint(dist) : KNN_UNDEF;
  }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;                                             // in every lane
}

// ---- pass 2: one wave per (receiver, column) ----
__global__ void __launch_bounds__(KNN_T)
k_knn_select(int64_t S, int F, int k, const float* __restrict__ X, const int64_t* __restrict__ rows_fit, int64_t n_fit,
             const int64_t* __restrict__ rows_q, int64_t n_q, const float* __restrict__ means,
             const float* __restrict__ scale, const float* __restrict__ shift, const int32_t* __restrict__ sel, int n_sel,
             int scatter, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ fit_mask,
             float* __restrict__ out_full, float* __restrict__ out_sel, int32_t* __restrict__ donors,
             int32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (KNN_T / 64) + (threadIdx.x >> 6);
  if (w >= n_q * F) return;                             // (wave-uniform; the kernel has no barrier)
  const int64_t i = w / F;
  const int c = (int)(w - i * F);
  const int64_t rq = knn_row(rows_q, i, S);
  const float v = rq < 0 ? __int_as_float(0x7fc00000) : X[rq * F + c];
  float val = v;
  int flag = (rq < 0 && c == 0) ? KNN_FLAG_BAD_ROW : 0, used = 0;
  if (!(v == v)) {
    const uint32_t* krow = keys + i * n_fit;
    unsigned long long prev = 0ull;
    float sum = 0.f;
    for (int r = 0; r < k; ++r) {
      unsigned long long best = ~0ull;
      for (int64_t t = lane; t < n_fit; t += 64) {
        if (!((fit_mask[t] >> c) & 1u)) continue;
        const uint32_t kb = krow[t];
        if (kb == KNN_UNDEF) continue;
        const unsigned long long key = ((unsigned long long)kb << 32) | (unsigned long long)t;
        if ((r == 0 || key > prev) && key < best) best = key;
      }
      best = wave_min_u64(best);
      if (best == ~0ull) break;                         // fewer than k candidates
      const int64_t t = (int64_t)(best & 0xffffffffull);
      sum += X[knn_row(rows_fit, t, S) * F + c];         // (a candidate's row is in range: its mask bit is set)
      if (donors && lane == 0) donors[w * k + r] = (int32_t)t;
      prev = best;
      ++used;
    }
    if (used > 0) {
      val = sum / (float)used;
    } else {
      val = means[c];
      flag |= 1;
    }
  }
  if (lane == 0) {
    flags[w] = flag;
    if (donors)
      for (int r = used; r < k; ++r) donors[w * k + r] = -1;
    if (out_full) out_full[w] = val;
    if (out_sel && (!scatter || rq >= 0)) {
      const int64_t row = scatter ? rq : i;
      for (int j = 0; j < n_sel; ++j)
        if (sel[j] == c) {
          float y = val;
          if (scale) y *= scale[c];
          if (shift) y += shift[c];
          out_sel[row * n_sel + j] = y;
        }
    }
  }
}

// ---- status = number of column-mean fallbacks, or minus the number of receiver rows outside the matrix ----
__global__ void __launch_bounds__(KNN_T)
k_knn_status(const int32_t* __restrict__ flags, int64_t n, int64_t* __restrict__ status) {
  __shared__ long long s_fb[KNN_T], s_bad[KNN_T];
  const int tid = threadIdx.x;
  long long fb = 0, bad = 0;
  for (int64_t e = tid; e < n; e += KNN_T) {
    const int f = flags[e];
    fb += f & 1;
    bad += (f & KNN_FLAG_BAD_ROW) ? 1 : 0;
  }
  s_fb[tid] = fb;
  s_bad[tid] = bad;
  __syncthreads();
  for (int o = KNN_T / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_fb[tid] += s_fb[tid + o];
      s_bad[tid] += s_bad[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) status[0] = s_bad[0] ? -(int64_t)s_bad[0] : (int64_t)s_fb[0];
}

static bool knn_sizes_ok(int64_t S, int F, int64_t n_fit) {
  return S >= 1 && F >= 1 && F <= KNN_MAXF && n_fit >= 1 && n_fit <= INT32_MAX;
}

extern "C" int igcn_knn_impute_stats(int64_t S, int F, const float* X, const int64_t* rows_fit, int64_t n_fit,
                                     int64_t* counts, float* means, void* stream) {
  IGCN_REQUIRE(knn_sizes_ok(S, F, n_fit), "knn_impute_stats: bad sizes S=%lld F=%d n_fit=%lld (1 <= F <= %d, n_fit >= 1)",
               (long long)S, F, (long long)n_fit, KNN_MAXF);
  IGCN_REQUIRE(X && counts && means, "knn_impute_stats: a NULL matrix or output");
  IGCN_REQUIRE(rows_fit || n_fit == S, "knn_impute_stats: no row list, but n_fit=%lld is not S=%lld", (long long)n_fit,
               (long long)S);
  hipLaunchKernelGGL(k_knn_stats, dim3(F), dim3(KNN_T), 0, (hipStream_t)stream, S, F, X, rows_fit, n_fit, counts, means);
  IGCN_CHECK_LAUNCH("knn_impute_stats");
  return IGCN_OK;
}

// keys [n_q, n_fit] + training masks [n_fit] + flags [n_q, F] (32-bit words each)
extern "C" size_t igcn_knn_impute_scratch_floats(int64_t n_q, int64_t n_fit) {
  if (n_q < 0 || n_fit < 1) return 0;
  return (size_t)n_q * (size_t)n_fit + (size_t)n_fit + (size_t)n_q * KNN_MAXF + 1;
}

extern "C" int igcn_knn_impute(int64_t S, int F, int k, const float* X, const int64_t* rows_fit, int64_t n_fit,
                               const int64_t* rows_q, int64_t n_q, const float* means, const float* scale,
                               const float* shift, const int32_t* sel, int n_sel, int scatter, float* out_full,
                               float* out_sel, int32_t* donors, int64_t* status, float* scratch, void* stream) {
  IGCN_REQUIRE(knn_sizes_ok(S, F, n_fit) && n_q >= 0,
               "knn_impute: bad sizes S=%lld F=%d n_fit=%lld n_q=%lld (1 <= F <= %d, n_fit >= 1, n_q >= 0)", (long long)S, F,
               (long long)n_fit, (long long)n_q, KNN_MAXF);
  IGCN_REQUIRE(k >= 1 && k <= KNN_MAXK, "knn_impute: k=%d outside 1..%d", k, KNN_MAXK);
  IGCN_REQUIRE(X && means && status && scratch, "knn_impute: a NULL matrix, means, status or scratch");
  IGCN_REQUIRE(rows_fit || n_fit == S, "knn_impute: no training row list, but n_fit=%lld is not S=%lld", (long long)n_fit,
               (long long)S);
  IGCN_REQUIRE(rows_q || n_q == S || n_q == 0, "knn_impute: no receiver row list, but n_q=%lld is not S=%lld",
               (long long)n_q, (long long)S);
  IGCN_REQUIRE(n_sel >= 0 && (n_sel == 0 || sel), "knn_impute: n_sel=%d without a column list", n_sel);
  IGCN_REQUIRE(!out_sel || n_sel >= 1, "knn_impute: out_sel without selected columns");
  IGCN_REQUIRE(n_q * F <= (int64_t)INT32_MAX * (KNN_T / 64), "knn_impute: n_q=%lld is too large", (long long)n_q);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* keys = (uint32_t*)scratch;
  uint32_t* fit_mask = keys + n_q * n_fit;
  int32_t* flags = (int32_t*)(fit_mask + n_fit);
  if (n_q > 0) {
    const int64_t by = igcn_cdiv(n_q, KNN_QC);
    IGCN_REQUIRE(by <= 65535, "knn_impute: n_q=%lld exceeds %d receivers per call", (long long)n_q, 65535 * KNN_QC);
    hipLaunchKernelGGL(k_knn_dist, dim3((unsigned)igcn_cdiv(n_fit, KNN_T), (unsigned)by), dim3(KNN_T), 0, st, S, F, X,
                       rows_fit, n_fit, rows_q, n_q, keys, fit_mask);
    IGCN_CHECK_LAUNCH("knn_impute (distances)");
    hipLaunchKernelGGL(k_knn_select, dim3((unsigned)igcn_cdiv(n_q * F, KNN_T / 64)), dim3(KNN_T), 0, st, S, F, k, X,
                       rows_fit, n_fit, rows_q, n_q, means, scale, shift, sel, n_sel, scatter, keys, fit_mask, out_full,
                       out_sel, donors, flags);
    IGCN_CHECK_LAUNCH("knn_impute (selection)");
  }
  hipLaunchKernelGGL(k_knn_status, dim3(1), dim3(KNN_T), 0, st, flags, n_q * F, status);
  IGCN_CHECK_LAUNCH("knn_impute (status)");
  return IGCN_OK;
}
