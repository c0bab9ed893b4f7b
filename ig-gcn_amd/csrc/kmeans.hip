// Lloyd's KMeans and greedy k-means++ seeding on the device, sklearn 1.7's cluster/_kmeans.py restated:
//   util/image_cluster.py:148-282   KMeans(n_clusters=2, init='k-means++', random_state=1000) on the t-SNE embedding
//                                   -> clust_y, and calculate_WSS (the inertia for k = 1..10).
//
//   igcn_kmeans_assign   labels = arg-min over the centres of the direct-difference squared distance (fp32 fma chain per
//                        lane, fixed wave tree; equal distances go to the LOWER centre), the distance to the own centre,
//                        and — per workgroup of 64 points, then combined in workgroup order — the clusters' counts and
//                        coordinate sums (fp64, added in point order), the inertia (fp64) and how many labels changed
//                        against what `labels` held before.
//   igcn_kmeans_update   centre = sum / count, rounded once to fp32.  Empty clusters, in ascending order, take the points
//                        farthest from their own centre, in descending order of distance (equal distances: the lower
//                        point first) — _relocate_empty_clusters_dense; a cluster left with nothing sits on the centre
//                        of the largest one (_average_centers).  Writes the total squared centre shift and a flag
//                        saying whether the assignment it follows changed any label.
//   igcn_kmeanspp_step   one step of _kmeans_plusplus: t candidates by an fp64 inclusive scan of the closest distances
//                        (stable_cumsum) and a left search of u_c * potential, each candidate's new potential, the best
//                        one kept (equal potentials: the first), the closest distances updated.
// No atomics, one writer per element, fixed orders: the same bits every run.  N <= 65536, d <= 1024, k <= 16
// (IGCN_KMEANS_MAX_N, IGCN_KMEANS_MAX_D, IGCN_KMEANS_MAX_K).
#include "common.h"

#define KM_T 256
#define KM_PTS 64               /* points per workgroup of the assignment */
#define KMPP_T 1024

__global__ void __launch_bounds__(KM_T)
k_kmeans_assign(int N, int d, int k, const float* __restrict__ X, const float* __restrict__ centers,
                int64_t* __restrict__ labels, float* __restrict__ mind, double* __restrict__ part_sums,
                int* __restrict__ part_cnt, double* __restrict__ part_inertia, int* __restrict__ part_chg) {
  __shared__ int s_lab[KM_PTS], s_chg[KM_PTS];
  __shared__ float s_min[KM_PTS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * KM_PTS, np = min(KM_PTS, N - n0);
  for (int pl = w; pl < np; pl += KM_T / 64) {            // one wave per point
    const float* x = X + (int64_t)(n0 + pl) * d;
    float best = 0.f;
    int bc = 0;
    for (int c = 0; c < k; ++c) {
      const float* ctr = centers + (int64_t)c * d;
      float a = 0.f;
      for (int f = lane; f < d; f += 64) {
        const float df = x[f] - ctr[f];
        a = fmaf(df, df, a);
      }
      a = wave_sum_all(a);
      if (c == 0 || a < best) {                           // strict: a tie keeps the lower centre
        best = a;
        bc = c;
      }
    }
    if (lane == 0) {
      s_lab[pl] = bc;
      s_min[pl] = best;
      s_chg[pl] = labels[n0 + pl] != (int64_t)bc;
      labels[n0 + pl] = (int64_t)bc;
      mind[n0 + pl] = best;
    }
  }
  __syncthreads();
  if (part_sums) {
    double* ps = part_sums + (int64_t)blockIdx.x * k * d;
    for (int f = tid; f < d; f += KM_T)
      for (int c = 0; c < k; ++c) {
        double s = 0.0;
        for (int pl = 0; pl < np; ++pl)
          if (s_lab[pl] == c) s += (double)X[(int64_t)(n0 + pl) * d + f];
        ps[(int64_t)c * d + f] = s;
      }
    if (tid < k) {
      int cnt = 0;
      for (int pl = 0; pl < np; ++pl) cnt += s_lab[pl] == tid;
      part_cnt[blockIdx.x * k + tid] = cnt;
    }
  }
  if (tid == 64) {
    double s = 0.0;
    int chg = 0;
    for (int pl = 0; pl < np; ++pl) {
      s += (double)s_min[pl];
      chg += s_chg[pl];
    }
    part_inertia[blockIdx.x] = s;
    part_chg[blockIdx.x] = chg;
  }
}

// stats: [0] inertia, [1] labels changed; igcn_kmeans_update adds [2] squared centre shift, [3] any-label-changed flag
__global__ void __launch_bounds__(KM_T)
k_kmeans_combine(int nblk, int d, int k, const double* __restrict__ part_sums, const int* __restrict__ part_cnt,
                 const double* __restrict__ part_inertia, const int* __restrict__ part_chg, int64_t* __restrict__ counts,
                 double* __restrict__ sums, double* __restrict__ stats) {
  const int e = blockIdx.x * KM_T + threadIdx.x;
  if (sums && e < k * d) {
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part_sums[(int64_t)b * k * d + e];
    sums[e] = s;
  }
  if (blockIdx.x != 0) return;
  if (counts && threadIdx.x < k) {
    int64_t c = 0;
    for (int b = 0; b < nblk; ++b) c += part_cnt[b * k + threadIdx.x];
    counts[threadIdx.x] = c;
  }
  if (threadIdx.x == 64) {
    double s = 0.0;
    int64_t chg = 0;
    for (int b = 0; b < nblk; ++b) {
      s += part_inertia[b];
      chg += part_chg[b];
    }
    stats[0] = s;
    stats[1] = (double)chg;
  }
}

__global__ void __launch_bounds__(KM_T)
k_kmeans_update(int N, int d, int k, const float* __restrict__ X, const int64_t* __restrict__ labels,
                const float* __restrict__ mind, const int64_t* __restrict__ counts, double* __restrict__ sums,
                float* __restrict__ centers, double* __restrict__ stats) {
  __shared__ long long s_cnt[IGCN_KMEANS_MAX_K];
  __shared__ unsigned long long s_key[KM_T];
  __shared__ double s_red[KM_T];
  __shared__ int s_big;
  const int tid = threadIdx.x;
  if (tid < k) s_cnt[tid] = counts[tid];
  __syncthreads();
  // empty clusters in ascending order <- farthest points in descending (distance, -index) order
  unsigned long long prev = ~0ull;
  for (int c = 0; c < k; ++c) {
    if (counts[c] != 0) continue;                         // (block-uniform) the clusters that CAME empty, like sklearn
    unsigned long long best = 0ull;                       // key 0 = none (a real key has a non-zero low word)
    for (int n = tid; n < N; n += KM_T) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(mind[n]) << 32) | (0xffffffffu - (unsigned)n);
      if (key < prev && key > best) best = key;
    }
    s_key[tid] = best;
    __syncthreads();
    for (int o = KM_T / 2; o > 0; o >>= 1) {
      if (tid < o && s_key[tid + o] > s_key[tid]) s_key[tid] = s_key[tid + o];
      __syncthreads();
    }
    best = s_key[0];
    __syncthreads();
    if (best == 0ull) break;                              // more empty clusters than points left
    prev = best;
    const int far = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
    const int old = (int)labels[far];
    for (int f = tid; f < d; f += KM_T) {
      const double v = (double)X[(int64_t)far * d + f];
      sums[(int64_t)old * d + f] -= v;
      sums[(int64_t)c * d + f] = v;
    }
    __syncthreads();
    if (tid == 0) {
      s_cnt[c] = 1;
      s_cnt[old] -= 1;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int big = 0;
    for (int c = 1; c < k; ++c)
      if (s_cnt[c] > s_cnt[big]) big = c;
    s_big = big;
  }
  __syncthreads();
  double shift = 0.0;
  for (int e = tid; e < k * d; e += KM_T) {
    const int c = e / d, f = e - c * d;
    const int src = s_cnt[c] > 0 ? c : s_big;
    const float v = s_cnt[src] > 0 ? (float)(sums[(int64_t)src * d + f] / (double)s_cnt[src]) : centers[e];
    const double df = (double)v - (double)centers[e];
    shift += df * df;
    centers[e] = v;                                       // (element e is read by this thread alone)
  }
  s_red[tid] = shift;
  __syncthreads();
  for (int o = KM_T / 2; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    stats[2] = s_red[0];
    stats[3] = stats[1] != 0.0 ? 1.0 : 0.0;               // the flag the host tests: did the assignment change a label
  }
}

// One workgroup; thread t owns the points [t chunk, (t + 1) chunk).
__global__ void __launch_bounds__(KMPP_T)
k_kmeanspp_step(int N, int d, int t, const float* __restrict__ X, const double* __restrict__ u,
                float* __restrict__ closest, double* __restrict__ pot, int64_t* __restrict__ chosen) {
  __shared__ double s_sum[KMPP_T];
  __shared__ double s_pot[IGCN_KMEANSPP_MAX_TRIALS];
  __shared__ int s_cnt[KMPP_T];
  __shared__ int s_id[IGCN_KMEANSPP_MAX_TRIALS];
  __shared__ int s_best;
  const int tid = threadIdx.x, chunk = (N + KMPP_T - 1) / KMPP_T;
  const int lo = min(N, tid * chunk), hi = min(N, lo + chunk);
  double s = 0.0;
  for (int n = lo; n < hi; ++n) s += (double)closest[n];
  s_sum[tid] = s;
  __syncthreads();
  if (tid == 0) {                                         // exclusive scan of the chunk sums, in order
    double run = 0.0;
    for (int i = 0; i < KMPP_T; ++i) {
      const double v = s_sum[i];
      s_sum[i] = run;
      run += v;
    }
  }
  __syncthreads();
  const double before = s_sum[tid], cur = pot[0];
  __syncthreads();
  for (int c = 0; c < t; ++c) {                           // searchsorted(cumsum, u_c * pot): how many scan values lie below
    const double val = u[c] * cur;
    double run = before;
    int cnt = 0;
    for (int n = lo; n < hi; ++n) {
      run += (double)closest[n];
      cnt += run < val;
    }
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int o = KMPP_T / 2; o > 0; o >>= 1) {
      if (tid < o) s_cnt[tid] += s_cnt[tid + o];
      __syncthreads();
    }
    if (tid == 0) s_id[c] = min(s_cnt[0], N - 1);
    __syncthreads();
  }
  for (int c = 0; c < t; ++c) {                           // the candidates' potentials
    const float* y = X + (int64_t)s_id[c] * d;
    double a = 0.0;
    for (int n = lo; n < hi; ++n) {
      const float* x = X + (int64_t)n * d;
      float q = 0.f;
      for (int f = 0; f < d; ++f) {
        const float df = x[f] - y[f];
        q = fmaf(df, df, q);
      }
      a += (double)fminf(closest[n], q);
    }
    s_sum[tid] = a;
    __syncthreads();
    for (int o = KMPP_T / 2; o > 0; o >>= 1) {
      if (tid < o) s_sum[tid] += s_sum[tid + o];
      __syncthreads();
    }
    if (tid == 0) s_pot[c] = s_sum[0];
    __syncthreads();
  }
  if (tid == 0) {
    int b = 0;
    for (int c = 1; c < t; ++c)
      if (s_pot[c] < s_pot[b]) b = c;
    s_best = s_id[b];
    pot[0] = s_pot[b];
    chosen[0] = (int64_t)s_id[b];
  }
  __syncthreads();
  const float* y = X + (int64_t)s_best * d;
  for (int n = lo; n < hi; ++n) {
    const float* x = X + (int64_t)n * d;
    float q = 0.f;
    for (int f = 0; f < d; ++f) {
      const float df = x[f] - y[f];
      q = fmaf(df, df, q);
    }
    closest[n] = fminf(closest[n], q);
  }
}

static bool km_sizes_ok(int64_t N, int d, int k) {
  return N >= 1 && N <= IGCN_KMEANS_MAX_N && d >= 1 && d <= IGCN_KMEANS_MAX_D && k >= 1 && k <= IGCN_KMEANS_MAX_K;
}

// in 4-byte words: part_inertia [nblk] fp64, part_sums [nblk, k, d] fp64, part_cnt [nblk, k], part_chg [nblk]
extern "C" size_t igcn_kmeans_scratch_floats(int64_t N, int d, int k) {
  if (!km_sizes_ok(N, d, k)) return 0;
  const size_t nblk = (size_t)igcn_cdiv(N, KM_PTS);
  return 2 * nblk + 2 * nblk * k * d + nblk * k + nblk + 2;
}

extern "C" int igcn_kmeans_assign(int64_t N, int d, int k, const float* X, const float* centers, int64_t* labels,
                                  float* mind, int64_t* counts, double* sums, double* stats, float* scratch,
                                  void* stream) {
  IGCN_REQUIRE(km_sizes_ok(N, d, k), "kmeans_assign: N=%lld d=%d k=%d outside 1 <= N <= %d, 1 <= d <= %d, 1 <= k <= %d",
               (long long)N, d, k, IGCN_KMEANS_MAX_N, IGCN_KMEANS_MAX_D, IGCN_KMEANS_MAX_K);
  IGCN_REQUIRE(X && centers && labels && mind && stats && scratch, "kmeans_assign: a NULL argument");
  IGCN_REQUIRE((counts != nullptr) == (sums != nullptr), "kmeans_assign: counts and sums come together");
  IGCN_REQUIRE(((uintptr_t)scratch & 7) == 0, "kmeans_assign: the scratch is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)igcn_cdiv(N, KM_PTS);
  double* part_inertia = (double*)scratch;
  double* part_sums = part_inertia + nblk;
  int* part_cnt = (int*)(part_sums + (size_t)nblk * k * d);
  int* part_chg = part_cnt + (size_t)nblk * k;
  hipLaunchKernelGGL(k_kmeans_assign, dim3(nblk), dim3(KM_T), 0, st, (int)N, d, k, X, centers, labels, mind,
                     sums ? part_sums : (double*)nullptr, part_cnt, part_inertia, part_chg);
  IGCN_CHECK_LAUNCH("kmeans_assign");
  hipLaunchKernelGGL(k_kmeans_combine, dim3((unsigned)igcn_cdiv((int64_t)k * d, KM_T)), dim3(KM_T), 0, st, nblk, d, k,
                     part_sums, part_cnt, part_inertia, part_chg, counts, sums, stats);
  IGCN_CHECK_LAUNCH("kmeans_assign (combine)");
  return IGCN_OK;
}

extern "C" int igcn_kmeans_update(int64_t N, int d, int k, const float* X, const int64_t* labels, const float* mind,
                                  const int64_t* counts, double* sums, float* centers, double* stats, void* stream) {
  IGCN_REQUIRE(km_sizes_ok(N, d, k), "kmeans_update: N=%lld d=%d k=%d outside 1 <= N <= %d, 1 <= d <= %d, 1 <= k <= %d",
               (long long)N, d, k, IGCN_KMEANS_MAX_N, IGCN_KMEANS_MAX_D, IGCN_KMEANS_MAX_K);
  IGCN_REQUIRE(X && labels && mind && counts && sums && centers && stats, "kmeans_update: a NULL argument");
  hipLaunchKernelGGL(k_kmeans_update, dim3(1), dim3(KM_T), 0, (hipStream_t)stream, (int)N, d, k, X, labels, mind, counts,
                     sums, centers, stats);
  IGCN_CHECK_LAUNCH("kmeans_update");
  return IGCN_OK;
}

extern "C" int igcn_kmeanspp_step(int64_t N, int d, int t, const float* X, const double* u, float* closest, double* pot,
                                  int64_t* chosen, void* stream) {
  IGCN_REQUIRE(km_sizes_ok(N, d, 1), "kmeanspp_step: N=%lld d=%d outside 1 <= N <= %d, 1 <= d <= %d", (long long)N, d,
               IGCN_KMEANS_MAX_N, IGCN_KMEANS_MAX_D);
  IGCN_REQUIRE(t >= 1 && t <= IGCN_KMEANSPP_MAX_TRIALS, "kmeanspp_step: t=%d outside 1..%d", t,
               IGCN_KMEANSPP_MAX_TRIALS);
  IGCN_REQUIRE(X && u && closest && pot && chosen, "kmeanspp_step: a NULL argument");
  hipLaunchKernelGGL(k_kmeanspp_step, dim3(1), dim3(KMPP_T), 0, (hipStream_t)stream, (int)N, d, t, X, u, closest, pot,
                     chosen);
  IGCN_CHECK_LAUNCH("kmeanspp_step");
  return IGCN_OK;
}
