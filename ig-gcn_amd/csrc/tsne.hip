// Exact t-SNE on the device, sklearn 1.7's method="exact" (manifold/_t_sne.py, manifold/_utils.pyx) restated:
//   util/image_cluster.py:148-282   TSNE(n_components=2, perplexity=40, init="pca", learning_rate="auto", method="exact")
//                                   of the normalised image features -> tsne_fdim, and through KMeans -> clust_y.
//
//   igcn_tsne_sqdist   D[i][j] = sum_f (x_if - x_jf)^2 by direct differences, fp32 fma chain in feature order: the bits of
//                      D[i][j] and D[j][i] are equal and the diagonal is exactly 0.
//   igcn_tsne_joint_p  _binary_search_perplexity + _joint_probabilities.  The search runs in fp64 like sklearn's (its
//                      tolerance of 1e-5 on an entropy of ~3.7 is a few fp32 roundings): one workgroup per row, the row's
//                      distances in LDS, at most 100 steps.  The conditional matrix is never stored: the second pass
//                      recomputes exp(-d_ij beta_i) / s_i and exp(-d_ji beta_j) / s_j (the same expressions, the same
//                      bits as in the search), divides by the total, clamps at double epsilon and rounds ONCE to fp32.
//                      The distances must be symmetric bit for bit, as igcn_tsne_sqdist's are: d_ji is read as d_ij.
//   igcn_tsne_grad     one pass over P per iteration, Y staged in LDS, one wave per row:
//                        attr_i = sum_j P_ij num_ij (y_i - y_j)   rep_i = sum_j num_ij^2 (y_i - y_j)   z_i = sum_{j != i} num_ij
//                      with num_ij = 1 / (1 + |y_i - y_j|^2) in fp32.  want_kl: a second kernel adds the row's share of
//                      sum_j P_ij log max(num_ij / Z, eps) in fp64 (it needs Z, so it follows the first; every 50th step).
//   igcn_tsne_update   one workgroup: Z in a fixed order, grad = 4 (e attr - rep / Z), sklearn's _gradient_descent step
//                      on (Y, update, gains) in place, and on check iterations the status record.
// No atomics, one writer per element, fixed-order reductions: the same bits every run.  S <= 4096
// (IGCN_TSNE_MAX_S), D <= 1024 (IGCN_TSNE_MAX_D).
#include "common.h"

#define TSNE_T 256              /* threads of every kernel here */
#define TSNE_EPS 2.220446049250313e-16   /* np.finfo(np.double).eps: sklearn's MACHINE_EPSILON */

__device__ __forceinline__ double wave_sum_all_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over a workgroup of TSNE_T threads, the same value in every thread; red: TSNE_T / 64 doubles of LDS.
__device__ __forceinline__ double block_sum_all_d(double v, double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = wave_sum_all_d(v);
  __syncthreads();                                       // protect `red` from a previous use
  if (lane == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < TSNE_T / 64; ++i) t += red[i];
  return t;
}

// ---- squared distances: a 16 x 16 tile of pairs per workgroup, 64 features per LDS chunk --------------------------
__global__ void __launch_bounds__(TSNE_T)
k_tsne_sqdist(int S, int D, const float* __restrict__ X, float* __restrict__ dist) {
  __shared__ float s_a[16][65], s_b[16][65];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  float acc = 0.f;
  for (int f0 = 0; f0 < D; f0 += 64) {
    const int nf = min(64, D - f0);
    for (int e = tid; e < 16 * 64; e += TSNE_T) {
      const int r = e >> 6, f = e & 63;
      s_a[r][f] = (i0 + r < S && f < nf) ? X[(int64_t)(i0 + r) * D + f0 + f] : 0.f;
      s_b[r][f] = (j0 + r < S && f < nf) ? X[(int64_t)(j0 + r) * D + f0 + f] : 0.f;
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const float d = s_a[ti][f] - s_b[tj][f];
      acc = fmaf(d, d, acc);
    }
    __syncthreads();
  }
  if (i0 + ti < S && j0 + tj < S) dist[(int64_t)(i0 + ti) * S + j0 + tj] = acc;
}

// ---- the perplexity search: one workgroup per row -------------------------------------------------------------------
__global__ void __launch_bounds__(TSNE_T)
k_tsne_beta(int S, double desired_entropy, const float* __restrict__ dist, double* __restrict__ betas,
            double* __restrict__ rownorm, double* __restrict__ rowtot) {
  __shared__ float s_d[IGCN_TSNE_MAX_S];
  __shared__ double s_red[2 * (TSNE_T / 64)];
  const int i = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < S; j += TSNE_T) s_d[j] = dist[(int64_t)i * S + j];
  __syncthreads();
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double beta = 1.0, beta_min = -inf, beta_max = inf, sp = 0.0, raw = 0.0;
  for (int l = 0; l < 100; ++l) {                         // every thread follows the same path: the sums are uniform
    double a = 0.0, b = 0.0;
    for (int j = tid; j < S; j += TSNE_T)
      if (j != i) {
        const double d = (double)s_d[j], p = exp(-d * beta);
        a += p;
        b += d * p;
      }
    raw = block_sum_all_d(a, s_red);
    const double sdp = block_sum_all_d(b, s_red + TSNE_T / 64);
    sp = raw == 0.0 ? 1e-8 : raw;
    const double diff = log(sp) + beta * (sdp / sp) - desired_entropy;
    if (fabs(diff) <= 1e-5 || l == 99) break;             // (after the last evaluation sklearn's P keeps THIS beta)
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == inf ? beta * 2.0 : (beta + beta_max) / 2.0;
    } else {
      beta_max = beta;
      beta = beta_min == -inf ? beta / 2.0 : (beta + beta_min) / 2.0;
    }
  }
  if (tid == 0) {
    betas[i] = beta;
    rownorm[i] = sp;
    rowtot[i] = raw / sp;                                 // the row's sum of conditional probabilities: 1, or 0 under the floor
  }
}

// out[0] = scale * sum of in[0..n) in a fixed order (one workgroup)
__global__ void __launch_bounds__(TSNE_T)
k_tsne_sum_d(const double* __restrict__ in, int n, double scale, double* __restrict__ out) {
  __shared__ double s_red[TSNE_T / 64];
  double a = 0.0;
  for (int j = threadIdx.x; j < n; j += TSNE_T) a += in[j];
  a = block_sum_all_d(a, s_red);
  if (threadIdx.x == 0) out[0] = scale * a;
}

__global__ void __launch_bounds__(TSNE_T)
k_tsne_psym(int S, const float* __restrict__ dist, const double* __restrict__ betas, const double* __restrict__ rownorm,
            const double* __restrict__ total, float* __restrict__ P, double* __restrict__ row_plogp,
            double* __restrict__ row_p) {
  __shared__ double s_red[2 * (TSNE_T / 64)];
  const int i = blockIdx.x, tid = threadIdx.x;
  const double bi = betas[i], si = rownorm[i], tot = fmax(total[0], TSNE_EPS);
  double a = 0.0, b = 0.0;
  for (int j = tid; j < S; j += TSNE_T) {
    float pf = 0.f;
    if (j != i) {
      const double dij = (double)dist[(int64_t)i * S + j];      // d_ji holds the same bits (a symmetric matrix is required):
      const double cij = exp(-dij * bi) / si;                  // row i serves both conditionals, with coalesced loads
      const double cji = exp(-dij * betas[j]) / rownorm[j];
      pf = (float)fmax((cij + cji) / tot, TSNE_EPS);
      a += (double)pf * log((double)pf);
      b += (double)pf;
    }
    P[(int64_t)i * S + j] = pf;
  }
  a = block_sum_all_d(a, s_red);
  b = block_sum_all_d(b, s_red + TSNE_T / 64);
  if (tid == 0) {
    row_plogp[i] = a;
    row_p[i] = b;
  }
}

// ---- the gradient pass ------------------------------------------------------------------------------------------------
// rowacc: [5][S] = attr_x, attr_y, rep_x, rep_y, z
__global__ void __launch_bounds__(TSNE_T)
k_tsne_grad(int S, const float* __restrict__ P, const float* __restrict__ Y, float* __restrict__ rowacc) {
  __shared__ float2 s_y[IGCN_TSNE_MAX_S];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int j = tid; j < S; j += TSNE_T) s_y[j] = reinterpret_cast<const float2*>(Y)[j];
  __syncthreads();
  const int i = blockIdx.x * (TSNE_T / 64) + (tid >> 6);
  if (i >= S) return;                                     // (wave-uniform; no barrier below)
  const float2 yi = s_y[i];
  const float* prow = P + (int64_t)i * S;
  float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, z = 0.f;
  for (int j = lane; j < S; j += 64) {
    const float2 yj = s_y[j];
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    const float num = 1.0f / (1.0f + fmaf(dy, dy, dx * dx));
    const float pn = prow[j] * num, n2 = num * num;
    ax = fmaf(pn, dx, ax);
    ay = fmaf(pn, dy, ay);
    rx = fmaf(n2, dx, rx);
    ry = fmaf(n2, dy, ry);
    if (j != i) z += num;
  }
  ax = wave_sum_all(ax);
  ay = wave_sum_all(ay);
  rx = wave_sum_all(rx);
  ry = wave_sum_all(ry);
  z = wave_sum_all(z);
  if (lane == 0) {
    rowacc[i] = ax;
    rowacc[S + i] = ay;
    rowacc[2 * S + i] = rx;
    rowacc[3 * S + i] = ry;
    rowacc[4 * S + i] = z;
  }
}

// Z from the rows' shares: ONE body for the KL pass and the update, so that both hold the same bits.  All TSNE_T threads
// of the workgroup call; red: 16 floats of LDS.
__device__ __forceinline__ float tsne_z(const float* __restrict__ zrow, int S, float* red) {
  float a = 0.f;
  for (int j = threadIdx.x; j < S; j += TSNE_T) a += zrow[j];
  return block_sum_all(a, red);
}

// klpart[i] = sum_{j != i} P_ij log max(num_ij / Z, eps), in fp64 from the fp32 embedding (the check iterations only)
__global__ void __launch_bounds__(TSNE_T)
k_tsne_kl(int S, const float* __restrict__ P, const float* __restrict__ Y, const float* __restrict__ rowacc,
          double* __restrict__ klpart) {
  __shared__ float2 s_y[IGCN_TSNE_MAX_S];
  __shared__ float s_red[16];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int j = tid; j < S; j += TSNE_T) s_y[j] = reinterpret_cast<const float2*>(Y)[j];
  const double Z = (double)tsne_z(rowacc + 4 * (int64_t)S, S, s_red);        // (barriers inside: s_y is complete after it)
  const int i = blockIdx.x * (TSNE_T / 64) + (tid >> 6);
  if (i >= S) return;
  const float2 yi = s_y[i];
  const float* prow = P + (int64_t)i * S;
  double a = 0.0;
  for (int j = lane; j < S; j += 64)
    if (j != i) {
      const float2 yj = s_y[j];
      const double dx = (double)yi.x - (double)yj.x, dy = (double)yi.y - (double)yj.y;
      const double q = fmax(1.0 / (1.0 + dx * dx + dy * dy) / Z, TSNE_EPS);
      a += (double)prow[j] * log(q);
    }
  a = wave_sum_all_d(a);
  if (lane == 0) klpart[i] = a;
}

// status: [0] KL divergence, [1] norm of the gains-scaled gradient (what sklearn's _gradient_descent tests), [2] Z,
// [3] the number of check iterations written so far
__global__ void __launch_bounds__(TSNE_T)
k_tsne_update(int S, float ex, float momentum, float lr, int check, const float* __restrict__ rowacc,
              const double* __restrict__ klpart, const double* __restrict__ pstats, float* __restrict__ Y,
              float* __restrict__ update, float* __restrict__ gains, float* __restrict__ grad_out,
              double* __restrict__ status) {
  __shared__ float s_red[16];
  __shared__ double s_redd[2 * (TSNE_T / 64)];
  const int tid = threadIdx.x;
  const float Z = tsne_z(rowacc + 4 * (int64_t)S, S, s_red);
  double sq = 0.0;
  for (int e = tid; e < 2 * S; e += TSNE_T) {
    const int i = e >> 1, d = e & 1;
    const float g = 4.0f * (ex * rowacc[d * S + i] - rowacc[(2 + d) * S + i] / Z);
    float u = update[e], gn = gains[e];
    gn = (u * g < 0.0f) ? gn + 0.2f : gn * 0.8f;
    gn = fmaxf(gn, 0.01f);
    const float gg = g * gn;
    u = momentum * u - lr * gg;
    update[e] = u;
    gains[e] = gn;
    Y[e] += u;
    if (grad_out) grad_out[e] = g;
    sq += (double)gg * (double)gg;
  }
  if (!check) return;                                     // (block-uniform)
  double kl = 0.0;
  for (int j = tid; j < S; j += TSNE_T) kl += klpart[j];
  sq = block_sum_all_d(sq, s_redd);
  kl = block_sum_all_d(kl, s_redd + TSNE_T / 64);
  if (tid == 0) {
    const double e = (double)ex;
    status[0] = e * (pstats[0] + log(e) * pstats[1]) - e * kl;
    status[1] = sqrt(sq);
    status[2] = (double)Z;
    status[3] += 1.0;
  }
}

static bool tsne_s_ok(int S) { return S >= IGCN_TSNE_MIN_S && S <= IGCN_TSNE_MAX_S; }

extern "C" int igcn_tsne_sqdist(int S, int D, const float* X, float* dist, void* stream) {
  IGCN_REQUIRE(tsne_s_ok(S) && D >= 1 && D <= IGCN_TSNE_MAX_D,
               "tsne_sqdist: S=%d D=%d outside %d <= S <= %d, 1 <= D <= %d", S, D, IGCN_TSNE_MIN_S, IGCN_TSNE_MAX_S,
               IGCN_TSNE_MAX_D);
  IGCN_REQUIRE(X && dist, "tsne_sqdist: a NULL matrix or output");
  const unsigned t = (unsigned)igcn_cdiv(S, 16);
  hipLaunchKernelGGL(k_tsne_sqdist, dim3(t, t), dim3(TSNE_T), 0, (hipStream_t)stream, S, D, X, dist);
  IGCN_CHECK_LAUNCH("tsne_sqdist");
  return IGCN_OK;
}

// rownorm [S] + rowtot [S] + total [1] + row_plogp [S] + row_p [S]
extern "C" size_t igcn_tsne_joint_p_scratch_doubles(int S) { return S < 1 ? 0 : 4 * (size_t)S + 1; }

extern "C" int igcn_tsne_joint_p(int S, double perplexity, const float* dist, float* P, double* betas, double* pstats,
                                 double* scratch, void* stream) {
  IGCN_REQUIRE(tsne_s_ok(S), "tsne_joint_p: S=%d outside %d <= S <= %d", S, IGCN_TSNE_MIN_S,
               IGCN_TSNE_MAX_S);
  IGCN_REQUIRE(perplexity > 0.0 && perplexity < (double)S, "tsne_joint_p: perplexity %g must lie in (0, S=%d)", perplexity, S);
  IGCN_REQUIRE(dist && P && betas && pstats && scratch, "tsne_joint_p: a NULL argument");
  hipStream_t st = (hipStream_t)stream;
  double *rownorm = scratch, *rowtot = scratch + S, *total = scratch + 2 * S, *row_plogp = total + 1, *row_p = row_plogp + S;
  hipLaunchKernelGGL(k_tsne_beta, dim3(S), dim3(TSNE_T), 0, st, S, log(perplexity), dist, betas, rownorm, rowtot);
  IGCN_CHECK_LAUNCH("tsne_joint_p (search)");
  hipLaunchKernelGGL(k_tsne_sum_d, dim3(1), dim3(TSNE_T), 0, st, rowtot, S, 2.0, total);   // sum(P + P^T)
  IGCN_CHECK_LAUNCH("tsne_joint_p (total)");
  hipLaunchKernelGGL(k_tsne_psym, dim3(S), dim3(TSNE_T), 0, st, S, dist, betas, rownorm, total, P, row_plogp, row_p);
  IGCN_CHECK_LAUNCH("tsne_joint_p (symmetrise)");
  hipLaunchKernelGGL(k_tsne_sum_d, dim3(1), dim3(TSNE_T), 0, st, row_plogp, S, 1.0, pstats);
  hipLaunchKernelGGL(k_tsne_sum_d, dim3(1), dim3(TSNE_T), 0, st, row_p, S, 1.0, pstats + 1);
  IGCN_CHECK_LAUNCH("tsne_joint_p (constants)");
  return IGCN_OK;
}

extern "C" int igcn_tsne_grad(int S, int want_kl, const float* P, const float* Y, float* rowacc, double* klpart,
                              void* stream) {
  IGCN_REQUIRE(tsne_s_ok(S), "tsne_grad: S=%d outside %d <= S <= %d", S, IGCN_TSNE_MIN_S,
               IGCN_TSNE_MAX_S);
  IGCN_REQUIRE(P && Y && rowacc && (!want_kl || klpart), "tsne_grad: a NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)igcn_cdiv(S, TSNE_T / 64);
  hipLaunchKernelGGL(k_tsne_grad, dim3(blocks), dim3(TSNE_T), 0, st, S, P, Y, rowacc);
  IGCN_CHECK_LAUNCH("tsne_grad");
  if (want_kl) {
    hipLaunchKernelGGL(k_tsne_kl, dim3(blocks), dim3(TSNE_T), 0, st, S, P, Y, rowacc, klpart);
    IGCN_CHECK_LAUNCH("tsne_grad (KL terms)");
  }
  return IGCN_OK;
}

extern "C" int igcn_tsne_update(int S, float exaggeration, float momentum, float lr, int check, const float* rowacc,
                                const double* klpart, const double* pstats, float* Y, float* update, float* gains,
                                float* grad_out, double* status, void* stream) {
  IGCN_REQUIRE(tsne_s_ok(S), "tsne_update: S=%d outside %d <= S <= %d", S, IGCN_TSNE_MIN_S,
               IGCN_TSNE_MAX_S);
  IGCN_REQUIRE(exaggeration >= 1.0f, "tsne_update: exaggeration %g below 1", (double)exaggeration);
  IGCN_REQUIRE(rowacc && Y && update && gains, "tsne_update: a NULL argument");
  IGCN_REQUIRE(!check || (klpart && pstats && status), "tsne_update: a check iteration needs klpart, pstats and status");
  hipLaunchKernelGGL(k_tsne_update, dim3(1), dim3(TSNE_T), 0, (hipStream_t)stream, S, exaggeration, momentum, lr, check,
                     rowacc, klpart, pstats, Y, update, gains, grad_out, status);
  IGCN_CHECK_LAUNCH("tsne_update");
  return IGCN_OK;
}
