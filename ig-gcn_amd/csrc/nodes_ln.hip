// LayerNorm over nodes + activation + node dropout + pooling: the stand-alone kernels of csrc/nodes_ln.h's arithmetic
// and their exports.  One set of kernels, templated on the activation policy: LnRelu is the GO network's block
// (igcn_nodes_ln_*), LnPrelu GUIDE's (igcn_nodes_ln_prelu_*: w_act / w_act_out of guide_go_model.py; d slope is a FINAL
// reduction of per-row partials summed in a fixed order, so two identical steps give the same bits).  A ReLU launch
// passes slope = da_part = NULL and never reads them.
#include "nodes_ln.h"

// ---- forward -------------------------------------------------------------------------------------------------------
template <class Act>
__global__ void __launch_bounds__(LN_T)
k_nodes_ln_fwd(int f, int N, int pool, float eps, const float* __restrict__ y, const float* __restrict__ gamma,
               const float* __restrict__ beta, const float* __restrict__ keep, const float* __restrict__ slope,
               float* __restrict__ z, float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  __shared__ float red[16];
  const int row = blockIdx.x, b = row / f;  // row = b * f + c
  const float* yr = y + (int64_t)row * N;
  float mean, rstd;
  ln_row_stats(yr, N, eps, red, mean, rstd);
  if (threadIdx.x == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
  const Act act(slope);
  float* zr = z + (int64_t)row * (N - pool);
  for (int n = pool + threadIdx.x; n < N; n += LN_T) {
    float t = act.fwd(ln_u(ln_xhat(yr[n], mean, rstd), gamma[n], beta[n]));
    if (keep) t *= keep[(int64_t)b * N + n];
    zr[n - pool] = t;
  }
}

// Register-resident form: the row (N <= 16384 floats, N and pool multiples of 4) is read ONCE with 16-byte loads and kept
// in registers for the mean, the variance and the normalisation (the scalar kernel makes three passes).  256 threads for
// rows up to 4096 nodes, 1024 beyond.
template <class Act>
__global__ void __launch_bounds__(LN_TMAX)
k_nodes_ln_fwd_v(int f, int N, int pool, float eps, const float* __restrict__ y, const float* __restrict__ gamma,
                 const float* __restrict__ beta, const float* __restrict__ keep, const float* __restrict__ slope,
                 float* __restrict__ z, float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  __shared__ float red[16];
  const int row = ln_row(), b = row / f, nv = N / 4;
  const float* yr = y + (int64_t)row * N;
  float4 v[LN_VPT];
  // the affine parameters and the dropout factors of the thread's slots are requested with the row, in front of the two
  // block sums (asked for behind them, their round trip was the tail of every workgroup of a 2560-workgroup latency chain)
  float4 g4[LN_VPT], be4[LN_VPT], k4[LN_VPT];
#pragma unroll
  for (int i = 0; i < LN_VPT; ++i) {
    const int q = threadIdx.x + i * (int)blockDim.x, n = 4 * q;
    v[i] = q < nv ? ld4(yr + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    g4[i] = be4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    k4[i] = make_float4(1.f, 1.f, 1.f, 1.f);
    if (q < nv && n >= pool) {
      g4[i] = ld4(gamma + n);
      be4[i] = ld4(beta + n);
      if (keep) k4[i] = ld4(keep + (int64_t)b * N + n);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_VPT; ++i) s += ln_sum4(v[i]);
  const float mean = block_sum_all(s, red) / (float)N;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < LN_VPT; ++i)
    if (threadIdx.x + i * (int)blockDim.x < nv) var += ln_sqdev4(v[i], mean);
  var = block_sum_all(var, red) / (float)N;
  const float rstd = 1.0f / sqrtf(var + eps);
  if (threadIdx.x == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
  const Act act(slope);
  float* zr = z + (int64_t)row * (N - pool);
#pragma unroll
  for (int i = 0; i < LN_VPT; ++i) {
    const int q = threadIdx.x + i * (int)blockDim.x, n = 4 * q;
    if (q < nv && n >= pool) {
      float4 o = ln_fwd(act, ln_u(ln_xhat(v[i], mean, rstd), g4[i], be4[i]));
      if (keep) ln_keep(o, k4[i]);
      *reinterpret_cast<float4*>(zr + (n - pool)) = o;
    }
  }
}

// the kernel the shape and the tensors allow; true: the 16-byte one
template <class Act>
static bool ln_launch_fwd(int B, int f, int N, int pool, float eps, const float* y, const float* gamma, const float* beta,
                          const float* keep, const float* slope, float* z, float* mean, float* rstd, hipStream_t st) {
  if constexpr (Act::kDispatch16) {
    if (ln_vec_ok(N, pool, y, gamma, beta, z, nullptr, keep)) {
      hipLaunchKernelGGL(k_nodes_ln_fwd_v<Act>, dim3(B * f), dim3(ln_threads(N)), 0, st, f, N, pool, eps, y, gamma, beta,
                         keep, slope, z, mean, rstd);
      return true;
    }
  }
  hipLaunchKernelGGL(k_nodes_ln_fwd<Act>, dim3(B * f), dim3(LN_T), 0, st, f, N, pool, eps, y, gamma, beta, keep, slope, z,
                     mean, rstd);
  return false;
}

// ---- backward: dy of one (sample, channel) row — and, with a slope, that row's share of d slope ------------------
template <class Act>
__global__ void __launch_bounds__(LN_T)
k_nodes_ln_bwd_dy(int f, int N, int pool, const float* __restrict__ y, const float* __restrict__ gamma,
                  const float* __restrict__ beta, const float* __restrict__ keep, const float* __restrict__ slope,
                  const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ dz,
                  float* __restrict__ dy, float* __restrict__ da_part) {
  __shared__ float red[16];
  const int row = blockIdx.x, b = row / f, M = N - pool;
  const float mu = mean[row], rs = rstd[row];
  const Act act(slope);
  const float* yr = y + (int64_t)row * N;
  const float* dzr = dz + (int64_t)row * M;
  // xhat and dxhat of node n, computed by both passes (the row does not stay in registers); sa: the d slope terms
  auto element = [&](int n, float& xh, float* sa) {
    xh = ln_xhat(yr[n], mu, rs);
    float e = 0.f;
    if (n >= pool) {
      float up = dzr[n - pool];
      if (keep) up *= keep[(int64_t)b * N + n];
      const float u = ln_u(xh, gamma[n], beta[n]);
      e = ln_up(act, u, up);
      if constexpr (Act::kHasSlope)
        if (sa) *sa += act.dslope(u, up);
    }
    return ln_dxhat(e, gamma[n]);
  };
  float s1 = 0.f, s2 = 0.f, sa = 0.f;
  for (int n = threadIdx.x; n < N; n += LN_T) {
    float xh;
    const float dxh = element(n, xh, &sa);
    s1 += dxh;
    s2 += ln_dot(dxh, xh);
  }
  s1 = block_sum_all(s1, red) / (float)N;
  s2 = block_sum_all(s2, red) / (float)N;
  if constexpr (Act::kHasSlope) {
    sa = block_sum_all(sa, red);
    if (threadIdx.x == 0) da_part[row] = sa;
  }
  float* dyr = dy + (int64_t)row * N;
  for (int n = threadIdx.x; n < N; n += LN_T) {
    float xh;
    const float dxh = element(n, xh, nullptr);
    dyr[n] = ln_dy<false>(rs, dxh, xh, s1, s2);
  }
}

template <class Act>
__global__ void __launch_bounds__(LN_TMAX)
k_nodes_ln_bwd_dy_v(int f, int N, int pool, const float* __restrict__ y, const float* __restrict__ gamma,
                    const float* __restrict__ beta, const float* __restrict__ keep, const float* __restrict__ slope,
                    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ dz,
                    float* __restrict__ dy, float* __restrict__ da_part) {
  __shared__ float red[16];
  const int row = ln_row(), b = row / f, nv = N / 4;
  const float mu = mean[row], rs = rstd[row];
  const Act act(slope);
  const float* yr = y + (int64_t)row * N;
  const float* dzr = dz + (int64_t)row * (N - pool);
  float4 xh[LN_VPT], dx[LN_VPT];
  float s1 = 0.f, s2 = 0.f, sa = 0.f;
#pragma unroll
  for (int i = 0; i < LN_VPT; ++i) {
    const int q = threadIdx.x + i * (int)blockDim.x, n = 4 * q;
    xh[i] = dx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < nv) {
      const float4 g = ld4(gamma + n);
      xh[i] = ln_xhat(ld4(yr + n), mu, rs);
      if (n >= pool) {
        const float4 be = ld4(beta + n);
        float4 up = ld4(dzr + (n - pool));
        if (keep) ln_keep(up, ld4(keep + (int64_t)b * N + n));
        const float4 u = ln_u(xh[i], g, be);
        if constexpr (Act::kHasSlope) {
          dx[i] = ln_dxhat(ln_up(act, u, up), g);
          sa += ln_dslope(act, u, up);
        } else {
          dx[i] = ln_up(act, u, ln_dxhat(up, g));       // gamma first: a masked element is +0 whatever gamma's sign
        }
      }
      s1 += ln_sum4(dx[i]);
      s2 += ln_dot4(dx[i], xh[i]);
    }
  }
  s1 = block_sum_all(s1, red) / (float)N;
  s2 = block_sum_all(s2, red) / (float)N;
  if constexpr (Act::kHasSlope) {
    sa = block_sum_all(sa, red);
    if (threadIdx.x == 0) da_part[row] = sa;
  }
  float* dyr = dy + (int64_t)row * N;
#pragma unroll
  for (int i = 0; i < LN_VPT; ++i) {
    const int q = threadIdx.x + i * (int)blockDim.x;
    if (q < nv) *reinterpret_cast<float4*>(dyr + 4 * q) = ln_dy<true>(rs, dx[i], xh[i], s1, s2);
  }
}

template <class Act>
static void ln_launch_dy(int B, int f, int N, int pool, const float* y, const float* gamma, const float* beta,
                         const float* keep, const float* slope, const float* mean, const float* rstd, const float* dz,
                         float* dy, float* da_part, hipStream_t st) {
  if constexpr (Act::kDispatch16) {
    if (ln_vec_ok(N, pool, y, gamma, beta, dz, dy, keep)) {
      hipLaunchKernelGGL(k_nodes_ln_bwd_dy_v<Act>, dim3(B * f), dim3(ln_threads(N)), 0, st, f, N, pool, y, gamma, beta,
                         keep, slope, mean, rstd, dz, dy, da_part);
      return;
    }
  }
  hipLaunchKernelGGL(k_nodes_ln_bwd_dy<Act>, dim3(B * f), dim3(LN_T), 0, st, f, N, pool, y, gamma, beta, keep, slope, mean,
                     rstd, dz, dy, da_part);
}

// ---- backward: the affine gradients.  dgamma[n] = sum_rows e xhat, dbeta[n] = sum_rows e over a chunk of LN_RC rows;
// partial [chunk][2][N] is summed over chunks (in order) by the final reduction -------------------------------------
// One layer's problem: what the kernels take, what the host keeps per layer, and an entry of the flat grid's table
struct LnAffProb {
  int rows, f, N, pool, gx, wg0;       // gx: workgroups across the nodes; wg0: the layer's first workgroup in a flat grid
  const float *y, *gamma, *beta, *keep, *slope, *mean, *rstd, *dz;
  float* partial;
};

// Block = 64 node lanes x 4 row groups
template <class Act>
__global__ void __launch_bounds__(256) k_nodes_ln_bwd_affine(const LnAffProb p) {
  __shared__ float sg[4][64], sb[4][64];
  const int nl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + nl, N = p.N;
  const int r0 = blockIdx.y * LN_RC, r1 = min(p.rows, r0 + LN_RC);
  float dg = 0.f, db = 0.f;
  if (n < N && n >= p.pool) {
    const float ga = p.gamma[n], be = p.beta[n];
    const Act act(p.slope);
    const int M = N - p.pool;
#pragma unroll Act::kAffineRows
    for (int row = r0 + rg; row < r1; row += 4) {      // unconditional, independent loads: several rows in flight
      const float yv = p.y[(int64_t)row * N + n];
      float up = p.dz[(int64_t)row * M + (n - p.pool)];
      if (p.keep) up *= p.keep[(int64_t)(row / p.f) * N + n];
      const float xh = ln_xhat(yv, p.mean[row], p.rstd[row]);
      ln_affine_acc<false>(ln_up(act, ln_u(xh, ga, be), up), xh, dg, db);
    }
  }
  sg[rg][nl] = dg;
  sb[rg][nl] = db;
  __syncthreads();
  if (rg == 0 && n < N) {
    float* prow = p.partial + (int64_t)blockIdx.y * 2 * N;
    prow[n] = (sg[0][nl] + sg[1][nl]) + (sg[2][nl] + sg[3][nl]);
    prow[N + n] = (sb[0][nl] + sb[1][nl]) + (sb[2][nl] + sb[3][nl]);
  }
}

// 16-bytes-per-lane form (N, pool multiples of 4, aligned rows): thread = (quad of nodes, row lane); one float4 of y,
// dz and keep per row instead of four scalar loads each.  Same chunk layout of the partials.  (bx, by): the workgroup's
// place across the nodes and the row chunks.
template <class Act>
LN_DEV void ln_bwd_affine_v_body(const int bx, const int by, const LnAffProb& p) {
  __shared__ float4 sg[16][16], sb[16][16];
  const int nq = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int n = (bx * 16 + nq) * 4, N = p.N;
  const int r0 = by * LN_RC, r1 = min(p.rows, r0 + LN_RC);
  float4 dg = make_float4(0.f, 0.f, 0.f, 0.f), db = dg;
  if (n < N && n >= p.pool) {
    const float4 ga = ld4(p.gamma + n), be = ld4(p.beta + n);
    const Act act(p.slope);
    const int M = N - p.pool;
#pragma unroll 4
    for (int row = r0 + rg; row < r1; row += 16) {
      const float4 yv = ld4(p.y + (int64_t)row * N + n);
      float4 up = ld4(p.dz + (int64_t)row * M + (n - p.pool));
      if (p.keep) ln_keep(up, ld4(p.keep + (int64_t)(row / p.f) * N + n));
      const float4 xh = ln_xhat(yv, p.mean[row], p.rstd[row]);
      ln_affine_acc<true>(ln_up(act, ln_u(xh, ga, be), up), xh, dg, db);
    }
  }
  sg[rg][nq] = dg;
  sb[rg][nq] = db;
  __syncthreads();
  if (rg == 0 && n < N) {
    float4 tg = make_float4(0.f, 0.f, 0.f, 0.f), tb = tg;
#pragma unroll
    for (int r = 0; r < 16; ++r) {                     // row lanes summed in order
      const float4 a = sg[r][nq], c = sb[r][nq];
      tg.x += a.x; tg.y += a.y; tg.z += a.z; tg.w += a.w;
      tb.x += c.x; tb.y += c.y; tb.z += c.z; tb.w += c.w;
    }
    float* prow = p.partial + (int64_t)by * 2 * N;
    *reinterpret_cast<float4*>(prow + n) = tg;
    *reinterpret_cast<float4*>(prow + N + n) = tb;
  }
}

template <class Act>
__global__ void __launch_bounds__(256) k_nodes_ln_bwd_affine_v(const LnAffProb p) {
  ln_bwd_affine_v_body<Act>((int)blockIdx.x, (int)blockIdx.y, p);
}

// The affine-gradient passes of SEVERAL LayerNorm layers in one flat grid: d gamma / d beta are parameter gradients —
// nothing in the backward reads them — so the passes of a whole backward can wait for its end and share one launch
// (four grids of 150-750 workgroups each, which otherwise run one after the other between the layers' dX kernels).
#define LN_AFF_MAX 4
struct LnAffGroup { int n; LnAffProb p[LN_AFF_MAX]; };
__global__ void __launch_bounds__(256) k_nodes_ln_bwd_affine_multi(const LnAffGroup G) {
  int pi = 0;
#pragma unroll
  for (int i = 1; i < LN_AFF_MAX; ++i)
    if (i < G.n && (int)blockIdx.x >= G.p[i].wg0) pi = i;
  const LnAffProb& p = G.p[pi];
  const int l = (int)blockIdx.x - p.wg0;
  ln_bwd_affine_v_body<LnRelu>(l % p.gx, l / p.gx, p);
}

static inline int64_t ln_chunks(int64_t rows) { return igcn_cdiv(rows, LN_RC); }
static LnAffProb ln_aff_prob(int B, int f, int N, int pool, const float* y, const float* gamma, const float* beta,
                             const float* keep, const float* slope, const float* mean, const float* rstd,
                             const float* dz, float* scratch) {
  LnAffProb p = {};
  p.rows = B * f; p.f = f; p.N = N; p.pool = pool; p.gx = (int)igcn_cdiv(N, 64);
  p.y = y; p.gamma = gamma; p.beta = beta; p.keep = keep; p.slope = slope; p.mean = mean; p.rstd = rstd; p.dz = dz;
  p.partial = scratch;
  return p;
}

// LN_AFF_GROUPED: nothing launched — the layer allows 16-byte accesses and the caller (group = true) puts it into a flat
// grid of its own.  LN_AFF_LAUNCHED: the layer's own launch is queued.
enum LnAffine { LN_AFF_LAUNCHED, LN_AFF_GROUPED };
template <class Act>
static LnAffine ln_launch_affine(const LnAffProb& p, bool group, hipStream_t st) {
  const dim3 grid((unsigned)p.gx, (unsigned)ln_chunks(p.rows));
  if constexpr (Act::kDispatch16) {
    if (ln_vec_ok(p.N, p.pool, p.y, p.gamma, p.beta, p.dz, p.partial, p.keep)) {
      if (group) return LN_AFF_GROUPED;
      hipLaunchKernelGGL(k_nodes_ln_bwd_affine_v<Act>, grid, dim3(256), 0, st, p);
      return LN_AFF_LAUNCHED;
    }
  }
  hipLaunchKernelGGL(k_nodes_ln_bwd_affine<Act>, grid, dim3(256), 0, st, p);
  return LN_AFF_LAUNCHED;
}

// ---- exports -------------------------------------------------------------------------------------------------------
extern "C" int igcn_nodes_ln_fwd(int B, int f, int N, int pool, float eps, const float* y, const float* gamma,
                                 const float* beta, const float* keep, float* z, float* mean, float* rstd,
                                 void* stream) {
  IGCN_REQUIRE(B > 0 && f > 0 && N > 0 && pool >= 0 && pool < N, "nodes_ln_fwd: bad sizes");
  const bool vec = ln_launch_fwd<LnRelu>(B, f, N, pool, eps, y, gamma, beta, keep, nullptr, z, mean, rstd,
                                         (hipStream_t)stream);
  IGCN_CHECK_LAUNCH(vec ? "nodes_ln_fwd_v" : "nodes_ln_fwd");
  return IGCN_OK;
}

extern "C" int igcn_nodes_ln_prelu_fwd(int B, int f, int N, int pool, float eps, const float* y, const float* gamma,
                                       const float* beta, const float* keep, const float* slope, float* z, float* mean,
                                       float* rstd, void* stream) {
  IGCN_REQUIRE(B > 0 && f > 0 && N > 0 && pool >= 0 && pool < N && slope, "nodes_ln_prelu_fwd: bad sizes");
  ln_launch_fwd<LnPrelu>(B, f, N, pool, eps, y, gamma, beta, keep, slope, z, mean, rstd, (hipStream_t)stream);
  IGCN_CHECK_LAUNCH("nodes_ln_prelu_fwd");
  return IGCN_OK;
}

// scratch: the chunk partials [chunks][2][N]; with a slope, the rows' d slope shares [B f] behind them
extern "C" size_t igcn_nodes_ln_bwd_scratch_floats(int B, int f, int N) {
  return (size_t)(ln_chunks((int64_t)B * f) * 2 * N + 64);
}
extern "C" size_t igcn_nodes_ln_prelu_bwd_scratch_floats(int B, int f, int N) {
  return (size_t)(ln_chunks((int64_t)B * f) * 2 * N + (int64_t)B * f + 64);
}

extern "C" int igcn_nodes_ln_bwd(int B, int f, int N, int pool, const float* y, const float* gamma,
                                 const float* beta, const float* keep, const float* mean, const float* rstd,
                                 const float* dz, float* dy, float* dgb /*[2,N]: dgamma then dbeta*/,
                                 float* scratch, void* stream) {
  IGCN_REQUIRE(B > 0 && f > 0 && N > 0 && pool >= 0 && pool < N, "nodes_ln_bwd: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  ln_launch_dy<LnRelu>(B, f, N, pool, y, gamma, beta, keep, nullptr, mean, rstd, dz, dy, nullptr, st);
  ln_launch_affine<LnRelu>(ln_aff_prob(B, f, N, pool, y, gamma, beta, keep, nullptr, mean, rstd, dz, scratch), false, st);
  IGCN_CHECK_LAUNCH("nodes_ln_bwd");
  return igcn_launch_reduce_rows_final(scratch, ln_chunks((int64_t)B * f), 2 * (int64_t)N, 2 * N, dgb, st);
}

extern "C" int igcn_nodes_ln_prelu_bwd(int B, int f, int N, int pool, const float* y, const float* gamma,
                                       const float* beta, const float* keep, const float* slope, const float* mean,
                                       const float* rstd, const float* dz, float* dy, float* dgb, float* dslope,
                                       float* scratch, void* stream) {
  IGCN_REQUIRE(B > 0 && f > 0 && N > 0 && pool >= 0 && pool < N && slope && dslope, "nodes_ln_prelu_bwd: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * f, chunks = ln_chunks(rows);
  float* da_part = scratch + chunks * 2 * N;
  ln_launch_dy<LnPrelu>(B, f, N, pool, y, gamma, beta, keep, slope, mean, rstd, dz, dy, da_part, st);
  ln_launch_affine<LnPrelu>(ln_aff_prob(B, f, N, pool, y, gamma, beta, keep, slope, mean, rstd, dz, scratch), false, st);
  IGCN_CHECK_LAUNCH("nodes_ln_prelu_bwd");
  const int rc = igcn_launch_reduce_rows_final(scratch, chunks, 2 * (int64_t)N, 2 * N, dgb, st);
  if (rc) return rc;
  return igcn_launch_reduce_rows_final(da_part, rows, 1, 1, dslope, st);
}

// The backward in two calls: igcn_nodes_ln_bwd_dy now, and the affine gradients of up to LN_AFF_MAX layers later in one
// launch (igcn_nodes_ln_bwd_affine_multi) — see k_nodes_ln_bwd_affine_multi.
extern "C" int igcn_nodes_ln_bwd_dy(int B, int f, int N, int pool, const float* y, const float* gamma,
                                    const float* beta, const float* keep, const float* mean, const float* rstd,
                                    const float* dz, float* dy, void* stream) {
  IGCN_REQUIRE(B > 0 && f > 0 && N > 0 && pool >= 0 && pool < N, "nodes_ln_bwd_dy: bad sizes");
  ln_launch_dy<LnRelu>(B, f, N, pool, y, gamma, beta, keep, nullptr, mean, rstd, dz, dy, nullptr, (hipStream_t)stream);
  IGCN_CHECK_LAUNCH("nodes_ln_bwd_dy");
  return IGCN_OK;
}

// table [n][13] int64 = {B, f, N, pool, y, gamma, beta, keep, mean, rstd, dz, scratch, dgb} per layer (pointers as
// integers; scratch of igcn_nodes_ln_bwd_scratch_floats, dgb [2,N]).  Layers whose tensors do not allow 16-byte
// accesses get their own launch of the scalar kernel.
extern "C" int igcn_nodes_ln_bwd_affine_multi(int n, const int64_t* table, void* stream) {
  IGCN_REQUIRE(n >= 1 && n <= LN_AFF_MAX && table != nullptr, "nodes_ln_bwd_affine_multi: 1..%d layers", LN_AFF_MAX);
  hipStream_t st = (hipStream_t)stream;
  LnAffGroup G = {};
  int wgs = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t* t = table + 13 * i;
    const int B = (int)t[0], f = (int)t[1], N = (int)t[2], pool = (int)t[3];
    IGCN_REQUIRE(B > 0 && f > 0 && N > 0 && pool >= 0 && pool < N && t[11] != 0,
                 "nodes_ln_bwd_affine_multi: bad layer %d", i);
    const LnAffProb p = ln_aff_prob(B, f, N, pool, (const float*)t[4], (const float*)t[5], (const float*)t[6],
                                    (const float*)t[7], nullptr, (const float*)t[8], (const float*)t[9],
                                    (const float*)t[10], (float*)t[11]);
    if (ln_launch_affine<LnRelu>(p, true, st) == LN_AFF_LAUNCHED) continue;
    LnAffProb& q = G.p[G.n++] = p;
    q.wg0 = wgs;
    wgs += q.gx * (int)ln_chunks(q.rows);
  }
  if (G.n > 0) {
    for (int i = G.n; i < LN_AFF_MAX; ++i) G.p[i] = G.p[0];
    hipLaunchKernelGGL(k_nodes_ln_bwd_affine_multi, dim3((unsigned)wgs), dim3(256), 0, st, G);
  }
  IGCN_CHECK_LAUNCH("nodes_ln_bwd_affine_multi");
  for (int i = 0; i < n; ++i) {
    const int64_t* t = table + 13 * i;
    const int N = (int)t[2];
    const int rc = igcn_launch_reduce_rows_final((float*)t[11], ln_chunks(t[0] * t[1]), 2 * (int64_t)N, 2 * N,
                                                 (float*)t[12], st);
    if (rc) return rc;
  }
  return IGCN_OK;
}
