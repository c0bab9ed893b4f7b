// What the narrow-output-layer kernels share (csrc/misc.hip: k_small_linear_fwd / _bwd; csrc/loss.hip: head_loss_body;
// csrc/cluster.hip: k_cluster_head_loss_fwd).  A narrow layer is y[r, c] = sum_k (x * keep)[r, k] W[c, k] + b[c] with
// C <= NH_MAXC outputs, computed by 256-thread workgroups with thread = (row, quad of K): kq = K / 4 lanes per row,
// 256 / kq rows per workgroup pass.  Plain inline functions over fixed-size register arrays (every class loop fully
// unrolled, c = 0..3, so the arrays stay in registers); every sum runs in one fixed order, and the one place where the
// compiler had a choice of rounding — the quad's a*b + c*d of nh_scores — is written out (see there).  A trainer's head
// kernel writes only what is its own: which loss terms exist, their weights and d loss / d scores.
#pragma once
#include "common.h"

#define NH_MAXC 4
// LDS of nh_wpart (and of nh_block_sums in front of it): [NH_MAXC][256 threads][4] weight-gradient quads, then
// [NH_MAXC][256] bias gradients
#define NH_RED_FLOATS (256 * 4 * NH_MAXC + 256 * NH_MAXC)

// THE support predicate of every kernel on this layout (one call per layer)
#define NH_OK_TEXT "K/4 a power of two <= 64 and 1 <= C <= 4 outputs per layer"
static inline bool narrow_head_ok(int K, int C) {
  const int kq = K / 4;
  return K > 0 && K % 4 == 0 && kq <= 64 && (kq & (kq - 1)) == 0 && C >= 1 && C <= NH_MAXC;
}
static inline int narrow_head_rows_per_pass(int K) { return 256 / (K / 4); }

// ---- geometry ---------------------------------------------------------------------------------------------------------
// kq is a power of two <= 64: 256 / kq is exact, so every thread has a row slot (rl < rpb always: no guard on it
// anywhere) and a row's kq lanes never straddle a wave.  The ONE liveness rule is row < rows.
struct NhGeom {
  int kq, q, rl, rpb;      // lanes per row, this thread's quad of K, its row slot in the pass, rows per pass
  int64_t row;             // blk * rpb + rl
};
__device__ __forceinline__ NhGeom nh_geom(int K, unsigned blk) {
  NhGeom g;
  g.kq = K / 4;
  g.q = threadIdx.x % g.kq;
  g.rl = threadIdx.x / g.kq;
  g.rpb = 256 / g.kq;
  g.row = (int64_t)blk * g.rpb + g.rl;
  return g;
}

// ---- loads --------------------------------------------------------------------------------------------------------------
// Loads only, no arithmetic: a kernel issues every load of its row (both layers' features and factors first, then
// their weight quads, then its labels) before the first use, so their latencies overlap.
// this thread's quad of row r and of its dropout factors (keep may be NULL: factors of one)
__device__ __forceinline__ void nh_load_x(const float* __restrict__ x, const float* __restrict__ keep, int64_t r, int K,
                                          int q, float4& xv, float4& kv) {
  xv = *reinterpret_cast<const float4*>(x + r * K + 4 * q);
  kv = make_float4(1.f, 1.f, 1.f, 1.f);
  if (keep) kv = *reinterpret_cast<const float4*>(keep + r * K + 4 * q);
}
// this thread's quad of W[c] for c < C, zeros otherwise
__device__ __forceinline__ void nh_load_w(const float* __restrict__ W, int K, int q, int C, float4 (&w)[NH_MAXC]) {
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c)
    w[c] = c < C ? *reinterpret_cast<const float4*>(W + c * K + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void nh_load(const float* __restrict__ x, const float* __restrict__ keep,
                                        const float* __restrict__ W, int64_t r, int K, int q, int C, float4& xv,
                                        float4& kv, float4 (&w)[NH_MAXC]) {
  nh_load_x(x, keep, r, K, q, xv, kv);
  nh_load_w(W, K, q, C, w);
}
// dropout of the input, fused: x * keep (what nh_scores and nh_back take as the layer's input)
__device__ __forceinline__ void nh_keep(float4& xv, const float4& kv) {
  xv.x *= kv.x; xv.y *= kv.y; xv.z *= kv.z; xv.w *= kv.w;
}

// ---- forward ------------------------------------------------------------------------------------------------------------
// s[c] = x . W[c] + b[c] in every lane of the row (c >= C: 0): the quad's products, the xor butterfly over the row's kq
// lanes — the four classes side by side in one loop: four independent shuffles in flight per step instead of four
// loops of dependent ones — then the bias (b may be NULL).  All kq lanes of a row call it together.
// The quad is (x.x w.x + x.y w.y) + (x.z w.z + x.w w.w) with one product of each pair rounded alone and the other fused
// onto it: ALONE1 / ALONE2 say that it is the FIRST product of the pair.  Left to the compiler's contraction this
// differed from call site to call site; each site names the order its kernel has always computed, so that results
// (and trained trajectories) stay what they were.
template <bool ALONE1, bool ALONE2>
__device__ __forceinline__ void nh_quad(const float4& xv, const float4 (&w)[NH_MAXC], float (&s)[NH_MAXC]) {
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c) {
    const float xy = ALONE1 ? fmaf(xv.y, w[c].y, xv.x * w[c].x) : fmaf(xv.x, w[c].x, xv.y * w[c].y);
    const float zw = ALONE2 ? fmaf(xv.w, w[c].w, xv.z * w[c].z) : fmaf(xv.z, w[c].z, xv.w * w[c].w);
    s[c] = xy + zw;
  }
}
__device__ __forceinline__ void nh_bias(const float* __restrict__ b, int C, float (&s)[NH_MAXC]) {
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c) s[c] += (c < C && b) ? b[c] : 0.f;
}
template <bool ALONE1, bool ALONE2>
__device__ __forceinline__ void nh_scores(const float4& xv, const float4 (&w)[NH_MAXC], const float* __restrict__ b, int C,
                                          int kq, float (&s)[NH_MAXC]) {
  nh_quad<ALONE1, ALONE2>(xv, w, s);
  for (int o = 1; o < kq; o <<= 1) {
#pragma unroll
    for (int c = 0; c < NH_MAXC; ++c) s[c] += __shfl_xor(s[c], o, 64);
  }
  nh_bias(b, C, s);
}
// Two layers over the same rows, as the two-head kernels have always issued them: class by class, the two layers'
// butterflies side by side in that class's loop.  (All eight chains in one loop is faster for such a kernel alone and
// slower for igcn_head_loss_gram_fwd, whose head workgroups share the chip with the Gram rows: DESIGN.md.)
template <bool A1, bool A2, bool B1, bool B2>
__device__ __forceinline__ void nh_scores2(const float4& x1, const float4 (&w1)[NH_MAXC], const float* __restrict__ b1, int C1,
                                           float (&s1)[NH_MAXC], const float4& x2, const float4 (&w2)[NH_MAXC],
                                           const float* __restrict__ b2, int C2, float (&s2)[NH_MAXC], int kq) {
  nh_quad<A1, A2>(x1, w1, s1);
  nh_quad<B1, B2>(x2, w2, s2);
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c)
    for (int o = 1; o < kq; o <<= 1) {
      s1[c] += __shfl_xor(s1[c], o, 64);
      s2[c] += __shfl_xor(s2[c], o, 64);
    }
  nh_bias(b1, C1, s1);
  nh_bias(b2, C2, s2);
}

// lp[c] = log_softmax(s[0..C))[c] = (s[c] - max) - log(sum exp(s - max)); lp[c >= C] is not to be used
__device__ __forceinline__ void nh_log_softmax(const float (&s)[NH_MAXC], int C, float (&lp)[NH_MAXC]) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c)
    if (c < C) m = fmaxf(m, s[c]);
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c)
    if (c < C) se += expf(s[c] - m);
  const float lse = logf(se);
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c) lp[c] = (s[c] - m) - lse;
}

// ---- backward of one row ------------------------------------------------------------------------------------------------
// From d[c] = d loss / d s[c] (zero for c >= C): dx[row] = (sum_c d[c] W[c]) * keep is stored, and the row's share of the
// weight / bias gradient, gw[c] = d[c] x and gb[c] = d[c], is left in registers for nh_wpart.
__device__ __forceinline__ void nh_back(const float (&d)[NH_MAXC], const float4 (&w)[NH_MAXC], const float4& xv,
                                        const float4& kv, float* __restrict__ dx_quad, float4 (&gw)[NH_MAXC],
                                        float (&gb)[NH_MAXC]) {
  float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c) {
    e.x += d[c] * w[c].x; e.y += d[c] * w[c].y; e.z += d[c] * w[c].z; e.w += d[c] * w[c].w;
    gw[c] = make_float4(d[c] * xv.x, d[c] * xv.y, d[c] * xv.z, d[c] * xv.w);
    gb[c] = d[c];
  }
  *reinterpret_cast<float4*>(dx_quad) = make_float4(e.x * kv.x, e.y * kv.y, e.z * kv.z, e.w * kv.w);
}
__device__ __forceinline__ void nh_zero(float4 (&gw)[NH_MAXC], float (&gb)[NH_MAXC]) {
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c) {
    gw[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    gb[c] = 0.f;
  }
}

// ---- block-level pieces -------------------------------------------------------------------------------------------------
// The reconstruction term of the block's rows of the stacked sweep: returns this thread's share of sum (x_hat - snps)^2
// (x_hat [rows, S] against snps [rows / 2, S] twice) and stores dxhat = weight * (x_hat - snps).
__device__ __forceinline__ float nh_recon(unsigned blk, int rpb, int rows, int S, const float* __restrict__ x_hat,
                                          const float* __restrict__ snps, float weight, float* __restrict__ dxhat) {
  const int64_t e0 = (int64_t)blk * rpb * S, e1 = min((int64_t)rows, (int64_t)(blk + 1) * rpb) * S;
  const int64_t half = (int64_t)(rows / 2) * S;
  float rec = 0.f;
  for (int64_t i = e0 + threadIdx.x; i < e1; i += 256) {
    const float d = x_hat[i] - snps[i < half ? i : i - half];
    rec += d * d;
    dxhat[i] = weight * d;
  }
  return rec;
}

// parts[blk][j] = the block's sum of v[j], j < N <= 5: wave_sum, four wave slots, (p0 + p1) + (p2 + p3).  Uses red[0, 4 N);
// ends with a barrier (red is free again).
template <int N>
__device__ __forceinline__ void nh_block_sums(float (&v)[N], float* red, float* __restrict__ parts, unsigned blk) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = wave_sum(v[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) red[4 * j + wv] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const float* p = red + 4 * threadIdx.x;
    parts[(int64_t)blk * N + threadIdx.x] = (p[0] + p[1]) + (p[2] + p[3]);
  }
  __syncthreads();
}

// One layer's C K + C floats of the block's partial row: prow[c K + k] = sum over the block's row slots l = 0..rpb-1, in
// that order, of gw[c] (column k), prow[C K + c] = the same sum of gb[c] — every channel staged at once in
// red[NH_RED_FLOATS] (one barrier pair, not one per channel), one thread per (channel, column) / per channel.  Ends with
// a barrier, so the next layer's call can follow directly.
__device__ __forceinline__ void nh_wpart(const NhGeom& g, int C, int K, const float4 (&gw)[NH_MAXC],
                                         const float (&gb)[NH_MAXC], float* red, float* __restrict__ prow) {
  float* redb = red + 256 * 4 * NH_MAXC;
#pragma unroll
  for (int c = 0; c < NH_MAXC; ++c) {      // (channels c >= C are staged too, unread: no branch per channel)
    float* rc = red + c * 1024;
    rc[threadIdx.x * 4 + 0] = gw[c].x; rc[threadIdx.x * 4 + 1] = gw[c].y;
    rc[threadIdx.x * 4 + 2] = gw[c].z; rc[threadIdx.x * 4 + 3] = gw[c].w;
    redb[c * 256 + threadIdx.x] = g.q == 0 ? gb[c] : 0.f;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < C * K; idx += 256) {
    const int c = idx / K, k = idx - c * K, qq = k / 4, j = k % 4;
    float t = 0.f;
    for (int l = 0; l < g.rpb; ++l) t += red[c * 1024 + (l * g.kq + qq) * 4 + j];
    prow[c * K + k] = t;
  }
  if (threadIdx.x < C) {
    float t = 0.f;
    for (int l = 0; l < g.rpb; ++l) t += redb[threadIdx.x * 256 + l * g.kq];
    prow[C * K + threadIdx.x] = t;
  }
  __syncthreads();
}
