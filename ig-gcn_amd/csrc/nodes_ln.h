// LayerNorm over a sample's nodes + activation + node dropout + level pooling (go_model.py:246-251, 273-275 and, with
// PReLU, guide_go_model.py): what every kernel of the block computes per element.  csrc/nodes_ln.hip holds the kernels
// and the exports, csrc/go.hip's ln_bwd_into_lds the backward folded into the LDS-resident layer backward.
//
//   xhat = (y - mean) rstd        u = xhat gamma + beta        z = act(u) keep             (nodes n >= pool only)
//   e = act'(u) (dz keep)         dxhat = e gamma              dy = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat))
//   d gamma = sum_rows e xhat     d beta = sum_rows e          d slope = sum (u > 0 ? 0 : u dz keep)
//
// The decision u > 0 selects which elements carry gradient: the forward makes it once and every backward form makes it
// again, so u has ONE spelling (ln_u: the product fused onto beta) and the decision one place (the activation policy).
// Every function here fixes its own rounding — contraction off, a fused multiply-add only where fmaf is written — and
// where the kernels have always differed the call site says which form it computes:
//
//   site                                     e xhat, dxhat xhat terms        dy                           masked dxhat
//   k_nodes_ln_bwd_dy (scalar)               alone (ln_dot)                  ln_dy<false>: xhat s2 alone  e gamma (-0 if gamma < 0)
//   k_nodes_ln_bwd_dy_v (16-byte)            alone (ln_dot4)                 ln_dy<true>: fused           ReLU: gamma first, so +0
//   k_nodes_ln_bwd_affine (scalar)           alone (ln_affine_acc<false>)
//   ln_bwd_affine_v_body (16-byte, multi)    fused (ln_affine_acc<true>)
//   ln_bwd_into_lds (go.hip)                 ln_dot4; ln_affine_acc<true>    ln_dy<true>                  e gamma
//
// The quad sums (ln_sum4, ln_dot4, ln_sqdev4) pair (x, y) and (z, w).
#pragma once
#include "common.h"

#define LN_T 256                // the scalar kernels, and the 16-byte ones for rows up to LN_T * 4 * LN_VPT nodes
#define LN_VPT 4                // float4 slots per thread of the 16-byte row kernels
#define LN_TMAX 1024            // their workgroup for longer rows (up to 16384 nodes: the 10 000-node hierarchy)
#define LN_RC 64                // rows per chunk of the affine pass: partial [chunk][2][N]

#define LN_DEV __device__ __forceinline__
#define LN_EXACT _Pragma("clang fp contract(off)")

// ---- activation policies ----------------------------------------------------------------------------------------------
// fwd(u); scale_up(u, up): the upstream gradient behind the activation.  kHasSlope: a learnt slope exists and
// dslope(u, up) is its gradient's term (no such member otherwise: ask the flag first).  kDispatch16: the launchers may
// take the 16-byte kernels.  kAffineRows: rows a thread of the scalar affine kernel keeps in flight (its unroll).
struct LnRelu {
  static constexpr bool kHasSlope = false, kDispatch16 = true;
  static constexpr int kAffineRows = 4;
  LN_DEV explicit LnRelu(const float*) {}
  LN_DEV float fwd(float u) const { return fmaxf(u, 0.f); }
  LN_DEV float scale_up(float u, float up) const { return u > 0.f ? up : 0.f; }
};
// nn.PReLU(): ONE slope a, read once from device memory (a captured step follows the optimiser).  GUIDE runs the scalar
// kernels at the schedule it was measured with: the 16-byte forms compile through this policy but are not dispatched.
struct LnPrelu {
  static constexpr bool kHasSlope = true, kDispatch16 = false;
  static constexpr int kAffineRows = 1;
  float a;
  LN_DEV explicit LnPrelu(const float* slope) : a(slope[0]) {}
  LN_DEV float fwd(float u) const { LN_EXACT return u > 0.f ? u : a * u; }
  LN_DEV float scale_up(float u, float up) const { LN_EXACT return u > 0.f ? up : a * up; }
  LN_DEV float dslope(float u, float up) const { LN_EXACT return u > 0.f ? 0.f : u * up; }
};

// ---- element functions ------------------------------------------------------------------------------------------------
LN_DEV float ln_xhat(float y, float mu, float rs) { LN_EXACT return (y - mu) * rs; }
LN_DEV float ln_u(float xh, float g, float be) { return fmaf(xh, g, be); }
// the masked upstream gradient e; up already carries the dropout factor (ln_keep)
template <class Act> LN_DEV float ln_up(const Act& act, float u, float up) { return act.scale_up(u, up); }
LN_DEV float ln_dxhat(float e, float g) { LN_EXACT return e * g; }
template <bool FUSED> LN_DEV float ln_dy(float rs, float dxh, float xh, float s1, float s2) {
  LN_EXACT const float t = dxh - s1;
  return rs * (FUSED ? fmaf(-xh, s2, t) : t - xh * s2);
}

LN_DEV float4 ln_xhat(const float4& y, float mu, float rs) {
  return make_float4(ln_xhat(y.x, mu, rs), ln_xhat(y.y, mu, rs), ln_xhat(y.z, mu, rs), ln_xhat(y.w, mu, rs));
}
LN_DEV float4 ln_u(const float4& xh, const float4& g, const float4& be) {
  return make_float4(ln_u(xh.x, g.x, be.x), ln_u(xh.y, g.y, be.y), ln_u(xh.z, g.z, be.z), ln_u(xh.w, g.w, be.w));
}
template <class Act> LN_DEV float4 ln_fwd(const Act& act, const float4& u) {
  return make_float4(act.fwd(u.x), act.fwd(u.y), act.fwd(u.z), act.fwd(u.w));
}
LN_DEV void ln_keep(float4& v, const float4& k) { v.x *= k.x; v.y *= k.y; v.z *= k.z; v.w *= k.w; }
template <class Act> LN_DEV float4 ln_up(const Act& act, const float4& u, const float4& up) {
  return make_float4(ln_up(act, u.x, up.x), ln_up(act, u.y, up.y), ln_up(act, u.z, up.z), ln_up(act, u.w, up.w));
}
LN_DEV float4 ln_dxhat(const float4& e, const float4& g) {
  return make_float4(ln_dxhat(e.x, g.x), ln_dxhat(e.y, g.y), ln_dxhat(e.z, g.z), ln_dxhat(e.w, g.w));
}
template <bool FUSED> LN_DEV float4 ln_dy(float rs, const float4& dxh, const float4& xh, float s1, float s2) {
  return make_float4(ln_dy<FUSED>(rs, dxh.x, xh.x, s1, s2), ln_dy<FUSED>(rs, dxh.y, xh.y, s1, s2),
                 ln_dy<FUSED>(rs, dxh.z, xh.z, s1, s2), ln_dy<FUSED>(rs, dxh.w, xh.w, s1, s2));
}
template <class Act> LN_DEV float ln_dslope(const Act& act, const float4& u, const float4& up) {
  return (act.dslope(u.x, up.x) + act.dslope(u.y, up.y)) + (act.dslope(u.z, up.z) + act.dslope(u.w, up.w));
}
// d gamma += e xhat — FUSED onto the sum, or the product rounded alone — and d beta += e
template <bool FUSED> LN_DEV void ln_affine_acc(float e, float xh, float& dg, float& db) {
  LN_EXACT dg = FUSED ? fmaf(e, xh, dg) : dg + e * xh;
  db += e;
}
template <bool FUSED> LN_DEV void ln_affine_acc(const float4& e, const float4& xh, float4& dg, float4& db) {
  ln_affine_acc<FUSED>(e.x, xh.x, dg.x, db.x);
  ln_affine_acc<FUSED>(e.y, xh.y, dg.y, db.y);
  ln_affine_acc<FUSED>(e.z, xh.z, dg.z, db.z);
  ln_affine_acc<FUSED>(e.w, xh.w, dg.w, db.w);
}
// one term of a row's sum of dxhat xhat, rounded alone (ln_dot4: a quad of them)
LN_DEV float ln_dot(float a, float b) { LN_EXACT return a * b; }
LN_DEV float ln_sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
LN_DEV float ln_dot4(const float4& a, const float4& b) { LN_EXACT return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
// sum of (v - mean)^2 over a quad: the second square of each pair rounded alone, the first fused onto it
LN_DEV float ln_sqdev4(const float4& v, float mean) {
  LN_EXACT const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
  return fmaf(a, a, b * b) + fmaf(c, c, d * d);
}

// ---- row geometry -----------------------------------------------------------------------------------------------------
// Which (sample, channel) row a workgroup of the 16-byte row kernels takes: XCD c the rows [c R/8, (c+1) R/8) in order, so
// that the f channel rows of a sample — which all read the sample's dropout factors keep[b, :] — meet in one L2
// (blockIdx.x taken as it comes puts them on f different XCDs).
LN_DEV int ln_row() {
  const int n = (int)gridDim.x, x = (int)blockIdx.x;
  return (n & 7) ? x : (x & 7) * (n >> 3) + (x >> 3);
}
static inline int ln_threads(int N) { return N <= LN_T * 4 * LN_VPT ? LN_T : LN_TMAX; }
// 16-byte accesses allowed: N and pool multiples of 4, a row fits the registers of one workgroup, aligned tensors
static inline bool ln_vec_ok(int N, int pool, const void* a, const void* b, const void* c, const void* d, const void* e,
                             const void* k) {
  auto al = [](const void* p) { return p == nullptr || ((uintptr_t)p % 16) == 0; };
  return N % 4 == 0 && pool % 4 == 0 && N <= LN_TMAX * 4 * LN_VPT && al(a) && al(b) && al(c) && al(d) && al(e) && al(k);
}

// ---- row statistics of the scalar forward ---------------------------------------------------------------------------
// mean and 1 / sqrt(var + eps) of yr[0..N) in every thread of an LN_T-thread workgroup: two strided passes, the squared
// deviation fused onto its sum; red >= 16 floats
LN_DEV void ln_row_stats(const float* __restrict__ yr, int N, float eps, float* red, float& mean, float& rstd) {
  float s = 0.f;
  for (int n = threadIdx.x; n < N; n += LN_T) s += yr[n];
  mean = block_sum_all(s, red) / (float)N;
  float v = 0.f;
  for (int n = threadIdx.x; n < N; n += LN_T) {
    const float d = yr[n] - mean;
    v = fmaf(d, d, v);
  }
  const float var = block_sum_all(v, red) / (float)N;
  rstd = 1.0f / sqrtf(var + eps);
}
