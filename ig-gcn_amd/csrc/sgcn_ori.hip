// SGCN_Ori's graph stack (kernel/sgcn.py:111-138), LDS-resident: gcn_norm once, h1 = relu(GCNConv1(x)) [R, F1],
// acts = GCNConv3(h1) [R, F3] WITHOUT ReLU (the Grad-CAM tap, final_conv_acts), h3 = relu(acts), and the head's input
// row z = [h1 node-major | h3 node-major] written in place — ONE kernel per direction, one 512-thread workgroup per graph,
// the phase structure of the uniform stack (csrc/sgcn_fused.hip, whose thread count was measured there) with two layers
// of DIFFERENT width.  The staged graph, gcn_norm and the list walks of a layer are csrc/gcn_lds.h, shared with it.
//
// What differs from igcn_sgcn_stack_*: the two widths (3 -> 32 -> 5 by default) are independent and need not sit on
// the 4 / 8 / 16 / 32 grid — inside LDS each is rounded up to a multiple of 4 (P1, P3: every access moves 16 bytes;
// padded weight rows / columns and bias entries are 0, so padded activation columns are exactly 0), HBM only ever sees
// the true widths; the last layer leaves the kernel before AND after ReLU; the backward returns the gradient at the
// tap (final_conv_grads) beside dx, d(edge weight) and the per-graph parameter-gradient row.
//
// Same preconditions as the uniform stack: block-diagonal batch of uniform graphs on the per-graph plan; sums run in
// the plan's stable by-target / by-source order, no atomics, deterministic.
#include "common.h"
#include "gcn_lds.h"

#define SO_T 512
#define SO_DB_PARTS 8         // thread groups that share the node range of a bias gradient

struct SoLayout {
  GraphLds t;                                                               // the staged graph
  GcnNormLds n;                                                             // gcn_norm: coefficients, lists, backward
  int w1t, b1, w3t, b3;                                                     // W1^T [H0][P1] | b1 [P1] | W3^T [P1][P3] | b3
  int h1, y1, h3, a;                                                        // transforms and layer outputs
  int w3, dy1, dy3, dh, dx0, redb, redw, prow;                              // backward
  int total;
};

__host__ __device__ inline int so_pad(int f) { return (f + 3) & ~3; }

// parameter-gradient row of one graph: dW1 [F1, H0] | db1 [F1] | dW3 [F3, F1] | db3 [F3]
__host__ __device__ inline int so_param_floats(int H0, int F1, int F3) { return F1 * H0 + F1 + F3 * F1 + F3; }

__host__ __device__ inline SoLayout so_layout(int R, int Emax, int H0, int F1, int F3, int backward) {
  SoLayout o;
  int p = 0;
  auto take = [&](int n) { int q = p; p += (n + 3) & ~3; return q; };
  const int P1 = so_pad(F1), P3 = so_pad(F3), PM = P1 > P3 ? P1 : P3;
  graph_lds_layout(o.t, R, Emax, H0, take);
  gcn_norm_layout(o.n, R, Emax, take);
  o.w1t = take(H0 * P1);
  o.b1 = take(P1);
  o.w3t = take(P1 * P3);
  o.b3 = take(P3);
  // the forward keeps one transform at a time (h1 and h3 share a buffer); the backward keeps both
  o.h1 = take(R * (backward ? P1 : PM));
  o.h3 = backward ? take(R * P3) : o.h1;
  o.y1 = take(R * P1);
  o.a = take(R * P3);
  o.w3 = o.dy1 = o.dy3 = o.dh = o.dx0 = o.redb = o.redw = o.prow = 0;
  if (backward) {
    graph_lds_layout_bwd(o.t, R, Emax, take);
    o.w3 = take(P3 * P1);                          // W3 [fo][fi] as stored (padded): dX1 = dH3 W3
    o.dy1 = take(R * P1);                          // d z's h1 block, then G1 in place, then v1
    o.dy3 = take(R * P3);                          // d z's h3 block, then G3 = the gradient at the tap in place
    o.dh = take(R * PM);
    o.dx0 = take(R * H0);
    o.redb = take(SO_DB_PARTS * IGCN_STACK_MAX_WIDTH);
    o.redw = take(2 * SO_T);                       // dW partials: parts * outputs <= 2 * SO_T (so_dw_parts)
    o.prow = take(so_param_floats(H0, F1, F3));
    // gcn_norm backward's per-position products go into G1 / the first transform, dead by then, when they fit
    const bool fits = Emax <= R * P1;
    gcn_norm_layout_bwd(o.n, R, Emax, fits ? o.dy1 : -1, fits ? o.h1 : -1, take);
  }
  o.total = p;
  return o;
}

extern "C" size_t igcn_sgcn_ori_lds_bytes(int R, int max_edges, int H0, int F1, int F3, int backward) {
  return (size_t)so_layout(R, max_edges, H0, F1, F3, backward).total * 4;
}

extern "C" int igcn_sgcn_ori_param_floats(int H0, int F1, int F3) { return so_param_floats(H0, F1, F3); }

struct SoArgs {
  int R, Emax, H0, F1, F3;
  const float *x_in, *ew_in;
  const int32_t *src32, *dst32, *tgt_ptr, *tgt_perm, *src_ptr, *src_perm, *loop_edge;
  const float *W1, *b1, *W3, *b3;
  int32_t* status;
};

// Stage the graph (graph_lds_load) and the weights, then gcn_norm and the by-target (backward: also by-source) lists
// (gcn_lists).  Returns the edge count or -1 (status bit 1) for a refused graph.  Ends WITHOUT a barrier behind the
// last list phase.
template <bool BWD>
__device__ __forceinline__ int so_stage(float* lds, const SoLayout& o, const SoArgs& a, int64_t nb, int32_t& eb) {
  const int tid = threadIdx.x, R = a.R, H0 = a.H0, F1 = a.F1, F3 = a.F3;
  const int P1 = so_pad(F1), P3 = so_pad(F3);
  const int ne = graph_lds_load<BWD>(lds, o.t, R, a.Emax, H0, nb, a.x_in, a.ew_in, a.src32, a.dst32, a.tgt_ptr,
                                     a.tgt_perm, a.src_ptr, a.src_perm, a.status, eb, SO_T);
  if (ne < 0) return -1;
  for (int i = tid; i < R; i += SO_T) lds_i32(lds, o.n.loop)[i] = a.loop_edge[nb + i];
  // weights, transposed and padded: W1t[fi][fo] (fo < P1), W3t[fi][fo] (fi < P1, fo < P3); padding = 0
  for (int j = tid; j < H0 * P1; j += SO_T) {
    const int fi = j / P1, fo = j - fi * P1;
    lds[o.w1t + j] = fo < F1 ? a.W1[fo * H0 + fi] : 0.f;
  }
  for (int j = tid; j < P1; j += SO_T) lds[o.b1 + j] = j < F1 ? a.b1[j] : 0.f;
  for (int j = tid; j < P1 * P3; j += SO_T) {
    const int fi = j / P3, fo = j - fi * P3;
    const float v = (fi < F1 && fo < F3) ? a.W3[fo * F1 + fi] : 0.f;
    lds[o.w3t + j] = v;
    if (BWD) lds[o.w3 + fo * P1 + fi] = v;
  }
  for (int j = tid; j < P3; j += SO_T) lds[o.b3 + j] = j < F3 ? a.b3[j] : 0.f;
  __syncthreads();
  gcn_lists<BWD>(lds, o.t, o.n, R, ne, eb, SO_T);
  return ne;
}

// H = X Wt (X [R, fin] with row stride ldx; Wt [fin][P]), work item = (node, output quad).  QUADS: fin is a multiple
// of 4 and the rows of X are read 16 bytes at a time.  No barrier inside.
template <bool QUADS>
__device__ __forceinline__ void so_transform(int R, int fin, const float* X, int ldx, const float* Wt, int P, float* H) {
  const int PQ = P >> 2;
  for (int e = threadIdx.x; e < R * PQ; e += SO_T) {
    const int i = e / PQ, q = e - i * PQ;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (QUADS) {
      for (int f4 = 0; f4 < fin; f4 += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(X + i * ldx + f4);
        const float4 w0 = *reinterpret_cast<const float4*>(Wt + (f4 + 0) * P + q * 4);
        const float4 w1 = *reinterpret_cast<const float4*>(Wt + (f4 + 1) * P + q * 4);
        const float4 w2 = *reinterpret_cast<const float4*>(Wt + (f4 + 2) * P + q * 4);
        const float4 w3 = *reinterpret_cast<const float4*>(Wt + (f4 + 3) * P + q * 4);
        acc.x += xv.x * w0.x; acc.y += xv.x * w0.y; acc.z += xv.x * w0.z; acc.w += xv.x * w0.w;
        acc.x += xv.y * w1.x; acc.y += xv.y * w1.y; acc.z += xv.y * w1.z; acc.w += xv.y * w1.w;
        acc.x += xv.z * w2.x; acc.y += xv.z * w2.y; acc.z += xv.z * w2.z; acc.w += xv.z * w2.w;
        acc.x += xv.w * w3.x; acc.y += xv.w * w3.y; acc.z += xv.w * w3.z; acc.w += xv.w * w3.w;
      }
    } else {
#pragma unroll
      for (int fi = 0; fi < IGCN_MAX_H0; ++fi)
        if (fi < fin) {
          const float xv = X[i * ldx + fi];
          const float4 w4 = *reinterpret_cast<const float4*>(Wt + fi * P + q * 4);
          acc.x += xv * w4.x; acc.y += xv * w4.y; acc.z += xv * w4.z; acc.w += xv * w4.w;
        }
    }
    *reinterpret_cast<float4*>(H + i * P + q * 4) = acc;
  }
}

// Y = act(A_hat H + b): the by-target walk in stored (reference) order, + self loop, + bias.  No barrier inside.
template <bool RELU>
__device__ __forceinline__ void so_aggregate(const float* lds, const SoLayout& o, int R, int P, const float* H,
                                             const float* bt, float* Y) {
  const int32_t* stptr = lds_i32(lds, o.t.tptr);
  const int32_t* stsrc = lds_i32(lds, o.n.tsrc);
  const int PQ = P >> 2;
  for (int e = threadIdx.x; e < R * PQ; e += SO_T) {
    const int i = e / PQ, q = e - i * PQ;
    float4 acc = gcn_walk4(stsrc, lds + o.n.twhat, stptr[i], stptr[i + 1], H, P, q);
    const float wl = lds[o.n.wloop + i];
    const float4 hs = *reinterpret_cast<const float4*>(H + i * P + q * 4);
    const float4 b4 = *reinterpret_cast<const float4*>(bt + q * 4);
    acc.x = acc.x + wl * hs.x + b4.x; acc.y = acc.y + wl * hs.y + b4.y;
    acc.z = acc.z + wl * hs.z + b4.z; acc.w = acc.w + wl * hs.w + b4.w;
    if (RELU) {
      acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
    }
    *reinterpret_cast<float4*>(Y + i * P + q * 4) = acc;
  }
}

// both layers out of LDS into LDS; ends behind a barrier
__device__ __forceinline__ void so_forward(float* lds, const SoLayout& o, int R, int H0, int P1, int P3) {
  so_transform<false>(R, H0, lds + o.t.x, H0, lds + o.w1t, P1, lds + o.h1);
  __syncthreads();                                 // (also orders the lists of so_stage before their first use)
  so_aggregate<true>(lds, o, R, P1, lds + o.h1, lds + o.b1, lds + o.y1);
  __syncthreads();
  so_transform<true>(R, P1, lds + o.y1, P1, lds + o.w3t, P3, lds + o.h3);
  __syncthreads();
  so_aggregate<false>(lds, o, R, P3, lds + o.h3, lds + o.b3, lds + o.a);
  __syncthreads();
}

__global__ void __launch_bounds__(SO_T)
k_sgcn_ori_fwd(const SoArgs a, float* __restrict__ z, float* __restrict__ acts) {
  extern __shared__ float so_lds[];
  const SoLayout o = so_layout(a.R, a.Emax, a.H0, a.F1, a.F3, 0);
  const int R = a.R, F1 = a.F1, F3 = a.F3, P1 = so_pad(F1), P3 = so_pad(F3);
  const int64_t nb = (int64_t)blockIdx.x * R;
  int32_t eb;
  if (so_stage<false>(so_lds, o, a, nb, eb) < 0) return;
  so_forward(so_lds, o, R, a.H0, P1, P3);
  // row g of z = [h1 node-major, R F1 | relu(acts) node-major, R F3]; acts [R, F3]: true widths, one pass each
  float* zrow = z + (int64_t)blockIdx.x * ((int64_t)R * (F1 + F3));
  for (int e = threadIdx.x; e < R * F1; e += SO_T) {
    const int i = e / F1, f = e - i * F1;
    zrow[e] = so_lds[o.y1 + i * P1 + f];
  }
  for (int e = threadIdx.x; e < R * F3; e += SO_T) {
    const int i = e / F3, f = e - i * F3;
    const float v = so_lds[o.a + i * P3 + f];
    acts[nb * F3 + e] = v;
    zrow[R * F1 + e] = fmaxf(v, 0.f);
  }
}

// dW partial groups for `nitems` work items per group producing `nout` outputs: as many as the workgroup has threads
// for and `redw` (2 * SO_T words) has room for, at most 16
__device__ __forceinline__ int so_dw_parts(int nitems, int nout) {
  int parts = SO_T / nitems;
  const int cap = 2 * SO_T / nout;
  parts = parts > cap ? cap : parts;
  return parts > 16 ? 16 : (parts < 1 ? 1 : parts);
}

// One layer's walk of the transposed lists: dH = A_hat^T G (by-source order), the coefficient gradients and the
// bias-gradient partials.  No barrier inside.
__device__ __forceinline__ void so_layer_bwd_lists(float* lds, const SoLayout& o, int R, int ne, int P, const float* G,
                                                   const float* H, float* dH) {
  const int32_t* ssptr = lds_i32(lds, o.t.sptr);
  const int PQ = P >> 2;
  for (int e = threadIdx.x; e < R * PQ; e += SO_T) {
    const int sn = e / PQ, q = e - sn * PQ;
    float4 acc = gcn_walk4(lds_i32(lds, o.n.bdst), lds + o.n.bwhat, ssptr[sn], ssptr[sn + 1], G, P, q);
    const float wl = lds[o.n.wloop + sn];
    const float4 gs = *reinterpret_cast<const float4*>(G + sn * P + q * 4);
    acc.x += wl * gs.x; acc.y += wl * gs.y; acc.z += wl * gs.z; acc.w += wl * gs.w;
    *reinterpret_cast<float4*>(dH + sn * P + q * 4) = acc;
  }
  gcn_coef_grads(lds, o.t, o.n, R, ne, G, H, P, PQ, SO_T);
  gcn_bias_partials(G, R, P, SO_DB_PARTS, lds + o.redb);      // (P <= 32: SO_DB_PARTS * P <= SO_T)
}

__global__ void __launch_bounds__(SO_T)
k_sgcn_ori_bwd(const SoArgs a, const float* __restrict__ dz, const float* __restrict__ dacts_in,
               float* __restrict__ dacts, float* __restrict__ dx_in, float* __restrict__ dew_in,
               float* __restrict__ dpar_partial, int NP) {
  extern __shared__ float so_lds[];
  float* lds = so_lds;
  const SoLayout o = so_layout(a.R, a.Emax, a.H0, a.F1, a.F3, 1);
  const int tid = threadIdx.x, R = a.R, H0 = a.H0, F1 = a.F1, F3 = a.F3, P1 = so_pad(F1), P3 = so_pad(F3);
  const int P1Q = P1 >> 2;
  const int64_t nb = (int64_t)blockIdx.x * R;
  int32_t eb;
  const int ne = so_stage<true>(lds, o, a, nb, eb);
  if (ne < 0) {                                        // refused graph: defined (zero) outputs, flagged in `status`
    for (int e = tid; e < R * H0; e += SO_T) dx_in[nb * H0 + e] = 0.f;
    for (int e = tid; e < NP; e += SO_T) dpar_partial[(int64_t)blockIdx.x * NP + e] = 0.f;
    if (dacts)
      for (int e = tid; e < R * F3; e += SO_T) dacts[nb * F3 + e] = 0.f;
    return;
  }
  // the incoming gradient row, into the padded layouts (padding = 0)
  const float* dzrow = dz + (int64_t)blockIdx.x * ((int64_t)R * (F1 + F3));
  for (int e = tid; e < R * P1; e += SO_T) {
    const int i = e / P1, f = e - i * P1;
    lds[o.dy1 + e] = f < F1 ? dzrow[i * F1 + f] : 0.f;
  }
  for (int e = tid; e < R * P3; e += SO_T) {
    const int i = e / P3, f = e - i * P3;
    lds[o.dy3 + e] = f < F3 ? dzrow[R * F1 + i * F3 + f] : 0.f;
  }
  for (int k = tid; k < ne; k += SO_T) lds[o.n.dwhat + k] = 0.f;
  for (int i = tid; i < R; i += SO_T) lds[o.n.dwloop + i] = 0.f;
  so_forward(lds, o, R, H0, P1, P3);                   // both transforms kept (h1, h3), outputs in y1 / a
  float* prow = lds + o.prow;
  const int off_b1 = F1 * H0, off_w3 = off_b1 + F1, off_b3 = off_w3 + F3 * F1;
  // ---- layer 3.  The tap: G3 = d h3 where acts > 0, exactly 0 elsewhere (+ a gradient the caller put on acts itself)
  for (int e = tid; e < R * P3; e += SO_T) {
    const int i = e / P3, f = e - i * P3;
    float g = lds[o.a + e] > 0.f ? lds[o.dy3 + e] : 0.f;
    if (f < F3) {
      if (dacts_in) g += dacts_in[nb * F3 + i * F3 + f];
      if (dacts) dacts[nb * F3 + i * F3 + f] = g;
    }
    lds[o.dy3 + e] = g;
  }
  __syncthreads();
  so_layer_bwd_lists(lds, o, R, ne, P3, lds + o.dy3, lds + o.h3, lds + o.dh);
  __syncthreads();
  if (tid < F3) {
    float acc = 0.f;
    for (int p2 = 0; p2 < SO_DB_PARTS; ++p2) acc += lds[o.redb + p2 * P3 + tid];
    prow[off_b3 + tid] = acc;
  }
  // dW3 = dH3^T h1 (partials; item = (fo, input quad, node part)) and G1 = (d z's h1 block + dH3 W3) * [h1 > 0], in place
  const int nq3 = P3 * P1Q, parts3 = so_dw_parts(nq3, P3 * P1);
  {
    const float* dH = lds + o.dh;
    for (int idx = tid; idx < parts3 * nq3; idx += SO_T) {
      const int e = idx % nq3, part = idx / nq3;
      const int fo = e / P1Q, q = e - fo * P1Q;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = part; i < R; i += parts3) {
        const float d = dH[i * P3 + fo];
        const float4 x4 = *reinterpret_cast<const float4*>(lds + o.y1 + i * P1 + q * 4);
        acc.x += d * x4.x; acc.y += d * x4.y; acc.z += d * x4.z; acc.w += d * x4.w;
      }
      *reinterpret_cast<float4*>(lds + o.redw + part * (P3 * P1) + fo * P1 + q * 4) = acc;
    }
    for (int e = tid; e < R * P1Q; e += SO_T) {
      const int i = e / P1Q, q = e - i * P1Q;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int fo = 0; fo < P3; ++fo) {
        const float d = dH[i * P3 + fo];
        const float4 w4 = *reinterpret_cast<const float4*>(lds + o.w3 + fo * P1 + q * 4);
        acc.x += d * w4.x; acc.y += d * w4.y; acc.z += d * w4.z; acc.w += d * w4.w;
      }
      const float4 g = *reinterpret_cast<const float4*>(lds + o.dy1 + e * 4);
      const float4 y4 = *reinterpret_cast<const float4*>(lds + o.y1 + e * 4);
      acc.x = y4.x > 0.f ? g.x + acc.x : 0.f; acc.y = y4.y > 0.f ? g.y + acc.y : 0.f;
      acc.z = y4.z > 0.f ? g.z + acc.z : 0.f; acc.w = y4.w > 0.f ? g.w + acc.w : 0.f;
      *reinterpret_cast<float4*>(lds + o.dy1 + e * 4) = acc;
    }
  }
  __syncthreads();
  // ---- layer 1.  dW3's partials meet here
  for (int e = tid; e < F3 * F1; e += SO_T) {
    const int fo = e / F1, fi = e - fo * F1;
    float acc = 0.f;
    for (int p2 = 0; p2 < parts3; ++p2) acc += lds[o.redw + p2 * (P3 * P1) + fo * P1 + fi];
    prow[off_w3 + e] = acc;
  }
  so_layer_bwd_lists(lds, o, R, ne, P1, lds + o.dy1, lds + o.h1, lds + o.dh);
  __syncthreads();
  if (tid < F1) {
    float acc = 0.f;
    for (int p2 = 0; p2 < SO_DB_PARTS; ++p2) acc += lds[o.redb + p2 * P1 + tid];
    prow[off_b1 + tid] = acc;
  }
  const int n1 = P1 * H0, parts1 = so_dw_parts(n1, n1);
  {
    const float* dH = lds + o.dh;
    for (int idx = tid; idx < parts1 * n1; idx += SO_T) {
      const int e = idx % n1, part = idx / n1;
      const int fo = e / H0, fi = e - fo * H0;
      float acc = 0.f;
      for (int i = part; i < R; i += parts1) acc += dH[i * P1 + fo] * lds[o.t.x + i * H0 + fi];
      lds[o.redw + idx] = acc;
    }
    for (int e = tid; e < R * H0; e += SO_T) {        // d x_in[i, fi] = sum_fo dH1[i, fo] W1[fo, fi]
      const int i = e / H0, fi = e - i * H0;
      float acc = 0.f;
      for (int fo = 0; fo < P1; ++fo) acc += dH[i * P1 + fo] * lds[o.w1t + fi * P1 + fo];
      lds[o.dx0 + e] = acc;
    }
  }
  // ---- gcn_norm backward; dW1's partials meet between its two halves
  gcn_norm_bwd_products(lds, o.t, o.n, ne, SO_T);
  __syncthreads();
  for (int e = tid; e < F1 * H0; e += SO_T) {          // dW1: rows fo < F1 of the padded partials
    float acc = 0.f;
    for (int p2 = 0; p2 < parts1; ++p2) acc += lds[o.redw + p2 * n1 + e];
    prow[e] = acc;
  }
  gcn_norm_bwd_edges(lds, o.t, o.n, R, ne, eb, dew_in, SO_T);
  for (int e = tid; e < R * H0; e += SO_T) dx_in[nb * H0 + e] = lds[o.dx0 + e];
  for (int e = tid; e < NP; e += SO_T) dpar_partial[(int64_t)blockIdx.x * NP + e] = prow[e];
}

static int so_check(const char* nm, int64_t n_graphs, int R, int max_edges, int H0, int F1, int F3, int backward) {
  IGCN_REQUIRE(n_graphs > 0 && n_graphs < ((int64_t)1 << 31) && R > 0 && max_edges >= 0, "%s: bad sizes", nm);
  IGCN_REQUIRE(n_graphs * R < ((int64_t)1 << 31), "%s: the batch's nodes must fit int32", nm);
  if (H0 < 1 || H0 > IGCN_MAX_H0 || F1 < 1 || F1 > IGCN_STACK_MAX_WIDTH || F3 < 1 || F3 > IGCN_STACK_MAX_WIDTH ||
      igcn_sgcn_ori_lds_bytes(R, max_edges, H0, F1, F3, backward) > IGCN_LDS_BUDGET_BYTES) {
    igcn_set_error("%s: needs 1 <= H0 <= %d, 1 <= F1, F3 <= %d and a graph that fits %d KB of LDS (R=%d, E<=%d, "
                   "H0=%d, F1=%d, F3=%d)", nm, IGCN_MAX_H0, IGCN_STACK_MAX_WIDTH, IGCN_LDS_BUDGET_BYTES / 1024, R, max_edges,
                   H0, F1, F3);
    return IGCN_ERR_UNSUPPORTED;
  }
  return IGCN_OK;
}

extern "C" int igcn_sgcn_ori_fwd(int64_t n_graphs, int R, int max_edges, int H0, int F1, int F3, const float* x_in,
                                 const float* ew_in, const int32_t* src32, const int32_t* dst32,
                                 const int32_t* tgt_ptr, const int32_t* tgt_perm, const int32_t* loop_edge,
                                 const float* W1, const float* b1, const float* W3, const float* b3, float* z,
                                 float* acts, int32_t* status, void* stream) {
  int rc = so_check("sgcn_ori_fwd", n_graphs, R, max_edges, H0, F1, F3, 0);
  if (rc) return rc;
  IGCN_REQUIRE(x_in && ew_in && src32 && dst32 && tgt_ptr && tgt_perm && loop_edge && W1 && b1 && W3 && b3 && z && acts,
               "sgcn_ori_fwd: null argument");
  const SoArgs a = {R, max_edges, H0, F1, F3, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, nullptr, nullptr,
                    loop_edge, W1, b1, W3, b3, status};
  const size_t lds = igcn_sgcn_ori_lds_bytes(R, max_edges, H0, F1, F3, 0);
  if (lds > 64 * 1024) IGCN_ALLOW_BIG_LDS(k_sgcn_ori_fwd);
  hipLaunchKernelGGL(k_sgcn_ori_fwd, dim3((unsigned)n_graphs), dim3(SO_T), lds, (hipStream_t)stream, a, z, acts);
  IGCN_CHECK_LAUNCH("sgcn_ori_fwd");
  return IGCN_OK;
}

extern "C" int igcn_sgcn_ori_bwd(int64_t n_graphs, int R, int max_edges, int H0, int F1, int F3, const float* x_in,
                                 const float* ew_in, const int32_t* src32, const int32_t* dst32,
                                 const int32_t* tgt_ptr, const int32_t* tgt_perm, const int32_t* src_ptr,
                                 const int32_t* src_perm, const int32_t* loop_edge, const float* W1, const float* b1,
                                 const float* W3, const float* b3, const float* dz, const float* dacts_in,
                                 float* dacts, float* dx_in, float* dew_in, float* dparams, float* scratch,
                                 int32_t* status, void* stream) {
  int rc = so_check("sgcn_ori_bwd", n_graphs, R, max_edges, H0, F1, F3, 1);
  if (rc) return rc;
  IGCN_REQUIRE(x_in && ew_in && src32 && dst32 && tgt_ptr && tgt_perm && src_ptr && src_perm && loop_edge && W1 && b1 &&
                   W3 && b3 && dz && dx_in && dew_in && dparams && scratch,
               "sgcn_ori_bwd: null argument");
  const SoArgs a = {R, max_edges, H0, F1, F3, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, src_ptr, src_perm,
                    loop_edge, W1, b1, W3, b3, status};
  const size_t lds = igcn_sgcn_ori_lds_bytes(R, max_edges, H0, F1, F3, 1);
  const int NP = so_param_floats(H0, F1, F3);
  hipStream_t st = (hipStream_t)stream;
  if (lds > 64 * 1024) IGCN_ALLOW_BIG_LDS(k_sgcn_ori_bwd);
  hipLaunchKernelGGL(k_sgcn_ori_bwd, dim3((unsigned)n_graphs), dim3(SO_T), lds, st, a, dz, dacts_in, dacts, dx_in,
                     dew_in, scratch, NP);
  IGCN_CHECK_LAUNCH("sgcn_ori_bwd");
  return igcn_launch_reduce_rows_final(scratch, n_graphs, NP, NP, dparams, st);
}
