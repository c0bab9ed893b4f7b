// What the "one workgroup per graph, everything in LDS" stack kernels share (csrc/sgcn_fused.hip, csrc/sgcn_ori.hip,
// csrc/gat_fused.hip): where the staged graph lives in LDS and how it gets there, PyG's gcn_norm on it (forward lists,
// backward down to d(edge weight)), and the list walks of one GCN layer.  Plain inline functions over two structs of
// LDS word offsets; sums run in the plan's stable list order, so every caller gets the same bits.  The workgroup's
// thread count nt, row strides and quad counts are ordinary arguments (compile-time constants after inlining where the
// caller's are: a loop whose stride the compiler knows batches its loads).
#pragma once
#include "common.h"

#ifndef GCN_LDS_PROBE          // a phase stamp inside gcn_lists (csrc/sgcn_fused.hip under -DSF_PROBE_ON)
#define GCN_LDS_PROBE(i)
#endif

__device__ __forceinline__ int32_t* lds_i32(float* lds, int off) { return reinterpret_cast<int32_t*>(lds + off); }
__device__ __forceinline__ const int32_t* lds_i32(const float* lds, int off) {
  return reinterpret_cast<const int32_t*>(lds + off);
}

// ---- the staged graph ------------------------------------------------------------------------------------------------
// x [R][H0]; per stored edge k: local endpoints src / dst and its value ew; the by-target list (positions
// [tptr[i], tptr[i+1]) hold the edges tperm[.] into node i) and, for a backward, the by-source list (sptr, sperm)
struct GraphLds {
  int x, ew, src, dst, tptr, tperm;
  int sptr, sperm;
};

// The layout functions give so_layout (csrc/sgcn_ori.hip) and gt_layout (csrc/gat_fused.hip) their block order; the
// backward's fields are taken by a call of their own, behind the caller's forward blocks.  sf_layout
// (csrc/sgcn_fused.hip) fills the structs itself: the order of the blocks is part of a kernel's speed, and
// k_sgcn_stack_bwd keeps the one it was tuned in (docs/LABLOG.md section C).
template <class Take>
__host__ __device__ inline void graph_lds_layout(GraphLds& t, int R, int Emax, int H0, Take&& take) {
  t.x = take(R * H0);
  t.ew = take(Emax);
  t.src = take(Emax);
  t.dst = take(Emax);
  t.tptr = take(R + 1);
  t.tperm = take(Emax);
  t.sptr = t.sperm = 0;
}

template <class Take>
__host__ __device__ inline void graph_lds_layout_bwd(GraphLds& t, int R, int Emax, Take&& take) {
  t.sptr = take(R + 1);
  t.sperm = take(Emax);
}

// Graph nb / R of the per-graph plan into LDS, indices rebased to the graph (nodes by nb, edges by eb = its first edge,
// handed back in eb_out).  Returns the edge count, or -1 with status bit 1 (GraphPlan.check) set and nothing stored
// when the count is not in [0, Emax]: a plan whose pointers run backwards is refused like one that is too large.
// Ends WITHOUT a barrier.
template <bool BWD>
__device__ __forceinline__ int graph_lds_load(float* lds, const GraphLds& t, int R, int Emax, int H0, int64_t nb,
                                              const float* __restrict__ x_in, const float* __restrict__ ew_in,
                                              const int32_t* __restrict__ src32, const int32_t* __restrict__ dst32,
                                              const int32_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt_perm,
                                              const int32_t* __restrict__ src_ptr, const int32_t* __restrict__ src_perm,
                                              int32_t* __restrict__ status, int32_t& eb_out, int nt) {
  const int tid = threadIdx.x;
  const int32_t eb = tgt_ptr[nb];
  const int ne = tgt_ptr[nb + R] - eb;
  eb_out = eb;
  if (ne > Emax || ne < 0) {
    if (tid == 0 && status) atomicOr(status, 2);
    return -1;
  }
  for (int i = tid; i < R * H0; i += nt) lds[t.x + i] = x_in[nb * H0 + i];
  for (int k = tid; k < ne; k += nt) {
    lds_i32(lds, t.src)[k] = src32[eb + k] - (int32_t)nb;
    lds_i32(lds, t.dst)[k] = dst32[eb + k] - (int32_t)nb;
    lds[t.ew + k] = ew_in[eb + k];
    lds_i32(lds, t.tperm)[k] = tgt_perm[eb + k] - eb;       // by-target position eb + p holds edge tgt_perm[.] of this graph
    if (BWD) lds_i32(lds, t.sperm)[k] = src_perm[eb + k] - eb;
  }
  for (int i = tid; i <= R; i += nt) {
    lds_i32(lds, t.tptr)[i] = tgt_ptr[nb + i] - eb;
    if (BWD) lds_i32(lds, t.sptr)[i] = src_ptr[nb + i] - eb;
  }
  return ne;
}

// ---- gcn_norm ----------------------------------------------------------------------------------------------------------
// PyG: stored loops are dropped and one loop per node is added whose weight is the LAST stored loop's, or 1.
// Per node: dis = deg^-1/2, wl = the loop's weight, wloop = its coefficient, loop = the batch-global id of the stored
// loop that counts (or -1; filled by the caller).  Per by-target position: the source node tsrc and the coefficient
// twhat; per by-source position (backward): the target node bdst and the coefficient bwhat.  The backward accumulates
// dwhat [edge] / dwloop [node] over the layers; ddeg, v1, v2 are scratch of gcn_norm_bwd_*.
struct GcnNormLds {
  int dis, wl, wloop, loop, tsrc, twhat;
  int bdst, bwhat, dwhat, dwloop, ddeg, v1, v2;
};

template <class Take>
__host__ __device__ inline void gcn_norm_layout(GcnNormLds& n, int R, int Emax, Take&& take) {
  n.dis = take(R);
  n.wl = take(R);
  n.wloop = take(R);
  n.loop = take(R);
  n.tsrc = take(Emax + 4);                         // (+4: the 4-wide list walk may read past the end; never used)
  n.twhat = take(Emax + 4);
  n.bdst = n.bwhat = n.dwhat = n.dwloop = n.ddeg = n.v1 = n.v2 = 0;
}

// dead1 / dead2: two caller buffers of at least Emax words each that are dead when gcn_norm_bwd_products runs (v1 / v2
// live there), or -1 for blocks of their own
template <class Take>
__host__ __device__ inline void gcn_norm_layout_bwd(GcnNormLds& n, int R, int Emax, int dead1, int dead2, Take&& take) {
  n.bdst = take(Emax + 4);
  n.bwhat = take(Emax + 4);
  n.dwhat = take(Emax);
  n.dwloop = take(R);
  n.ddeg = take(R);
  n.v1 = dead1 >= 0 ? dead1 : take(Emax);
  n.v2 = dead2 >= 0 ? dead2 : take(Emax);
}

// From the staged graph and n.loop to the lists every layer walks.  The entries are laid out in list order (tsrc,
// twhat; bdst, bwhat): every later walk reads two consecutive arrays instead of chasing permutation -> edge ->
// endpoint.  Short phases with a thread per list POSITION or per node — a thread per node walking its list through
// the permutation was a serial chain of dependent LDS reads on R of the workgroup's threads.  Ends WITHOUT a barrier:
// the caller's next __syncthreads() orders the coefficient arrays before their first use.
template <bool BWD>
__device__ __forceinline__ void gcn_lists(float* lds, const GraphLds& t, const GcnNormLds& n, int R, int ne,
                                          int32_t eb, int nt) {
  const int tid = threadIdx.x;
  const int32_t* ssrc = lds_i32(lds, t.src);
  const int32_t* sdst = lds_i32(lds, t.dst);
  const int32_t* stptr = lds_i32(lds, t.tptr);
  const int32_t* stperm = lds_i32(lds, t.tperm);
  int32_t* stsrc = lds_i32(lds, n.tsrc);
  for (int p = tid; p < ne; p += nt) {
    const int k = stperm[p];
    const int sk = ssrc[k];
    stsrc[p] = sk;
    lds[n.twhat + p] = sk != sdst[k] ? lds[t.ew + k] : 0.f;      // stored loops are replaced by the added loop
  }
  __syncthreads();
  for (int i = tid; i < R; i += nt) {
    float deg = 0.f;
    for (int p = stptr[i]; p < stptr[i + 1]; ++p) deg += lds[n.twhat + p];     // list order (loops add an exact 0)
    const int32_t le = lds_i32(lds, n.loop)[i];
    const float lw = le >= 0 ? lds[t.ew + (le - eb)] : 1.f;
    deg += lw;
    float d = 1.0f / sqrtf(deg);
    if (deg == 0.f) d = 0.f;
    lds[n.dis + i] = d;
    lds[n.wl + i] = lw;
    lds[n.wloop + i] = d * lw * d;
  }
  __syncthreads();
  GCN_LDS_PROBE(2);
  for (int p = tid; p < ne; p += nt)
    lds[n.twhat + p] = lds[n.dis + stsrc[p]] * lds[n.twhat + p] * lds[n.dis + sdst[stperm[p]]];
  if (BWD) {
    // the transposed lists (edges out of a source) in BY-SOURCE order, for dH = A_hat^T G
    const int32_t* ssperm = lds_i32(lds, t.sperm);
    int32_t* sbdst = lds_i32(lds, n.bdst);
    for (int p = tid; p < ne; p += nt) {               // (the source of position p is the source of the edge stored there)
      const int k = ssperm[p];
      const int i = ssrc[k], tn = sdst[k];
      sbdst[p] = tn;
      lds[n.bwhat + p] = tn != i ? lds[n.dis + i] * lds[t.ew + k] * lds[n.dis + tn] : 0.f;
    }
  }
}

// gcn_norm backward, first half: the two sums of a node — over the edges it sends (by-source list) and over those it
// receives (by-target list) — as products per list POSITION (v1 by-source, v2 by-target order); the per-node form
// chased permutation -> edge -> endpoint through ~8 dependent LDS reads.  The caller puts a barrier behind it.
__device__ __forceinline__ void gcn_norm_bwd_products(float* lds, const GraphLds& t, const GcnNormLds& n, int ne,
                                                      int nt) {
  const int32_t* ssrc = lds_i32(lds, t.src);
  const int32_t* sdst = lds_i32(lds, t.dst);
  const int32_t* ssperm = lds_i32(lds, t.sperm);
  const int32_t* stperm = lds_i32(lds, t.tperm);
  const int32_t* sbdst = lds_i32(lds, n.bdst);
  const int32_t* stsrc = lds_i32(lds, n.tsrc);
  for (int p = threadIdx.x; p < ne; p += nt) {
    const int k1 = ssperm[p], tn = sbdst[p];
    lds[n.v1 + p] = tn != ssrc[k1] ? lds[n.dwhat + k1] * lds[t.ew + k1] * lds[n.dis + tn] : 0.f;
    const int k2 = stperm[p], sn = stsrc[p];
    lds[n.v2 + p] = sn != sdst[k2] ? lds[n.dwhat + k2] * lds[t.ew + k2] * lds[n.dis + sn] : 0.f;
  }
}

// second half: short sums of consecutive words per node -> d deg, a barrier, then d(edge weight) of every stored edge
// of the graph to dew_in[eb + k].  Of a node's stored loops only the one that counted (n.loop) gets the loop's gradient.
// Its two steps are functions of their own for a caller that consumes the edge gradients instead of storing them
// (k_sgcn_stack_bwd's masked copy, csrc/sgcn_fused.hip).
__device__ __forceinline__ void gcn_norm_bwd_ddeg(float* lds, const GraphLds& t, const GcnNormLds& n, int R, int nt) {
  const int32_t* ssptr = lds_i32(lds, t.sptr);
  const int32_t* stptr = lds_i32(lds, t.tptr);
  for (int i = threadIdx.x; i < R; i += nt) {
    float dd = 0.f;
    for (int p = ssptr[i]; p < ssptr[i + 1]; ++p) dd += lds[n.v1 + p];     // list order; stored loops add an exact 0
    for (int p = stptr[i]; p < stptr[i + 1]; ++p) dd += lds[n.v2 + p];
    const float di = lds[n.dis + i];
    dd += 2.f * lds[n.dwloop + i] * lds[n.wl + i] * di;
    lds[n.ddeg + i] = -0.5f * di * di * di * dd;
  }
}

// d(edge weight) of stored edge k of the graph (behind gcn_norm_bwd_ddeg and a barrier)
__device__ __forceinline__ float gcn_norm_bwd_edge(const float* lds, const GraphLds& t, const GcnNormLds& n, int32_t eb,
                                                   int k) {
  const int s = lds_i32(lds, t.src)[k], tn = lds_i32(lds, t.dst)[k];
  float g;
  if (s != tn) {
    g = lds[n.dis + s] * lds[n.dis + tn] * lds[n.dwhat + k] + lds[n.ddeg + tn];
  } else {
    g = (lds_i32(lds, n.loop)[s] == eb + k) ? lds[n.ddeg + s] + lds[n.dis + s] * lds[n.dis + s] * lds[n.dwloop + s]
                                            : 0.f;
  }
  return g;
}

__device__ __forceinline__ void gcn_norm_bwd_edges(float* lds, const GraphLds& t, const GcnNormLds& n, int R, int ne,
                                                   int32_t eb, float* __restrict__ dew_in, int nt) {
  gcn_norm_bwd_ddeg(lds, t, n, R, nt);
  __syncthreads();
  for (int k = threadIdx.x; k < ne; k += nt) dew_in[eb + k] = gcn_norm_bwd_edge(lds, t, n, eb, k);
}

// ---- the list walks of one layer -------------------------------------------------------------------------------------
// sum over the list positions [p0, p1), in order, of coef[p] * rows[idx[p] * ld + 4 q .. + 4): four entries per step
// (their reads overlap), every LDS access 16 bytes.  Both lists of a direction go through here: Y = A_hat H by target
// (tsrc, twhat), dH = A_hat^T G by source (bdst, bwhat); the self-loop term, bias and ReLU stay with the caller.
__device__ __forceinline__ float4 gcn_walk4(const int32_t* idx, const float* coef, int p0, int p1, const float* rows,
                                            int ld, int q) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = p0; p < p1; p += 4) {
    int ij[4];
    float cj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ij[j] = idx[p + j];
      cj[j] = coef[p + j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (p + j < p1) {
        const float4 r4 = *reinterpret_cast<const float4*>(rows + ij[j] * ld + q * 4);
        acc.x += cj[j] * r4.x; acc.y += cj[j] * r4.y; acc.z += cj[j] * r4.z; acc.w += cj[j] * r4.w;
      }
  }
  return acc;
}

// coefficient gradients of one layer (G, H [R][ld], nq quads per row), accumulated over the layers:
// per stored edge dwhat[k] += G[dst] . H[src] (stored loops skipped); then per node dwloop[i] += G[i] . H[i]
__device__ __forceinline__ void gcn_coef_grads(float* lds, const GraphLds& t, const GcnNormLds& n, int R, int ne,
                                               const float* G, const float* H, int ld, int nq, int nt) {
  const int32_t* ssrc = lds_i32(lds, t.src);
  const int32_t* sdst = lds_i32(lds, t.dst);
  for (int k = threadIdx.x; k < ne + R; k += nt) {
    int sn, tn;
    float* dstp;
    if (k < ne) {
      sn = ssrc[k];
      tn = sdst[k];
      if (sn == tn) continue;
      dstp = lds + n.dwhat + k;
    } else {
      sn = tn = k - ne;
      dstp = lds + n.dwloop + sn;
    }
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < nq; ++c) {
      const float4 g4 = *reinterpret_cast<const float4*>(G + tn * ld + c * 4);
      const float4 h4 = *reinterpret_cast<const float4*>(H + sn * ld + c * 4);
      acc += g4.x * h4.x;
      acc += g4.y * h4.y;
      acc += g4.z * h4.z;
      acc += g4.w * h4.w;
    }
    *dstp += acc;
  }
}

// bias gradient, first half: `parts` thread groups of F lanes share the node range of G [R][F]; partial (part, fo)
// lands in red[part * F + fo] (parts * F <= the workgroup's threads); the caller sums them behind its next barrier
__device__ __forceinline__ void gcn_bias_partials(const float* G, int R, int F, int parts, float* red) {
  const int tid = threadIdx.x;
  if (tid < parts * F) {
    const int fo = tid % F, part = tid / F;
    float acc = 0.f;
    for (int i = part; i < R; i += parts) acc += G[i * F + fo];
    red[tid] = acc;
  }
}
