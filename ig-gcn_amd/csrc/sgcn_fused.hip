// The SGCN stack of one brain graph, LDS-resident: gcn_norm + L x (X W^T, scatter-aggregate, + bias, ReLU) + the
// jumping-knowledge concatenation of kernel/sgcn_img_snp.py:218-224 (PyG GCNConv x L) as ONE
// kernel per direction, one 512-thread workgroup per graph.
//
// A 90-ROI graph is tiny (90 x 3 inputs, 270 edges, 90 x 16 activations per layer): as separate launches (norm x 2,
// GEMM + aggregate per layer, concat; a dozen more backward) every kernel sits on the dispatch floor and the
// activations make an HBM / L2 round trip between each pair.  Here the graph's node features, edge lists and
// coefficients are staged in LDS once, every layer runs out of LDS, and HBM sees the compulsory traffic only:
// x, the edge list and its weights in; the concatenated layer outputs out (SURVEY §8d "fused SGCN forward lower bound").
// The backward kernel recomputes the forward in LDS (cheaper than saving it) and writes dx, d(edge weight) and one
// row of parameter-gradient partials per graph.
//
// Preconditions (checked by the host wrappers / guaranteed by the per-graph plan builders): a block-diagonal batch of
// uniform graphs (R nodes each, graph g = nodes [gR, (g+1)R), its edges contiguous in stored order), edge lists
// from the graph plan.  Sums run in the plan's stable (reference scatter) order; no atomics: deterministic.
//
// The staged graph's LDS layout, gcn_norm (lists and backward) and the list walks of a layer are csrc/gcn_lds.h, shared
// with the other LDS stacks; what is here is this stack's own: the register-batched staging, the transforms, the
// parameter gradients and the front kernel's plan build and masks.
#include "common.h"

// phase stamps for tools/sgcn_probe.py and tools/front_probe.py (-DSF_PROBE_ON); gcn_lists of csrc/gcn_lds.h stamps too
#ifdef SF_PROBE_ON
__device__ long long sf_probe_buf[8 * 16];
#define SF_PROBE(i) do { if (threadIdx.x == 0 && blockIdx.x < 8) sf_probe_buf[blockIdx.x * 16 + (i)] = wall_clock64(); } while (0)
extern "C" int igcn_debug_sf_probe(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(sf_probe_buf), sizeof(long long) * 8 * 16);
}
#else
#define SF_PROBE(i)
#endif
#define GCN_LDS_PROBE(i) SF_PROBE(i)
#include "gcn_lds.h"

// threads per workgroup (= per graph).  The kernels are chains of ~20 barrier-separated phases over ~1.5 k work items;
// measured at the bench shape (512 graphs, hot): forward 16.7 / 12.6 / 12.3 us and backward 52 / 40 / 53 us with
// 256 / 512 / 1024 threads.
#define SF_T 512           // forward
#define SF_TB 512          // backward

struct SfParams {
  const float* W[IGCN_STACK_MAX_LAYERS];     // W_l [F, Fin_l] row-major (Fin_0 = H0, then F)
  const float* b[IGCN_STACK_MAX_LAYERS];     // b_l [F]
};

// LDS carve-out shared by both kernels (all offsets in 4-byte words)
struct SfLayout {
  GraphLds t;                                      // the staged graph
  GcnNormLds n;                                    // gcn_norm: coefficients, lists, backward
  int wallT, act, wall;                            // forward part
  int ycat;                                        // [R][L*F] layer outputs
  int g, dh, dx, red, dycat, prow;                 // backward part
  int fprob, fct, fcs, fsperm, fe;                 // front part (k_sgcn_front_fwd)
  int total;
};

// front = 1: the forward kernel that also BUILDS the graph's plan and its masks (k_sgcn_front_fwd) — histograms, the
// by-source permutation, the mask's node factors and edge probabilities live in LDS until the one store burst at the end
__host__ __device__ inline SfLayout sf_layout(int R, int Emax, int H0, int F, int L, int backward, int front = 0) {
  SfLayout o;
  int p = 0;
  auto take = [&](int n) { int q = p; p += (n + 3) & ~3; return q; };
  const int fin_max = F > H0 ? F : H0;
  // The two shared structs, filled HERE and not by graph_lds_layout / gcn_norm_layout: the order of the blocks is
  // part of this kernel's speed (the same code over the shared functions' order: backward 26.0 -> 26.9 us at the
  // bench shape, docs/LABLOG.md section C), so the hot kernel keeps the order it was tuned in.
  o.t.x = take(R * H0);
  o.n.dis = take(R);
  o.n.wl = take(R);
  o.n.wloop = take(R);
  o.t.ew = take(Emax);
  take(Emax);     // reserved (once the by-edge coefficients): LDS per workgroup decides how many graphs share a CU
  o.t.src = take(Emax);
  o.t.dst = take(Emax);
  o.t.tptr = take(R + 1);
  o.t.tperm = take(Emax);
  o.n.tsrc = take(Emax + 4);                       // (+4: the 4-wide list walk may read past the end; never used)
  o.n.twhat = take(Emax + 4);
  // every layer's weights, fetched with the graph (one round trip): wallT = W_l TRANSPOSED (Wt[fi][fo]: the F lanes of
  // a node read consecutive words in the transforms) | b_l; wall = W_l [fo][fi] as stored (backward: dX = dH W)
  o.wallT = take(L * (F * fin_max + F));
  o.wall = take(backward ? L * (F * fin_max + F) : 0);
  o.n.loop = take(R);
  // activations: the transforms H_l (the forward keeps the current one only, the backward all of them) and the
  // concatenated layer outputs Y [R][L*F], which leave for HBM in ONE coalesced pass at the end — a store in front of
  // a barrier makes the whole workgroup wait for its acknowledgement, so nothing is stored before the last barrier
  o.act = take((backward ? L : 1) * R * F);
  o.ycat = take(R * L * F);
  o.g = o.dh = o.dx = o.red = o.dycat = o.prow = 0;
  o.t.sptr = o.t.sperm = 0;
  o.n.bdst = o.n.bwhat = o.n.dwhat = o.n.dwloop = o.n.ddeg = o.n.v1 = o.n.v2 = 0;
  o.fprob = o.fct = o.fcs = o.fsperm = o.fe = 0;
  if (front) {
    o.fprob = take(R * H0);
    o.fct = take(R + 1);
    o.fcs = take(R + 1);
    o.fsperm = take(Emax);
    o.fe = take(Emax);
  }
  if (backward) {
    o.t.sptr = take(R + 1);
    o.t.sperm = take(Emax);
    o.g = take(R * F);
    o.dh = take(R * F);
    // gcn_norm backward's per-position products go into G / dH, dead by then, when they fit
    o.n.v1 = Emax <= R * F ? o.g : take(Emax);
    o.n.v2 = Emax <= R * F ? o.dh : take(Emax);
    o.dx = take(R * fin_max);
    o.n.dwhat = take(Emax);
    o.n.dwloop = take(R);
    o.n.ddeg = take(R);
    o.red = take(SF_TB + (SF_TB > F * fin_max ? SF_TB : F * fin_max));
    o.dycat = take(R * L * F);
    o.prow = take(L * (F * fin_max + F));
    o.n.bdst = take(Emax + 4);
    o.n.bwhat = take(Emax + 4);
  }
  o.total = p;
  return o;
}

extern "C" size_t igcn_sgcn_stack_lds_bytes(int R, int max_edges, int H0, int F, int L, int backward) {
  return (size_t)sf_layout(R, max_edges, H0, F, L, backward).total * 4;
}

// Stage the graph: node features, edges (local endpoints, weights), lists, and the gcn_norm coefficients (gcn_lists).
// Returns the graph's edge count, or -1 (nothing staged beyond the fixed-size arrays) when it exceeds Emax.
// Its own load sequence, not graph_lds_load's: the loads whose size is fixed by R go out FIRST, together with the two
// pointer words that give the graph's edge range: the edge arrays then follow one round trip later instead of two
// (the range used to be fetched, and waited for, in front of everything).
template <bool BWD>
__device__ __forceinline__ int sf_stage(float* lds, const SfLayout& o, int R, int Emax, int H0, int64_t nb,
                                        const float* __restrict__ x_in, const float* __restrict__ ew_in,
                                        const int32_t* __restrict__ src32, const int32_t* __restrict__ dst32,
                                        const int32_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt_perm,
                                        const int32_t* __restrict__ src_ptr, const int32_t* __restrict__ src_perm,
                                        const int32_t* __restrict__ loop_edge, const SfParams& prm, int F, int L,
                                        int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  const int32_t eb = tgt_ptr[nb];                      // workgroup-uniform: scalar loads, waited for where first used
  const int ne = tgt_ptr[nb + R] - eb;
  const int wstride = F * (F > H0 ? F : H0) + F;
  // weights and biases of all layers as one flat list [W_0 | b_0 | W_1 | b_1 | ...]: entry j of layer l lands at
  // wall + l * wstride + j.  The first two entries per thread ride in the register batch below.
  auto wsrc = [&](int j, int& dst, int& dstT) -> const float* {
    int off = 0;
    for (int l = 0; l < L; ++l) {
      const int fin = l == 0 ? H0 : F, nw = F * fin, n = nw + F;
      if (j < off + n) {
        const int r = j - off;
        dst = o.wall + l * wstride + r;
        dstT = o.wallT + l * wstride + (r < nw ? (r % fin) * F + r / fin : r);
        return r < nw ? prm.W[l] + r : prm.b[l] + (r - nw);
      }
      off += n;
    }
    dst = dstT = -1;
    return nullptr;
  };
  const int wtotal = F * H0 + F + (L - 1) * (F * F + F);
  float wv[2];
  int wd[2], wdT[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float* src = wsrc(tid + j * (int)blockDim.x, wd[j], wdT[j]);
    wv[j] = src ? *src : 0.f;
  }
  int32_t* ssrc = lds_i32(lds, o.t.src);
  int32_t* sdst = lds_i32(lds, o.t.dst);
  int32_t* stptr = lds_i32(lds, o.t.tptr);
  int32_t* stperm = lds_i32(lds, o.t.tperm);
  // ONE batch of loads per thread, parked in registers: x, the loop edges, the list pointers — and, as soon as the
  // (scalar) edge range has arrived, this thread's edge of every edge array; only then the LDS stores.  The vector
  // loads of the first group are still in flight when the second group goes out: one round trip, not two.
  float xv[4];
  int32_t lp = 0, tp[2] = {0, 0}, sp[2] = {0, 0};
  const int nx = R * H0, bd = (int)blockDim.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) xv[j] = tid + j * bd < nx ? x_in[nb * H0 + tid + j * bd] : 0.f;
  if (tid < R) lp = loop_edge[nb + tid];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = tid + j * bd;
    if (i <= R) {
      tp[j] = tgt_ptr[nb + i];
      if (BWD) sp[j] = src_ptr[nb + i];
    }
  }
  if (ne > Emax) {                                     // host-checked; never corrupt LDS — and never go unnoticed:
    if (tid == 0 && status) atomicOr(status, 2);       // bit 1 of the plan's status word (GraphPlan.check)
    return -1;
  }
  int32_t es = 0, ed = 0, et = 0, ep = 0;
  float ev = 0.f;
  if (tid < ne) {
    es = src32[eb + tid];
    ed = dst32[eb + tid];
    ev = ew_in[eb + tid];
    et = tgt_perm[eb + tid];
    if (BWD) ep = src_perm[eb + tid];
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (wd[j] >= 0) {
      lds[wdT[j]] = wv[j];
      if (BWD) lds[wd[j]] = wv[j];
    }
  for (int j = tid + 2 * bd; j < wtotal; j += bd) {
    int dst, dstT;
    const float v = *wsrc(j, dst, dstT);
    lds[dstT] = v;
    if (BWD) lds[dst] = v;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (tid + j * bd < nx) lds[o.t.x + tid + j * bd] = xv[j];
  for (int i = tid + 4 * bd; i < nx; i += bd) lds[o.t.x + i] = x_in[nb * H0 + i];
  for (int i = tid; i < R; i += bd) lds_i32(lds, o.n.loop)[i] = i == tid ? lp : loop_edge[nb + i];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = tid + j * bd;
    if (i <= R) {
      stptr[i] = tp[j] - eb;
      if (BWD) lds_i32(lds, o.t.sptr)[i] = sp[j] - eb;
    }
  }
  for (int i = tid + 2 * bd; i <= R; i += bd) {
    stptr[i] = tgt_ptr[nb + i] - eb;
    if (BWD) lds_i32(lds, o.t.sptr)[i] = src_ptr[nb + i] - eb;
  }
  if (tid < ne) {
    ssrc[tid] = es - (int32_t)nb;
    sdst[tid] = ed - (int32_t)nb;
    lds[o.t.ew + tid] = ev;
    stperm[tid] = et - eb;                         // by-target position eb + k holds edge tgt_perm[.] of this graph
    if (BWD) lds_i32(lds, o.t.sperm)[tid] = ep - eb;
  }
  for (int k = tid + bd; k < ne; k += bd) {
    ssrc[k] = src32[eb + k] - (int32_t)nb;
    sdst[k] = dst32[eb + k] - (int32_t)nb;
    lds[o.t.ew + k] = ew_in[eb + k];
    stperm[k] = tgt_perm[eb + k] - eb;
    if (BWD) lds_i32(lds, o.t.sperm)[k] = src_perm[eb + k] - eb;
  }
  __syncthreads();
  SF_PROBE(1);
  gcn_lists<BWD>(lds, o.t, o.n, R, ne, eb, bd);
  return ne;
}

// H = X W^T (X [R, fin], row stride ldx, at `xin`), then Y = relu(A_hat H + b) (row stride ldy): one layer, out of LDS
// into LDS
template <int F>
__device__ __forceinline__ void sf_layer(float* lds, const SfLayout& o, int R, int fin, const float* xin, int ldx,
                                         float* H, float* Y, int ldy, const float* Wt, const float* bt) {
  // Wt = the layer's weights TRANSPOSED in LDS (Wt[fi][fo], staged that way with the graph: the F lanes of a node
  // read consecutive words, not a stride-fin column), bt = its bias
  const int tid = threadIdx.x;
  const int32_t* stptr = lds_i32(lds, o.t.tptr);
  const int32_t* stsrc = lds_i32(lds, o.n.tsrc);
  // work item = (node, output quad): every LDS access moves 16 bytes (one weight-row quad serves four FMAs, one
  // gathered activation quad four more) — with one item per output word the phase is bound by the LDS instruction
  // rate, two 4-byte reads per FMA.  Dot products fully unrolled: the reads of an item are issued together.
  constexpr int FQ = F / 4;
  if (fin == F) {
    for (int e = tid; e < R * FQ; e += (int)blockDim.x) {
      const int i = e / FQ, q = e - i * FQ;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int f4 = 0; f4 < FQ; ++f4) {
        const float4 xv = *reinterpret_cast<const float4*>(xin + i * ldx + f4 * 4);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 w4 = *reinterpret_cast<const float4*>(Wt + (f4 * 4 + j) * F + q * 4);
          acc.x += xs[j] * w4.x; acc.y += xs[j] * w4.y; acc.z += xs[j] * w4.z; acc.w += xs[j] * w4.w;
        }
      }
      *reinterpret_cast<float4*>(H + i * F + q * 4) = acc;
    }
  } else {
    for (int e = tid; e < R * FQ; e += (int)blockDim.x) {
      const int i = e / FQ, q = e - i * FQ;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int fi = 0; fi < IGCN_MAX_H0; ++fi)
        if (fi < fin) {
          const float xv = xin[i * ldx + fi];
          const float4 w4 = *reinterpret_cast<const float4*>(Wt + fi * F + q * 4);
          acc.x += xv * w4.x; acc.y += xv * w4.y; acc.z += xv * w4.z; acc.w += xv * w4.w;
        }
      *reinterpret_cast<float4*>(H + i * F + q * 4) = acc;
    }
  }
  __syncthreads();
  for (int e = tid; e < R * FQ; e += (int)blockDim.x) {
    const int i = e / FQ, q = e - i * FQ;
    // stored order of the target's edges (reference order)
    float4 acc = gcn_walk4(stsrc, lds + o.n.twhat, stptr[i], stptr[i + 1], H, F, q);
    const float wl = lds[o.n.wloop + i];
    const float4 hs = *reinterpret_cast<const float4*>(H + i * F + q * 4);
    const float4 b4 = *reinterpret_cast<const float4*>(bt + q * 4);
    acc.x = fmaxf(acc.x + wl * hs.x + b4.x, 0.f);            // + self loop, + bias in the reference's order, ReLU
    acc.y = fmaxf(acc.y + wl * hs.y + b4.y, 0.f);
    acc.z = fmaxf(acc.z + wl * hs.z + b4.z, 0.f);
    acc.w = fmaxf(acc.w + wl * hs.w + b4.w, 0.f);
    *reinterpret_cast<float4*>(Y + i * ldy + q * 4) = acc;
  }
  __syncthreads();
}

template <int F>
__global__ void __launch_bounds__(SF_T)
k_sgcn_stack_fwd(int R, int Emax, int H0, int L, const float* __restrict__ x_in, const float* __restrict__ ew_in,
                 const int32_t* __restrict__ src32, const int32_t* __restrict__ dst32,
                 const int32_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt_perm,
                 const int32_t* __restrict__ loop_edge, SfParams prm, float* __restrict__ xcat,
                 int32_t* __restrict__ status) {
  extern __shared__ float sf_lds[];
  const SfLayout o = sf_layout(R, Emax, H0, F, L, 0);
  const int64_t nb = (int64_t)blockIdx.x * R;
  SF_PROBE(0);
  if (sf_stage<false>(sf_lds, o, R, Emax, H0, nb, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, nullptr, nullptr,
                      loop_edge, prm, F, L, status) < 0)
    return;
  float* H = sf_lds + o.act;
  float* Y = sf_lds + o.ycat;
  const int D = L * F;
  SF_PROBE(3);
  for (int l = 0; l < L; ++l) {
    // layer l owns columns [l F, (l+1) F) of the concatenated output rows and reads the columns of layer l-1
    const float* wl = sf_lds + o.wallT + l * (F * (F > H0 ? F : H0) + F);
    sf_layer<F>(sf_lds, o, R, l == 0 ? H0 : F, l == 0 ? sf_lds + o.t.x : Y + (l - 1) * F, l == 0 ? H0 : D, H, Y + l * F, D,
                wl, wl + F * (l == 0 ? H0 : F));
    SF_PROBE(4 + l);
  }
  // jumping-knowledge concatenation: the rows are already laid out [R][L F] — one coalesced 16-byte pass
  for (int e = threadIdx.x; e < R * D / 4; e += SF_T)
    reinterpret_cast<float4*>(xcat + nb * D)[e] = reinterpret_cast<const float4*>(Y)[e];
  SF_PROBE(8);
}

// ---- the FRONT of a train step's image branch as one launch ---------------------------------------------------------
// plan build (csrc/plan.hip: k_plan_segmented) -> masks of both passes + loss_probability + the SNP mask (csrc/sgcn.hip:
// k_edge_mask_fwd<true>) -> the stack above were three dependent launches of one workgroup per graph each (11.7 + 6.3 +
// 9.0 us at the bench shape, every one of them a latency chain over the same 270 edges).  Here workgroup (copy, graph) of
// the stacked (plain | masked) batch reads the graph's int64 edge list ONCE, groups it by target and by source in LDS
// (histograms, one-wave scan, stable placement — the arithmetic of plan_segmented_body), forms its pass's inputs (the
// masked copy: x * prob, e = sigmoid(<xm_src | xm_dst, prob_bias>), ew * e, its share of the regulariser, its row of the
// SNP mask; the plain copy: x, ew as they are), runs gcn_norm and the layers out of LDS, and only then writes everything
// the rest of the step reads — the plan arrays of the batch and of its 2-copy replica (the backward kernels and the mask
// backward walk them), x_in / ew_in / e, the regulariser partials, xcat — in one burst behind the last barrier.
// Extra workgroups behind the 2 G graph workgroups carry the step's dropout rider (csrc/dropout.h), as the plan build's did.
#include "dropout.h"
#include "mask_reg.h"
struct SfFront {
  int64_t n_nodes, n_edges;
  int n_graphs;
  const int64_t *ei, *node_ptr, *edge_ptr;
  int32_t *src32, *dst32, *tgt_ptr, *tgt_perm, *src_ptr, *src_perm, *loop_edge;             // plan of the batch
  int32_t *r_src32, *r_dst32, *r_tgt_ptr, *r_tgt_perm, *r_src_ptr, *r_src_perm, *r_loop_edge;   // of its 2-copy replica
  int32_t* status;
  const float *x, *prob, *pb, *ew;
  float *x_in, *ew_in, *e;
  const float* snps_logits;       // [n_snps]
  int n_snps;
  float l1_x, ent_x, l1_e, ent_e, eps;
  float* reg_partial;             // [n_graphs]: their SUM is loss_probability
  const float* snps_feat;         // [n_graphs, n_snps]
  float* snps_full;               // [2 n_graphs, n_snps] = (feat | feat * sigmoid(logits))
};

template <int F>
__global__ void __launch_bounds__(SF_T)
k_sgcn_front_fwd(int R, int Emax, int H0, int L, const SfFront fr, SfParams prm, float* __restrict__ xcat,
                 int64_t d_total, const DropSegs d_segs, unsigned long long* __restrict__ d_state,
                 float* __restrict__ d_out, const DropCounters d_cnt, unsigned d_blocks) {
  extern __shared__ float sf_lds[];
  const int G = fr.n_graphs;
  if ((int)blockIdx.x >= 2 * G) {                // the dropout rider: two of its 256-thread blocks per carrier workgroup
    dropout_masks_body(2u * (blockIdx.x - 2u * (unsigned)G) + (threadIdx.x >> 8), d_blocks, d_total, d_segs, d_state, d_out,
                       d_cnt, threadIdx.x & 255u);
    return;
  }
  float* lds = sf_lds;
  const SfLayout o = sf_layout(R, Emax, H0, F, L, 0, 1);
  const int tid = threadIdx.x, bd = (int)blockDim.x;
  const int copy = (int)blockIdx.x / G, g = (int)blockIdx.x - copy * G;
  SF_PROBE(0);
  // (uniform graphs: the node offset is g R — the loads of x do not wait for a pointer; node_ptr must agree, below)
  const int64_t nb = (int64_t)g * R, nb_given = fr.node_ptr[g], eb64 = fr.edge_ptr[g];
  const int nn = (int)(fr.node_ptr[g + 1] - nb_given), ne = (int)(fr.edge_ptr[g + 1] - eb64);
  const int32_t N32 = (int32_t)fr.n_nodes, E32 = (int32_t)fr.n_edges;
  // node features and mask factors: requested BEFORE the pointer words are waited for (the host has checked that the
  // batch holds n_graphs * R nodes, so the addresses are inside x whatever the pointers say)
  const int nx = R * H0;
  float xv[4], pv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + j * bd;
    xv[j] = i < nx ? fr.x[nb * H0 + i] : 0.f;
    pv[j] = (copy && i < nx) ? fr.prob[i] : 1.f;
  }
  // the offsets come from device memory (a loader may have handed over garbage): refuse anything that is not a graph of
  // R nodes inside the batch with at most Emax edges — status bit 0 (not a block-diagonal batch) / bit 1 (too many edges)
  if (nn != R || nb_given != nb || ne < 0 || eb64 < 0 || nb + nn > fr.n_nodes || eb64 + ne > fr.n_edges) {
    if (tid == 0) atomicOr(fr.status, 1);
    return;
  }
  if (ne > Emax) {
    if (tid == 0) atomicOr(fr.status, 2);
    return;
  }
  const int32_t eb = (int32_t)eb64;
  int32_t* ssrc = lds_i32(lds, o.t.src);
  int32_t* sdst = lds_i32(lds, o.t.dst);
  int32_t* stptr = lds_i32(lds, o.t.tptr);
  int32_t* stperm = lds_i32(lds, o.t.tperm);
  int32_t* sloop = lds_i32(lds, o.n.loop);
  int32_t* ct = lds_i32(lds, o.fct);
  int32_t* cs = lds_i32(lds, o.fcs);
  int32_t* ssperm = lds_i32(lds, o.fsperm);
  // ---- stage: one batch of loads per thread (edge endpoints, weight; node features and mask factors are on their way)
  int64_t es[2] = {0, 0}, ed[2] = {0, 0};
  float ev[2] = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = tid + j * bd;
    if (k < ne) {
      es[j] = fr.ei[eb64 + k];
      ed[j] = fr.ei[fr.n_edges + eb64 + k];
      ev[j] = fr.ew[eb64 + k];
    }
  }
  const int wstride = F * (F > H0 ? F : H0) + F;
  const int wtotal = F * H0 + F + (L - 1) * (F * F + F);
  for (int j = tid; j < wtotal; j += bd) {                        // W_l transposed | b_l, as sf_stage lays them out
    int off = 0;
    for (int l = 0; l < L; ++l) {
      const int fin = l == 0 ? H0 : F, nw = F * fin, n = nw + F;
      if (j < off + n) {
        const int r = j - off;
        lds[o.wallT + l * wstride + (r < nw ? (r % fin) * F + r / fin : r)] = r < nw ? prm.W[l][r] : prm.b[l][r - nw];
        break;
      }
      off += n;
    }
  }
  for (int i = tid; i <= R; i += bd) { ct[i] = 0; cs[i] = 0; }
  for (int i = tid; i < R; i += bd) sloop[i] = -1;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = tid + j * bd;
    if (k < ne) {
      int64_t s = es[j] - nb, d = ed[j] - nb;
      if (s < 0 || s >= R || d < 0 || d >= R) { bad = true; s = 0; d = 0; }
      ssrc[k] = (int32_t)s;
      sdst[k] = (int32_t)d;
      lds[o.t.ew + k] = ev[j];
    }
  }
  for (int k = tid + 2 * bd; k < ne; k += bd) {                   // graphs with more than 2 * 512 edges
    int64_t s = fr.ei[eb64 + k] - nb, d = fr.ei[fr.n_edges + eb64 + k] - nb;
    if (s < 0 || s >= R || d < 0 || d >= R) { bad = true; s = 0; d = 0; }
    ssrc[k] = (int32_t)s;
    sdst[k] = (int32_t)d;
    lds[o.t.ew + k] = fr.ew[eb64 + k];
  }
  if (bad) atomicOr(fr.status, 1);                                 // an edge leaves its graph: not a PyG batch
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid + j * bd;
    if (i < nx) lds[o.t.x + i] = xv[j] * pv[j];                      // the masked copy's x * prob (plain: x * 1 = x)
  }
  for (int i = tid + 4 * bd; i < nx; i += bd) lds[o.t.x + i] = fr.x[nb * H0 + i] * (copy ? fr.prob[i] : 1.f);
  __syncthreads();
  SF_PROBE(1);
  // ---- plan: histograms by target / by source, last stored loop per node
  for (int k = tid; k < ne; k += bd) {
    const int s = ssrc[k], d = sdst[k];
    atomicAdd(&ct[d + 1], 1);
    atomicAdd(&cs[s + 1], 1);
    if (s == d) atomicMax(&sloop[s], k);
  }
  __syncthreads();
  if (tid < 64) {                                                  // both scans by one wave (plan_segmented_body)
    const int per = (R + 64) / 64, lo = tid * per, hi = min(R + 1, lo + per);
    int st = 0, ss = 0;
    for (int i = lo; i < hi; ++i) { st += ct[i]; ss += cs[i]; }
    int pt = st, ps = ss;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int a = __shfl_up(pt, off, 64), b = __shfl_up(ps, off, 64);
      if (tid >= off) { pt += a; ps += b; }
    }
    int rt = pt - st, rs = ps - ss;
    for (int i = lo; i < hi; ++i) {
      rt += ct[i]; rs += cs[i];
      ct[i] = rt; cs[i] = rs;
    }
  }
  __syncthreads();
  SF_PROBE(2);
  // stable placement (one thread per edge: its slot = the number of EARLIER edges with the same key), the masked copy's
  // edge probabilities beside it
  const float* pbv = fr.pb;
  float racc = 0.f;
  for (int k = tid; k < ne; k += bd) {
    const int kd = sdst[k], ks = ssrc[k];
    int rd = 0, rs = 0;
#pragma unroll 8
    for (int j = 0; j < k; ++j) {
      rd += (sdst[j] == kd);
      rs += (ssrc[j] == ks);
    }
    stperm[ct[kd] + rd] = k;
    ssperm[cs[ks] + rs] = k;
    if (copy) {
      float z = 0.f;
      for (int h = 0; h < H0; ++h) z += lds[o.t.x + ks * H0 + h] * pbv[h];
      for (int h = 0; h < H0; ++h) z += lds[o.t.x + kd * H0 + h] * pbv[H0 + h];
      const float p = 1.f / (1.f + expf(-z));
      lds[o.fe + k] = p;
      racc += em_reg_term(p, fr.l1_e, fr.ent_e, fr.eps) / (float)fr.n_edges;
    }
  }
  for (int i = tid; i <= R; i += bd) stptr[i] = ct[i];
  for (int i = tid; i < R; i += bd) {                              // (gcn_lists reads batch-global loop edge ids)
    const int32_t l = sloop[i];
    sloop[i] = l >= 0 ? eb + l : -1;
  }
  __syncthreads();
  SF_PROBE(3);
  if (copy)
    for (int k = tid; k < ne; k += bd) lds[o.t.ew + k] = lds[o.t.ew + k] * lds[o.fe + k];     // ew * e
  __syncthreads();
  gcn_lists<false>(lds, o.t, o.n, R, ne, eb, bd);
  SF_PROBE(4);          // (the first barrier inside sf_layer orders its lists before their use)
  float* H = lds + o.act;
  float* Y = lds + o.ycat;
  const int D = L * F;
  for (int l = 0; l < L; ++l) {
    const float* wl = lds + o.wallT + l * wstride;
    sf_layer<F>(lds, o, R, l == 0 ? H0 : F, l == 0 ? lds + o.t.x : Y + (l - 1) * F, l == 0 ? H0 : D, H, Y + l * F, D, wl,
                wl + F * (l == 0 ? H0 : F));
  }
  SF_PROBE(5);
  // loss_probability: the edge term of this graph; workgroup (1, 0) adds the two node-level means (the same sums as
  // k_edge_mask_fwd<true>, grouped per graph instead of per 256 edges)
  if (copy) {
    if (g == 0) {
      const int64_t np = (int64_t)R * H0;
      for (int i = tid; i < np; i += bd)
        racc += em_reg_term(1.f / (1.f + expf(-fr.prob[i])), fr.l1_x, fr.ent_x, fr.eps) / (float)np;
      if (fr.snps_logits)
        for (int i = tid; i < fr.n_snps; i += bd)
          racc += em_reg_term(1.f / (1.f + expf(-fr.snps_logits[i])), fr.l1_x, fr.ent_x, fr.eps) / (float)fr.n_snps;
    }
    racc = block_sum_all(racc, lds + o.n.dis);                       // (dis is dead behind the last layer)
    if (tid == 0) fr.reg_partial[g] = racc;
  }
  SF_PROBE(6);
  // ---- the one store burst -----------------------------------------------------------------------------------------
  const int64_t nbo = (int64_t)copy * fr.n_nodes + nb, ebo = (int64_t)copy * fr.n_edges + eb64;
  for (int q = tid; q < R * D / 4; q += bd)
    reinterpret_cast<float4*>(xcat + nbo * D)[q] = reinterpret_cast<const float4*>(Y)[q];
  for (int i = tid; i < nx; i += bd) fr.x_in[nbo * H0 + i] = lds[o.t.x + i];
  for (int k = tid; k < ne; k += bd) {
    fr.ew_in[ebo + k] = lds[o.t.ew + k];
    if (copy) fr.e[eb64 + k] = lds[o.fe + k];
    const int32_t s = (int32_t)nb + ssrc[k], d = (int32_t)nb + sdst[k];
    const int32_t tp = eb + stperm[k], sp = eb + ssperm[k];
    fr.r_src32[ebo + k] = s + copy * N32;
    fr.r_dst32[ebo + k] = d + copy * N32;
    fr.r_tgt_perm[ebo + k] = tp + copy * E32;
    fr.r_src_perm[ebo + k] = sp + copy * E32;
    if (!copy) {
      fr.src32[eb64 + k] = s;
      fr.dst32[eb64 + k] = d;
      fr.tgt_perm[eb64 + k] = tp;
      fr.src_perm[eb64 + k] = sp;
    }
  }
  for (int i = tid; i < R; i += bd) {
    const int32_t tp = eb + ct[i], sp = eb + cs[i], le = sloop[i];
    fr.r_tgt_ptr[nbo + i] = tp + copy * E32;
    fr.r_src_ptr[nbo + i] = sp + copy * E32;
    fr.r_loop_edge[nbo + i] = le >= 0 ? le + copy * E32 : -1;
    if (!copy) {
      fr.tgt_ptr[nb + i] = tp;
      fr.src_ptr[nb + i] = sp;
      fr.loop_edge[nb + i] = le;
    }
  }
  if (g == G - 1 && tid == 0) {
    if (copy) {
      fr.r_tgt_ptr[2 * fr.n_nodes] = 2 * E32;
      fr.r_src_ptr[2 * fr.n_nodes] = 2 * E32;
    } else {
      fr.tgt_ptr[fr.n_nodes] = E32;
      fr.src_ptr[fr.n_nodes] = E32;
    }
  }
  if (fr.snps_feat)
    for (int j = tid; j < fr.n_snps; j += bd) {
      const float v = fr.snps_feat[(int64_t)g * fr.n_snps + j];
      fr.snps_full[((int64_t)copy * G + g) * fr.n_snps + j] =
          copy ? v * (1.f / (1.f + __expf(-fr.snps_logits[j]))) : v;                         // = k_snps_mask_fwd, bit for bit
    }
  SF_PROBE(7);
}

// parameter-gradient partial row of one graph: [ dW_0 (F x H0) | db_0 (F) | dW_1 (F x F) | db_1 | ... ]
__host__ __device__ inline int sf_param_offset(int l, int H0, int F) {
  return l == 0 ? 0 : (F * H0 + F) + (l - 1) * (F * F + F);
}

extern "C" int igcn_sgcn_stack_param_floats(int H0, int F, int L) { return sf_param_offset(L, H0, F); }

// The edge-mask backward's node pass (k_edge_mask_bwd_nodes<4> of csrc/sgcn.hip) for the stacked (plain | masked) batch
// of a train step, done by the masked copy's workgroups of k_sgcn_stack_bwd<F, true>: graph g of the masked copy is
// workgroup n_graphs + g, and what that pass fetches — the lists, d_xm (dX of layer 0) and d_ewm (gcn_norm's edge
// gradients) — is in its LDS already, in graph-local numbering.  x, prob, ew, e, d_e are the batch's own (plain) arrays.
struct SfMaskBwd {
  int n_graphs, n_edges;                           // of ONE copy
  const float *x, *prob, *pb, *ew, *e;
  const float* d_e;                                // or NULL
  const float* greg;                               // d loss / d (regulariser), device scalar; or NULL
  float l1_e, ent_e, eps, inv_ne;
  float* gx;                                       // [N, H0]  g_i * x_i
  float* g_part;                                   // [N, H0]  g_i: the tail launch writes dx = g * prob + dx_plain
  float* pb_partial;                               // [n_graphs, 2 IGCN_MAX_H0]  (sum_i x_i prob S_i | sum_i x_i prob T_i)
};

// dz_k = up_k e_k (1 - e_k) as its two factors, a_k = up_k e_k into A and b_k = 1 - e_k into Bf: a lane of the node pass
// takes its first list entry as a_k b_k and every further one as one fused multiply-add onto its sum, and the sums
// here are held to those bits — so the roundings are spelled out and nothing is left to contraction.
__device__ __forceinline__ void sf_mask_edge_term(const SfMaskBwd& mk, float gre, float d_ewm, float ewk, float ek,
                                                  float dek, float& a, float& b) {
  float up;
  {
#pragma clang fp contract(off)
    up = d_ewm * ewk + dek;
  }
  if (mk.greg) up = __fmaf_rn(gre, em_reg_grad(ek, mk.l1_e, mk.ent_e, mk.eps), up);
  {
#pragma clang fp contract(off)
    a = up * ek;
    b = 1.f - ek;
  }
}

// one lane's share of a node's list [p0, p1) (entries p0 + sub, p0 + sub + 4, ... in list order)
__device__ __forceinline__ float sf_mask_list_sum(const int32_t* perm, const float* A, const float* Bf, int p0, int p1,
                                                  int sub) {
  float s = 0.f;
  int p = p0 + sub;
  if (p < p1) {
#pragma clang fp contract(off)
    const int k = perm[p];
    s = A[k] * Bf[k];
  }
  for (p += 4; p < p1; p += 4) {
    const int k = perm[p];
    s = __fmaf_rn(A[k], Bf[k], s);
  }
  return s;
}

template <int F, bool MASK>
__global__ void __launch_bounds__(SF_TB)
k_sgcn_stack_bwd(int R, int Emax, int H0, int L, const float* __restrict__ x_in, const float* __restrict__ ew_in,
                 const int32_t* __restrict__ src32, const int32_t* __restrict__ dst32,
                 const int32_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt_perm,
                 const int32_t* __restrict__ src_ptr, const int32_t* __restrict__ src_perm,
                 const int32_t* __restrict__ loop_edge, SfParams prm, const float* __restrict__ dxcat,
                 const float* __restrict__ dxcat2 /*a second consumer's gradient, added on load; or NULL*/,
                 float* __restrict__ dx_in, float* __restrict__ dew_in, float* __restrict__ dpar_partial, int P,
                 int32_t* __restrict__ status, SfMaskBwd mk) {
  extern __shared__ float sf_lds[];
  const SfLayout o = sf_layout(R, Emax, H0, F, L, 1);
  const int tid = threadIdx.x;
  const int64_t nb = (int64_t)blockIdx.x * R;
  // MASK: the masked copy's workgroups consume d_xm / d_ewm themselves (below) instead of storing dx_in / dew_in
  const bool masked = MASK && (int)blockIdx.x >= mk.n_graphs;
  const int64_t nbp = nb - (int64_t)mk.n_graphs * R;   // the graph's first node in the batch's own numbering
  SF_PROBE(8);
  const int32_t eb = tgt_ptr[nb];
  const int D = L * F;
  // the incoming gradient rows travel with the staging loads: issued first, parked in registers, stored behind them
  float4 dyv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    dyv[j] = tid + j * SF_TB < R * D / 4 ? reinterpret_cast<const float4*>(dxcat + nb * D)[tid + j * SF_TB]
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
  if (dxcat2) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (tid + j * SF_TB < R * D / 4) {
        const float4 b = reinterpret_cast<const float4*>(dxcat2 + nb * D)[tid + j * SF_TB];
        dyv[j].x += b.x; dyv[j].y += b.y; dyv[j].z += b.z; dyv[j].w += b.w;
      }
  }
  const int ne = sf_stage<true>(sf_lds, o, R, Emax, H0, nb, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, src_ptr,
                                src_perm, loop_edge, prm, F, L, status);
  if (ne < 0) {                                        // refused graph: defined (zero) outputs, flagged in `status`
    if (masked) {
      for (int e = tid; e < R * H0; e += SF_TB) mk.gx[nbp * H0 + e] = mk.g_part[nbp * H0 + e] = 0.f;
      if (tid < 2 * IGCN_MAX_H0) mk.pb_partial[(int64_t)((int)blockIdx.x - mk.n_graphs) * 2 * IGCN_MAX_H0 + tid] = 0.f;
    } else {
      for (int e = tid; e < R * H0; e += SF_TB) dx_in[nb * H0 + e] = 0.f;
    }
    for (int e = tid; e < P; e += SF_TB) dpar_partial[(int64_t)blockIdx.x * P + e] = 0.f;
    return;
  }
  SF_PROBE(9);
  const int32_t* ssptr = lds_i32(sf_lds, o.t.sptr);
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (tid + j * SF_TB < R * D / 4) reinterpret_cast<float4*>(sf_lds + o.dycat)[tid + j * SF_TB] = dyv[j];
  for (int e = tid + 2 * SF_TB; e < R * D / 4; e += SF_TB)
  {
    float4 a = reinterpret_cast<const float4*>(dxcat + nb * D)[e];
    if (dxcat2) {
      const float4 b = reinterpret_cast<const float4*>(dxcat2 + nb * D)[e];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    reinterpret_cast<float4*>(sf_lds + o.dycat)[e] = a;
  }
  // ---- forward, every transform kept: H_l at act + l R F; outputs in the concatenated layout
  float* Ycat = sf_lds + o.ycat;
  for (int l = 0; l < L; ++l) {
    const float* wl = sf_lds + o.wallT + l * (F * (F > H0 ? F : H0) + F);
    sf_layer<F>(sf_lds, o, R, l == 0 ? H0 : F, l == 0 ? sf_lds + o.t.x : Ycat + (l - 1) * F, l == 0 ? H0 : D,
                sf_lds + o.act + l * R * F, Ycat + l * F, D, wl, wl + F * (l == 0 ? H0 : F));
  }
  SF_PROBE(10);
  for (int k = tid; k < ne; k += SF_TB) sf_lds[o.n.dwhat + k] = 0.f;
  for (int i = tid; i < R; i += SF_TB) sf_lds[o.n.dwloop + i] = 0.f;
  float* G = sf_lds + o.g;
  float* dH = sf_lds + o.dh;
  float* dX = sf_lds + o.dx;
  float* prow = sf_lds + o.prow;                       // this graph's parameter-gradient row, stored at the very end
  // ---- backward, last layer first.  Sums over the graph's nodes (db, dW) are split over thread groups whose
  // partials meet in `red` (db) / `red + SF_TB` (dW) behind the next barrier; the dW partials of a layer are summed
  // at the top of the next iteration (or after the loop).
  float* red_db = sf_lds + o.red;
  float* red_dw = sf_lds + o.red + SF_TB;
  int pend_off = -1, pend_n = 0, pend_parts = 0;       // dW partials waiting (in red_dw or in a dead H_l)
  const float* pend_src = red_dw;
  for (int l = L - 1; l >= 0; --l) {
    SF_PROBE(11 + (L - 1 - l));
    const int fin = l == 0 ? H0 : F;
    const float* H = sf_lds + o.act + l * R * F;
    const float* Y = Ycat + l * F;                     // row stride D
    const float* xin = l == 0 ? sf_lds + o.t.x : Ycat + (l - 1) * F;
    const int ldx = l == 0 ? H0 : D;
    if (pend_off >= 0)                                 // dW of the layer above
      for (int e = tid; e < pend_n; e += SF_TB) {
        float acc = 0.f;
        for (int p2 = 0; p2 < pend_parts; ++p2) acc += pend_src[p2 * pend_n + e];
        prow[pend_off + e] = acc;
      }
    // work items are (node, feature quad) / edges with 16-byte LDS accesses throughout (see sf_layer)
    constexpr int FQ = F / 4;
    // G = (d xcat[:, l] + d X_l from the layer above) * [Y_l > 0]
    for (int e = tid; e < R * FQ; e += SF_TB) {
      const int i = e / FQ, q = e - i * FQ;
      float4 g = *reinterpret_cast<const float4*>(sf_lds + o.dycat + i * D + l * F + q * 4);
      if (l < L - 1) {
        const float4 d4 = *reinterpret_cast<const float4*>(dX + i * F + q * 4);
        g.x += d4.x; g.y += d4.y; g.z += d4.z; g.w += d4.w;
      }
      const float4 y4 = *reinterpret_cast<const float4*>(Y + i * D + q * 4);
      g.x = y4.x > 0.f ? g.x : 0.f; g.y = y4.y > 0.f ? g.y : 0.f;
      g.z = y4.z > 0.f ? g.z : 0.f; g.w = y4.w > 0.f ? g.w : 0.f;
      *reinterpret_cast<float4*>(G + i * F + q * 4) = g;
    }
    const float* Wl = sf_lds + o.wall + l * (F * (F > H0 ? F : H0) + F);            // W_l [fo][fi] for dX = dH W
    __syncthreads();
    // dH = A_hat^T G (by-source lists, four entries per step); coefficient gradients accumulate over the layers
    for (int e = tid; e < R * FQ; e += SF_TB) {
      const int sn = e / FQ, q = e - sn * FQ;
      float4 acc = gcn_walk4(lds_i32(sf_lds, o.n.bdst), sf_lds + o.n.bwhat, ssptr[sn], ssptr[sn + 1], G, F, q);
      const float wl = sf_lds[o.n.wloop + sn];
      const float4 gs = *reinterpret_cast<const float4*>(G + sn * F + q * 4);
      acc.x += wl * gs.x; acc.y += wl * gs.y; acc.z += wl * gs.z; acc.w += wl * gs.w;
      *reinterpret_cast<float4*>(dH + sn * F + q * 4) = acc;
    }
    gcn_coef_grads(sf_lds, o.t, o.n, R, ne, G, H, F, FQ, SF_TB);
    constexpr int DB_PARTS = SF_TB / F < 16 ? SF_TB / F : 16;
    gcn_bias_partials(G, R, F, DB_PARTS, red_db);      // bias gradient: 16 thread groups share the node range
    __syncthreads();
    if (tid < F) {
      float acc = 0.f;
#pragma unroll
      for (int p2 = 0; p2 < DB_PARTS; ++p2) acc += red_db[p2 * F + tid];
      prow[sf_param_offset(l, H0, F) + F * fin + tid] = acc;
    }
    // dW_l = dH^T X_{l-1} (partials)   and   dX_{l-1} = dH W_l
    if (fin == F) {
      // work item = (fo, input quad, node part): one dH word and one 16-byte X read feed four FMAs (with one item per
      // output word the 90-node sums were 180 4-byte LDS reads per thread)
      // partials in H_l (R F floats): the transform of this layer has served its last reader (the coefficient gradients
      // above) and no lower layer touches it
      const int n_out = F * F, nq = F * FQ;
      int parts = SF_TB / nq;
      const int cap = (R * F) / n_out;                  // whole [F, F] partials that fit H_l
      float* pdst = sf_lds + o.act + l * R * F;
      if (cap < 1) {                                    // fewer nodes than features: one partial, in `red` (>= F F floats)
        pdst = red_dw;
        parts = 1;
      } else {
        parts = parts > cap ? cap : parts;
      }
      parts = parts > 16 ? 16 : (parts < 1 ? 1 : parts);
      for (int idx = tid; idx < parts * nq; idx += SF_TB) {
        const int e = idx % nq, part = idx / nq;
        const int fo = e / FQ, q = e - fo * FQ;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = part; i < R; i += parts) {
          const float d = dH[i * F + fo];
          const float4 x4 = *reinterpret_cast<const float4*>(xin + i * ldx + q * 4);
          acc.x += d * x4.x; acc.y += d * x4.y; acc.z += d * x4.z; acc.w += d * x4.w;
        }
        *reinterpret_cast<float4*>(pdst + part * n_out + fo * F + q * 4) = acc;
      }
      pend_off = sf_param_offset(l, H0, F);
      pend_n = n_out;
      pend_parts = parts;
      pend_src = pdst;
    } else {
      const int n_out = F * fin;
      int parts = SF_TB / n_out;
      parts = parts > 16 ? 16 : (parts < 1 ? 1 : parts);
      for (int idx = tid; idx < parts * n_out; idx += SF_TB) {
        const int e = idx % n_out, part = idx / n_out;
        const int fo = e / fin, fi = e - fo * fin;
        float acc = 0.f;
        for (int i = part; i < R; i += parts) acc += dH[i * F + fo] * xin[i * ldx + fi];
        red_dw[idx] = acc;
      }
      pend_off = sf_param_offset(l, H0, F);
      pend_n = n_out;
      pend_parts = parts;
      pend_src = red_dw;
    }
    if (fin == F) {
      for (int e = tid; e < R * FQ; e += SF_TB) {      // d X_{l-1}[i, quad] = sum_fo dH[i, fo] W[fo, quad]
        const int i = e / FQ, q = e - i * FQ;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < FQ; ++c) {
          const float4 d4 = *reinterpret_cast<const float4*>(dH + i * F + c * 4);
          const float ds[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float4 w4 = *reinterpret_cast<const float4*>(Wl + (c * 4 + j) * F + q * 4);
            acc.x += ds[j] * w4.x; acc.y += ds[j] * w4.y; acc.z += ds[j] * w4.z; acc.w += ds[j] * w4.w;
          }
        }
        *reinterpret_cast<float4*>(dX + i * F + q * 4) = acc;
      }
    } else {
      for (int e = tid; e < R * fin; e += SF_TB) {
        const int i = e / fin, fi = e - i * fin;
        float acc = 0.f;
#pragma unroll
        for (int fo = 0; fo < F; ++fo) acc += dH[i * F + fo] * Wl[fo * fin + fi];
        dX[e] = acc;                                  // layer 0: d x_in, stored after the last barrier
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < pend_n; e += SF_TB) {          // dW of layer 0
    float acc = 0.f;
    for (int p2 = 0; p2 < pend_parts; ++p2) acc += pend_src[p2 * pend_n + e];
    prow[pend_off + e] = acc;
  }
  SF_PROBE(13);
  // the masked copy's own operands — this thread's edge and this thread's (node, feature) element — are requested here,
  // three phases ahead of their first use, and cost no register during the layer loop
  const int32_t ebp = eb - mk.n_edges;                 // the graph's first edge in the batch's own numbering
  float m_e = 0.f, m_ew = 0.f, m_de = 0.f, m_x = 0.f, m_p = 0.f;
  if (masked) {
    if (tid < ne) {
      m_e = mk.e[ebp + tid];
      m_ew = mk.ew[ebp + tid];
      if (mk.d_e) m_de = mk.d_e[ebp + tid];
    }
    if (tid < R * H0) {
      m_x = mk.x[nbp * H0 + tid];
      m_p = mk.prob[tid];
    }
  }
  // ---- gcn_norm backward (k_gcn_norm_bwd_deg / _edge of sgcn.hip, per graph)
  gcn_norm_bwd_products(sf_lds, o.t, o.n, ne, SF_TB);
  __syncthreads();
  if (!masked) {
    gcn_norm_bwd_edges(sf_lds, o.t, o.n, R, ne, eb, dew_in, SF_TB);
    for (int e = tid; e < R * H0; e += SF_TB) dx_in[nb * H0 + e] = dX[e];
  } else {
    // ---- edge-mask backward, node pass (formula and order of summation: k_edge_mask_bwd_nodes<4> of csrc/sgcn.hip).
    // v1 / v2, ddeg, dwloop and dX are reused as their last readers finish: the edge factors a_k | b_k, S_i, T_i and
    // x_i prob.
    gcn_norm_bwd_ddeg(sf_lds, o.t, o.n, R, SF_TB);
    __syncthreads();
    float* A = sf_lds + o.n.v1;
    float* Bf = sf_lds + o.n.v2;
    const float gre = mk.greg ? mk.greg[0] * mk.inv_ne : 0.f;
    for (int k = tid; k < ne; k += SF_TB) {
      const float d_ewm = gcn_norm_bwd_edge(sf_lds, o.t, o.n, eb, k);
      const bool own = k == tid;
      const float ek = own ? m_e : mk.e[ebp + k], ewk = own ? m_ew : mk.ew[ebp + k];
      const float dek = own ? m_de : (mk.d_e ? mk.d_e[ebp + k] : 0.f);
      float a, b;
      sf_mask_edge_term(mk, gre, d_ewm, ewk, ek, dek, a, b);
      A[k] = a;
      Bf[k] = b;
    }
    __syncthreads();
    float* Ss = sf_lds + o.n.ddeg;                     // S_i = sum_{k: src = i} dz_k, T_i = sum_{k: dst = i} dz_k:
    float* Ts = sf_lds + o.n.dwloop;                   // four lanes per node, combined as group_sum_all<4> does
    const int32_t* stptr = lds_i32(sf_lds, o.t.tptr);
    for (int idx = tid; idx < 4 * R; idx += SF_TB) {
      const int i = idx >> 2, sub = idx & 3;
      float S = sf_mask_list_sum(lds_i32(sf_lds, o.t.sperm), A, Bf, ssptr[i], ssptr[i + 1], sub);
      float T = sf_mask_list_sum(lds_i32(sf_lds, o.t.tperm), A, Bf, stptr[i], stptr[i + 1], sub);
      S = group_sum_all<4>(S);
      T = group_sum_all<4>(T);
      if (sub == 0) {
        Ss[i] = S;
        Ts[i] = T;
      }
    }
    __syncthreads();
    // g_i = d_xm_i + pb[:h0] S_i + pb[h0:] T_i per (node, feature) element; the first element of a thread leaves with
    // the last stores of the kernel (nothing is stored in front of a barrier)
    float g0 = 0.f, gx0 = 0.f;
    for (int e = tid; e < R * H0; e += SF_TB) {
      const int i = e / H0, h = e - i * H0;
      const bool own = e == tid;
      const float xv = own ? m_x : mk.x[nbp * H0 + e], pv = own ? m_p : mk.prob[e];
      float g, gxv, xp;
      {
#pragma clang fp contract(off)
        g = dX[e] + mk.pb[h] * Ss[i] + mk.pb[H0 + h] * Ts[i];
        gxv = g * xv;
        xp = xv * pv;
      }
      dX[e] = xp;
      if (own) {
        g0 = g;
        gx0 = gxv;
      } else {
        mk.g_part[nbp * H0 + e] = g;
        mk.gx[nbp * H0 + e] = gxv;
      }
    }
    __syncthreads();
    // the graph's bias-gradient partial row: 16 row lanes x 16 column slots, lanes combined in order (the layout
    // k_edge_mask_bwd_prob sums: S columns at [0, h0), T columns at [IGCN_MAX_H0, IGCN_MAX_H0 + h0))
    static_assert(2 * IGCN_MAX_H0 <= 16 && SF_TB >= 256, "the bias-gradient partials take 16 x 16 threads");
    const int rl = tid >> 4, cs = tid & 15;
    if (tid < 256) {
      float t = 0.f;
      if (cs < 2 * H0) {
        const int h = cs < H0 ? cs : cs - H0;
        const float* st = cs < H0 ? Ss : Ts;
        for (int i = rl; i < R; i += 16) t += dX[i * H0 + h] * st[i];
      }
      red_db[tid] = t;
    }
    __syncthreads();
    if (tid < 2 * H0) {
      float a = 0.f;
      for (int l = 0; l < 16; ++l) a += red_db[l * 16 + tid];
      mk.pb_partial[(int64_t)((int)blockIdx.x - mk.n_graphs) * 2 * IGCN_MAX_H0 + (tid < H0 ? tid : IGCN_MAX_H0 + tid - H0)] = a;
    }
    if (tid < R * H0) {
      mk.g_part[nbp * H0 + tid] = g0;
      mk.gx[nbp * H0 + tid] = gx0;
    }
  }
  for (int e = tid; e < P; e += SF_TB) dpar_partial[(int64_t)blockIdx.x * P + e] = prow[e];
  SF_PROBE(14);
}

// The launch switches below instantiate F = 4, 8, 16 and 32 only (default: 32): igcn_stack_width_ok must admit no other
static_assert(IGCN_STACK_MIN_WIDTH == 4 && IGCN_STACK_MAX_WIDTH == 32,
              "a new layer width needs a kernel instance and a case in every launch switch of this file");
static int sf_check(const char* nm, int64_t n_graphs, int R, int max_edges, int H0, int F, int L, int backward) {
  IGCN_REQUIRE(n_graphs > 0 && R > 0 && max_edges >= 0 && H0 >= 1 && H0 <= IGCN_MAX_H0 && L >= 1 &&
                   L <= IGCN_STACK_MAX_LAYERS,
               "%s: bad sizes (1 <= H0 <= %d, 1 <= L <= %d)", nm, IGCN_MAX_H0, IGCN_STACK_MAX_LAYERS);
  if (!igcn_stack_width_ok(F) ||
      igcn_sgcn_stack_lds_bytes(R, max_edges, H0, F, L, backward) > IGCN_LDS_BUDGET_BYTES) {
    igcn_set_error("%s: needs F in {4, 8, 16, 32} and a graph that fits %d KB of LDS (R=%d, E<=%d, F=%d, L=%d)", nm,
                   IGCN_LDS_BUDGET_BYTES / 1024, R, max_edges, F, L);
    return IGCN_ERR_UNSUPPORTED;
  }
  return IGCN_OK;
}

extern "C" int igcn_sgcn_stack_fwd(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                                   const float* ew_in, const int32_t* src32, const int32_t* dst32,
                                   const int32_t* tgt_ptr, const int32_t* tgt_perm, const int32_t* loop_edge,
                                   const float* const* W /*HOST [L]*/, const float* const* b /*HOST [L]*/, float* xcat,
                                   int32_t* status /*device word or NULL*/, void* stream) {
  int rc = sf_check("sgcn_stack_fwd", n_graphs, R, max_edges, H0, F, L, 0);
  if (rc) return rc;
  IGCN_REQUIRE(((uintptr_t)xcat & 15) == 0, "sgcn_stack_fwd: xcat must be 16-byte aligned");
  SfParams prm = {};
  for (int l = 0; l < L; ++l) { prm.W[l] = W[l]; prm.b[l] = b[l]; }
  const size_t lds = igcn_sgcn_stack_lds_bytes(R, max_edges, H0, F, L, 0);
  hipStream_t st = (hipStream_t)stream;
#define SF_FWD(FV)                                                                                                \
  {                                                                                                               \
    if (lds > 64 * 1024) IGCN_ALLOW_BIG_LDS((k_sgcn_stack_fwd<FV>));                                              \
    hipLaunchKernelGGL((k_sgcn_stack_fwd<FV>), dim3((unsigned)n_graphs), dim3(SF_T), lds, st, R, max_edges, H0, L, \
                       x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, loop_edge, prm, xcat, status);                \
  }
  switch (F) {
    case 4: SF_FWD(4) break;
    case 8: SF_FWD(8) break;
    case 16: SF_FWD(16) break;
    default: SF_FWD(32) break;
  }
#undef SF_FWD
  IGCN_CHECK_LAUNCH("sgcn_stack_fwd");
  return IGCN_OK;
}

extern "C" size_t igcn_sgcn_front_lds_bytes(int R, int max_edges, int H0, int F, int L) {
  return (size_t)sf_layout(R, max_edges, H0, F, L, 0, 1).total * 4;
}

// The front of the image branch of a train step (see k_sgcn_front_fwd): plan of the batch + of its 2-copy replica, the
// stacked (plain | masked) inputs x_in [2N, H0] / ew_in [2E], the edge mask e [E], loss_probability as reg_partial
// [n_graphs] (their sum), the SNP mask snps_full [2 n_graphs, n_snps], and xcat [2N, L F] — one launch, which also
// carries a dropout rider waiting on the stream.  Uniform graphs of R nodes, at most max_edges edges each.
extern "C" int igcn_sgcn_front_fwd(int64_t n_nodes, int64_t n_edges, int n_graphs, int R, int max_edges, int H0, int F,
                                   int L, const int64_t* edge_index, const int64_t* node_ptr, const int64_t* edge_ptr,
                                   int32_t* const* plan /*HOST [7]: src32 dst32 tgt_ptr tgt_perm src_ptr src_perm loop_edge*/,
                                   int32_t* const* plan2 /*HOST [7]: the same arrays of the 2-copy replica*/,
                                   int32_t* status, const float* x, const float* prob, const float* prob_bias,
                                   const float* ew, float* x_in, float* ew_in, float* e, const float* snps_logits,
                                   int n_snps, float l1_x, float ent_x, float l1_e, float ent_e, float eps,
                                   float* reg_partial, const float* snps_feat, float* snps_full,
                                   const float* const* W /*HOST [L]*/, const float* const* b /*HOST [L]*/, float* xcat,
                                   void* stream) {
  int rc = sf_check("sgcn_front_fwd", 2 * (int64_t)n_graphs, R, max_edges, H0, F, L, 0);
  if (rc) return rc;
  IGCN_REQUIRE(n_graphs > 0 && n_nodes == (int64_t)n_graphs * R && n_edges > 0 && 2 * n_nodes < ((int64_t)1 << 31) &&
                   2 * n_edges < ((int64_t)1 << 31),
               "sgcn_front_fwd: uniform graphs of R nodes, sizes of the 2-copy batch inside int32");
  IGCN_REQUIRE(edge_index && node_ptr && edge_ptr && plan && plan2 && status && x && prob && prob_bias && ew && x_in &&
                   ew_in && e && reg_partial && xcat && ((uintptr_t)xcat & 15) == 0,
               "sgcn_front_fwd: null argument / xcat not 16-byte aligned");
  IGCN_REQUIRE(n_snps >= 0 && (snps_feat == nullptr || (snps_logits && snps_full && n_snps > 0)),
               "sgcn_front_fwd: the SNP mask needs logits and an output");
  for (int i = 0; i < 7; ++i) IGCN_REQUIRE(plan[i] && plan2[i], "sgcn_front_fwd: null plan array %d", i);
  const size_t lds = igcn_sgcn_front_lds_bytes(R, max_edges, H0, F, L);
  if (lds > IGCN_LDS_BUDGET_BYTES) {
    igcn_set_error("sgcn_front_fwd: a graph of %d nodes / %d edges does not fit LDS", R, max_edges);
    return IGCN_ERR_UNSUPPORTED;
  }
  SfParams prm = {};
  for (int l = 0; l < L; ++l) { prm.W[l] = W[l]; prm.b[l] = b[l]; }
  SfFront fr = {n_nodes, n_edges, n_graphs, edge_index, node_ptr, edge_ptr,
                plan[0], plan[1], plan[2], plan[3], plan[4], plan[5], plan[6],
                plan2[0], plan2[1], plan2[2], plan2[3], plan2[4], plan2[5], plan2[6],
                status, x, prob, prob_bias, ew, x_in, ew_in, e, snps_logits, snps_logits ? n_snps : 0, l1_x, ent_x, l1_e,
                ent_e, eps, reg_partial, snps_feat, snps_full};
  hipStream_t st = (hipStream_t)stream;
  DropJob job = {};
  const bool ride = igcn_rider_dropout_take(st, job);
  const unsigned grid = 2u * (unsigned)n_graphs + (ride ? (job.blocks + 1u) / 2u : 0u);
#define SF_FRONT(FV)                                                                                              \
  {                                                                                                               \
    if (lds > 64 * 1024) IGCN_ALLOW_BIG_LDS((k_sgcn_front_fwd<FV>));                                              \
    hipLaunchKernelGGL((k_sgcn_front_fwd<FV>), dim3(grid), dim3(SF_T), lds, st, R, max_edges, H0, L, fr, prm, xcat, \
                       job.total, job.sg, job.state, job.out, job.cnt, job.blocks);                                \
  }
  switch (F) {
    case 4: SF_FRONT(4) break;
    case 8: SF_FRONT(8) break;
    case 16: SF_FRONT(16) break;
    default: SF_FRONT(32) break;
  }
#undef SF_FRONT
  IGCN_CHECK_LAUNCH("sgcn_front_fwd");
  return IGCN_OK;
}

// one launch of k_sgcn_stack_bwd: mk == NULL the plain kernel, else the one whose masked copy does the mask's node pass
static int sf_launch_bwd(const char* nm, int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                         const float* ew_in, const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                         const int32_t* tgt_perm, const int32_t* src_ptr, const int32_t* src_perm,
                         const int32_t* loop_edge, const float* const* W, const float* const* b, const float* dxcat,
                         const float* dxcat2, float* dx_in, float* dew_in, float* dparams, float* scratch,
                         int32_t* status, const SfMaskBwd* mk, hipStream_t st) {
  int rc = sf_check(nm, n_graphs, R, max_edges, H0, F, L, 1);
  if (rc) return rc;
  IGCN_REQUIRE(((uintptr_t)dxcat & 15) == 0 && ((uintptr_t)dxcat2 & 15) == 0,
               "%s: dxcat / dxcat2 must be 16-byte aligned", nm);
  SfParams prm = {};
  for (int l = 0; l < L; ++l) { prm.W[l] = W[l]; prm.b[l] = b[l]; }
  const size_t lds = igcn_sgcn_stack_lds_bytes(R, max_edges, H0, F, L, 1);
  const int P = igcn_sgcn_stack_param_floats(H0, F, L);
#define SF_BWD(FV, MV)                                                                                            \
  {                                                                                                               \
    if (lds > 64 * 1024) IGCN_ALLOW_BIG_LDS((k_sgcn_stack_bwd<FV, MV>));                                          \
    hipLaunchKernelGGL((k_sgcn_stack_bwd<FV, MV>), dim3((unsigned)n_graphs), dim3(SF_TB), lds, st, R, max_edges,  \
                       H0, L, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, src_ptr, src_perm, loop_edge, prm,    \
                       dxcat, dxcat2, dx_in, dew_in, scratch, P, status, mk ? *mk : SfMaskBwd{});                \
  }
#define SF_BWD_F(MV)                                                                                              \
  switch (F) {                                                                                                    \
    case 4: SF_BWD(4, MV) break;                                                                                  \
    case 8: SF_BWD(8, MV) break;                                                                                  \
    case 16: SF_BWD(16, MV) break;                                                                                \
    default: SF_BWD(32, MV) break;                                                                                \
  }
  if (mk) SF_BWD_F(true) else SF_BWD_F(false)
#undef SF_BWD_F
#undef SF_BWD
  IGCN_CHECK_LAUNCH(nm);
  return igcn_launch_reduce_rows_final(scratch, n_graphs, P, P, dparams, st);
}

extern "C" int igcn_sgcn_stack_bwd(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                                   const float* ew_in, const int32_t* src32, const int32_t* dst32,
                                   const int32_t* tgt_ptr, const int32_t* tgt_perm, const int32_t* src_ptr,
                                   const int32_t* src_perm, const int32_t* loop_edge, const float* const* W,
                                   const float* const* b, const float* dxcat, const float* dxcat2, float* dx_in,
                                   float* dew_in,
                                   float* dparams /*[param_floats]*/, float* scratch /*[n_graphs * param_floats]*/,
                                   int32_t* status /*device word or NULL*/, void* stream) {
  return sf_launch_bwd("sgcn_stack_bwd", n_graphs, R, max_edges, H0, F, L, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm,
                       src_ptr, src_perm, loop_edge, W, b, dxcat, dxcat2, dx_in, dew_in, dparams, scratch, status, nullptr,
                       (hipStream_t)stream);
}

// igcn_sgcn_stack_bwd on the 2-copy (plain | masked) plan of a train step + igcn_edge_mask_bwd_reg, as TWO launches
// instead of three: the masked copy's workgroups do the mask's node pass (SfMaskBwd), k_edge_mask_bwd_prob stays the tail
// and also writes dx.  n_graphs / n_edges: of ONE copy.  dx_plain [N, H0] and dew_plain [E] receive the plain copy's
// stack gradients; mask_scratch: 2 N H0 + n_graphs * 2 IGCN_MAX_H0 floats (gx | g | the graphs' bias-gradient rows).
extern "C" int igcn_sgcn_stack_bwd_mask(int64_t n_graphs, int64_t n_edges, int R, int max_edges, int H0, int F, int L,
                                        const float* x_in, const float* ew_in, const int32_t* src32, const int32_t* dst32,
                                        const int32_t* tgt_ptr, const int32_t* tgt_perm, const int32_t* src_ptr,
                                        const int32_t* src_perm, const int32_t* loop_edge, const float* const* W,
                                        const float* const* b, const float* dxcat, const float* dxcat2, float* dx_plain,
                                        float* dew_plain, float* dparams, float* scratch, int32_t* status, const float* x,
                                        const float* prob, const float* prob_bias, const float* ew, const float* e,
                                        const float* d_e, const float* d_reg, const float* snps_logits, int n_snps,
                                        float l1_x, float ent_x, float l1_e, float ent_e, float eps, float* dx,
                                        float* dprob, float* dprob_bias, float* dsnps, float* mask_scratch,
                                        const float* snps_feat, int snps_rows, const float* d_snps_full, void* stream) {
  IGCN_REQUIRE(n_graphs > 0 && n_edges > 0 && 2 * n_graphs * R < ((int64_t)1 << 31) && 2 * n_edges < ((int64_t)1 << 31) &&
                   n_edges < 16 * n_graphs * R,
               "sgcn_stack_bwd_mask: a sparse batch whose 2-copy sizes stay inside int32");
  IGCN_REQUIRE(x && prob && prob_bias && ew && e && dx_plain && dew_plain && dprob && dprob_bias && mask_scratch,
               "sgcn_stack_bwd_mask: null argument");
  const int64_t n = n_graphs * R;
  float* gx = mask_scratch;
  float* g_part = gx + n * H0;
  float* part = g_part + n * H0;
  const SfMaskBwd mk = {(int)n_graphs, (int)n_edges, x, prob, prob_bias, ew, e, d_e, d_reg, l1_e, ent_e, eps,
                        1.0f / (float)n_edges, gx, g_part, part};
  hipStream_t st = (hipStream_t)stream;
  int rc = sf_launch_bwd("sgcn_stack_bwd_mask", 2 * n_graphs, R, max_edges, H0, F, L, x_in, ew_in, src32, dst32, tgt_ptr,
                         tgt_perm, src_ptr, src_perm, loop_edge, W, b, dxcat, dxcat2, dx_plain, dew_plain, dparams, scratch,
                         status, &mk, st);
  if (rc) return rc;
  const EmReg rg = {d_reg, snps_logits, dsnps, snps_logits ? n_snps : 0, l1_x, ent_x, l1_e, ent_e, eps, snps_feat, nullptr,
                    d_snps_full, snps_feat ? snps_rows : 0};
  return igcn_launch_edge_mask_bwd_tail(n, R, H0, gx, part, n_graphs, g_part, dx_plain, dx, dprob, dprob_bias, prob, rg, st);
}
