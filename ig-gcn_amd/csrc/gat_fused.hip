// The GATConv stack of one brain graph, LDS-resident: L x (PyG 2.0.2 GATConv(heads=1, edge_dim=1, add_self_loops,
// fill_value='mean'), ReLU) + the jumping-knowledge concatenation of kernel/gcn_img_snp.py:217-221 with ifUseGAT as ONE
// kernel per direction, one 256-thread workgroup per graph.  The staged graph (its LDS layout and loader) is
// csrc/gcn_lds.h, shared with the GCN stacks; the edge array there called ew holds this stack's edge attribute ea.
//
// One layer, for a target i with incoming list E(i) (stored self-loops skipped: src == dst) plus one virtual loop whose
// edge value is the mean of ea over E(i) (0 for an empty list):
//   h = x W^T,  a_s = h . att_src,  a_d = h . att_dst,  c = lin_edge[:, 0] . att_edge
//   z_e = leaky_relu(a_s[src] + a_d[i] + ea_e c, 0.2),  alpha_e = exp(z_e - max z) / (sum exp(z - max z) + 1e-16)
//   y_i = relu(sum_e alpha_e h[src_e] + bias)
// The graph (x, the edge endpoints / values, the by-target lists of the per-graph plan) and every layer's parameters
// are staged in LDS once; HBM sees x and the edges in, the concatenated rows out.  The backward recomputes the forward
// in LDS (keeping every layer's alpha and node logits), then walks the layers top-down: ReLU mask, softmax backward
// (dz = alpha (dalpha - sum alpha dalpha)), leaky-ReLU slope, the two sources of dh (aggregation by source, the logit
// terms), the parameter gradients as one row per graph (summed by a final reduction, igcn_reduce_defer) and dx.
// With the edge attributes trained (SGCN_GAT's masked pass: EW instantiation, igcn_gat_stack_bwd_ew) each thread also
// owns the stored edges k = tid, tid + 256, ... and adds, layer by layer into its own element of dew,
//   d ea_k = c_l (dpre_l[k] + dpre_l[Emax + dst_k] / cnt_dst)      (the logit term + the mean-valued virtual loop)
// with cnt_i = the number of kept (src != dst) edges into i; a stored self-loop gets an exact 0.
// igcn_gat_stack_alpha hands out what the forward drops: every layer's alpha as dense [R][R] maps (k_gat_stack_alpha).
//
// Preconditions (host wrappers / per-graph plan builder): uniform graphs of R nodes (graph g = nodes [gR, (g+1)R), its
// edges contiguous in stored order); sums run in list order; no atomics: deterministic.
#include "common.h"
#include "gcn_lds.h"

#define GT_T 256
#define GT_SLOPE 0.2f

struct GtParams {
  // per layer: W [F, Fin] | bias [F] | att_src [F] | att_dst [F] | lin_edge [F] | att_edge [F]
  const float* p[6 * IGCN_STACK_MAX_LAYERS];
};

// offset of layer l's block in the flat parameter list (and in a gradient row): W | b | att_src | att_dst | le | ae
__host__ __device__ inline int gt_param_offset(int l, int H0, int F) {
  return l == 0 ? 0 : (F * H0 + 5 * F) + (l - 1) * (F * F + 5 * F);
}

struct GtLayout {
  GraphLds t;                                                                   // the staged graph
  int lea, prm, wt, ce, h, lgs, lgd, alpha, y;                                  // both directions
  int dcur, dh, dpre, das, dad, prow, red;                                      // backward
  int icnt;                                                                     // backward with d(edge attribute)
  int total;
};

// backward: 0 forward, 1 backward, 2 backward with the edge-attribute gradient (1 + one word per node)
__host__ __device__ inline GtLayout gt_layout(int R, int Emax, int H0, int F, int L, int backward) {
  GtLayout o;
  int p = 0;
  auto take = [&](int n) { int q = p; p += (n + 3) & ~3; return q; };
  const int fin_max = F > H0 ? F : H0;
  const int EA = Emax + R;                         // alpha / dpre: stored edge k at k, node i's virtual loop at Emax + i
  const int LK = backward ? L : 1;                 // the backward keeps every layer's logits and alpha
  graph_lds_layout(o.t, R, Emax, H0, take);
  o.lea = take(R);                                 // the virtual loop's edge value (mean of the kept incoming ea)
  o.prm = take(gt_param_offset(L, H0, F));         // every layer's parameters as stored
  o.wt = take(L * F * fin_max);                    // W_l transposed [fin][F]: the F lanes of a node read consecutive words
  o.ce = take(L);
  o.h = take(R * F);
  o.lgs = take(LK * R);
  o.lgd = take(LK * R);
  o.alpha = take(LK * EA);
  o.y = take(R * L * F);                           // concatenated layer outputs [R][L F]
  o.dcur = o.dh = o.dpre = o.das = o.dad = o.prow = o.red = o.icnt = 0;
  if (backward) {
    graph_lds_layout_bwd(o.t, R, Emax, take);
    o.dcur = take(R * F);                          // d(layer output), masked by the ReLU
    o.dh = take(R * F);
    o.dpre = take(EA);                             // d(pre-activation logit) per edge / virtual loop
    o.das = take(R);
    o.dad = take(R);
    o.prow = take(gt_param_offset(L, H0, F));
    o.red = take(4);
    if (backward == 2) o.icnt = take(R);           // 1 / (kept incoming edges of node i), 0 for none
  }
  o.total = p;
  return o;
}

extern "C" size_t igcn_gat_stack_lds_bytes(int R, int max_edges, int H0, int F, int L, int backward) {
  return (size_t)gt_layout(R, max_edges, H0, F, L, backward).total * 4;
}

extern "C" int igcn_gat_stack_param_floats(int H0, int F, int L) { return gt_param_offset(L, H0, F); }

__device__ __forceinline__ float gt_lrelu(float z) { return z > 0.f ? z : GT_SLOPE * z; }

// Stage graph nb/R: x, edges, lists (by-source too for the backward), parameters; then per-layer c and the loop values.
// Returns the edge count, or -1 for a refused graph (graph_lds_load: nothing of LDS touched; status bit 1 set).
// EW: also keep 1 / cnt of every target (the share of the virtual loop's gradient each kept edge takes).
template <bool BWD, bool EW = false>
__device__ int gt_stage(float* lds, const GtLayout& o, int R, int Emax, int H0, int F, int L, int64_t nb,
                        const float* __restrict__ x_in, const float* __restrict__ ew_in,
                        const int32_t* __restrict__ src32, const int32_t* __restrict__ dst32,
                        const int32_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt_perm,
                        const int32_t* __restrict__ src_ptr, const int32_t* __restrict__ src_perm,
                        const GtParams& prm, int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  int32_t eb;
  const int ne = graph_lds_load<BWD>(lds, o.t, R, Emax, H0, nb, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, src_ptr,
                                     src_perm, status, eb, GT_T);
  if (ne < 0) return -1;
  const int32_t* src = lds_i32(lds, o.t.src);
  const int32_t* tptr = lds_i32(lds, o.t.tptr);
  const int32_t* tperm = lds_i32(lds, o.t.tperm);
  const int fin_max = F > H0 ? F : H0;
  const int P = gt_param_offset(L, H0, F);
  for (int j = tid; j < P; j += GT_T) {
    int l = 0;
    while (l + 1 < L && j >= gt_param_offset(l + 1, H0, F)) ++l;
    const int fin = l == 0 ? H0 : F, r = j - gt_param_offset(l, H0, F), nw = F * fin;
    float v;
    if (r < nw) {
      v = prm.p[6 * l][r];
      lds[o.wt + l * F * fin_max + (r % fin) * F + r / fin] = v;
    } else {
      const int part = (r - nw) / F, f = (r - nw) - part * F;
      v = prm.p[6 * l + 1 + part][f];
    }
    lds[o.prm + j] = v;
  }
  __syncthreads();
  for (int l = tid; l < L; l += GT_T) {               // c_l = lin_edge[:, 0] . att_edge
    const float* b = lds + o.prm + gt_param_offset(l, H0, F) + F * (l == 0 ? H0 : F);
    float c = 0.f;
    for (int f = 0; f < F; ++f) c += b[3 * F + f] * b[4 * F + f];
    lds[o.ce + l] = c;
  }
  for (int i = tid; i < R; i += GT_T) {              // add_self_loops(fill_value='mean') over the kept edges of target i
    float s = 0.f;
    int cnt = 0;
    for (int p = tptr[i]; p < tptr[i + 1]; ++p) {
      const int k = tperm[p];
      if (src[k] != i) {
        s += lds[o.t.ew + k];
        ++cnt;
      }
    }
    lds[o.lea + i] = cnt ? s / (float)cnt : 0.f;
    if (EW) lds[o.icnt + i] = cnt ? 1.f / (float)cnt : 0.f;
  }
  __syncthreads();
  return ne;
}

// One forward layer out of LDS into LDS: H = Xin W^T, the node logits, the edge softmax per target (alpha stored per
// stored edge and per virtual loop), Y[:, l F:(l+1) F] = relu(sum alpha h[src] + bias).
template <int F>
__device__ void gt_layer_fwd(float* lds, const GtLayout& o, int R, int Emax, int H0, int L, int l, float* lgs,
                             float* lgd, float* alpha) {
  const int tid = threadIdx.x;
  constexpr int FQ = F / 4;
  const int fin = l == 0 ? H0 : F, D = L * F;
  const float* xin = l == 0 ? lds + o.t.x : lds + o.y + (l - 1) * F;
  const int ldx = l == 0 ? H0 : D;
  const int fin_max = F > H0 ? F : H0;
  const float* wt = lds + o.wt + l * F * fin_max;
  const float* pb = lds + o.prm + gt_param_offset(l, H0, F) + F * fin;      // b | att_src | att_dst | le | ae
  float* H = lds + o.h;
  const int32_t* src = lds_i32(lds, o.t.src);
  const int32_t* tptr = lds_i32(lds, o.t.tptr);
  const int32_t* tperm = lds_i32(lds, o.t.tperm);
  for (int e = tid; e < R * FQ; e += GT_T) {
    const int i = e / FQ, q = e - i * FQ;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int fi = 0; fi < fin; ++fi) {
      const float xv = xin[i * ldx + fi];
      const float4 w4 = *reinterpret_cast<const float4*>(wt + fi * F + q * 4);
      acc.x += xv * w4.x; acc.y += xv * w4.y; acc.z += xv * w4.z; acc.w += xv * w4.w;
    }
    *reinterpret_cast<float4*>(H + i * F + q * 4) = acc;
  }
  __syncthreads();
  for (int i = tid; i < R; i += GT_T) {
    float s = 0.f, d = 0.f;
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const float hv = H[i * F + f];
      s += hv * pb[F + f];
      d += hv * pb[2 * F + f];
    }
    lgs[i] = s;
    lgd[i] = d;
  }
  __syncthreads();
  const float c = lds[o.ce + l];
  for (int i = tid; i < R; i += GT_T) {
    const float zd = lgd[i];
    const float zl = gt_lrelu(lgs[i] + zd + lds[o.lea + i] * c);
    float m = zl;
    const int p0 = tptr[i], p1 = tptr[i + 1];
    for (int p = p0; p < p1; ++p) {
      const int k = tperm[p], s = src[k];
      if (s != i) m = fmaxf(m, gt_lrelu(lgs[s] + zd + lds[o.t.ew + k] * c));
    }
    float sum = 0.f;
    for (int p = p0; p < p1; ++p) {                   // list order, the virtual loop last (PyG appends the loops)
      const int k = tperm[p], s = src[k];
      float ev = 0.f;
      if (s != i) {
        ev = __expf(gt_lrelu(lgs[s] + zd + lds[o.t.ew + k] * c) - m);
        sum += ev;
      }
      alpha[k] = ev;
    }
    const float el = __expf(zl - m);
    sum += el;
    const float den = sum + 1e-16f;
    for (int p = p0; p < p1; ++p) {
      const int k = tperm[p];
      alpha[k] = alpha[k] / den;
    }
    alpha[Emax + i] = el / den;
  }
  __syncthreads();
  float* Y = lds + o.y + l * F;
  for (int e = tid; e < R * FQ; e += GT_T) {
    const int i = e / FQ, q = e - i * FQ;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = tptr[i]; p < tptr[i + 1]; ++p) {
      const int k = tperm[p], s = src[k];
      if (s == i) continue;
      const float a = alpha[k];
      const float4 h4 = *reinterpret_cast<const float4*>(H + s * F + q * 4);
      acc.x += a * h4.x; acc.y += a * h4.y; acc.z += a * h4.z; acc.w += a * h4.w;
    }
    const float al = alpha[Emax + i];
    const float4 h4 = *reinterpret_cast<const float4*>(H + i * F + q * 4);
    const float4 b4 = *reinterpret_cast<const float4*>(pb + q * 4);
    acc.x = fmaxf(acc.x + al * h4.x + b4.x, 0.f);
    acc.y = fmaxf(acc.y + al * h4.y + b4.y, 0.f);
    acc.z = fmaxf(acc.z + al * h4.z + b4.z, 0.f);
    acc.w = fmaxf(acc.w + al * h4.w + b4.w, 0.f);
    *reinterpret_cast<float4*>(Y + i * D + q * 4) = acc;
  }
  __syncthreads();
}

template <int F>
__global__ void __launch_bounds__(GT_T)
k_gat_stack_fwd(int R, int Emax, int H0, int L, const float* __restrict__ x_in, const float* __restrict__ ew_in,
                const int32_t* __restrict__ src32, const int32_t* __restrict__ dst32,
                const int32_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt_perm, GtParams prm,
                float* __restrict__ xcat, int32_t* __restrict__ status) {
  extern __shared__ float gt_lds[];
  const GtLayout o = gt_layout(R, Emax, H0, F, L, 0);
  const int64_t nb = (int64_t)blockIdx.x * R;
  const int D = L * F;
  if (gt_stage<false>(gt_lds, o, R, Emax, H0, F, L, nb, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, nullptr,
                      nullptr, prm, status) < 0) {
    for (int e = threadIdx.x; e < R * D; e += GT_T) xcat[nb * D + e] = 0.f;    // refused graph: defined output
    return;
  }
  for (int l = 0; l < L; ++l) gt_layer_fwd<F>(gt_lds, o, R, Emax, H0, L, l, gt_lds + o.lgs, gt_lds + o.lgd,
                                              gt_lds + o.alpha);
  // the rows are laid out [R][L F] already: one coalesced 16-byte pass
  for (int e = threadIdx.x; e < R * D / 4; e += GT_T)
    reinterpret_cast<float4*>(xcat + nb * D)[e] = reinterpret_cast<const float4*>(gt_lds + o.y)[e];
}

// The attention coefficients of every layer as dense maps, G [graph][l][source row][target column] (igcn_gat_stack_alpha):
// the forward above — gt_stage and gt_layer_fwd on the forward's own LDS layout, so alpha is what the forward used — and,
// after each layer and before the next one overwrites alpha, the layer's [R][R] block built in LDS one tile of TC
// target columns at a time (behind the layout: one [R][TC] block) and stored with consecutive lanes on consecutive
// columns.  Column c of a tile is walked by NP = 256 / TC threads, thread (c, part) owning the source rows s with
// s % NP == part: one writer per element, the stored copies of an edge added in list order, the diagonal set to the
// added loop's alpha by its owner (stored self-loops are skipped: PyG removes them), zeros stored like everything else.
static int gt_alpha_tile(int R, int Emax, int H0, int F, int L) {
  const size_t base = (size_t)gt_layout(R, Emax, H0, F, L, 0).total * 4;
  for (int tc = 64; tc >= 1; tc >>= 1)
    if (base + (size_t)R * tc * 4 <= IGCN_LDS_BUDGET_BYTES) return tc;
  return 0;
}

template <int F>
__global__ void __launch_bounds__(GT_T)
k_gat_stack_alpha(int R, int Emax, int H0, int L, int TC, const float* __restrict__ x_in,
                  const float* __restrict__ ew_in, const int32_t* __restrict__ src32,
                  const int32_t* __restrict__ dst32, const int32_t* __restrict__ tgt_ptr,
                  const int32_t* __restrict__ tgt_perm, GtParams prm, float* __restrict__ G,
                  int32_t* __restrict__ status) {
  extern __shared__ float gt_lds[];
  const GtLayout o = gt_layout(R, Emax, H0, F, L, 0);
  const int tid = threadIdx.x;
  const int64_t nb = (int64_t)blockIdx.x * R;
  float* Gb = G + (int64_t)blockIdx.x * L * R * R;
  if (gt_stage<false>(gt_lds, o, R, Emax, H0, F, L, nb, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, nullptr,
                      nullptr, prm, status) < 0) {
    for (int64_t e = tid; e < (int64_t)L * R * R; e += GT_T) Gb[e] = 0.f;      // refused graph: defined output
    return;
  }
  const int32_t* src = lds_i32(gt_lds, o.t.src);
  const int32_t* tptr = lds_i32(gt_lds, o.t.tptr);
  const int32_t* tperm = lds_i32(gt_lds, o.t.tperm);
  const float* alpha = gt_lds + o.alpha;
  float* tile = gt_lds + o.total;                                               // [R][TC]
  const int NP = GT_T / TC;
  const int c = tid / NP, part = tid - c * NP;
  bool bad = false;
  for (int l = 0; l < L; ++l) {
    gt_layer_fwd<F>(gt_lds, o, R, Emax, H0, L, l, gt_lds + o.lgs, gt_lds + o.lgd, gt_lds + o.alpha);
    float* Gl = Gb + (int64_t)l * R * R;
    for (int j0 = 0; j0 < R; j0 += TC) {
      const int w = min(TC, R - j0);
      for (int e = tid; e < R * TC; e += GT_T) tile[e] = 0.f;
      __syncthreads();
      if (c < w) {
        const int j = j0 + c;
        for (int p = tptr[j]; p < tptr[j + 1]; ++p) {
          const int k = tperm[p], s = src[k];
          if (s == j) continue;
          if (s < 0 || s >= R) {                                                // the edge leaves its graph
            bad = true;
            continue;
          }
          if (s % NP == part) tile[s * TC + c] += alpha[k];
        }
        if (j % NP == part) tile[j * TC + c] = alpha[Emax + j];
      }
      __syncthreads();
      for (int e = tid; e < R * w; e += GT_T) {
        const int i = e / w, cc = e - i * w;
        Gl[(int64_t)i * R + j0 + cc] = tile[i * TC + cc];
      }
      __syncthreads();                                                          // (the next tile zeroes it again)
    }
  }
  if (bad && status) atomicOr(status, 1);
}

template <int F, bool EW>
__global__ void __launch_bounds__(GT_T)
k_gat_stack_bwd(int R, int Emax, int H0, int L, const float* __restrict__ x_in, const float* __restrict__ ew_in,
                const int32_t* __restrict__ src32, const int32_t* __restrict__ dst32,
                const int32_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt_perm,
                const int32_t* __restrict__ src_ptr, const int32_t* __restrict__ src_perm, GtParams prm,
                const float* __restrict__ dxcat, float* __restrict__ dx_in /*or NULL*/,
                float* __restrict__ dpar_partial, int P, int32_t* __restrict__ status,
                float* __restrict__ dew /*[sum E], EW only*/) {
  extern __shared__ float gt_lds[];
  const GtLayout o = gt_layout(R, Emax, H0, F, L, EW ? 2 : 1);
  const int tid = threadIdx.x;
  const int64_t nb = (int64_t)blockIdx.x * R;
  const int D = L * F, EA = Emax + R;
  const int fin_max = F > H0 ? F : H0;
  if (gt_stage<true, EW>(gt_lds, o, R, Emax, H0, F, L, nb, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, src_ptr,
                         src_perm, prm, status) < 0) {
    if (dx_in)
      for (int e = tid; e < R * H0; e += GT_T) dx_in[nb * H0 + e] = 0.f;
    if (EW) {                                         // refused graph: its edges get a defined (zero) gradient too
      const int32_t eb = tgt_ptr[nb], ne = tgt_ptr[nb + R] - eb;
      for (int k = tid; k < ne; k += GT_T) dew[eb + k] = 0.f;
    }
    for (int e = tid; e < P; e += GT_T) dpar_partial[(int64_t)blockIdx.x * P + e] = 0.f;
    return;
  }
  for (int l = 0; l < L; ++l)
    gt_layer_fwd<F>(gt_lds, o, R, Emax, H0, L, l, gt_lds + o.lgs + l * R, gt_lds + o.lgd + l * R,
                    gt_lds + o.alpha + l * EA);
  const int32_t* src = lds_i32(gt_lds, o.t.src);
  const int32_t* dst = lds_i32(gt_lds, o.t.dst);
  const int32_t* tptr = lds_i32(gt_lds, o.t.tptr);
  const int32_t* tperm = lds_i32(gt_lds, o.t.tperm);
  const int32_t* sptr = lds_i32(gt_lds, o.t.sptr);
  const int32_t* sperm = lds_i32(gt_lds, o.t.sperm);
  float* H = gt_lds + o.h;
  float* dcur = gt_lds + o.dcur;
  float* dH = gt_lds + o.dh;
  float* dpre = gt_lds + o.dpre;
  float* das = gt_lds + o.das;
  float* dad = gt_lds + o.dad;
  float* prow = gt_lds + o.prow;
  constexpr int FQ = F / 4;
  for (int l = L - 1; l >= 0; --l) {
    const int fin = l == 0 ? H0 : F;
    const float* xin = l == 0 ? gt_lds + o.t.x : gt_lds + o.y + (l - 1) * F;
    const int ldx = l == 0 ? H0 : D;
    const float* wt = gt_lds + o.wt + l * F * fin_max;
    const float* W = gt_lds + o.prm + gt_param_offset(l, H0, F);             // [F][fin] as stored
    const float* pb = W + F * fin;                                           // b | att_src | att_dst | le | ae
    float* gW = prow + gt_param_offset(l, H0, F);
    float* gb = gW + F * fin;
    const float* lgs = gt_lds + o.lgs + l * R;
    const float* lgd = gt_lds + o.lgd + l * R;
    const float* alpha = gt_lds + o.alpha + l * EA;
    const float c = gt_lds[o.ce + l];
    const float* Y = gt_lds + o.y + l * F;
    // (a) h of this layer again (the forward kept the last layer's only); d(output) through the ReLU, into dcur —
    //     which holds d(input) of the layer above (none for the top layer)
    for (int e = tid; e < R * FQ; e += GT_T) {
      const int i = e / FQ, q = e - i * FQ;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int fi = 0; fi < fin; ++fi) {
        const float xv = xin[i * ldx + fi];
        const float4 w4 = *reinterpret_cast<const float4*>(wt + fi * F + q * 4);
        acc.x += xv * w4.x; acc.y += xv * w4.y; acc.z += xv * w4.z; acc.w += xv * w4.w;
      }
      *reinterpret_cast<float4*>(H + i * F + q * 4) = acc;
      float4 g = reinterpret_cast<const float4*>(dxcat + (nb + i) * D + l * F)[q];
      if (l < L - 1) {
        const float4 u = *reinterpret_cast<const float4*>(dcur + i * F + q * 4);
        g.x += u.x; g.y += u.y; g.z += u.z; g.w += u.w;
      }
      const float4 y4 = *reinterpret_cast<const float4*>(Y + i * D + q * 4);
      g.x = y4.x > 0.f ? g.x : 0.f;
      g.y = y4.y > 0.f ? g.y : 0.f;
      g.z = y4.z > 0.f ? g.z : 0.f;
      g.w = y4.w > 0.f ? g.w : 0.f;
      *reinterpret_cast<float4*>(dcur + i * F + q * 4) = g;
    }
    __syncthreads();
    // (b) per target: dalpha_e = dy_i . h[src_e]; softmax backward; leaky-ReLU slope -> dpre; d a_d[i]
    for (int i = tid; i < R; i += GT_T) {
      const int p0 = tptr[i], p1 = tptr[i + 1];
      const float* dy = dcur + i * F;
      float sa = 0.f;
      for (int p = p0; p < p1; ++p) {
        const int k = tperm[p], s = src[k];
        float da = 0.f;
        if (s != i) {
#pragma unroll
          for (int f = 0; f < F; ++f) da += dy[f] * H[s * F + f];
          sa += alpha[k] * da;
        }
        dpre[k] = da;                                 // dalpha for now
      }
      float dal = 0.f;
#pragma unroll
      for (int f = 0; f < F; ++f) dal += dy[f] * H[i * F + f];
      const float al = alpha[Emax + i];
      sa += al * dal;
      const float zd = lgd[i];
      float sd = 0.f;
      for (int p = p0; p < p1; ++p) {
        const int k = tperm[p], s = src[k];
        float g = 0.f;
        if (s != i) {
          const float dz = alpha[k] * (dpre[k] - sa);
          g = lgs[s] + zd + gt_lds[o.t.ew + k] * c > 0.f ? dz : GT_SLOPE * dz;
          sd += g;
        }
        dpre[k] = g;
      }
      const float dzl = al * (dal - sa);
      const float gl = lgs[i] + zd + gt_lds[o.lea + i] * c > 0.f ? dzl : GT_SLOPE * dzl;
      dpre[Emax + i] = gl;
      dad[i] = sd + gl;
    }
    __syncthreads();
    // (c) d a_s by source; d bias; d c (one wave)
    for (int n = tid; n < R; n += GT_T) {
      float s = 0.f;
      for (int q = sptr[n]; q < sptr[n + 1]; ++q) s += dpre[sperm[q]];     // stored loops carry an exact 0
      das[n] = s + dpre[Emax + n];
    }
    for (int f = tid; f < F; f += GT_T) {
      float s = 0.f;
      for (int i = 0; i < R; ++i) s += dcur[i * F + f];
      gb[f] = s;
    }
    if (tid >= GT_T - IGCN_WAVE) {
      const int lane = tid - (GT_T - IGCN_WAVE);
      const int ne = tptr[R];
      float s = 0.f;
      for (int k = lane; k < ne; k += IGCN_WAVE) s += dpre[k] * gt_lds[o.t.ew + k];
      for (int i = lane; i < R; i += IGCN_WAVE) s += dpre[Emax + i] * gt_lds[o.lea + i];
      s = wave_sum(s);
      if (lane == 0) gt_lds[o.red] = s;
    }
    if (EW) {
      // d ea of this layer into the thread's own edges (the top layer writes, the others add: no atomics); the
      // dpre[Emax + dst] / icnt[dst] gathers are indexed LDS reads, same-address lanes broadcast
      float* dew_g = dew + tgt_ptr[nb];
      const int ne = tptr[R];
      for (int k = tid; k < ne; k += GT_T) {
        const int t = dst[k];
        const float g = src[k] != t ? c * (dpre[k] + dpre[Emax + t] * gt_lds[o.icnt + t]) : 0.f;
        dew_g[k] = l == L - 1 ? g : dew_g[k] + g;
      }
    }
    __syncthreads();
    // (d) dh = (aggregation, by source) + (logit terms); d att_src, d att_dst, d lin_edge, d att_edge
    for (int e = tid; e < R * F; e += GT_T) {
      const int n = e / F, f = e - n * F;
      float s = 0.f;
      for (int q = sptr[n]; q < sptr[n + 1]; ++q) {
        const int k = sperm[q], t = dst[k];
        if (t != n) s += alpha[k] * dcur[t * F + f];
      }
      s += alpha[Emax + n] * dcur[n * F + f];
      dH[e] = s + das[n] * pb[F + f] + dad[n] * pb[2 * F + f];
    }
    for (int j = tid; j < 2 * F; j += GT_T) {
      const int f = j % F;
      const float* dl = j < F ? das : dad;
      float s = 0.f;
      for (int n = 0; n < R; ++n) s += dl[n] * H[n * F + f];
      gb[F + j] = s;                                  // d att_src | d att_dst
    }
    for (int f = tid; f < F; f += GT_T) {
      const float dc = gt_lds[o.red];
      gb[3 * F + f] = dc * pb[4 * F + f];             // d lin_edge = dc * att_edge
      gb[4 * F + f] = dc * pb[3 * F + f];             // d att_edge = dc * lin_edge
    }
    __syncthreads();
    // (e) dW = dh^T Xin; d(input) = dh W (into dcur for the layer below, or dx_in for layer 0)
    for (int j = tid; j < F * fin; j += GT_T) {
      const int fo = j / fin, fi = j - fo * fin;
      float s = 0.f;
      for (int n = 0; n < R; ++n) s += dH[n * F + fo] * xin[n * ldx + fi];
      gW[j] = s;
    }
    if (l > 0 || dx_in) {
      for (int e = tid; e < R * fin; e += GT_T) {
        const int n = e / fin, fi = e - n * fin;
        float s = 0.f;
#pragma unroll
        for (int fo = 0; fo < F; ++fo) s += dH[n * F + fo] * W[fo * fin + fi];
        if (l > 0) dcur[e] = s;
        else dx_in[nb * H0 + e] = s;
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < P; e += GT_T) dpar_partial[(int64_t)blockIdx.x * P + e] = prow[e];
}

// The launch switches below instantiate F = 4, 8, 16 and 32 only (default: 32): igcn_stack_width_ok must admit no other
static_assert(IGCN_STACK_MIN_WIDTH == 4 && IGCN_STACK_MAX_WIDTH == 32,
              "a new layer width needs a kernel instance and a case in every launch switch of this file");
static int gt_check(const char* nm, int64_t n_graphs, int R, int max_edges, int H0, int F, int L, int backward) {
  IGCN_REQUIRE(n_graphs > 0 && R > 0 && max_edges >= 0, "%s: bad sizes", nm);
  if (!igcn_stack_width_ok(F) || H0 < 1 || H0 > IGCN_MAX_H0 || L < 1 || L > IGCN_STACK_MAX_LAYERS ||
      igcn_gat_stack_lds_bytes(R, max_edges, H0, F, L, backward) > IGCN_LDS_BUDGET_BYTES) {
    igcn_set_error("%s: needs F in {4, 8, 16, 32}, 1 <= H0 <= %d, 1 <= L <= %d and a graph that fits %d KB of LDS "
                   "(R=%d, E<=%d, H0=%d, F=%d, L=%d)", nm, IGCN_MAX_H0, IGCN_STACK_MAX_LAYERS, IGCN_LDS_BUDGET_BYTES / 1024,
                   R, max_edges, H0, F, L);
    return IGCN_ERR_UNSUPPORTED;
  }
  return IGCN_OK;
}

extern "C" int igcn_gat_stack_fwd(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                                  const float* ew_in, const int32_t* src32, const int32_t* dst32,
                                  const int32_t* tgt_ptr, const int32_t* tgt_perm, const float* const* params,
                                  float* xcat, int32_t* status, void* stream) {
  int rc = gt_check("gat_stack_fwd", n_graphs, R, max_edges, H0, F, L, 0);
  if (rc) return rc;
  IGCN_REQUIRE(x_in && ew_in && src32 && dst32 && tgt_ptr && tgt_perm && params && xcat,
               "gat_stack_fwd: null argument");
  IGCN_REQUIRE(((uintptr_t)xcat & 15) == 0, "gat_stack_fwd: xcat must be 16-byte aligned");
  GtParams prm = {};
  for (int j = 0; j < 6 * L; ++j) {
    IGCN_REQUIRE(params[j], "gat_stack_fwd: null parameter %d", j);
    prm.p[j] = params[j];
  }
  const size_t lds = igcn_gat_stack_lds_bytes(R, max_edges, H0, F, L, 0);
  hipStream_t st = (hipStream_t)stream;
#define GT_FWD(FV)                                                                                                \
  {                                                                                                               \
    if (lds > 64 * 1024) IGCN_ALLOW_BIG_LDS((k_gat_stack_fwd<FV>));                                               \
    hipLaunchKernelGGL((k_gat_stack_fwd<FV>), dim3((unsigned)n_graphs), dim3(GT_T), lds, st, R, max_edges, H0, L,  \
                       x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, prm, xcat, status);                          \
  }
  switch (F) {
    case 4: GT_FWD(4) break;
    case 8: GT_FWD(8) break;
    case 16: GT_FWD(16) break;
    default: GT_FWD(32) break;
  }
#undef GT_FWD
  IGCN_CHECK_LAUNCH("gat_stack_fwd");
  return IGCN_OK;
}

extern "C" int igcn_gat_stack_alpha_tile(int R, int max_edges, int H0, int F, int L) {
  if (R <= 0 || max_edges < 0 || !igcn_stack_width_ok(F) || H0 < 1 || H0 > IGCN_MAX_H0 || L < 1 ||
      L > IGCN_STACK_MAX_LAYERS)
    return 0;
  return gt_alpha_tile(R, max_edges, H0, F, L);
}

extern "C" int igcn_gat_stack_alpha(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                                    const float* ew_in, const int32_t* src32, const int32_t* dst32,
                                    const int32_t* tgt_ptr, const int32_t* tgt_perm, const float* const* params,
                                    float* G, int32_t* status, void* stream) {
  int rc = gt_check("gat_stack_alpha", n_graphs, R, max_edges, H0, F, L, 0);
  if (rc) return rc;
  const int tc = gt_alpha_tile(R, max_edges, H0, F, L);
  if (tc == 0) {
    igcn_set_error("gat_stack_alpha: no column of the [R, R] map fits beside the stack in %d KB of LDS (R=%d, E<=%d, "
                   "H0=%d, F=%d, L=%d)", IGCN_LDS_BUDGET_BYTES / 1024, R, max_edges, H0, F, L);
    return IGCN_ERR_UNSUPPORTED;
  }
  IGCN_REQUIRE(x_in && ew_in && src32 && dst32 && tgt_ptr && tgt_perm && params && G, "gat_stack_alpha: null argument");
  GtParams prm = {};
  for (int j = 0; j < 6 * L; ++j) {
    IGCN_REQUIRE(params[j], "gat_stack_alpha: null parameter %d", j);
    prm.p[j] = params[j];
  }
  const size_t lds = igcn_gat_stack_lds_bytes(R, max_edges, H0, F, L, 0) + (size_t)R * tc * 4;
  hipStream_t st = (hipStream_t)stream;
#define GT_ALPHA(FV)                                                                                               \
  {                                                                                                                \
    if (lds > 64 * 1024) IGCN_ALLOW_BIG_LDS((k_gat_stack_alpha<FV>));                                              \
    hipLaunchKernelGGL((k_gat_stack_alpha<FV>), dim3((unsigned)n_graphs), dim3(GT_T), lds, st, R, max_edges, H0, L, \
                       tc, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, prm, G, status);                          \
  }
  switch (F) {
    case 4: GT_ALPHA(4) break;
    case 8: GT_ALPHA(8) break;
    case 16: GT_ALPHA(16) break;
    default: GT_ALPHA(32) break;
  }
#undef GT_ALPHA
  IGCN_CHECK_LAUNCH("gat_stack_alpha");
  return IGCN_OK;
}

// Both backward entry points: EW selects the instantiation that also writes dew (and its LDS layout, code 2).
template <bool EW>
static int gt_bwd_launch(const char* nm, int64_t n_graphs, int R, int max_edges, int H0, int F, int L,
                         const float* x_in, const float* ew_in, const int32_t* src32, const int32_t* dst32,
                         const int32_t* tgt_ptr, const int32_t* tgt_perm, const int32_t* src_ptr,
                         const int32_t* src_perm, const float* const* params, const float* dxcat, float* dx_in,
                         float* dew, float* dparams, float* scratch, int32_t* status, void* stream) {
  int rc = gt_check(nm, n_graphs, R, max_edges, H0, F, L, EW ? 2 : 1);
  if (rc) return rc;
  IGCN_REQUIRE(x_in && ew_in && src32 && dst32 && tgt_ptr && tgt_perm && src_ptr && src_perm && params && dxcat &&
                   dparams && scratch && (dew || !EW),
               "%s: null argument", nm);
  IGCN_REQUIRE(((uintptr_t)dxcat & 15) == 0, "%s: dxcat must be 16-byte aligned", nm);
  GtParams prm = {};
  for (int j = 0; j < 6 * L; ++j) {
    IGCN_REQUIRE(params[j], "%s: null parameter %d", nm, j);
    prm.p[j] = params[j];
  }
  const size_t lds = igcn_gat_stack_lds_bytes(R, max_edges, H0, F, L, EW ? 2 : 1);
  const int P = igcn_gat_stack_param_floats(H0, F, L);
  hipStream_t st = (hipStream_t)stream;
#define GT_BWD(FV)                                                                                                \
  {                                                                                                               \
    if (lds > 64 * 1024) IGCN_ALLOW_BIG_LDS((k_gat_stack_bwd<FV, EW>));                                           \
    hipLaunchKernelGGL((k_gat_stack_bwd<FV, EW>), dim3((unsigned)n_graphs), dim3(GT_T), lds, st, R, max_edges,    \
                       H0, L, x_in, ew_in, src32, dst32, tgt_ptr, tgt_perm, src_ptr, src_perm, prm, dxcat, dx_in, \
                       scratch, P, status, dew);                                                                  \
  }
  switch (F) {
    case 4: GT_BWD(4) break;
    case 8: GT_BWD(8) break;
    case 16: GT_BWD(16) break;
    default: GT_BWD(32) break;
  }
#undef GT_BWD
  IGCN_CHECK_LAUNCH(nm);
  return igcn_launch_reduce_rows_final(scratch, n_graphs, P, P, dparams, st);
}

extern "C" int igcn_gat_stack_bwd(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                                  const float* ew_in, const int32_t* src32, const int32_t* dst32,
                                  const int32_t* tgt_ptr, const int32_t* tgt_perm, const int32_t* src_ptr,
                                  const int32_t* src_perm, const float* const* params, const float* dxcat,
                                  float* dx_in, float* dparams, float* scratch, int32_t* status, void* stream) {
  return gt_bwd_launch<false>("gat_stack_bwd", n_graphs, R, max_edges, H0, F, L, x_in, ew_in, src32, dst32, tgt_ptr,
                              tgt_perm, src_ptr, src_perm, params, dxcat, dx_in, nullptr, dparams, scratch, status,
                              stream);
}

// The same backward with d(loss)/d(ew_in) as one more output: dew [sum E], every element written (0 at stored loops).
extern "C" int igcn_gat_stack_bwd_ew(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                                     const float* ew_in, const int32_t* src32, const int32_t* dst32,
                                     const int32_t* tgt_ptr, const int32_t* tgt_perm, const int32_t* src_ptr,
                                     const int32_t* src_perm, const float* const* params, const float* dxcat,
                                     float* dx_in, float* dew, float* dparams, float* scratch, int32_t* status,
                                     void* stream) {
  return gt_bwd_launch<true>("gat_stack_bwd_ew", n_graphs, R, max_edges, H0, F, L, x_in, ew_in, src32, dst32, tgt_ptr,
                             tgt_perm, src_ptr, src_perm, params, dxcat, dx_in, dew, dparams, scratch, status, stream);
}
