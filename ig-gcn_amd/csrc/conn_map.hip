// Per-edge values -> dense region x region maps (the learned connective-importance mask of cal_probability,
// kernel/sgcn_img_snp.py:133-151, laid out like the reference's data.A: source row, target column).
//
// A workgroup owns (graph b, tile of TC consecutive target columns [j0, j0 + TC)) and builds the tile for ALL R source
// rows in LDS, [R][TC] floats (two of them when the copy counts are wanted): zero it, walk the by-target lists of its
// columns — positions [tgt_ptr[bR + j0], tgt_ptr[bR + j0 + TC)) of the plan, one contiguous range — and store the tile
// with consecutive lanes on consecutive columns.  Every element of map / cnt is stored exactly once by the launch, zeros
// included: no fill in front, nothing overwritten in global memory.
// One writer per element, no atomics: column c is walked by NP = 256 / TC threads, thread (c, part) applying only the
// entries whose source row s has s % NP == part — each element (s, c) has one owner, which meets the stored copies of
// its edge in list order (the stable order of the target-grouped plan = stored order), so duplicates are added in
// stored order and the result is bit-identical from run to run.  The NP threads of a column read the same list words
// (one broadcast per wave); a complete 512-node graph walks 512-entry lists with 16 threads each instead of one.
// An entry whose edge id, target or source does not belong to the column's graph is not written and sets status bit 0.
// LDS: TC = the largest power of two <= 64 with R * TC * 4 * (1 or 2) bytes <= 64 KB — no raised LDS limit, two
// workgroups per CU beside each other: 64 columns at R = 90 (45 KB with counts), 16 at R = 270 and R = 512, 1 up to
// R = 8192 (16 384 without counts); beyond that the launch is refused on the host.
#include "common.h"

#define CM_T 256
#define CM_LDS (64 * 1024)

static int cm_tile(int R, int want_count) {
  if (R <= 0) return 0;
  for (int tc = 64; tc >= 1; tc >>= 1)
    if ((size_t)R * tc * sizeof(float) * (want_count ? 2 : 1) <= CM_LDS) return tc;
  return 0;
}

extern "C" int igcn_edge_dense_map_supported(int R, int want_count) { return cm_tile(R, want_count); }

template <bool CNT>
__global__ void __launch_bounds__(CM_T)
k_edge_dense_map(int R, int TC, int tiles, int64_t n_edges, const float* __restrict__ values,
                 const int32_t* __restrict__ src32, const int32_t* __restrict__ dst32,
                 const int32_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt_perm, float* __restrict__ map,
                 float* __restrict__ cnt, int32_t* __restrict__ status) {
  extern __shared__ float cm_lds[];                          // map tile [R][TC] (| count tile [R][TC])
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / tiles;
  const int j0 = (int)(blockIdx.x % tiles) * TC;
  const int w = min(TC, R - j0);                             // columns of this tile
  const int64_t nb = b * R;
  float* tm = cm_lds;
  float* tc = cm_lds + R * TC;
  for (int e = tid; e < R * TC * (CNT ? 2 : 1); e += CM_T) cm_lds[e] = 0.f;
  __syncthreads();
  const int NP = CM_T / TC;
  const int c = tid / NP, part = tid - c * NP;               // (TC * NP == CM_T: every thread has a column)
  bool bad = false;
  if (c < w) {
    const int64_t t = nb + j0 + c;                           // the target node
    int64_t p0 = tgt_ptr[t], p1 = tgt_ptr[t + 1];
    if (p0 < 0 || p1 > n_edges || p0 > p1) {                 // a plan whose pointers run backwards or past the end
      bad = true;
      p1 = p0 = 0;
    }
    for (int64_t p = p0; p < p1; ++p) {
      const int64_t k = tgt_perm[p];
      if (k < 0 || k >= n_edges) {
        bad = true;
        continue;
      }
      const int64_t s = (int64_t)src32[k] - nb;
      if (dst32[k] != t || s < 0 || s >= R) {                // the edge leaves its graph: flagged, not written
        bad = true;
        continue;
      }
      if ((int)(s % NP) == part) {
        tm[s * TC + c] += values[k];
        if (CNT) tc[s * TC + c] += 1.f;
      }
    }
  }
  if (bad && status) atomicOr(status, 1);
  __syncthreads();
  float* om = map + nb * R + j0;
  for (int e = tid; e < R * w; e += CM_T) {
    const int i = e / w, cc = e - i * w;
    om[(int64_t)i * R + cc] = tm[i * TC + cc];
  }
  if (CNT) {
    float* oc = cnt + nb * R + j0;
    for (int e = tid; e < R * w; e += CM_T) {
      const int i = e / w, cc = e - i * w;
      oc[(int64_t)i * R + cc] = tc[i * TC + cc];
    }
  }
}

extern "C" int igcn_edge_dense_map(int64_t n_graphs, int R, int64_t n_edges, const float* values, const int32_t* src32,
                                   const int32_t* dst32, const int32_t* tgt_ptr, const int32_t* tgt_perm, float* map,
                                   float* cnt, int32_t* status, void* stream) {
  IGCN_REQUIRE(n_graphs > 0 && R > 0 && n_edges >= 0 && n_edges < ((int64_t)1 << 31) &&
                   n_graphs * R < ((int64_t)1 << 31),
               "edge_dense_map: bad sizes");
  const int tc = cm_tile(R, cnt != nullptr);
  if (tc == 0) {
    igcn_set_error("edge_dense_map: R=%d: one target column of the map%s exceeds the %d KB of LDS a workgroup takes", R,
                   cnt ? " and of the counts" : "", CM_LDS / 1024);
    return IGCN_ERR_UNSUPPORTED;
  }
  IGCN_REQUIRE((values || n_edges == 0) && src32 && dst32 && tgt_ptr && tgt_perm && map,
               "edge_dense_map: null argument");
  const int64_t tiles = igcn_cdiv(R, tc);
  IGCN_REQUIRE(n_graphs * tiles < ((int64_t)1 << 31), "edge_dense_map: too many tiles for one grid");
  const size_t lds = (size_t)R * tc * sizeof(float) * (cnt ? 2 : 1);
  hipStream_t st = (hipStream_t)stream;
  if (cnt)
    hipLaunchKernelGGL((k_edge_dense_map<true>), dim3((unsigned)(n_graphs * tiles)), dim3(CM_T), lds, st, R, tc,
                       (int)tiles, n_edges, values, src32, dst32, tgt_ptr, tgt_perm, map, cnt, status);
  else
    hipLaunchKernelGGL((k_edge_dense_map<false>), dim3((unsigned)(n_graphs * tiles)), dim3(CM_T), lds, st, R, tc,
                       (int)tiles, n_edges, values, src32, dst32, tgt_ptr, tgt_perm, map, cnt, status);
  IGCN_CHECK_LAUNCH("edge_dense_map");
  return IGCN_OK;
}
