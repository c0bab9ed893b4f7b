// Connected components of P small graphs at once: the second half of the network-based statistic (include/igcn.h:
// igcn_nbs_components; the first half is igcn_perm_supra, csrc/perm_test.hip).  Row p of `bits` is the [R, R] entry set of
// relabelling p (bit e & 31 of word e >> 5, e = i R + j: source row i, target column j).  Nodes i != j are joined when
// bit (i, j) OR bit (j, i) is set; the extent of a component is the number of set bits whose source row lies in it.
//
// One wave per relabelling, two nodes a lane (R <= 128):
//   1. the row's <= 512 words are staged in LDS;
//   2. a lane cuts its nodes' R-bit adjacency rows out of them (the row starts at bit i R, not word-aligned) and counts
//      their set bits;
//   3. it ORs in the transpose, bit by bit from the staged words, and clears the diagonal: four words a node, in registers;
//   4. minimum-label propagation with one pointer jump a pass (label[i] <- min over the neighbours, then through that
//      node's own label), all reads before all writes, until a wave ballot says that no lane changed.  A label is always a
//      node of the same component with an index <= the node's own, so the fixed point is the component's smallest index,
//      whatever the graph.  The worst case is a path whose labels descend along it, where the smallest label moves
//      one node a pass without the jump.  The loop is bounded by R + 2 passes, which plain propagation cannot exceed;
//   5. the row counts are added to the root's extent by LDS integer atomics (integer addition: one result in any order).
// One writer per output element.
#include "common.h"

#define NB_MAX IGCN_NBS_MAX_ROIS
#define NB_WORDS (NB_MAX * NB_MAX / 32)

__global__ void __launch_bounds__(64)
k_nbs_components(int R, const unsigned* __restrict__ bits, int64_t ldw, int32_t* __restrict__ max_extent,
                 int32_t* __restrict__ label, int32_t* __restrict__ extent) {
  __shared__ unsigned wb[NB_WORDS + 2];                 // (a cut reads one word behind the last: zeros)
  __shared__ int lab[NB_MAX];
  __shared__ int ext[NB_MAX];
  const int p = blockIdx.x, lane = threadIdx.x;
  const unsigned* row = bits + (int64_t)p * ldw;
  const int nw = (R * R + 31) >> 5;
  for (int x = lane; x < NB_WORDS + 2; x += 64) wb[x] = x < nw ? row[x] : 0u;
  for (int i = lane; i < NB_MAX; i += 64) {
    lab[i] = i;
    ext[i] = 0;
  }
  __syncthreads();

  unsigned adj[2][4];
  int cnt[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    cnt[h] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      adj[h][k] = 0u;
      const int nb = R - 32 * k;                        // bits of the row that this word holds
      if (i < R && nb > 0) {
        const int o = i * R + 32 * k;
        const unsigned long long two = ((unsigned long long)wb[(o >> 5) + 1] << 32) | wb[o >> 5];
        unsigned v = (unsigned)(two >> (o & 31));
        if (nb < 32) v &= (1u << nb) - 1u;
        cnt[h] += __popc(v);
        for (int jj = 0; jj < 32 && jj < nb; ++jj) {    // the transpose: bit (j, i), j = 32 k + jj
          const int pos = (32 * k + jj) * R + i;
          v |= ((wb[pos >> 5] >> (pos & 31)) & 1u) << jj;
        }
        if (k == (i >> 5)) v &= ~(1u << (i & 31));      // a diagonal bit joins nothing
        adj[h][k] = v;
      }
    }
  }

  for (int pass = 0; pass < R + 2; ++pass) {
    int next[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      int best = lab[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned m = adj[h][k];
        while (m) {
          const int j = 32 * k + __ffs(m) - 1;
          m &= m - 1u;
          best = min(best, lab[j]);
        }
      }
      next[h] = min(best, lab[best]);                   // the pointer jump
    }
    __syncthreads();                                    // all reads before all writes
    bool changed = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (next[h] < lab[i]) {
        lab[i] = next[h];
        changed = true;
      }
    }
    __syncthreads();
    if (__ballot(changed) == 0ull) break;
  }

#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    if (i < R && cnt[h] > 0) atomicAdd(&ext[lab[i]], cnt[h]);
  }
  __syncthreads();
  int mx = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    if (i < R) {
      const int l = lab[i], x = ext[l];
      mx = max(mx, x);
      if (label) label[(int64_t)p * R + i] = l;
      if (extent) extent[(int64_t)p * R + i] = x;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) max_extent[p] = mx;
}

extern "C" int igcn_nbs_components(int P, int R, const void* bits, int64_t ldw, int32_t* max_extent, int32_t* label,
                                   int32_t* extent, void* stream) {
  const char* who = "nbs_components";
  IGCN_REQUIRE(R >= 2 && R <= IGCN_NBS_MAX_ROIS, "%s: R=%d regions outside [2,%d]", who, R, IGCN_NBS_MAX_ROIS);
  IGCN_REQUIRE(P >= 1 && P <= IGCN_PERM_MAX_P, "%s: P=%d relabellings in one launch outside [1,%d]", who, P,
               IGCN_PERM_MAX_P);
  IGCN_REQUIRE(bits && max_extent, "%s: a null buffer", who);
  IGCN_REQUIRE(((uintptr_t)bits & 3) == 0, "%s: the bits must be 4-byte aligned", who);
  const int nw = (R * R + 31) / 32;
  IGCN_REQUIRE(ldw >= nw, "%s: bits row stride %lld words below %d (R=%d: %d entries, 32 a word)", who, (long long)ldw, nw,
               R, R * R);
  hipLaunchKernelGGL(k_nbs_components, dim3(P), dim3(64), 0, (hipStream_t)stream, R, (const unsigned*)bits, ldw,
                     max_extent, label, extent);
  IGCN_CHECK_LAUNCH(who);
  return IGCN_OK;
}
