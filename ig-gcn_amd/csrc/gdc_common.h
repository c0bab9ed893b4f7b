// What the two routes of the graph-diffusion pre-transform share (csrc/gdc.hip: a graph's system in one workgroup's LDS;
// csrc/gdc_tiled.hip: in a global-memory workspace), and the contract of selection and emission both keep.
// The diffusion matrix of graph g is S = scale * M (scale = alpha or e^-t, applied where M is read); a column owns `cap`
// slots, cap = k (top-k) or R (threshold).
//   * top-k (util_gdc.py:25-31): the first k entries of the column in the order of preference "larger value, then LARGER
//     row" (a stable ascending argsort keeps the later of two equals); threshold (util_gdc.py:33-38): the entries >= eps;
//   * the column is divided by the sum of what it kept (top-k: summed in the order of preference; threshold: rows
//     ascending); a column whose sum is <= 0 is left unscaled;
//   * a kept entry that is exactly 0 is not an edge (scipy's coo_matrix drops it);
//   * graph g owns the slots [g*R*cap, (g+1)*R*cap): its edges in (row, col) order with g*R added to both indices, then
//     (-1, -1, 0) padding; counts[g] = #edges.  A graph that is not read (GDC_NOT_READ) is all padding, count 0;
//   * every slot has exactly one writer: no atomics on the outputs, the result is bit-reproducible.
// How a route finds the kept set is its own (gdc.hip: row bit sets in LDS; gdc_tiled.hip: a threshold pair per column).
#pragma once
#include "common.h"

#define GDC_HEAT_DEGREE 14                              // Taylor degree; the remainder bound stands at k_gdc_heat (gdc.hip)

// How S is sparsified (igcn.h IGCN_GDC_TOPK / IGCN_GDC_THRESHOLD) and how many slots a column owns
struct GdcSparsify {
  int mode, k, cap;
  double eps;
};

static inline GdcSparsify gdc_sparsify(int sparsify, int k, double eps, int R) {
  const int cap = sparsify == IGCN_GDC_TOPK ? k : R;
  return GdcSparsify{sparsify, cap, cap, eps};
}

// The argument check of both entry points; `who` names the entry point in the messages.  alpha_min: the route's lower
// bound on alpha — 0 for the open interval (0,1], else [alpha_min,1] with the ppr_terms doubling terms that bound buys.
#define GDC_BAD_SIZES "%s: bad sizes B=%d R=%d"
static inline int gdc_check_args(const char* who, int B, int R, int kernel, double param, int sparsify, int k, double eps,
                                 double alpha_min, int ppr_terms, int max_R) {
  IGCN_REQUIRE(kernel == IGCN_GDC_PPR || kernel == IGCN_GDC_HEAT, "%s: unknown kernel %d", who, kernel);
  IGCN_REQUIRE(sparsify == IGCN_GDC_TOPK || sparsify == IGCN_GDC_THRESHOLD, "%s: unknown sparsifier %d", who, sparsify);
  if (sparsify == IGCN_GDC_TOPK) {
    IGCN_REQUIRE(B >= 0 && R > 0 && k > 0 && k <= R, GDC_BAD_SIZES " k=%d", who, B, R, k);
  } else {
    IGCN_REQUIRE(B >= 0 && R > 0, GDC_BAD_SIZES, who, B, R);
    IGCN_REQUIRE(eps == eps, "%s: eps is not a number", who);
  }
  if (kernel == IGCN_GDC_HEAT)
    IGCN_REQUIRE(param > 0.0 && param <= 64.0, "%s: t=%g outside (0,64]", who, param);
  else if (alpha_min > 0.0)
    IGCN_REQUIRE(param >= alpha_min && param <= 1.0, "%s: alpha=%g outside [%g,1] (at most %d doubling terms)", who,
                 param, alpha_min, ppr_terms);
  else
    IGCN_REQUIRE(param > 0.0 && param <= 1.0, "%s: alpha=%g outside (0,1]", who, param);
  if (R > max_R) {
    igcn_set_error("%s: R=%d exceeds the kernel's limit (max R = %d)", who, R, max_R);
    return IGCN_ERR_UNSUPPORTED;
  }
  return IGCN_OK;
}

// Which matrix graph g of the batch is — subject[g] of the dataset, g itself without a subject list — and whether it is
// read at all: an index outside the dataset is never turned into an address, the graph is handed over EMPTY, which the
// consumer's plan build reports in its status word.  (Macros, so that both stand in the kernel's own expression: as
// inline functions they compile to other scalar code in front of the same kernel body.)
#define GDC_SUBJECT_OF(subject, g) ((subject) ? (subject)[g] : (int64_t)(g))
#define GDC_NOT_READ(subject, sj, n_subjects) ((subject) && ((sj) < 0 || (sj) >= (n_subjects)))

// The heat kernel's scaling exponent: the smallest s <= cap with nrm / 2^s <= 1/2 (the cap: an input outside the
// contract must not spin here, and the tiled route's host launches no more squarings than that)
__device__ __forceinline__ int gdc_scaling_exponent(double nrm, int cap) {
  int s = 0;
  while (nrm > 0.5 && s < cap) {
    nrm *= 0.5;
    ++s;
  }
  return s;
}
