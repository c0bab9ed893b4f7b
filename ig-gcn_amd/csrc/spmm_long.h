// The long-list walk of the SNP <-> GO map kernels (k_spmm_long_lds, csrc/go.hip) for every kernel that has a sample's
// operand vector in LDS: the list sums of the map and of a producer that stages the vector itself (csrc/readout.hip)
// are the same code, so they are the same numbers.
#pragma once
#include "common.h"

#ifndef SPMM_PROBE
#define SPMM_PROBE(i)
#endif
__device__ __forceinline__ float spmm_wave_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true));   // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, true));   // row_mirror
  const int ri = __float_as_int(v);
  return (__int_as_float(__builtin_amdgcn_readlane(ri, 0)) + __int_as_float(__builtin_amdgcn_readlane(ri, 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(ri, 32)) + __int_as_float(__builtin_amdgcn_readlane(ri, 48)));
}
#define SPMM_LT 512
#define SPMM_LU 3
#define SPMM_RM 7
// sum_c == 0: out[b, c, j] = sum_{q in list j} val[c, vk?] * vec[idx[q]]                        (vec [L] in LDS)
// sum_c == 1: out[b, j]    = sum_{q in list j} sum_c val[c, vk?] * vec[c, idx[q]]                (vec [C][L] in LDS)
// for the SPMM_LT threads of a workgroup, after the barrier behind the staging of vec.
__device__ __forceinline__ void
spmm_long_walk(const float* __restrict__ sp_lds, int b, int C, int L, int n_out, int64_t nnz, int sum_c,
               const int32_t* __restrict__ ptr_, const int32_t* __restrict__ idx, const int32_t* __restrict__ vk,
               const float* __restrict__ val, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nc_out = sum_c ? 1 : C, nc_in = sum_c ? C : 1;
  constexpr int NWV = SPMM_LT / 64;
  for (int jb = w; jb < n_out; jb += NWV * SPMM_RM) {
    // SPMM_RM lists per wave AT ONCE: their pointers, then the first SPMM_LU stride-64 entries of every list, then the
    // values, then the LDS gathers — the dependent round trips of a list overlap with those of its siblings
    int32_t q0[SPMM_RM], q1[SPMM_RM];
#pragma unroll
    for (int m = 0; m < SPMM_RM; ++m) {
      const int j = jb + m * NWV;
      q0[m] = j < n_out ? ptr_[j] : 0;
      q1[m] = j < n_out ? ptr_[j + 1] : 0;
    }
    for (int co = 0; co < nc_out; ++co) {
      float acc[SPMM_RM];
      int32_t r[SPMM_RM][SPMM_LU], k[SPMM_RM][SPMM_LU];
#pragma unroll
      for (int m = 0; m < SPMM_RM; ++m) {
        acc[m] = 0.f;
#pragma unroll
        for (int u = 0; u < SPMM_LU; ++u) {
          const int32_t qq = q0[m] + lane + 64 * u;
          const bool ok = qq < q1[m];
          r[m][u] = ok ? idx[qq] : -1;
          k[m][u] = ok ? (vk ? vk[qq] : qq) : 0;
        }
      }
#pragma unroll
      for (int m = 0; m < SPMM_RM; ++m) {
#pragma unroll
        for (int u = 0; u < SPMM_LU; ++u)
          for (int ci = 0; ci < nc_in; ++ci) {
            const float v = r[m][u] >= 0 ? val[(int64_t)(co + ci) * nnz + k[m][u]] : 0.f;
            acc[m] += v * sp_lds[ci * L + (r[m][u] >= 0 ? r[m][u] : 0)];
          }
        for (int32_t q = q0[m] + lane + 64 * SPMM_LU; q < q1[m]; q += 64)       // lists beyond 64 SPMM_LU entries
          for (int ci = 0; ci < nc_in; ++ci)
            acc[m] += val[(int64_t)(co + ci) * nnz + (vk ? vk[q] : q)] * sp_lds[ci * L + idx[q]];
      }
#pragma unroll
      for (int m = 0; m < SPMM_RM; ++m) {                // seven wave sums on the VALU (DPP rows + v_readlane), not as seven
        const int j = jb + m * NWV;                      // six-step chains of LDS-pipe permutes
        const float t = spmm_wave_sum(acc[m]);
        if (lane == 0 && j < n_out) out[((int64_t)b * nc_out + co) * n_out + j] = t;
      }
    }
    if (jb == w) SPMM_PROBE(2);
  }
}
