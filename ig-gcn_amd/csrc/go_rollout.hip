// Attention roll-out through the GO encoder (go_model.py:219-251; Abnar & Zuidema's roll-out restricted to the pooled
// hierarchy): one mixing step per encoder layer on the coefficients igcn_go_attn_coeffs (go.hip) hands out.
#include "common.h"

// Relevance is channel-major [B, S, N] like the layer activations: lanes run over nodes, a sample's S rows are
// contiguous.  A workgroup owns (sample, chunk of CH relevance columns): it copies the chunk [CH, N] into LDS once, then
// every thread takes kept rows r = pool + tid, pool + tid + T, ... and walks the row's list, gathering the CH values
// of each neighbour from LDS (the gathers never leave the CU; alpha, col and beta are read once per chunk):
//   out[c, r - pool] = (sum_e alpha_e R[c, col_e] + beta_r R[c, r]) / (sum_e alpha_e + beta_r)
// A row without a list copies R[c, r] (exactly).  One writer per element, sums in list order, no atomics.
// LDS: CH * N floats, CH the largest of 8 / 4 / 2 / 1 within GO_RO_LDS = 80 KB — two workgroups of 1024 threads per CU
// beside each other at any size (160 KB of LDS, 2048 threads) — so 8 columns up to 2560 nodes, 4 (48 KB at the
// 3000-node DAG) up to 5120, 2 up to 10 240, 1 up to 20 480 nodes; above that the layer is refused.
#define GO_RO_T 1024
#define GO_RO_LDS (80 * 1024)

static int go_rollout_chunk(int N) {
  for (int ch = 8; ch >= 1; ch >>= 1)
    if ((size_t)ch * (size_t)N * sizeof(float) <= GO_RO_LDS) return ch;
  return 0;
}

extern "C" int igcn_go_rollout_chunk(int N) { return N > 0 ? go_rollout_chunk(N) : 0; }

template <int CH>
__global__ void __launch_bounds__(GO_RO_T)
k_go_rollout_layer(int N, int S, int pool, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                   const float* __restrict__ alpha, const float* __restrict__ beta, const float* __restrict__ r_in,
                   int64_t r_in_bs, float* __restrict__ r_out) {
  extern __shared__ float rs[];                              // [CH][N]
  const int b = blockIdx.y, s0 = blockIdx.x * CH, ns = min(CH, S - s0), M = N - pool;
  const float* rb = r_in + (int64_t)b * r_in_bs + (int64_t)s0 * N;
  for (int i = threadIdx.x; i < ns * N; i += blockDim.x) rs[i] = rb[i];
  __syncthreads();
  const float* ab = alpha + (int64_t)b * row_ptr[N];
  const float* bb = beta + (int64_t)b * N;
  float* ob = r_out + ((int64_t)b * S + s0) * M;
  for (int r = pool + threadIdx.x; r < N; r += blockDim.x) {
    const int32_t p0 = row_ptr[r], p1 = row_ptr[r + 1];
    float acc[CH], den = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0.f;
    for (int32_t e = p0; e < p1; ++e) {
      const float a = ab[e];
      const int m = col[e];
      den += a;
#pragma unroll
      for (int c = 0; c < CH; ++c)
        if (c < ns) acc[c] += a * rs[c * N + m];
    }
    const float g = bb[r];
    den += g;
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (c < ns) {
        const float own = rs[c * N + r];
        ob[(int64_t)c * M + (r - pool)] = p1 > p0 ? (acc[c] + g * own) / den : own;
      }
  }
}

extern "C" int igcn_go_rollout_layer(int B, int N, int S, int pool, const int32_t* row_ptr, const int32_t* col,
                                     const float* alpha, const float* beta, const float* r_in,
                                     int64_t r_in_batch_stride, float* r_out, void* stream) {
  IGCN_REQUIRE(B > 0 && B <= 65535 && N > 0 && S > 0 && pool >= 0 && pool < N, "go_rollout_layer: bad sizes");
  IGCN_REQUIRE(r_in_batch_stride == 0 || r_in_batch_stride >= (int64_t)S * N,
               "go_rollout_layer: r_in_batch_stride must be 0 (one R shared by all samples) or at least S * N");
  const int ch = go_rollout_chunk(N);
  if (ch == 0) {
    igcn_set_error("go_rollout_layer: N=%d nodes: one relevance column exceeds the %d KB of LDS a workgroup takes", N,
                   GO_RO_LDS / 1024);
    return IGCN_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const int rows = N - pool;
  const int threads = (int)(igcn_cdiv(rows < GO_RO_T ? rows : GO_RO_T, IGCN_WAVE) * IGCN_WAVE);
  const size_t lds = (size_t)ch * (size_t)N * sizeof(float);
  dim3 grid((unsigned)igcn_cdiv(S, ch), (unsigned)B);
#define CALL(CHV)                                                                                                    \
  do {                                                                                                               \
    IGCN_ALLOW_BIG_LDS((k_go_rollout_layer<CHV>));                                                                   \
    hipLaunchKernelGGL((k_go_rollout_layer<CHV>), grid, dim3(threads), lds, st, N, S, pool, row_ptr, col, alpha, beta, \
                       r_in, r_in_batch_stride, r_out);                                                              \
  } while (0)
  if (ch == 8) CALL(8);
  else if (ch == 4) CALL(4);
  else if (ch == 2) CALL(2);
  else CALL(1);
#undef CALL
  IGCN_CHECK_LAUNCH("go_rollout_layer");
  return IGCN_OK;
}
