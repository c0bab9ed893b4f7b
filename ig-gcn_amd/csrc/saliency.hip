// ROI x modality saliency maps from passes the models already run.
//
// Every reference forward sets data.x.requires_grad = True and keeps self.input (kernel/sgcn_img_snp.py:210-211,
// kernel/sgcn.py:113,362, kernel/gcn_img_snp.py) so that data.x.grad can be read as an input-gradient saliency, and
// SGCN_Ori fills the Grad-CAM taps final_conv_acts / final_conv_grads (kernel/sgcn.py:16-17,72,124-126); nothing in the
// reference forms a map from either.  The two kernels here do:
//
// k_saliency_maps — gradient x input (M = 1, no baseline) and the midpoint-rule integrated gradients (M path points):
//   attr[b,r,h] = (x[b,r,h] - base[.,r,h]) * ((1/M) * sum_{m<M} dx[m,b,r,h])      (m ascending, one thread per element)
//   roi[b,r]    = sum_{h<H0} |attr[b,r,h]|                                         (h ascending, one thread per row)
//   norm: both divided by the subject's largest roi (IEEE division); a subject whose largest roi is 0 is left as it is.
// One workgroup of 256 threads per subject.  The subject's attr tile [R, H0] and its roi [R] are built in LDS, the
// maximum is a fixed tree, and every element of attr / roi is stored exactly once, zeros included: one writer per
// element, no atomics, the same bits every run.  x, base and every dx[m] are read once, consecutive lanes on
// consecutive elements.  LDS budget: 34 KB static (8192 + 512 floats + the reduction scratch), so R <= 512,
// R * H0 <= 8192 and 1 <= M <= 4096 (IGCN_SALIENCY_MAX_ROIS, _MAX_ELEMS, _MAX_STEPS) — IGCN_ERR_UNSUPPORTED outside, nothing is truncated.  R = 54, H0 = 1 is the SNP
// vector.
//
// k_grad_cam — the Grad-CAM map of the taps:
//   alpha[b,k] = (1/R) * sum_{r<R} grads[b,r,k]      cam[b,r] = max(0, sum_{k<K} alpha[b,k] * acts[b,r,k])
//   norm: cam divided by the subject's maximum; a subject whose maximum is 0 stays at zero.
// One workgroup of 256 threads per subject.  alpha: thread (part p, column k), P = 256 / K parts, sums rows p, p + P, ...
// in ascending order (consecutive lanes on consecutive columns) and thread k adds the P partials in order.  cam: one
// wave per row — lane l adds columns l, l + 64, l + 128 in order, then a fixed xor tree.  LDS budget: 4 KB static
// (alpha, its partials, the R cam values, the reduction scratch): neither tile is staged — grads and acts are each
// streamed from global memory exactly once, so nothing is re-read however large R * K is.  Bounds: 1 <= R <= 512 (the
// configs[4] size), 1 <= K <= 160 (IGCN_GRAD_CAM_MAX_WIDTH); IGCN_ERR_UNSUPPORTED outside.  Every element of cam / alpha is
// stored exactly once.
#include "common.h"

#define SAL_T 256

// Block-wide maximum of non-negative values (blockDim.x = SAL_T); `red` holds >= 4 floats.  Result in all threads.
__device__ __forceinline__ float sal_block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();  // protect `red` from a previous use
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
  for (int i = 1; i < SAL_T / 64; ++i) t = fmaxf(t, red[i]);
  return t;
}

// base_mode: 0 = zeros (base not read), 1 = [R, H0] broadcast over subjects, 2 = [B R, H0]
__global__ void __launch_bounds__(SAL_T)
k_saliency_maps(int R, int H0, int M, int64_t total, const float* __restrict__ x, const float* __restrict__ base,
                int base_mode, const float* __restrict__ dx, int norm, float* __restrict__ attr,
                float* __restrict__ roi) {
  __shared__ float s_attr[IGCN_SALIENCY_MAX_ELEMS];
  __shared__ float s_roi[IGCN_SALIENCY_MAX_ROIS];
  __shared__ float s_red[SAL_T / 64];
  const int tid = threadIdx.x;
  const int n = R * H0;                                       // elements of one subject
  const int64_t off = (int64_t)blockIdx.x * n;
  const float inv_m = 1.0f / (float)M;
  for (int e = tid; e < n; e += SAL_T) {
    const float* g = dx + off + e;
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += g[(int64_t)m * total];
    float d = x[off + e];
    if (base_mode == 1) d -= base[e];
    else if (base_mode == 2) d -= base[off + e];
    s_attr[e] = d * (s * inv_m);
  }
  __syncthreads();
  float mx = 0.f;
  for (int r = tid; r < R; r += SAL_T) {
    float s = 0.f;
    for (int h = 0; h < H0; ++h) s += fabsf(s_attr[r * H0 + h]);
    s_roi[r] = s;
    mx = fmaxf(mx, s);
  }
  mx = sal_block_max(mx, s_red);                              // (its barriers also publish s_roi)
  const bool scale = norm && mx > 0.f;
  for (int e = tid; e < n; e += SAL_T) attr[off + e] = scale ? s_attr[e] / mx : s_attr[e];
  float* o_roi = roi + (int64_t)blockIdx.x * R;
  for (int r = tid; r < R; r += SAL_T) o_roi[r] = scale ? s_roi[r] / mx : s_roi[r];
}

extern "C" int igcn_saliency_maps(int B, int R, int H0, int M, const float* x, const float* base, int base_per_subject,
                                  const float* dx, int norm, float* attr, float* roi, void* stream) {
  IGCN_REQUIRE(B > 0 && R > 0 && H0 > 0 && M > 0, "saliency_maps: B=%d R=%d H0=%d M=%d", B, R, H0, M);
  if (R > IGCN_SALIENCY_MAX_ROIS || (int64_t)R * H0 > IGCN_SALIENCY_MAX_ELEMS || M > IGCN_SALIENCY_MAX_STEPS) {
    igcn_set_error("saliency_maps: R=%d H0=%d M=%d: needs R <= %d, R * H0 <= %d (the subject's tile in LDS) and M <= %d",
                   R, H0, M, IGCN_SALIENCY_MAX_ROIS, IGCN_SALIENCY_MAX_ELEMS, IGCN_SALIENCY_MAX_STEPS);
    return IGCN_ERR_UNSUPPORTED;
  }
  IGCN_REQUIRE(x && dx && attr && roi, "saliency_maps: null argument");
  const int64_t total = (int64_t)B * R * H0;
  IGCN_REQUIRE(total * M < ((int64_t)1 << 40), "saliency_maps: too many gradient elements");
  const int mode = base ? (base_per_subject ? 2 : 1) : 0;
  hipLaunchKernelGGL(k_saliency_maps, dim3((unsigned)B), dim3(SAL_T), 0, (hipStream_t)stream, R, H0, M, total, x, base,
                     mode, dx, norm, attr, roi);
  IGCN_CHECK_LAUNCH("saliency_maps");
  return IGCN_OK;
}

__global__ void __launch_bounds__(SAL_T)
k_grad_cam(int R, int K, const float* __restrict__ acts, const float* __restrict__ grads, int norm,
           float* __restrict__ cam, float* __restrict__ alpha) {
  __shared__ float s_part[SAL_T];                             // [P][K] partial column sums, P * K <= 256
  __shared__ float s_alpha[IGCN_GRAD_CAM_MAX_WIDTH];
  __shared__ float s_cam[IGCN_SALIENCY_MAX_ROIS];
  __shared__ float s_red[SAL_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t off = (int64_t)blockIdx.x * R * K;
  const float* g = grads + off;
  const float* a = acts + off;
  const int P = SAL_T / K;
  if (tid < P * K) {
    const int p = tid / K, k = tid - p * K;
    float s = 0.f;
    for (int r = p; r < R; r += P) s += g[(int64_t)r * K + k];
    s_part[tid] = s;
  }
  __syncthreads();
  if (tid < K) {
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += s_part[p * K + tid];
    s *= 1.0f / (float)R;
    s_alpha[tid] = s;
    alpha[(int64_t)blockIdx.x * K + tid] = s;
  }
  __syncthreads();
  for (int r = w; r < R; r += SAL_T / 64) {
    const float* row = a + (int64_t)r * K;
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s = __fmaf_rn(s_alpha[k], row[k], s);
    s = wave_sum_all(s);
    if (lane == 0) s_cam[r] = fmaxf(s, 0.f);
  }
  __syncthreads();
  float mx = 0.f;
  for (int r = tid; r < R; r += SAL_T) mx = fmaxf(mx, s_cam[r]);
  mx = sal_block_max(mx, s_red);
  const bool scale = norm && mx > 0.f;
  float* o = cam + (int64_t)blockIdx.x * R;
  for (int r = tid; r < R; r += SAL_T) o[r] = scale ? s_cam[r] / mx : s_cam[r];
}

extern "C" int igcn_grad_cam(int B, int R, int K, const float* acts, const float* grads, int norm, float* cam,
                             float* alpha, void* stream) {
  IGCN_REQUIRE(B > 0 && R > 0 && K > 0, "grad_cam: B=%d R=%d K=%d", B, R, K);
  if (R > IGCN_SALIENCY_MAX_ROIS || K > IGCN_GRAD_CAM_MAX_WIDTH) {
    igcn_set_error("grad_cam: R=%d K=%d: needs R <= %d and K <= %d", R, K, IGCN_SALIENCY_MAX_ROIS,
                   IGCN_GRAD_CAM_MAX_WIDTH);
    return IGCN_ERR_UNSUPPORTED;
  }
  IGCN_REQUIRE(acts && grads && cam && alpha, "grad_cam: null argument");
  hipLaunchKernelGGL(k_grad_cam, dim3((unsigned)B), dim3(SAL_T), 0, (hipStream_t)stream, R, K, acts, grads, norm, cam,
                     alpha);
  IGCN_CHECK_LAUNCH("grad_cam");
  return IGCN_OK;
}
