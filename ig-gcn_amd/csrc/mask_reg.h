// loss_probability (kernel/sgcn_img_snp.py:153-181) riding in the mask kernels (igcn_edge_mask_{fwd,bwd}_reg, and the
// front kernel of csrc/sgcn_fused.hip): the same term / derivative as csrc/loss.hip's stand-alone regulariser.  For p in (0,1):
//   r(p) = l1 p - ent (p log(p + eps) + (1 - p) log(1 - p + eps))
#pragma once
#include "common.h"
__device__ __forceinline__ float em_reg_term(float p, float l1, float ent, float eps) {
  return l1 * fabsf(p) - ent * (p * logf(p + eps) + (1.f - p) * logf((1.f - p) + eps));
}
__device__ __forceinline__ float em_reg_grad(float p, float l1, float ent, float eps) {
  return l1 - ent * (logf(p + eps) + p / (p + eps) - logf((1.f - p) + eps) - (1.f - p) / ((1.f - p) + eps));
}

struct EmReg {                    // greg == NULL: no regulariser in this launch
  const float* greg;              // backward: d loss / d (regulariser), device scalar
  const float* snps;              // SNP mask logits [n_snps] (may be NULL)
  float* dsnps;                   // backward: their gradient (regulariser part + mask part)
  int n_snps;
  float l1_x, ent_x, l1_e, ent_e, eps;
  // the SNP mask itself (cal_probability :147-151) for the stacked sweep: feat [B, n_snps] -> full [2B, n_snps] =
  // (feat | feat * sigmoid(logits)); backward: d_full [2B, n_snps] (its masked half is read)
  const float* feat;
  float* full;
  const float* d_full;
  int B;
};

// The tail of the edge-mask backward as a launch of its own behind a node pass that ran elsewhere (k_sgcn_stack_bwd's
// masked copy, csrc/sgcn_fused.hip): k_edge_mask_bwd_prob (csrc/sgcn.hip) over gx [N, h0] and `rows` bias-gradient
// partial rows, plus, with dx, the workgroups that write dx = g_part * prob + dx_plain.
int igcn_launch_edge_mask_bwd_tail(int64_t n_nodes, int rois, int h0, const float* gx, const float* partial, int64_t rows,
                                   const float* g_part, const float* dx_plain, float* dx, float* dprob, float* dprob_bias,
                                   const float* prob, const EmReg& rg, hipStream_t st);
