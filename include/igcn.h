/* igcn.h — C ABI of libigcn.so: hand-written gfx950 (CDNA4) kernels for IG-GCN's hot path.
 *
 * The reference (Houliang-Zhou/IG-GCN) is pure Python with no FFI: the path is entered through
 * kernel/sgcn_img_snp.py (SGCN_GCN_IMGSNP) and kernel/go_model.py (Gene_ontology_network), whose sparse
 * arithmetic lives in PyG 2.0.2 / torch-scatter 2.0.9 / torch.sparse.  Each entry point below names the
 * reference operator call site(s) it replaces (paths relative to the reference repo).
 *
 * Conventions
 *  - every pointer is a CALLER-OWNED DEVICE pointer (contiguous, from tensor.data_ptr()); the library
 *    never allocates, frees, copies to host or synchronises; all work is enqueued on `stream`
 *    (a hipStream_t passed as void*), so every call may be captured into a hipGraph.
 *  - float = fp32.  edge_index stays int64 at the boundary (PyG surface, sgcn_data.py:268-269); the plan
 *    holds int32 copies/permutations for the kernels.
 *  - return 0 on success, a negative IGCN_ERR_* otherwise; igcn_last_error() gives a thread-local text.
 *  - "CSR" = (ptr[n_rows+1], idx[nnz]) int32.  GO activations are CHANNEL-MAJOR: [B, f, N] (node index
 *    fastest) so that every access with consecutive nodes on consecutive lanes is coalesced.
 */
#ifndef IGCN_H
#define IGCN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define IGCN_OK 0
#define IGCN_ERR_BADARG (-1)
#define IGCN_ERR_LAUNCH (-2)
#define IGCN_ERR_UNSUPPORTED (-3)

/* ABI revision: bumped whenever a prototype below changes (argument added, removed or re-ordered).  igcn_version()
 * returns the revision the library was built from; a binding written against a different one must refuse to call
 * (igcn_amd/_lib.py does). */
#define IGCN_ABI_VERSION 441
int igcn_version(void);
const char* igcn_last_error(void);
/* A/B switches, set ONCE by the binding when it loads the library (from the IGCN_* environment variables): bit 0 no tiled
 * list walks, 1 no LDS-staged dense aggregation, 2 untiled CSR map kernels, 3 global-memory GO attention backward, 4 print
 * deferred reductions, 5 fp32 attention core under bf16 transforms, 8 gene read-out apply pass and gene decoding as two launches; gemm_bn_cap > 0 caps the GEMM tile width, attn_chunk_rows > 0 the rows per LDS chunk of the streamed
 * attention kernels (sweeps).  No launch path reads the environment. */
int igcn_configure(unsigned options, int gemm_bn_cap, int attn_chunk_rows);

/* Limits.  Every `#define IGCN_<NAME> <decimal literal>` of this header is the ONE place that number is written: the
 * kernels use the macro, and the Python binding reads it from this file (igcn_amd/_lib.py: LIMITS), as it reads the
 * prototypes.  Plain literals only (1048576, not 1 << 20): the binding evaluates no expression.  A limit stands next
 * to the entry points it bounds; the ones below bound several families.
 *   IGCN_LDS_BUDGET_BYTES  150 KB: what an LDS-resident graph stack (igcn_sgcn_stack_*, igcn_sgcn_ori_*,
 *                          igcn_gat_stack_*), the staged attention kernels and the long-list SpMM may ask for.
 *   IGCN_LDS_MAX_BYTES     160 KB: the dynamic-LDS ceiling of a gfx950 workgroup, raised per kernel on first use.
 *   IGCN_MAX_H0            input features per node of the edge masks and of every graph stack.
 *   IGCN_STACK_MAX_LAYERS  layers of igcn_sgcn_stack_*, igcn_gat_stack_*, igcn_dense_sgcn_*.
 *   IGCN_STACK_MIN_WIDTH, IGCN_STACK_MAX_WIDTH  layer widths: the powers of two in this range for igcn_sgcn_stack_* and
 *                          igcn_gat_stack_* (F in {4,8,16,32}), any width up to the maximum for igcn_sgcn_ori_*. */
#define IGCN_LDS_BUDGET_BYTES 153600
#define IGCN_LDS_MAX_BYTES 163840
#define IGCN_MAX_H0 8
#define IGCN_STACK_MAX_LAYERS 4
#define IGCN_STACK_MIN_WIDTH 4
#define IGCN_STACK_MAX_WIDTH 32

/* ------------------------------------------------------------------------------------------------
 * Graph plan: replaces the index work PyG's gcn_norm/propagate redo in every GCNConv call
 * (mask src!=dst, cat, arange, scatter index math; call sites kernel/sgcn_img_snp.py:218,221).
 * Built once per batch and shared by both forward passes, loss_probability and the backward.
 *   src32/dst32 [E]   int32 copies of edge_index rows
 *   tgt_ptr [N+1], tgt_perm [E] : edges grouped by TARGET node, original edge order kept inside a
 *                                 group (stable) => per-target sums run in the reference's scatter order
 *   src_ptr [N+1], src_perm [E] : same, grouped by SOURCE node (transposed structure for the backward)
 *   loop_edge [N]               : id of the LAST stored self-loop of node i, or -1
 * workspace: igcn_graph_plan_workspace_bytes(n_nodes, n_edges) bytes.
 */
size_t igcn_graph_plan_workspace_bytes(int64_t n_nodes, int64_t n_edges);
/* ------------------------------------------------------------------------------------------------
 * The GATConv stack of kernel/gcn_img_snp.py with ifUseGAT (PyG 2.0.2 GATConv(in, F, edge_dim=1): heads 1,
 * negative_slope 0.2, add_self_loops with fill_value 'mean', bias) x L, each followed by ReLU, + the jumping-knowledge
 * concatenation, for batches of SMALL UNIFORM graphs: ONE LDS-resident kernel per direction, one workgroup per graph,
 * on the per-graph plan (src32, dst32, tgt_ptr, tgt_perm; src_ptr, src_perm for the backward).  Per layer and target i:
 * h = x W^T, z_e = leaky_relu(h[src].att_src + h[i].att_dst + ea_e (lin_edge[:,0].att_edge)) over i's stored incoming
 * edges with src != dst plus one virtual loop whose ea is the mean of those edges' ea (0 if none), alpha = the edge
 * softmax over them (max-subtracted, + 1e-16 in the denominator), y_i = relu(sum alpha h[src] + bias).
 * F in {4,8,16,32}, L <= 4 (IGCN_STACK_MAX_LAYERS), H0 <= 8 (IGCN_MAX_H0) and igcn_gat_stack_lds_bytes(...) <= 150 KB
 * (IGCN_LDS_BUDGET_BYTES), IGCN_ERR_UNSUPPORTED otherwise.
 * params: HOST array of 6 L device pointers, per layer W [F, Fin_l] (Fin_0 = H0, then F), bias [F], att_src [F],
 * att_dst [F], lin_edge [F], att_edge [F].  ew_in [E]: the scalar edge attributes (igcn_gat_stack_bwd: data, no gradient).
 * Backward recomputes the forward in LDS; outputs dx_in [N, H0] (or NULL: not computed) and dparams
 * [igcn_gat_stack_param_floats] = the six gradients of layer 0 in the order above, then layer 1, ... (scratch: n_graphs
 * * that many floats; the sum over graphs is a final reduction in the sense of igcn_reduce_defer). */
size_t igcn_gat_stack_lds_bytes(int R, int max_edges, int H0, int F, int L, int backward);
int igcn_gat_stack_param_floats(int H0, int F, int L);
int igcn_gat_stack_fwd(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                       const float* ew_in, const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                       const int32_t* tgt_perm, const float* const* params, float* xcat, int32_t* status, void* stream);
int igcn_gat_stack_bwd(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                       const float* ew_in, const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                       const int32_t* tgt_perm, const int32_t* src_ptr, const int32_t* src_perm,
                       const float* const* params, const float* dxcat, float* dx_in, float* dparams, float* scratch,
                       int32_t* status, void* stream);
/* The same backward when the edge attributes are trained: kernel/sgcn.py:235-267 (SGCN_GAT.forward) passes edge_attr =
 * edge_weight * edge_prob to every GATConv of the masked pass, and kernel/train_eval_sgcn.py:305-308 backpropagates
 * through it into prob_bias / prob.  One more output dew [sum E] = d(loss)/d(ew_in), every element written: for a stored
 * edge k with src != dst and target i, sum_l c_l (dpre_l[k] + dpre_l[loop of i] / cnt_i) with c_l = lin_edge_l .
 * att_edge_l, dpre the gradient of the pre-leaky-ReLU logits and cnt_i the number of such edges into i (the logit term
 * and the 'mean' fill value of the added self-loop); exactly 0 for a stored self-loop (PyG removes it).  Same kernel
 * template, one workgroup per graph, no atomics; LDS: igcn_gat_stack_lds_bytes(..., backward = 2). */
int igcn_gat_stack_bwd_ew(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                          const float* ew_in, const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                          const int32_t* tgt_perm, const int32_t* src_ptr, const int32_t* src_perm,
                          const float* const* params, const float* dxcat, float* dx_in, float* dew, float* dparams,
                          float* scratch, int32_t* status, void* stream);
/* The coefficients the GATConv layers of that stack form and drop — what PyG hands out under
 * return_attention_weights=True (kernel/gcn_img_snp.py:217-221 with ifUseGAT, kernel/sgcn.py:235-267 SGCN_GAT.forward)
 * — as dense region x region maps, source row and target column like the reference's data.A:
 *   G [n_graphs, L, R, R]: G[g,l,i,j] = the sum over the stored copies of edge (i -> j), i != j, of alpha_l; G[g,l,j,j] =
 *   alpha_l of target j's added self-loop (stored self-loops contribute exactly 0: PyG removes them; a target without
 *   incoming edges has 1); 0 elsewhere.  Every target column sums to 1 up to the 1e-16 of the denominator.
 * Arguments and limits of igcn_gat_stack_fwd, G in place of xcat.  One workgroup per graph runs the forward's own
 * staging and layer functions on the forward's LDS layout and, after each layer, builds that layer's block one tile
 * of igcn_gat_stack_alpha_tile(...) target columns at a time in LDS (one [R, tile] block behind the layout, the whole
 * within 150 KB = IGCN_LDS_BUDGET_BYTES; 0 = nothing fits: IGCN_ERR_UNSUPPORTED): every element stored exactly once,
 * zeros included, one writer per element, no atomics, copies added in list order: bit-identical from run to run. */
int igcn_gat_stack_alpha_tile(int R, int max_edges, int H0, int F, int L);
int igcn_gat_stack_alpha(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                         const float* ew_in, const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                         const int32_t* tgt_perm, const float* const* params, float* G, int32_t* status, void* stream);
int igcn_graph_plan_build(int64_t n_nodes, int64_t n_edges, const int64_t* edge_index /*[2,E]*/,
                          int32_t* src32, int32_t* dst32, int32_t* tgt_ptr, int32_t* tgt_perm,
                          int32_t* src_ptr, int32_t* src_perm, int32_t* loop_edge,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Same plan for a block-diagonal PyG batch of SMALL graphs, one workgroup per graph, everything in LDS (no
 * device-wide sort): graph g owns nodes [node_ptr[g],node_ptr[g+1]) and edges [edge_ptr[g],edge_ptr[g+1]) (int64
 * device arrays of n_graphs+1 entries, as Batch.from_data_list records them; batch.py:24-123).  Limits: 1024 nodes
 * (IGCN_SEG_MAX_NODES) and 4096 edges (IGCN_SEG_MAX_EDGES) per graph (IGCN_ERR_UNSUPPORTED otherwise: use
 * igcn_graph_plan_build_tiled / igcn_graph_plan_build).
 * `status` (device int32, zeroed by the caller) is set non-zero if a graph exceeds the limits or an edge leaves its
 * graph. */
#define IGCN_SEG_MAX_NODES 1024
#define IGCN_SEG_MAX_EDGES 4096
int igcn_graph_plan_build_segmented(int64_t n_nodes, int64_t n_edges, int n_graphs, const int64_t* edge_index,
                                    const int64_t* node_ptr, const int64_t* edge_ptr,
                                    int64_t max_nodes_per_graph, int64_t max_edges_per_graph,
                                    int32_t* src32, int32_t* dst32, int32_t* tgt_ptr, int32_t* tgt_perm,
                                    int32_t* src_ptr, int32_t* src_perm, int32_t* loop_edge, int32_t* status,
                                    void* stream);
/* The same build, also filling the plan of `copies` disjoint copies of the batch (the seven arrays
 * igcn_graph_plan_replicate derives: copies*E, copies*E, copies*N+1, copies*E, copies*N+1, copies*E, copies*N). */
int igcn_graph_plan_build_segmented_rep(int64_t n_nodes, int64_t n_edges, int n_graphs, const int64_t* edge_index,
                                        const int64_t* node_ptr, const int64_t* edge_ptr, int64_t max_nodes_per_graph,
                                        int64_t max_edges_per_graph, int32_t* src32, int32_t* dst32, int32_t* tgt_ptr,
                                        int32_t* tgt_perm, int32_t* src_ptr, int32_t* src_perm, int32_t* loop_edge,
                                        int32_t* status, int copies, int32_t* o_src32, int32_t* o_dst32,
                                        int32_t* o_tgt_ptr, int32_t* o_tgt_perm, int32_t* o_src_ptr, int32_t* o_src_perm,
                                        int32_t* o_loop_edge, void* stream);

/* Same plan for a PyG batch whose graphs have at most 1024 nodes and ANY number of edges (the dense 512-ROI graphs of
 * the stress configuration: 262 144 edges each): a hand-written one-pass stable counting sort per graph over tiles of
 * 4096 edges (histogram / scan / ranked scatter, three launches for both groupings), the node id inside its graph
 * being the digit.  Same outputs and `status` convention as the segmented build; workspace:
 * igcn_graph_plan_tiled_workspace_bytes(n_graphs, max_nodes_per_graph, max_edges_per_graph) bytes. */
size_t igcn_graph_plan_tiled_workspace_bytes(int n_graphs, int64_t max_nodes_per_graph, int64_t max_edges_per_graph);
int igcn_graph_plan_build_tiled(int64_t n_nodes, int64_t n_edges, int n_graphs, const int64_t* edge_index,
                                const int64_t* node_ptr, const int64_t* edge_ptr,
                                int64_t max_nodes_per_graph, int64_t max_edges_per_graph,
                                int32_t* src32, int32_t* dst32, int32_t* tgt_ptr, int32_t* tgt_perm,
                                int32_t* src_ptr, int32_t* src_perm, int32_t* loop_edge, int32_t* status,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Plan of `copies` disjoint copies of the batch (node g*N+i, edge g*E+k) derived from an existing plan without
 * sorting again; output arrays are sized for copies*N nodes / copies*E edges. */
int igcn_graph_plan_replicate(int64_t n_nodes, int64_t n_edges, int copies,
                              const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                              const int32_t* tgt_perm, const int32_t* src_ptr, const int32_t* src_perm,
                              const int32_t* loop_edge,
                              int32_t* o_src32, int32_t* o_dst32, int32_t* o_tgt_ptr, int32_t* o_tgt_perm,
                              int32_t* o_src_ptr, int32_t* o_src_perm, int32_t* o_loop_edge, void* stream);

/* Per-edge values as dense region x region maps — the connective-importance mask e of cal_probability
 * (kernel/sgcn_img_snp.py:133-151; kernel/sgcn.py:198-209,321-332), or the weight edge_weight * e the convolutions
 * consume, laid out like the reference's data.A / coo_matrix(A).row, .col (source row, target column) for uniform
 * graphs of R nodes on the plan arrays (graph g = nodes [gR, (g+1)R)):
 *   map [n_graphs, R, R]: map[g,i,j] = the sum, in stored order, of values[k] over the stored copies k of edge
 *   (gR + i -> gR + j); 0 where none is stored.  cnt [n_graphs, R, R] (or NULL): the number of copies, as fp32.
 * One workgroup per (graph, tile of igcn_edge_dense_map_supported(R, cnt != NULL) target columns) builds the tile in
 * LDS (<= 64 KB) and stores it once: every element of map / cnt is written exactly once by the launch, zeros included
 * (no fill in front), one writer per element, no atomics, bit-identical from run to run.  Any per-target degree, ragged
 * edge counts, graphs without edges.  An edge whose ends lie in different graphs is not written and sets bit 0 of
 * `status` (device int32, or NULL).  igcn_edge_dense_map_supported = 0 (R above 8192 with counts, 16 384 without):
 * IGCN_ERR_UNSUPPORTED before anything runs. */
int igcn_edge_dense_map_supported(int R, int want_count);
int igcn_edge_dense_map(int64_t n_graphs, int R, int64_t n_edges, const float* values, const int32_t* src32,
                        const int32_t* dst32, const int32_t* tgt_ptr, const int32_t* tgt_perm, float* map,
                        float* cnt /*or NULL*/, int32_t* status /*or NULL*/, void* stream);

/* ROI x modality saliency maps.  Every reference forward sets data.x.requires_grad = True and keeps self.input
 * (kernel/sgcn_img_snp.py:210-211, kernel/sgcn.py:113,362, kernel/gcn_img_snp.py) only so that data.x.grad can be read as
 * an input-gradient saliency, and SGCN_Ori fills the Grad-CAM taps final_conv_acts / final_conv_grads
 * (kernel/sgcn.py:16-17,72,124-126); the reference forms no map from either.
 *
 * igcn_saliency_maps: gradient x input (M = 1, base NULL) and midpoint-rule integrated gradients (M path points).
 *   x [B R, H0]; base NULL (zeros), [R, H0] broadcast over subjects (base_per_subject = 0) or [B R, H0]
 *   (base_per_subject = 1); dx [M, B R, H0]: the input gradients of the M path points.
 *   attr [B, R, H0] = (x - base) * ((1/M) * sum_m dx[m]), m ascending;  roi [B, R] = sum_h |attr|, h ascending.
 *   norm = 1: a subject's attr and roi are divided by that subject's largest roi; a subject whose largest roi is 0 is
 *   left as it is.  The SNP vector is R = 54, H0 = 1.
 * igcn_grad_cam: acts, grads [B R, K] (the pre-ReLU conv3 activations and their gradient);
 *   alpha [B, K] = (1/R) sum_r grads[b,r,k];  cam [B, R] = max(0, sum_k alpha[b,k] acts[b,r,k]);
 *   norm = 1: cam divided by the subject's maximum; a subject whose maximum is 0 stays at zero.
 * Both: one workgroup per subject, fixed-order reductions, no atomics, every output element stored exactly once (zeros
 * included), bit-identical from run to run.  LDS: igcn_saliency_maps holds the subject's attr tile and roi, 34 KB static
 * — R <= 512 (IGCN_SALIENCY_MAX_ROIS), R * H0 <= 8192 (IGCN_SALIENCY_MAX_ELEMS), M <= 4096
 * (IGCN_SALIENCY_MAX_STEPS); igcn_grad_cam holds alpha, its partial sums and the R cam values, 4 KB static,
 * and streams acts and grads from global memory once each (no tile is staged, nothing re-read) — R <= 512, K <= 160
 * (IGCN_GRAD_CAM_MAX_WIDTH).
 * IGCN_ERR_UNSUPPORTED outside these bounds, before anything runs; nothing is truncated.  Per-class cohort sums:
 * igcn_attn_map_accumulate with Lq = R, Lk = H0 (or 1). */
#define IGCN_SALIENCY_MAX_ROIS 512
#define IGCN_SALIENCY_MAX_ELEMS 8192
#define IGCN_SALIENCY_MAX_STEPS 4096
#define IGCN_GRAD_CAM_MAX_WIDTH 160
int igcn_saliency_maps(int B, int R, int H0, int M, const float* x, const float* base /*or NULL*/, int base_per_subject,
                       const float* dx, int norm, float* attr, float* roi, void* stream);
int igcn_grad_cam(int B, int R, int K, const float* acts, const float* grads, int norm, float* cam, float* alpha,
                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * Learned regional / connective importance masks — cal_probability, kernel/sgcn_img_snp.py:133-151.
 *   xm[i,:]  = x[i,:] * prob[i % rois,:]
 *   e[k]     = sigmoid( [xm[src_k] || xm[dst_k]] . prob_bias )          ewm[k] = ew[k] * e[k]
 * x_plain [N,h0] / ew_plain [E] (may be NULL): plain copies of x / ew written alongside — the train step stacks the
 * plain and the masked pass (train() :521,523) into one batch, and xm / x_plain (ewm / ew_plain) are then the two
 * halves of the stacked tensors.
 */
int igcn_edge_mask_fwd(int64_t n_nodes, int64_t n_edges, int rois, int h0,
                       const float* x, const float* prob, const float* prob_bias, const float* ew,
                       const int32_t* src32, const int32_t* dst32,
                       float* xm, float* e, float* ewm, float* x_plain, float* ew_plain, void* stream);
/* d_xm [N,h0] may be NULL (=0); d_ewm, d_e [E] may be NULL; d_x_plain [N,h0] (may be NULL) is the gradient of the
 * plain copy, added into dx.  Outputs: dx [N,h0], dprob [rois,h0], dprob_bias [2*h0].
 * scratch: float[ N*h0 + 16*ceil(N/4) + 16 ]. */
int igcn_edge_mask_bwd(int64_t n_nodes, int64_t n_edges, int rois, int h0,
                       const float* x, const float* prob, const float* prob_bias, const float* ew,
                       const float* e, const float* d_xm, const float* d_ewm, const float* d_e,
                       const float* d_x_plain, const int32_t* tgt_ptr, const int32_t* tgt_perm,
                       const int32_t* src_ptr, const int32_t* src_perm,
                       float* dx, float* dprob, float* dprob_bias, float* scratch, void* stream);

/* The same two entry points with loss_probability (kernel/sgcn_img_snp.py:153-181) riding along — in a train step the
 * regulariser reads exactly what the mask launch has in registers (e per edge, prob, the SNP mask logits):
 *   forward: reg_partial [igcn_edge_mask_reg_blocks(...)] workgroup partials whose SUM is
 *            mean r_x(sigmoid(prob)) + mean r_e(e) + mean r_x(sigmoid(snps_logits))     (snps_logits NULL: without it)
 *   backward: d_reg [1] (device) = d loss / d (that sum); its edge part joins d_e inside the node pass, its prob part
 *            dprob, and dsnps [n_snps] receives the SNP logits' part.
 * Same arithmetic as igcn_mask_reg_{fwd,bwd}; two launches less per step. */
int igcn_edge_mask_reg_blocks(int64_t n_nodes, int64_t n_edges, int h0, int n_snps, int snps_rows);
/* snps_feat [snps_rows, n_snps] (or NULL): the launch also writes the SNP mask of the stacked sweep (cal_probability
 * :147-151), snps_full [2 snps_rows, n_snps] = (snps_feat | snps_feat * sigmoid(snps_logits)); the backward then takes
 * d_snps_full and adds sum_b d_masked[b,k] snps_feat[b,k] sigmoid'(logit_k) to dsnps — four launches of a train step
 * (mask, SNP mask, regulariser, and their backward pair) become the mask's two. */
int igcn_edge_mask_fwd_reg(int64_t n_nodes, int64_t n_edges, int rois, int h0, const float* x, const float* prob,
                           const float* prob_bias, const float* ew, const int32_t* src32, const int32_t* dst32, float* xm,
                           float* e, float* ewm, float* x_plain, float* ew_plain, const float* snps_logits, int n_snps,
                           float l1_x, float ent_x, float l1_e, float ent_e, float eps, float* reg_partial,
                           const float* snps_feat, int snps_rows, float* snps_full, void* stream);
int igcn_edge_mask_bwd_reg(int64_t n_nodes, int64_t n_edges, int rois, int h0, const float* x, const float* prob,
                           const float* prob_bias, const float* ew, const float* e, const float* d_xm, const float* d_ewm,
                           const float* d_e, const float* d_x_plain, const int32_t* tgt_ptr, const int32_t* tgt_perm,
                           const int32_t* src_ptr, const int32_t* src_perm, const float* d_reg, const float* snps_logits,
                           int n_snps, float l1_x, float ent_x, float l1_e, float ent_e, float eps, float* dx, float* dprob,
                           float* dprob_bias, float* dsnps, float* scratch, const float* snps_feat, int snps_rows,
                           const float* d_snps_full, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GCN normalisation — PyG gcn_norm inside GCNConv (kernel/sgcn_img_snp.py:218,221):
 * stored self-loops are replaced by one loop per node (weight wl = last stored loop weight, else 1),
 *   deg[i] = sum_{k: dst=i, src!=dst} ew[k] + wl[i] ;  dis = deg^-1/2 (inf -> 0)
 *   what[k] = dis[src]*ew[k]*dis[dst]  (0 at stored loops) ;  what_loop[i] = dis[i]*wl[i]*dis[i]
 * Computed ONCE per forward pass (the reference recomputes it in every layer); the L layers and the
 * backward all read the same coefficient arrays.
 */
int igcn_gcn_norm_fwd(int64_t n_nodes, int64_t n_edges, const float* ew,
                      const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr, const int32_t* tgt_perm,
                      const int32_t* src_perm, const int32_t* loop_edge, float* dis, float* wl,
                      float* what, float* what_loop, void* tstream /*[E] x 8 B*/, void* sstream /*[E] x 8 B*/,
                      void* stream);
/* tstream[p] = {int32 source node, float coefficient} of the p-th edge of the by-TARGET grouping, sstream[p] =
 * {int32 target node, float coefficient} of the p-th edge of the by-SOURCE grouping: the aggregation kernels stream
 * these 8-byte records coalesced instead of chasing permutation -> edge -> endpoint. */
/* dwhat [E] (entries of stored loops ignored) and dwhat_loop [N] are d(loss)/d(coefficient) summed over all
 * layers.  Output dew [E].  scratch: float[N]. */
int igcn_gcn_norm_bwd(int64_t n_nodes, int64_t n_edges, const float* ew, const float* dis, const float* wl,
                      const float* dwhat, const float* dwhat_loop,
                      const int32_t* src32, const int32_t* dst32,
                      const int32_t* tgt_ptr, const int32_t* tgt_perm,
                      const int32_t* src_ptr, const int32_t* src_perm, const int32_t* loop_edge,
                      float* dew, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GCN scatter-aggregate (the north-star kernel) — GCNConv.propagate + bias (+ the F.relu of
 * kernel/sgcn_img_snp.py:218,221):
 *   out[t, :F] = act( sum_{p in group(t)} tstream[p].w * h[tstream[p].idx,:] + what_loop[t]*h[t,:] + bias )
 * summed in the reference's scatter order (non-loop edges in stored order, then the loop).
 * h [N,F] row stride ld_h; out row stride ld_out (so a layer can write its column slice of the JK-concat
 * buffer of :223 directly).  relu != 0 applies max(.,0).  Three launch shapes, picked from the arguments:
 * thread = (target, feature quad) for low in-degree (brain graphs, k = 3); for an average in-degree >= 16 one wave per
 * target in which every lane moves 16 bytes per memory instruction (F/4 lanes per feature row, 64/(F/4) edge slots);
 * and, when `nodes_per_graph` (uniform graph size of a block-diagonal batch, 0 = unknown) is given, the average
 * in-degree is >= 64 and a graph's rows fit 64 KB of LDS (the dense 512-ROI graphs of the stress configuration), a
 * workgroup per 64 targets of one graph that stages the graph's rows in LDS and streams the 8-byte records from HBM
 * (two per 16-byte load) — per-target sums then run lane-parallel, not in the sequential scatter order.
 */
int igcn_gcn_propagate_fwd(int64_t n_nodes, int64_t n_edges, int F, int nodes_per_graph /*0 = unknown*/,
                           const float* h, int64_t ld_h, const void* tstream, const float* what_loop, const float* bias,
                           const int32_t* tgt_ptr, float* out, int64_t ld_out, int relu, void* stream);
/* Backward of the above.  g = dout * (out>0 if relu).  Outputs:
 *   dh [N,F] (row stride ld_dh)  = A_hat^T g          dbias [F] (may be NULL)
 *   dwhat [E] = g[dst_k].h[src_k] (0 at stored loops), dwhat_loop [N] = g[i].h[i]   (only when need_dw != 0)
 * scratch: igcn_gcn_propagate_bwd_scratch_floats(n_nodes, F) floats (block partials of dbias + the ReLU-masked
 * copy of dout that the per-edge kernels gather). */
size_t igcn_gcn_propagate_bwd_scratch_floats(int64_t n_nodes, int F);
int igcn_gcn_propagate_bwd(int64_t n_nodes, int64_t n_edges, int F, int nodes_per_graph /*0 = unknown*/,
                           const float* dout, int64_t ld_dout, const float* out, int64_t ld_out, int relu,
                           const float* h, int64_t ld_h, const void* sstream, const float* what_loop,
                           const int32_t* src32, const int32_t* dst32, const int32_t* src_ptr,
                           float* dh, int64_t ld_dh, float* dbias,
                           int need_dw, float* dwhat, float* dwhat_loop,
                           float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The whole SGCN stack of kernel/sgcn_img_snp.py:218-224 for batches of SMALL UNIFORM graphs, LDS-resident: PyG
 * gcn_norm + L x (X W_l^T, scatter-aggregate, + b_l, ReLU) + the jumping-knowledge concatenation as ONE kernel per
 * direction, one workgroup per graph (north_star: "LDS staging of per-block node features").  HBM carries only the
 * compulsory traffic of SURVEY §8d's "fused SGCN forward lower bound": x_in [n_graphs*R, H0], the graph's edges and
 * ew_in in, xcat [n_graphs*R, L*F] out.  Needs a block-diagonal batch (graph g = nodes [gR, (g+1)R), its edges
 * contiguous in stored order — what the per-graph plan builders verify), at most `max_edges` edges per graph,
 * F in {4,8,16,32}, L <= 4 (IGCN_STACK_MAX_LAYERS), H0 <= 8 (IGCN_MAX_H0) and igcn_sgcn_stack_lds_bytes(...) <= 150 KB
 * (IGCN_LDS_BUDGET_BYTES), IGCN_ERR_UNSUPPORTED otherwise: use
 * igcn_gcn_norm_* / igcn_gemm_f32 / igcn_gcn_propagate_*.  W / b: HOST arrays of L device pointers, W_l [F, Fin_l]
 * row-major (Fin_0 = H0, then F), b_l [F].
 * Backward recomputes the forward in LDS; outputs dx_in [N, H0], dew_in [E] and dparams
 * [igcn_sgcn_stack_param_floats] = dW_0 | db_0 | dW_1 | db_1 | ... (scratch: n_graphs * that many floats; the sum over
 * graphs is a final reduction in the sense of igcn_reduce_defer).  dxcat2 (or NULL): the gradient of a second consumer
 * of xcat, added to dxcat while the rows are staged (the attention query and the head inputs both read xcat). */
size_t igcn_sgcn_stack_lds_bytes(int R, int max_edges, int H0, int F, int L, int backward);
int igcn_sgcn_stack_param_floats(int H0, int F, int L);
int igcn_sgcn_stack_fwd(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                        const float* ew_in, const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                        const int32_t* tgt_perm, const int32_t* loop_edge, const float* const* W,
                        const float* const* b, float* xcat, int32_t* status, void* stream);
int igcn_sgcn_stack_bwd(int64_t n_graphs, int R, int max_edges, int H0, int F, int L, const float* x_in,
                        const float* ew_in, const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                        const int32_t* tgt_perm, const int32_t* src_ptr, const int32_t* src_perm,
                        const int32_t* loop_edge, const float* const* W, const float* const* b, const float* dxcat,
                        const float* dxcat2, float* dx_in, float* dew_in, float* dparams, float* scratch,
                        int32_t* status, void* stream);
/* igcn_sgcn_stack_bwd on the 2-copy (plain | masked) plan of a train step together with igcn_edge_mask_bwd_reg, as two
 * launches instead of three: the masked copy's workgroups of the stack kernel hold the mask backward's per-node operands
 * in LDS (lists, d_xm, d_ewm) and do its node pass themselves, in the summation order of the sparse node kernel; the tail
 * launch sums dprob / dprob_bias / dsnps and writes dx.  Sparse batches only (n_edges < 16 nodes).  n_graphs, n_edges: of
 * ONE copy; the plan arrays, x_in, ew_in, dxcat, dxcat2 and scratch (2 n_graphs * param_floats) are the 2-copy ones.
 * dx_plain [N, H0] / dew_plain [E]: the plain copy's stack gradients (dx_plain is added into dx).  d_e, d_reg, dx, dsnps
 * may be NULL.  mask_scratch: 2 N H0 + 16 n_graphs floats.  Every output but dprob_bias has the bits of the two calls;
 * dprob_bias is summed per graph and not per 64 nodes. */
int igcn_sgcn_stack_bwd_mask(int64_t n_graphs, int64_t n_edges, int R, int max_edges, int H0, int F, int L,
                             const float* x_in, const float* ew_in, const int32_t* src32, const int32_t* dst32,
                             const int32_t* tgt_ptr, const int32_t* tgt_perm, const int32_t* src_ptr,
                             const int32_t* src_perm, const int32_t* loop_edge, const float* const* W,
                             const float* const* b, const float* dxcat, const float* dxcat2, float* dx_plain,
                             float* dew_plain, float* dparams, float* scratch, int32_t* status, const float* x,
                             const float* prob, const float* prob_bias, const float* ew, const float* e,
                             const float* d_e, const float* d_reg, const float* snps_logits, int n_snps, float l1_x,
                             float ent_x, float l1_e, float ent_e, float eps, float* dx, float* dprob,
                             float* dprob_bias, float* dsnps, float* mask_scratch, const float* snps_feat,
                             int snps_rows, const float* d_snps_full, void* stream);
/* THE FRONT OF THE IMAGE BRANCH OF A TRAIN STEP AS ONE LAUNCH (kernel/sgcn_img_snp.py:133-151 cal_probability, :153-181
 * loss_probability, :218-224 the GCNConv stack; train() :521-523 runs them for the plain and the masked pass): for a batch
 * of n_graphs uniform graphs of R nodes (at most max_edges edges each, edge_index int64 [2, n_edges] with per-graph
 * offsets node_ptr / edge_ptr [n_graphs + 1]) workgroup (copy, graph) of the stacked (plain | masked) batch builds the
 * graph's plan in LDS — what igcn_graph_plan_build_segmented_rep(copies = 2) writes: `plan` = the seven arrays of the
 * batch, `plan2` = those of its 2-copy replica — forms the pass's inputs (x_in [2N, H0], ew_in [2E], the edge mask e [E]
 * = igcn_edge_mask_fwd_reg's outputs, reg_partial [n_graphs] whose SUM is loss_probability, snps_full [2 n_graphs, n_snps]
 * = (snps_feat | snps_feat * sigmoid(snps_logits)); snps_feat NULL: no SNP mask) and runs igcn_sgcn_stack_fwd's layers:
 * xcat [2N, L F].  Same arithmetic, in the same order, as the three launches it replaces (the regulariser's partial sums
 * are grouped per graph instead of per 256 edges).  A dropout rider waiting on the stream (igcn_rider_dropout) is carried
 * by this launch.  status: bit 0 = the batch is not block diagonal in the declared segments / not uniform, bit 1 = a graph
 * has more than max_edges edges (its outputs are not written). */
size_t igcn_sgcn_front_lds_bytes(int R, int max_edges, int H0, int F, int L);
int igcn_sgcn_front_fwd(int64_t n_nodes, int64_t n_edges, int n_graphs, int R, int max_edges, int H0, int F, int L,
                        const int64_t* edge_index, const int64_t* node_ptr, const int64_t* edge_ptr,
                        int32_t* const* plan /*HOST [7]*/, int32_t* const* plan2 /*HOST [7]*/, int32_t* status,
                        const float* x, const float* prob, const float* prob_bias, const float* ew, float* x_in,
                        float* ew_in, float* e, const float* snps_logits, int n_snps, float l1_x, float ent_x, float l1_e,
                        float ent_e, float eps, float* reg_partial, const float* snps_feat, float* snps_full,
                        const float* const* W /*HOST [L]*/, const float* const* b /*HOST [L]*/, float* xcat, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SGCN_Ori's graph stack (kernel/sgcn.py:111-148: conv1, ReLU, conv3, the Grad-CAM tap, ReLU, final_z), LDS-resident
 * like igcn_sgcn_stack_* and on the same per-graph plan, with two layers of INDEPENDENT width: per graph
 *   h1 = relu(GCNConv1(x)) [R, F1],  acts = GCNConv3(h1) [R, F3] (no ReLU: final_conv_acts, :124),  h3 = relu(acts);
 * gcn_norm runs once.  Row g of z [n_graphs, R*F1 + R*F3] = [h1 of graph g node-major | h3 of graph g node-major]: the
 * reference's final_z (:128-138) written in place; acts [n_graphs*R, F3].  1 <= H0 <= 8 (IGCN_MAX_H0), 1 <= F1, F3 <= 32
 * (IGCN_STACK_MAX_WIDTH; any value: a width is rounded up to a multiple of 4 inside LDS only) and
 * igcn_sgcn_ori_lds_bytes(...) <= 150 KB (IGCN_LDS_BUDGET_BYTES), otherwise
 * IGCN_ERR_UNSUPPORTED.  W1 [F1, H0], b1 [F1], W3 [F3, F1], b3 [F3].  A graph with more than max_edges edges sets status
 * bit 1 and leaves its outputs unwritten.
 * Backward recomputes the forward in LDS: dx_in [N, H0], dew_in [E] (every element written), dparams
 * [igcn_sgcn_ori_param_floats] = dW1 | db1 | dW3 | db3 (scratch: n_graphs * that many floats; the sum over graphs is a
 * final reduction in the sense of igcn_reduce_defer), and dacts [n_graphs*R, F3] (or NULL) = d(loss)/d(acts): dz's h3
 * block where acts > 0 and exactly 0 elsewhere — what the reference's hook stores as final_conv_grads (:71-72,125).
 * dacts_in (or NULL): a gradient the caller holds on acts itself, added at the tap (and then part of dacts). */
size_t igcn_sgcn_ori_lds_bytes(int R, int max_edges, int H0, int F1, int F3, int backward);
int igcn_sgcn_ori_param_floats(int H0, int F1, int F3);
int igcn_sgcn_ori_fwd(int64_t n_graphs, int R, int max_edges, int H0, int F1, int F3, const float* x_in,
                      const float* ew_in, const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                      const int32_t* tgt_perm, const int32_t* loop_edge, const float* W1, const float* b1,
                      const float* W3, const float* b3, float* z, float* acts, int32_t* status, void* stream);
int igcn_sgcn_ori_bwd(int64_t n_graphs, int R, int max_edges, int H0, int F1, int F3, const float* x_in,
                      const float* ew_in, const int32_t* src32, const int32_t* dst32, const int32_t* tgt_ptr,
                      const int32_t* tgt_perm, const int32_t* src_ptr, const int32_t* src_perm,
                      const int32_t* loop_edge, const float* W1, const float* b1, const float* W3, const float* b3,
                      const float* dz, const float* dacts_in, float* dacts, float* dx_in, float* dew_in,
                      float* dparams, float* scratch, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of a bias-free projection y = x W^T (x [M, K], W [N, K]) in ONE pass over the gradient G = dL/dy [M, N]:
 * dX [M, K] = G W and dW [N, K] = G^T X — the packed input projection of nn.MultiheadAttention
 * (kernel/sgcn_img_snp.py:240-241), whose key | value gradient is a 52 MB tensor that two separate GEMMs read twice.
 * K == 32, N in {32, 64} (igcn_proj_bwd_supported); scratch: igcn_proj_bwd_scratch_floats(M, N) floats; dW is a final
 * reduction in the sense of igcn_reduce_defer. */
int igcn_proj_bwd_supported(int64_t M, int N, int K);
int igcn_proj_bwd_blocks(int64_t M);
size_t igcn_proj_bwd_scratch_floats(int64_t M, int N);   /* per projection, for every igcn_proj_bwd* entry point */
int igcn_proj_bwd(int64_t M, int N, int K, const float* G, const float* X, const float* W, float* dX, float* dW,
                  float* scratch, void* stream);
/* two projections with the same K in ONE launch (the query block and the key | value block of the packed in-projection) */
int igcn_proj_bwd_pair(int64_t M1, int N1, const float* G1, const float* X1, const float* W1, float* dX1, float* dW1,
                       float* scratch1, int64_t M2, int N2, const float* G2, const float* X2, const float* W2,
                       float* dX2, float* dW2, float* scratch2, int K, void* stream);
/* ... with the bias gradients db_i [N_i] = column sums of G_i from the same pass (NULL: not wanted); the first db_zero_i
 * entries are written as exact zeros (the attention's key bias).  scratch_i: igcn_proj_bwd_scratch_floats(M_i, N_i)
 * floats; db_i are final reductions like dW_i. */
int igcn_proj_bwd_pair_bias(int64_t M1, int N1, const float* G1, const float* X1, const float* W1, float* dX1, float* dW1,
                            float* scratch1, float* db1, int db_zero1, int64_t M2, int N2, const float* G2,
                            const float* X2, const float* W2, float* dX2, float* dW2, float* scratch2, float* db2,
                            int db_zero2, int K, void* stream);
/* Forward of the same projections, y = x W^T + b (bias [N] or NULL), as ONE streaming launch for up to two of them
 * (M2 = 0: the first alone): W and b resident in LDS, x read once, y written in contiguous runs — the in-projection's
 * reduction depth is 32, so the general tiled GEMM's K loop and per-column-tile re-reads of x only cost.  Same shape
 * limits as igcn_proj_bwd_supported; exact fp32. */
int igcn_proj_fwd_blocks(int64_t M);
int igcn_proj_fwd_pair(int64_t M1, int N1, const float* X1, const float* W1, const float* b1, float* Y1, int64_t M2, int N2,
                       const float* X2, const float* W2, const float* b2, float* Y2, int K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the two heads' first layers y = relu(x W^T + b) (kernel/sgcn_img_snp.py:299 lin1, :302 lin1_regr; x [R, C]
 * the head inputs, W [64, C]) in one pass over the wide operands: g = dy * (y > 0), db = column sums of g, dx = g W,
 * dW = g^T x — x and W read once, dx written once, no masked copy of dy, no separate bias-gradient launch.
 * Hidden width H == 64, C even (igcn_head_bwd_supported); y_i NULL = no ReLU; C2 = 0 = the first layer alone.  With
 * R > 128 the rows are split: dW_i / db_i are then final reductions in the sense of igcn_reduce_defer over partials in
 * scratch_i (igcn_head_bwd_scratch_floats(R, C_i) floats; must stay alive until the flush).  Exact fp32. */
int igcn_head_bwd_supported(int R, int H, int C);
size_t igcn_head_bwd_scratch_floats(int R, int C);
int igcn_head_bwd_pair(int R, int H, int C1, const float* dy1, const float* y1, const float* W1, const float* X1,
                       float* dX1, float* dW1, float* db1, float* scratch1, int C2, const float* dy2, const float* y2,
                       const float* W2, const float* X2, float* dX2, float* dW2, float* db2, float* scratch2,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * SGCN over DENSE brain graphs (BASELINE configs[4]): batches whose graphs are COMPLETE — all R x R (source, target)
 * pairs stored in row-major order, i.e. a dense adjacency turned into COO — so that edge_attr IS the matrix
 * ew[g][src][dst] and edge_index carries no information.  Replaces, for such batches, cal_probability
 * (kernel/sgcn_img_snp.py:133-151), PyG gcn_norm + GCNConv x L + ReLU + concatenation (:218-224) and the edge part of
 * loss_probability (:153-181) of BOTH passes of a train step: every edge pass reads the 4-byte weight once and
 * recomputes mask / coefficient on the fly; the aggregations run on the matrix cores (csrc/sgcn_dense.hip).
 *   igcn_dense_blocks_check : verifies edge k of graph g == (g R + k / R, g R + k % R) — a 16-byte-per-edge read stream.
 *                             status: device int32[2]; status[1] = the LATEST check's verdict (cleared in front of every
 *                             check, 1 on a mismatch), status[0] |= 4 on a mismatch (sticky; a host-side check reads it).
 *   igcn_dense_sgcn_fwd(status, check_edge_index): status = those words, or NULL.  A set verdict turns the first layer's
 *                             features — hence every output and the loss — into NaN (a batch that is not row-major
 *                             complete must not train silently).  check_edge_index != NULL: the check of THIS batch
 *                             rides in the forward's first edge pass (extra workgroups of that launch stream the
 *                             index pairs) instead of a launch of its own in front; NULL: the verdict of an earlier
 *                             igcn_dense_blocks_check on the stream is consumed.
 *   igcn_dense_sgcn_supported: 64 <= R <= 1024, R % 64 == 0, F == 16, L <= 4, H0 <= 8.
 *   copies = 1: one pass (first_masked = isExplain); copies = 2: rows [0, G R) of xcat = plain pass, [G R, 2 G R) = masked.
 *   W / b: HOST arrays of L device pointers (W_l [F, Fin_l] row-major, Fin_0 = H0).  ws: igcn_dense_sgcn_ws_floats
 *   floats, written by fwd and read by bwd.  reg_partials [igcn_dense_sgcn_reg_blocks]: un-reduced partials of
 *   loss_probability (their SUM is the loss; NULL or copies == 1 plain: not written); snps_prob may be NULL.
 *   bwd: dxcat2 = the gradient of a second consumer of xcat (attention query | head inputs), added to dxcat where it is
 *   read, or NULL; d_reg = d loss / d (every partial), one device float (NULL: 0); outputs dx [G R, H0] (both passes' sum),
 *   dprob [R, H0], dprob_bias [2 H0], dsnps_prob [n_snps] (regulariser part only; may be NULL) and dparams
 *   [igcn_sgcn_stack_param_floats] = dW_0 | db_0 | dW_1 | ... (final reductions in the sense of igcn_reduce_defer);
 *   bws: igcn_dense_sgcn_bwd_ws_floats floats of scratch. */
int igcn_dense_blocks_check(int64_t n_graphs, int R, const int64_t* edge_index, int32_t* status, void* stream);
int igcn_dense_sgcn_supported(int R, int H0, int F, int L);
size_t igcn_dense_sgcn_ws_floats(int64_t n_graphs, int R, int L, int copies);
size_t igcn_dense_sgcn_bwd_ws_floats(int64_t n_graphs, int R, int H0, int L, int copies);
int igcn_dense_sgcn_reg_blocks(int64_t n_graphs, int R);
int igcn_dense_sgcn_fwd(int64_t n_graphs, int R, int H0, int F, int L, int copies, int first_masked, const float* x,
                        const float* prob, const float* prob_bias, const float* ew, const float* const* W,
                        const float* const* b, const float* snps_prob, int n_snps, float l1_x, float ent_x, float l1_e,
                        float ent_e, float eps, float* xcat, float* reg_partials, float* ws, int32_t* status,
                        const int64_t* check_edge_index, void* stream);
int igcn_dense_sgcn_bwd(int64_t n_graphs, int R, int H0, int F, int L, int copies, int first_masked, const float* x,
                        const float* prob, const float* prob_bias, const float* ew, const float* const* W,
                        const float* snps_prob, int n_snps, float l1_x, float ent_x, float l1_e, float ent_e, float eps,
                        const float* xcat, const float* dxcat, const float* dxcat2, const float* d_reg, const float* ws,
                        float* bws, float* dx, float* dprob, float* dprob_bias, float* dsnps_prob, float* dparams,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense feature transform on the matrix cores (f32-input MFMA 16x16x4, exact fp32):
 *   out[M,N] = act( A[M,K] . W[N,K]^T + bias )      — GCNConv.lin (kernel/sgcn_img_snp.py:34-49),
 *   lin1 / lin1_regr / lin2 / lin2_regr (:62-84,289-301).  General strided form so the same kernel
 *   serves forward (NT), input-gradient (NN) and weight-gradient (TN, split over the long M axis):
 *   C[m,n] = sum_k A[m*sam + k*sak] * B[n*sbn + k*sbk]  (+ bias[n]) ; C row stride ldc.
 * split_k > 1 writes split_k partial slabs into `scratch` (float[split_k*M*N]) and reduces them in order
 * (deterministic).  act: 0 none, 1 relu.
 */
/* Narrow output layer y[R,C] = x[R,K] W[C,K]^T + b[C] with C <= 4 (lin2 / lin2_regr, kernel/sgcn_img_snp.py:289-301)
 * as one VALU kernel per direction.  K/4 must be a power of two <= 64; x, W, dx 16-byte aligned.
 * Backward: dx [R,K] (may be NULL) and dwb [C*K + C] = dW (row-major [C,K]) followed by db.
 * scratch: igcn_small_linear_bwd_scratch_floats(R, K, C). */
size_t igcn_small_linear_bwd_scratch_floats(int64_t R, int K, int C);
/* `keep` [R,K] (may be NULL): dropout factors {0, 1/(1-p)} of the INPUT (F.dropout in front of lin2 / lin2_regr,
 * kernel/sgcn_img_snp.py:289,299), applied inside the kernels: y = (x * keep) W^T + b. */
int igcn_small_linear_fwd(int64_t R, int K, int C, const float* x, const float* keep, const float* W, const float* b,
                          float* y, void* stream);
int igcn_small_linear_bwd(int64_t R, int K, int C, const float* x, const float* keep, const float* W,
                          const float* dy, float* dx, float* dwb, float* scratch, void* stream);
/* Two such layers over inputs of the same [R, K] shape in one launch each way (lin2 and lin2_regr of the two heads):
 * per layer the arguments of igcn_small_linear_{fwd,bwd}. */
int igcn_small_linear_pair_fwd(int64_t R, int K, int C0, const float* x0, const float* keep0, const float* W0,
                               const float* b0, float* y0, int C1, const float* x1, const float* keep1,
                               const float* W1, const float* b1, float* y1, void* stream);
int igcn_small_linear_pair_bwd(int64_t R, int K, int C0, const float* x0, const float* keep0, const float* W0,
                               const float* dy0, float* dx0, float* dwb0, float* scratch0, int C1, const float* x1,
                               const float* keep1, const float* W1, const float* dy1, float* dx1, float* dwb1,
                               float* scratch1, void* stream);

/* SNP importance mask of cal_probability (kernel/sgcn_img_snp.py:147-151): out [B,S] = snps * sigmoid(p),
 * sp [S] = sigmoid(p).  Backward: dp [S] from dout [B,S] and/or dsp [S] (either may be NULL); snps gets no gradient. */
int igcn_snps_mask_fwd(int B, int S, const float* snps, const float* p, float* out, float* sp,
                       float* plain /* [B,S] copy of snps for the stacked batch, or NULL */, void* stream);
int igcn_snps_mask_bwd(int B, int S, const float* snps, const float* p, const float* dout, const float* dsp,
                       float* dp, void* stream);

/* Inputs of the two MLP heads (kernel/sgcn_img_snp.py:284-297) in one pass, R = passes * bsz rows (pass-major):
 *   out_z [R,W] = (img + cross) / 2;  out_lin [R,W+L] = out_z | latent;
 *   feat [R,W+L+P] = out_lin | (x * prob)[row % bsz]   (x [bsz,P] = data.x per sample, prob [P]; P = 0: feat NULL).
 * Backward: any of d_out_z / d_out_lin / d_feat may be NULL; d_mid [R,W] is the gradient of img and of cross,
 * d_latent [R,L], dx [bsz,P], dprob [P] (the last two only when P > 0).  W, L, P even. */
int igcn_head_inputs_fwd(int64_t R, int bsz, int W, int L, int P, const float* img, const float* cross,
                         const float* latent, const float* x, const float* prob, float* out_z, float* out_lin,
                         float* feat, void* stream);
int igcn_head_inputs_bwd(int64_t R, int bsz, int W, int L, int P, const float* d_out_z, const float* d_out_lin,
                         const float* d_feat, const float* x, const float* prob, float* d_mid, float* d_latent,
                         float* dx, float* dprob, void* stream);
/* The same backward that also takes the ReLU backward and the bias gradient of the layer whose POST-ReLU output `cross`
 * [R, W] is (relu(out_proj(.)), kernel/sgcn_img_snp.py:241-242; W = positions x D features): d_cross [R, W] = the gradient
 * of that layer's pre-activation (d_mid where cross > 0), db [D] = its column sums by feature, through the partial rows
 * db_part [igcn_head_inputs_bwd_blocks(R, W, L)][D] and a final reduction that is deferred while the stream defers.
 * D a power of two, 2 <= D <= 64, W % D == 0. */
/* igcn_head_inputs_fwd with the layer in front computed on the way: cross [R, W] = relu(o Wp^T + bp) per graph node
 * (o [R, W] = [R, W / D nodes, D features], Wp [D, D], bp [D]: relu(out_proj(.)), kernel/sgcn_img_snp.py:241-242), written
 * as well (the backward's ReLU mask, igcn_head_inputs_bwd_relu).  fp32 FMAs in k order.  D a power of two in [2, 64]
 * dividing W. */
int igcn_outproj_head_inputs_fwd(int64_t R, int bsz, int W, int L, int P, int D, const float* o, const float* Wp,
                                 const float* bp, const float* img, const float* latent, const float* x, const float* prob,
                                 float* cross, float* out_z, float* out_lin, float* feat, void* stream);
int igcn_head_inputs_bwd_blocks(int64_t R, int W, int L);
int igcn_head_inputs_bwd_relu(int64_t R, int bsz, int W, int L, int P, const float* d_out_z, const float* d_out_lin,
                              const float* d_feat, const float* x, const float* prob, float* d_mid, float* d_latent,
                              float* dx, float* dprob, const float* cross, float* d_cross, int D, float* db_part,
                              float* db, void* stream);

/* out[r, p*F + c] = parts[p][r, c], p < nparts <= 4: concatenation of the GCN layer outputs along the feature axis
 * (kernel/sgcn_img_snp.py:223-224, kernel/sgcn.py:376-377 `torch.cat(xs, dim=1)`).  F % 4 == 0, 16-byte aligned
 * tensors; `parts` is a HOST array of device pointers. */
int igcn_concat_cols(int64_t rows, int F, int nparts, const float* const* parts, float* out, void* stream);

/* Hand-over of a new batch to a captured train step (train.GraphedTrainStep.load; the reference's
 * `data = data.to(device)`, kernel/train_eval_sgcn_img_snps.py:517): up to IGCN_COPY_MULTI_MAX device-to-device copies
 * of arbitrary byte counts as ONE launch — x, edge_index, edge_attr, snps_feat, y, clini_score, tsne_fdim, clust_y, ptr,
 * edge_ptr of a batch are ten tensors of 1 KB - 1 MB, i.e. ten ~4 us copy launches in front of a 0.8 ms step otherwise.
 * dst / src / nbytes are HOST arrays [n]; ranges must not overlap.  16-byte lanes where both ends are aligned. */
#define IGCN_COPY_MULTI_MAX 16
int igcn_copy_multi(int n, void* const* dst, const void* const* src, const int64_t* nbytes, void* stream);

/* Dense image of a sparse map (the SNP <-> GO maps of kernel/go_model.py:208-215,281-282 as dense products, small
 * batches): image[c * image_stride + pos[k]] = val[c * val_stride + k] for c < channels, k < nnz (pos int64 [nnz]: row *
 * n_cols + col of every non-zero; the other entries of `image` are not touched), and the way back for the value
 * gradients: out [channels, nnz], out[c][k] = image[c * image_stride + pos[k]]. */
int igcn_image_put(int channels, int64_t nnz, const int64_t* pos, const float* val, int64_t val_stride, float* image,
                   int64_t image_stride, void* stream);
int igcn_image_take(int channels, int64_t nnz, const int64_t* pos, const float* image, int64_t image_stride, float* out,
                    void* stream);

/* Block-diagonal collation (Batch.from_data_list, batch.py:24-123) of B graphs drawn from a dataset of UNIFORM graphs held
 * as stacked device tensors, every key in ONE launch: idx int64 [B] (device) = the subjects; per key c < n (HOST arrays):
 * kind[c] == 0: dst_c [B, row] = src_c [idx[b], row] with row_bytes[c] bytes per graph (a multiple of 4);
 * kind[c] == 1: an `*index*` key — src_c [S, 2, E] int64, dst_c [2, B E] = concatenation along the last dim with graph b's
 * entries offset by b * nodes_per_graph (batch.py:98-104); row_bytes[c] = 2 * E * 8.  An idx[b] outside [0, n_subjects)
 * is not read: its rows are zeros, its index entries -1 (a consumer's plan build reports those in its status word). */
int igcn_gather_batch(int n, int B, int64_t nodes_per_graph, int64_t n_subjects, const int64_t* idx, void* const* dst,
                      const void* const* src, const int64_t* row_bytes, const int* kind, void* stream);

/* Measurement aid (bench.py roofline): the launch of igcn_gcn_propagate_fwd for (n_nodes, F) — thread =
 * (target, feature quad), or one wave per target when `dense` — with the body removed: mode 0 = empty kernel,
 * mode 1 = only the 16-byte store of each output row.  What the dispatch of that grid costs when no byte is read. */
int igcn_launch_floor(int64_t n_nodes, int F, int dense, int mode, float* out, void* stream);

/* Graph read-out of the `graph_pool=True` branch (kernel/sgcn_img_snp.py:230-235,246-252): PyG 2.0.2
 * global_mean_pool | global_max_pool | global_add_pool over the nodes of each graph, concatenated.  Uniform graphs of
 * `nodes_per_graph` nodes (the model's contract): x [n_graphs*nodes_per_graph, D] -> out [n_graphs, 3*D].
 * argmax [n_graphs, D] int32 (node index inside the graph, first maximum) is saved for the backward:
 * dx[g*R+r, d] = dout[g,d]/R + dout[g,2D+d] + (r == argmax[g,d]) * dout[g,D+d]. */
int igcn_graph_pool_fwd(int64_t n_graphs, int nodes_per_graph, int D, const float* x, float* out, int32_t* argmax,
                        void* stream);
int igcn_graph_pool_bwd(int64_t n_graphs, int nodes_per_graph, int D, const float* dout, const int32_t* argmax,
                        float* dx, void* stream);

/* Backward glue of out = act(A W^T + bias) (ops.Linear; lin1 / lin2 / GCNConv.lin of kernel/sgcn_img_snp.py:34-84):
 * g = dy * [y > 0] when `y` (the ReLU output) is given — then `g` receives the masked gradient the two GEMMs of
 * the backward read — and db[c] = sum_r g[r,c] (y == NULL: g unused, db = column sums of dy).  dy, y, g [rows, cols]
 * row-major, cols <= 256.  scratch: igcn_bias_grad_scratch_floats(rows, cols) floats. */
size_t igcn_bias_grad_scratch_floats(int64_t rows, int cols);
int igcn_bias_grad(int64_t rows, int cols, const float* dy, const float* y, float* g, float* db, float* scratch,
                   void* stream);
/* out[0:cols] = column sums of x [rows, cols]; out[cols : cols + zero_cols] = 0 (a gradient block known to vanish,
 * written by the launch that sums its neighbour: the key bias of nn.MultiheadAttention, kernel/sgcn_img_snp.py:240 —
 * a softmax over keys cannot see a key bias).  scratch: igcn_bias_grad_scratch_floats(rows, cols + zero_cols). */
int igcn_col_sums(int64_t rows, int cols, int zero_cols, const float* x, float* out, float* scratch, void* stream);
/* Two igcn_bias_grad / igcn_col_sums problems of the same [rows, cols] shape in one launch: per problem dy, optional
 * ReLU reference y (then g = dy * [y > 0] is written), db [cols + zero_cols] with zero_cols structurally zero
 * entries behind the sums, scratch of igcn_bias_grad_scratch_floats(rows, cols + zero_cols) floats. */
int igcn_bias_grad_pair(int64_t rows, int cols, const float* dy0, const float* y0, float* g0, float* db0,
                        int zero_cols0, float* scratch0, const float* dy1, const float* y1, float* g1, float* db1,
                        int zero_cols1, float* scratch1, void* stream);

/* `act`: 0 = none, 1 = ReLU; bit 0x100 = the output is a final parameter gradient (deferred reductions, below).
 * The split the library's launch heuristic prefers for (M, N, K): callers size `scratch` with it and pass it as
 * `split_k` (any other value >= 1 is honoured too). */
int igcn_gemm_f32_split_k(int64_t M, int64_t N, int64_t K);
int igcn_gemm_f32(int64_t M, int64_t N, int64_t K,
                  const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbn, int64_t sbk,
                  const float* bias, float* C, int64_t ldc, int act, int split_k, float* scratch,
                  void* stream);

/* The same product with bf16 operands (BASELINE configs[4]: "bf16 feature transforms on CDNA4 MFMA"): A and B are
 * rounded to bf16 (round-to-nearest-even) while they are staged into LDS, multiplied on v_mfma_f32_16x16x32_bf16,
 * accumulated and written in fp32.  Tensors stay fp32 in memory: same arguments, launch shapes and split-K
 * convention as igcn_gemm_f32, so a model flag swaps the two (GCNConv.lin, the attention projections, lin1 /
 * lin1_regr of kernel/sgcn_img_snp.py:34-84,239-241).  Exact w.r.t. an fp64 product of the bf16-rounded operands up
 * to fp32 accumulation order. */
int igcn_gemm_bf16(int64_t M, int64_t N, int64_t K,
                   const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbn, int64_t sbk,
                   const float* bias, float* C, int64_t ldc, int act, int split_k, float* scratch,
                   void* stream);
/* act | 0x200 (igcn_gemm_f32 / igcn_gemm_bf16; no bias, no activation, ldc == N): LEAVE the split-K slabs un-summed in
 * `scratch` ([igcn_gemm_effective_split(K, split_k)][M, N], slab order = K order) for a consumer that sums them while it
 * loads them (igcn_bn1d_fwd_slabs); with an effective split of 1 the product is written to C as usual. */
int igcn_gemm_effective_split(int64_t K, int split_k);
/* The launch plan of igcn_gemm_f32 (bf16 == 0) / igcn_gemm_bf16 (bf16 != 0) for these arguments: the function those
 * entry points run to choose their kernel instantiation, as a query.  Host only (no GPU needed): A and B are never
 * dereferenced, only their low address bits are read.  `act` with its 0x100 / 0x200 bits as passed to the product.
 * out [8] (host) = { bn, vw, pf, arf, brf, split_eff, kps, sum_form }:
 *   bn         tile width (16, 32, 64)                 vw   floats per operand load (4, 2, 1)
 *   pf         K tiles in flight ahead of LDS (1, 2; 0 for bf16: that kernel has no such parameter)
 *   arf, brf   A / B is read with its row axis as the contiguous one
 *   split_eff  K slices that run (= igcn_gemm_effective_split)       kps   K elements per slice
 *   sum_form   what follows the product launch: 0 nothing (split_eff == 1), 1 the column walk over the slabs (with bias /
 *              activation; members of a grouped launch share one such launch), 2 the block-per-output tree, 3 the
 *              final row sum of a parameter gradient (deferred inside igcn_reduce_defer), 4 nothing: the slabs are left
 *              to the caller (act | 0x200). */
int igcn_gemm_plan(int bf16, int64_t M, int64_t N, int64_t K, const float* A, int64_t sam, int64_t sak,
                   const float* B, int64_t sbn, int64_t sbk, int64_t ldc, int has_bias, int act, int split_k,
                   int64_t* out);

/* Batched-sum variant: C = sum_z A_z . B_z^T with A_z = A + z*a_batch, B_z = B + z*b_batch (element offsets),
 * every z covering the whole K; slabs are summed in z order.  Used for weight gradients whose reduction index is
 * (sample, node) over channel-major activations.  Long K is additionally sliced (<= 16 ways).
 * scratch: float[16*batch*M*N]. */
int igcn_gemm_f32_batched_sum(int64_t M, int64_t N, int64_t K, int batch,
                              const float* A, int64_t sam, int64_t sak, int64_t a_batch,
                              const float* B, int64_t sbn, int64_t sbk, int64_t b_batch,
                              float* C, int64_t ldc, float* scratch, void* stream);
/* `batch` independent products of one shape in one launch: C_z [M,N] = A_z B_z^T with A_z = A + z*a_batch,
 * B_z = B + z*b_batch, C_z = C + z*c_batch (element offsets).  split_k > 1 (see igcn_gemm_f32_split_k) needs
 * scratch of batch*split_k*M*N floats; the slabs of every product are summed by one more launch. */
int igcn_gemm_f32_batched(int64_t M, int64_t N, int64_t K, int batch, const float* A, int64_t sam, int64_t sak,
                          int64_t a_batch, const float* B, int64_t sbn, int64_t sbk, int64_t b_batch, float* C,
                          int64_t c_batch, int64_t ldc, int split_k, float* scratch, void* stream);
/* n (1..4) products of DIFFERENT shapes in one launch (the dX and dW products of a linear layer's backward): table
 * [n][16] int64 = {M, N, K, A, sam, sak, B, sbn, sbk, bias, C, ldc, act, split_k, scratch, bf16} per problem, each
 * field as the igcn_gemm_f32 argument of that name (pointers as integers); bf16 != 0 in the first problem: operands
 * rounded to bf16 as in igcn_gemm_bf16.  Same products as n igcn_gemm_f32 / igcn_gemm_bf16 calls; where K is split, the
 * slabs of a member are added in slab order (one launch for all members that need a plain sum) — the single-product entry
 * points choose their slab sum by shape (a tree for few outputs x many slabs, igcn_gemm_f32_batched likewise), so a split
 * product agrees with them to fp32 rounding, not bit for bit.  Within one entry point results are reproducible run to run. */
int igcn_gemm_f32_grouped(int n, const int64_t* table, void* stream);
/* The launch igcn_gemm_f32_grouped makes of `table` on its own (waiting riders are not looked at; host only, nothing
 * behind the table's pointers is read): out [4] (host) = { bn, vw, pf, grouped } — the instantiation common to the
 * members (pf 0 for bf16) and grouped = 1, or grouped = 0 when the members run as ordinary launches one after the other
 * (n == 1, or a member that only allows scalar loads).  Fails where igcn_gemm_f32_grouped refuses the table. */
int igcn_gemm_group_plan(int n, const int64_t* table, int64_t* out);
/* Products QUEUED for `stream` (same table format; at most 4 waiting) and carried by the next igcn_gemm_f32_grouped on it
 * — if they fit beside its own products (4 in all) and share its operand type — as further members of that launch,
 * slab sums included.  For products that are ready together but issued by different parts of the host code (the heads'
 * first layers in the model's forward, the Gram matrices in the loss function).  igcn_gemm_rider_flush launches what
 * nobody carried.  Operands and outputs must stay alive until the carrying launch. */
int igcn_gemm_rider(void* stream, int n, const int64_t* table);
int igcn_gemm_rider_flush(void* stream);
/* Forget every rider still waiting on the stream (mask job, products) WITHOUT launching it — at the start of a step that
 * may follow one which failed between queueing a rider and its carrier (the buffers it points at may be gone). */
int igcn_rider_cancel(void* stream);
/* HOST-SIDE QUEUES OF THE LIBRARY — the complete list, with the ordering contract of each.  All are keyed by the stream
 * handle, hold raw device pointers that the CALLER keeps alive, never launch anything by themselves, and are empty at the
 * end of every step (igcn_stream_pending == 0; ig-gcn_amd/train.py asserts it under IGCN_DEBUG_SYNC=1):
 *   1. deferred reductions   igcn_reduce_defer(stream, 1) .. igcn_reduce_flush[_tick](stream): every "sum the block
 *      partials" launch issued on the stream in between (and igcn_reduce_rows_final, igcn_loss_final) is queued; the flush
 *      runs them in issue order in one launch.  The
 *      partial buffers must outlive the flush; igcn_reduce_defer(stream, 0) + flush also runs on the error path.
 *   2. the dropout rider     igcn_rider_dropout(stream, ...): at most ONE job; carried by the NEXT
 *      igcn_graph_plan_build_segmented[_rep], igcn_sgcn_front_fwd (which builds the plan itself) or igcn_dense_sgcn_fwd
 *      (complete graphs: no plan build; its first edge pass carries the job) on the stream and by nothing else;
 *      igcn_rider_flush launches it alone.
 *   3. product riders        igcn_gemm_rider(stream, ...): at most 4 products; carried, all or none, by the NEXT
 *      igcn_gemm_f32_grouped on the stream with room for them and the same operand type; igcn_gemm_rider_flush launches
 *      them alone.
 * A rider is only ever picked up by the entry point named above: any other launch on the stream passes it by, so the
 * caller issues rider -> (independent launches) -> carrier or flush and must not read the rider's outputs before that.
 * igcn_rider_cancel forgets 2 and 3 without launching (start of a step that may follow a failed one).
 * igcn_stream_pending(stream) = entries of 1 + jobs of 2 + products of 3 still waiting on that stream.
 * Implementation: ig-gcn_amd/csrc/pending.h — one record per stream for all three, one map, one lock. */
int igcn_stream_pending(void* stream);

/* ------------------------------------------------------------------------------------------------
 * GO read-outs: per-node linear + BatchNorm1d(#nodes) + ReLU, fused — go_model.py:117-121,254
 * (conc_for_attention, D = dim_snps_atten), :123-128,255 (conc + B, D = 1), :130-136,278 (conc_D + B_D, D = 1):
 *   pre[b,n,:] = W x[b,:,n]   (x [B,F,N] channel-major, W [D,F])
 *   out[b,n,:] = relu((pre - mean_n)*rstd_n*gamma[n] + beta[n])      out [B,N,D]
 * BatchNorm1d(N) on [B,N,D] normalises every node over (batch, feature); training != 0 uses batch statistics
 * (biased variance) and updates running_mean/var (momentum, unbiased variance), else the running ones.
 * `groups` > 1 splits the B samples into equal consecutive groups that are normalised independently and update
 * the running statistics one after the other (= that many successive module calls; used to run the plain and the
 * masked forward pass of a train step as one launch).
 * scratch: igcn_node_linear_bn_scratch_floats(B,N).
 */
size_t igcn_node_linear_bn_scratch_floats(int B, int N, int groups);
/* Host only: 1 for the (F, D) the read-out kernels are built for, else 0 — F = 5 with D in {1,2,3,4,5,6,8,10,12,16,20,24,
 * 30,32,48} or a multiple of 16 from 64 to 160 (row-coalesced kernels from D = 16), and (F, D) = (2, 1).  Exactly what
 * igcn_node_linear_bn_{fwd,bwd} accept; any other shape is refused there with IGCN_ERR_UNSUPPORTED. */
int igcn_node_linear_bn_supported(int F, int D);
int igcn_node_linear_bn_fwd(int B, int F, int N, int D, int groups, const float* x, const float* W,
                            const float* gamma, const float* beta, float* running_mean, float* running_var,
                            int training, float momentum, float eps,
                            const float* keep /*[B,N] dropout factors of the output, D == 1 only; NULL = none*/,
                            float* out, float* save_mean /*[groups,N]*/, float* save_rstd /*[groups,N]*/,
                            float* scratch, void* stream);
/* The D == 1 read-out in front of the gene decoding (go_model.py:278-282) with its map: igcn_node_linear_bn_fwd (out
 * [B,N]) followed by igcn_spmm_fwd_strided(B, 1, J, N, nnz, row_ptr, col, val, val_stride, out, y) with the apply pass
 * and the map forward as ONE launch — the workgroup of a sample computes its row of `out` into LDS (and stores it: both
 * backward passes read it) and walks the J lists there.  Same expressions and sums as the two calls: out, y [B,1,J],
 * the saved and the running statistics are theirs bit for bit.  igcn_node_linear_bn_apply_map_ok: covered (F = 2, D = 1,
 * the row fits 64 KB of LDS, the map's rows are long lists; 0 under option bit 8, IGCN_NO_MAP_FUSED) — anything else:
 * IGCN_ERR_UNSUPPORTED.  Backward: igcn_node_linear_bn_bwd and igcn_spmm_bwd as for the two calls. */
int igcn_node_linear_bn_apply_map_ok(int F, int D, int N, int J, int64_t nnz);
int igcn_node_linear_bn_apply_map_fwd(int B, int F, int N, int groups, const float* x, const float* W,
                                      const float* gamma, const float* beta, float* running_mean, float* running_var,
                                      int training, float momentum, float eps, const float* keep, float* out,
                                      float* save_mean, float* save_rstd, float* scratch, int J, int64_t nnz,
                                      const int32_t* row_ptr, const int32_t* col, const float* val, int64_t val_stride,
                                      float* y, void* stream);
/* Outputs dx [B,F,N], dW [D,F], dgb [2,N] = (dgamma, dbeta).  dW = sum_{b,n} dpre[b,n,:] (x) x[b,:,n] is formed in
 * registers when D*F <= 16 or the rows are 16-byte quads handled by the row-coalesced kernels (D = 16, 32, 64..160: one
 * [D,F] partial per workgroup, summed in order), else on the MFMA batched-sum GEMM.
 * scratch: igcn_node_linear_bn_bwd_scratch_floats(B,F,N,D,groups). */
size_t igcn_node_linear_bn_bwd_scratch_floats(int B, int F, int N, int D, int groups);
int igcn_node_linear_bn_bwd(int B, int F, int N, int D, int groups, int training, const float* x, const float* W,
                            const float* gamma, const float* beta, const float* save_mean, const float* save_rstd,
                            const float* dout, const float* keep, float* dx, float* dW, float* dgb, float* scratch,
                            void* stream);
/* Two read-outs of the SAME input x [B,F,N] in paired launches (go_model.py:254-255: conc_for_attention, D1 outputs per
 * node, and conc, D2 = 1 with fused dropout keep2): three launches forward and three backward for both, their grids
 * sharing the chip.  Per side the arguments of igcn_node_linear_bn_{fwd,bwd} (scratch sizes as there).
 * igcn_node_linear_bn_pair_supported(F, D1, D2) != 0 for the shapes the paired kernels cover (F = 5, D1 = 32, D2 = 1). */
int igcn_node_linear_bn_pair_supported(int F, int D1, int D2);
int igcn_node_linear_bn_pair_fwd(int B, int F, int N, int groups, const float* x, int training,
                                 int D1, const float* W1, const float* gamma1, const float* beta1,
                                 float* running_mean1, float* running_var1, float momentum1, float eps1, float* out1,
                                 float* save_mean1, float* save_rstd1, float* scratch1,
                                 int D2, const float* W2, const float* gamma2, const float* beta2,
                                 float* running_mean2, float* running_var2, float momentum2, float eps2,
                                 const float* keep2, float* out2, float* save_mean2, float* save_rstd2, float* scratch2,
                                 void* stream);
int igcn_node_linear_bn_pair_bwd(int B, int F, int N, int groups, int training, const float* x,
                                 int D1, const float* W1, const float* gamma1, const float* beta1,
                                 const float* save_mean1, const float* save_rstd1, const float* dout1, float* dx1,
                                 float* dW1, float* dgb1, float* scratch1,
                                 int D2, const float* W2, const float* gamma2, const float* beta2,
                                 const float* save_mean2, const float* save_rstd2, const float* dout2,
                                 const float* keep2, float* dx2, float* dW2, float* dgb2, float* scratch2, void* stream);

/* BatchNorm1d(C) (+ReLU when relu != 0) on a 2-D input [B,C] with the same grouped-statistics semantics —
 * the latent MLP of go_model.py:138-146.  save_mean/save_rstd are [groups,C]. */
int igcn_bn1d_fwd(int B, int C, int groups, const float* x, const float* gamma, const float* beta,
                  float* running_mean, float* running_var, int training, float momentum, float eps, int relu,
                  const float* keep /*[B,C] dropout factors of the output or NULL*/,
                  float* y, float* save_mean, float* save_rstd, void* stream);
int igcn_bn1d_bwd(int B, int C, int groups, int training, int relu, const float* x, const float* gamma,
                  const float* beta, const float* save_mean, const float* save_rstd, const float* dy,
                  const float* keep, float* dx, float* dgamma, float* dbeta, void* stream);
/* The same forward on a column whose split-K slabs the product in front left un-summed (igcn_gemm_f32 with act | 0x200):
 * the latent MLP's wide layer, kernel/go_model.py:138-146 (Linear -> BatchNorm1d -> ReLU -> Dropout).  `slabs`
 * [n_slabs][B, C] are summed in slab order while the column is loaded; x_out [B, C] receives the sum (igcn_bn1d_bwd's
 * operand).  groups <= 2 and B / groups <= 1024 (igcn_bn1d_fwd_supported). */
int igcn_bn1d_fwd_supported(int B, int groups);
int igcn_bn1d_fwd_slabs(int B, int C, int groups, const float* slabs, int n_slabs, float* x_out, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, int training, float momentum,
                        float eps, int relu, const float* keep, float* y, float* save_mean, float* save_rstd,
                        void* stream);
/* The gene read-out (igcn_node_linear_bn_apply_map_fwd / igcn_node_linear_bn_bwd with F = 2, D = 1: the leading
 * arguments are theirs) whose launches carry the latent MLP's BatchNorm1d stages (kernel/go_model.py:278-285): the
 * first C workgroups of a carrying launch run a stage's channels, the others the read-out pass — the same kernel
 * bodies as the separate launches, so every output is theirs bit for bit; the products between the stages are launched
 * by the same call.  A stage whose carrier does not launch (forward without training: no statistics pass) gets the
 * launch it has in igcn_bn1d_*.  igcn_gene_tail_supported: igcn_node_linear_bn_apply_map_ok for the read-out and
 * igcn_bn1d_fwd_supported for stages of Bl samples.
 * `table` (host): records of 40 int64 words.
 *   BatchNorm stage {kind, B, C, groups, relu, n_slabs, momentum, eps, x, gamma, beta, keep, dy, running_mean,
 *     running_var, y, mean, rstd, x_out, dgamma, dbeta}: kind 1 = igcn_bn1d_fwd, 2 = igcn_bn1d_fwd_slabs (x = slabs),
 *     3 = igcn_bn1d_bwd (mean / rstd = the saved ones, y = dx); momentum and eps as the bit pattern of a double.
 *   product stage {form, ...}: 1 = igcn_gemm_f32 of the igcn_gemm_f32_grouped record behind it, 2 = {n <= 2, n such
 *     records} as one igcn_gemm_f32_grouped, 3 = igcn_small_linear_fwd {R, K, C, x, keep, W, b, y},
 *     4 = igcn_small_linear_bwd {R, K, C, x, keep, W, dy, dx, dwb, scratch}.
 * forward  table = {BatchNorm 1, product 2, BatchNorm 2}: statistics + BatchNorm 1 | finalize | product 2 |
 *          apply-and-map + BatchNorm 2 (product 1 is the caller's, launched before).
 * backward table = {BatchNorm 2, products 2, BatchNorm 1, products 1}: statistics + BatchNorm 2 | products 2 | chunk
 *          sum | apply + BatchNorm 1 | products 1 | the read-out's parameter-gradient sums (deferred as usual). */
int igcn_gene_tail_supported(int F, int D, int N, int J, int64_t nnz, int Bl, int groups);
int igcn_gene_tail_fwd(int B, int F, int N, int groups, const float* x, const float* W, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, int training, float momentum,
                       float eps, const float* keep, float* out, float* save_mean, float* save_rstd, float* scratch,
                       int J, int64_t nnz, const int32_t* row_ptr, const int32_t* col, const float* val,
                       int64_t val_stride, float* y, const int64_t* table, void* stream);
int igcn_gene_tail_bwd(int B, int F, int N, int groups, int training, const float* x, const float* W,
                       const float* gamma, const float* beta, const float* save_mean, const float* save_rstd,
                       const float* dout, const float* keep, float* dx, float* dW, float* dgb, float* scratch,
                       const int64_t* table, void* stream);

/* Dropout factors of every site of a forward pass in ONE launch (the reference draws them site by site: nn.Dropout /
 * nn.Dropout2d / F.dropout, kernel/go_model.py:104,113,128,136,143, kernel/sgcn_img_snp.py:289,299).  out [total]:
 * element i of segment k (segments given by their END offsets, HOST arrays, <= igcn_dropout_max_segments()) is 0 with probability seg_p[k],
 * else 1/(1-seg_p[k]); consumed as `keep` by igcn_nodes_ln_*, igcn_node_linear_bn_*, igcn_bn1d_*, igcn_small_linear_*.
 * Counter-based integer-hash generator; `state` = device uint64[igcn_dropout_state_words()], word 0 = the stream
 * counter (seed), every other word 0 (arrival counts, left at 0 by every launch): the last workgroup of a launch
 * advances the counter, so every replay of a captured launch draws fresh masks. */
int igcn_dropout_max_segments(void);   /* sites one igcn_dropout_masks launch takes; callers split longer lists */
int igcn_dropout_state_words(void);
int igcn_dropout_masks(int64_t total, int n_segments, const int64_t* seg_end, const float* seg_p, void* state,
                       float* out, int n_counters, int64_t* const* counters, int64_t counter_inc, void* stream);
/* The same job as a RIDER: not launched, but queued for `stream` (at most one per stream) and carried by the next
 * igcn_graph_plan_build_segmented[_rep] on that stream — extra workgroups of the plan build's grid draw the masks (both
 * launches depend on nothing a train step computes; as two roles of one grid they overlap).  igcn_rider_flush launches a
 * job nobody carried as a launch of its own (nothing waiting: nothing happens). */
int igcn_rider_dropout(void* stream, int64_t total, int n_segments, const int64_t* seg_end, const float* seg_p, void* state,
                       float* out, int n_counters, int64_t* const* counters, int64_t counter_inc);
int igcn_rider_flush(void* stream);
/* counters (HOST array of <= 8 device int64 pointers, or n_counters = 0): each is bumped by counter_inc by the launch —
 * BatchNorm's num_batches_tracked (kernel/go_model.py:119-146), which advance exactly when the masks are drawn.
 *
 * out[i] = sum_k parts[k][i], k < n <= 4 (HOST array of device pointers, 16-byte aligned): the gradient of a tensor
 * with several consumers in one launch instead of autograd's pairwise adds (ops.GradFan). */
int igcn_sum_n(int64_t numel, int n, const float* const* parts, float* out, void* stream);
/* The same sum for a LEAF's gradient (nothing reads it before the optimiser): while igcn_reduce_defer is on it joins the
 * deferred final reductions and is performed by igcn_reduce_flush's single launch — parts must stay alive until then;
 * otherwise it is igcn_sum_n.  Same summation order either way. */
int igcn_sum_n_final(int64_t numel, int n, const float* const* parts, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mask regulariser — loss_probability, kernel/sgcn_img_snp.py:153-181:
 *   loss = mean r_x(sigmoid(prob)) + mean r_e(e) + mean r_x(sigmoid(snps_prob)),
 *   r(p) = l1*|p| - ent*(p log(p+eps) + (1-p) log(1-p+eps))
 * prob [n_prob] and snps [n_snps] are logits, e [n_edge] the edge mask of igcn_edge_mask_fwd.
 * scratch: float[1024].  gout: device scalar d(loss_total)/d(loss).
 */
/* loss == NULL: no final sum — the igcn_mask_reg_blocks(n_prob + n_edge + n_snps) block partials stay in scratch for
 * the consumer to add up (igcn_loss_head_fwd, prob_rows). */
int igcn_mask_reg_blocks(int64_t n_total);
int igcn_mask_reg_fwd(int64_t n_prob, int64_t n_edge, int64_t n_snps, const float* prob, const float* e,
                      const float* snps, float l1_x, float ent_x, float l1_e, float ent_e, float eps,
                      float* loss, float* scratch, void* stream);
int igcn_mask_reg_bwd(int64_t n_prob, int64_t n_edge, int64_t n_snps, const float* prob, const float* e,
                      const float* snps, float l1_x, float ent_x, float l1_e, float ent_e, float eps,
                      const float* gout, float* dprob, float* de, float* dsnps, void* stream);
/* The same with weights l1_s, ent_s of its own for the snps group (the cluster-label model's loss_probability,
 * kernel/sgcn_img_snp_clusterlabel.py:114-144, whose L1 terms of prob and snps_prob are normalised differently: l1_x =
 * lamda_x_l1 H_0, l1_s = lamda_x_l1 54 against the means taken here).  Same loss == NULL mode, block count and scratch;
 * with l1_s = l1_x, ent_s = ent_x the same bits as igcn_mask_reg_{fwd,bwd}. */
int igcn_mask_reg3_fwd(int64_t n_prob, int64_t n_edge, int64_t n_snps, const float* prob, const float* e,
                       const float* snps, float l1_x, float ent_x, float l1_e, float ent_e, float l1_s, float ent_s,
                       float eps, float* loss, float* scratch, void* stream);
int igcn_mask_reg3_bwd(int64_t n_prob, int64_t n_edge, int64_t n_snps, const float* prob, const float* e,
                       const float* snps, float l1_x, float ent_x, float l1_e, float ent_e, float l1_s, float ent_s,
                       float eps, const float* gout, float* dprob, float* de, float* dsnps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batch-level losses from ONE Gram matrix G = s s^T [B,B] of the fused features s [B, R*D]:
 *   out[0] = consist_loss (kernel/sgcn_img_snp.py:183-196) = sum_ij Lap_ij G_ij / B^2
 *   out[1] = OrthogonalConstraint (:198-205) = (sum_ij G_ij^2/(G_ii G_jj) - 2B + RD)/B^2
 * igcn_rbf_laplacian builds Lap = diag(W1) - W, W = exp(-gamma*||t_i-t_j||^2) (util/image_cluster.py:15-31;
 * t == NULL: W = 1).  The backward writes S = dG + dG^T [B,B] (ds = S s); gout [2] is a device array.
 * `groups` Gram matrices that share the Laplacian (the passes of a batched sweep: G [groups,B,B], out / gout
 * [groups,2], S [groups,B,B]) take one launch.  scratch (fwd): float[2 B groups].
 */
int igcn_rbf_laplacian(int B, int T, float gamma, const float* t, float* Lap, void* stream);
/* out == NULL: no final sum — the row partials [B][groups*2] stay in scratch (igcn_loss_head_fwd, gram_rows). */
int igcn_gram_loss_fwd(int B, int RD, int groups, const float* G, const float* Lap, float* out, float* scratch,
                       void* stream);
int igcn_gram_loss_bwd(int B, int groups, const float* G, const float* Lap, const float* gout, float* S,
                       void* stream);
/* igcn_gram_loss_fwd with the RBF Laplacian of consist_loss (util/image_cluster.py:15-31; tsne [B, T], or NULL: W = 1)
 * evaluated inside the row walk instead of read: lap_out [B, B] is an OUTPUT (igcn_gram_loss_bwd reads it) — no
 * igcn_rbf_laplacian launch in the train step. */
int igcn_gram_loss_fwd_rbf(int B, int RD, int groups, const float* G, const float* tsne, int T, float gamma, float* lap_out,
                           float* out, float* scratch, void* stream);
/* ... that also writes S [groups, B, B] = the output of igcn_gram_loss_bwd for the upstream gradient gout [groups, 2]
 * given here as a HOST array (groups <= 4), bit for bit: a train step knows its d loss / d (consist, orth) — the loss
 * weights — when it launches the forward, and then has no Gram-loss backward launch. */
int igcn_gram_loss_fwd_rbf_unit(int B, int RD, int groups, const float* G, const float* tsne, int T, float gamma,
                                float* lap_out, float* out, float* scratch, const float* gout, float* S, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cross-attention core of nn.MultiheadAttention (kernel/sgcn_img_snp.py:240) on the projection outputs in place:
 *   q [B,Lq,D] (query projection), kv [B,Lk,2,D] (key|value projection as ONE GEMM output), D = H*head_dim
 *   o [B,Lq,D] = per head softmax(q k^T / sqrt(head_dim)) v, heads concatenated; lse [B,H,Lq] saved for the backward
 * One workgroup per (sample, head); no head transposes or contiguous copies on either side.  The backward returns
 * dq [B,Lq,D] and dkv [B,Lk,2,D] in the layouts the projection-gradient GEMMs read.
 * head_dim <= 96 runs on the matrix cores (exact-fp32 MFMA, any Lq; head columns zero-padded in LDS to a multiple of 4
 * up to 32 and to 48 / 64 / 80 / 96 above); when K, V — and Q, dO in the backward — of one head fit LDS one workgroup
 * per (sample, head) keeps them resident, otherwise the other side of the attention is streamed through LDS in chunks
 * (512 queries x 1300 keys of the 512-ROI configuration; every head wider than 32 at the model's 90 x 400).
 * igcn_attn_core_lds_bytes: dynamic LDS needed (96 KB = the streamed form), 0 = shape not covered (head_dim > 96).
 */
size_t igcn_attn_core_lds_bytes(int D, int H, int Lq, int Lk, int backward);
size_t igcn_attn_core_bwd_scratch_floats(int B, int H, int Lq);
int igcn_attn_core_fwd(int B, int D, int H, int Lq, int Lk, const float* q, const float* kv, float* o, float* lse,
                       void* stream);
int igcn_attn_core_bwd(int B, int D, int H, int Lq, int Lk, const float* q, const float* kv, const float* o,
                       const float* lse, const float* dout, float* dq, float* dkv,
                       float* scratch /* igcn_attn_core_bwd_scratch_floats(): rowsum(o*do) of the chunked path */,
                       void* stream);
/* The same core with bf16 OPERANDS on v_mfma_f32_16x16x32_bf16 (BASELINE configs[4] "bf16 feature transforms on
 * CDNA4 MFMA"): q k^T, p v and the three gradient products take operands rounded to bf16 and accumulate in fp32; the
 * softmax, lse and delta stay fp32, and every tensor stays fp32 in HBM (same layouts and signatures as above; scratch
 * is always needed).  head_dim must be 16 (igcn_attn_core_bf16_supported); any Lq, Lk (both sides streamed through
 * LDS in chunks).  Tolerance vs the fp32 core: ~4e-3 relative on o, ~1e-2 on the gradients (tests/test_gpu_ops.py). */
int igcn_attn_core_bf16_supported(int D, int H, int Lq, int Lk);
int igcn_attn_core_bf16_fwd(int B, int D, int H, int Lq, int Lk, const float* q, const float* kv, float* o, float* lse,
                            void* stream);
int igcn_attn_core_bf16_bwd(int B, int D, int H, int Lq, int Lk, const float* q, const float* kv, const float* o,
                            const float* lse, const float* dout, float* dq, float* dkv, float* scratch, void* stream);

/* The attention core on SPLIT bf16 operands (csrc/attn_split.hip; head_dim 16): every fp32 operand is carried as a bf16
 * head and a bf16 remainder (x = hi + lo to 2^-17 |x|) and every product runs on v_mfma_f32_16x16x32_bf16 — fp32-grade
 * results (the 1e-4 / 1e-3 bounds of igcn_attn_core_fwd / _bwd hold, tests/test_gpu_ops.py) at the bf16 rate of the
 * matrix cores.  Arguments as igcn_attn_core_fwd / igcn_attn_core_bwd. */
int igcn_attn_core_split_supported(int D, int H, int Lq, int Lk);
int igcn_attn_core_split_fwd(int B, int D, int H, int Lq, int Lk, const float* q, const float* kv, float* o, float* lse,
                             void* stream);
/* (backward: one workgroup per (sample, head), <= 128 queries and >= 128 keys — igcn_attn_core_split_bwd_supported) */
int igcn_attn_core_split_bwd_supported(int D, int H, int Lq, int Lk);
int igcn_attn_core_split_bwd(int B, int D, int H, int Lq, int Lk, const float* q, const float* kv, const float* o,
                             const float* lse, const float* dout, float* dq, float* dkv, float* scratch, void* stream);

/* The attention WEIGHTS nn.MultiheadAttention returns next to its output (kernel/sgcn_img_snp.py:240,
 * ``attn_output, attn_output_weights = self.multihead_attn(...)``): the head-averaged softmax
 *   w[b,i,j] = (1/H) sum_h softmax_j(q_h[b,i] . k_h[b,j] / sqrt(head_dim))        w [B,Lq,Lk]
 * on the projection outputs in place (q [B,Lq,D], kv [B,Lk,2,D]: only the key half is read).  Exact fp32 operands on
 * v_mfma_f32_16x16x4_f32; the kernel takes its own row maximum and row sum (it does not read the forward's lse), keeps
 * the head average inside the lane that stores the element — one writer per element, no atomics, bit-reproducible —
 * and streams the keys through LDS in chunks when all heads' keys do not fit (igcn_attn_weights_chunk_rows: keys per
 * chunk, 0 = resident).  Covered: head_dim <= 96 with 16 keys of all H heads in the kernel's 72 KB of LDS (D up to
 * ~1000), any Lq, any Lk; anything else: IGCN_ERR_UNSUPPORTED. */
int igcn_attn_weights_supported(int D, int H, int Lq, int Lk);
int igcn_attn_weights_chunk_rows(int D, int H, int Lq, int Lk);
int igcn_attn_weights(int B, int D, int H, int Lq, int Lk, const float* q, const float* kv, float* w, void* stream);
/* Per-class sums of a batch of such maps (kernel/sgcn_img_snp.py:240; the ROI x GO-term table of a cohort):
 * sums[y[b]] += w[b] in sample order with fp64 accumulators (one thread per map element, no atomics), counts[y[b]] += 1;
 * labels outside [0, C) are skipped and counted in state[0].  sums [C,Lq,Lk] double, counts [C] and state [1] int64. */
int igcn_attn_map_accumulate(int B, int Lq, int Lk, int C, const float* w, const int64_t* y, double* sums,
                             int64_t* counts, int64_t* state, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sparse SNP<->GO maps with learnable non-zeros — gene encoding go_model.py:208-215 (C=2 channels,
 * rows = GO nodes, cols = SNPs) and gene decoding :281-282 (C=1, rows = SNPs, cols = GO nodes):
 *   y[b,c,i] = sum_{k in row i} val[c,k] * x[b, col[k]]          x [B,J], y [B,C,I], val [C,nnz]
 * Backward needs the transposed structure: t_ptr [J+1], t_row [nnz] (row of each entry in column order),
 * t_k [nnz] (its position in the row-major value array).
 * The structure is shared by all samples and small: the kernels read it once per workgroup and reuse it across a tile
 * of samples whose operand rows sit in LDS (short lists: thread per output row; ~150-entry lists: workgroup per sample
 * with its vector in LDS, wave per output; value gradients: a few samples' vectors in LDS, thread per non-zero).
 * dval is a parameter gradient: its final sum over the workgroups' partial rows takes part in the deferred
 * reductions (igcn_reduce_defer).  scratch: igcn_spmm_bwd_scratch_floats(...) floats.
 */
int igcn_spmm_fwd(int B, int C, int I, int J, int64_t nnz, const int32_t* row_ptr, const int32_t* col,
                  const float* val, const float* x, float* y, void* stream);
size_t igcn_spmm_bwd_scratch_floats(int B, int C, int I, int J, int64_t nnz);
int igcn_spmm_bwd(int B, int C, int I, int J, int64_t nnz, const int32_t* row_ptr, const int32_t* col,
                  const int32_t* row_of /*[nnz]*/, const int32_t* t_ptr, const int32_t* t_row, const int32_t* t_k,
                  const float* val, const float* x, const float* dy,
                  float* dx /*[B,J] or NULL*/, float* dval /*[C,nnz] or NULL*/,
                  float* scratch /* needed when dval != NULL */, void* stream);
/* The value rows of the C channels at a constant stride instead of one [C, nnz] tensor: val + c * val_stride (floats,
 * >= nnz) — the per-channel parameter vectors of go_model.py:67 as the optimiser lays them out in its flat buffer, so
 * that no concatenation runs in front of every step.  dval stays one contiguous [C, nnz] output. */
int igcn_spmm_fwd_strided(int B, int C, int I, int J, int64_t nnz, const int32_t* row_ptr, const int32_t* col,
                          const float* val, int64_t val_stride, const float* x, float* y, void* stream);
int igcn_spmm_bwd_strided(int B, int C, int I, int J, int64_t nnz, const int32_t* row_ptr, const int32_t* col,
                          const int32_t* row_of, const int32_t* t_ptr, const int32_t* t_row, const int32_t* t_k,
                          const float* val, int64_t val_stride, const float* x, const float* dy, float* dx, float* dval,
                          float* scratch, void* stream);
/* The value-gradient half of igcn_spmm_bwd for one or two maps in ONE launch (call igcn_spmm_bwd with dval = NULL for
 * the input gradients): table [n][12] int64 = {B, C, I, J, nnz, col, row_of, x, dy, dval, scratch, 0} per map. */
int igcn_spmm_bwd_dval_multi(int n, const int64_t* table, void* stream);
/* Which kernel the map entry points above launch for these sizes: the function they run to choose it, as a query.  Host
 * only (no GPU needed, nothing is launched or dereferenced).  pass: IGCN_SPMM_PASS_FWD (y), IGCN_SPMM_PASS_DX (the dx half
 * of igcn_spmm_bwd), IGCN_SPMM_PASS_DVAL (its dval half, and each map of igcn_spmm_bwd_dval_multi).
 * out [4] (host) = { route, tile, lds_bytes, workgroups }:
 *   route  FWD / DX: IGCN_SPMM_LONG_LDS (lists of more than 8 entries on average, the operand vector of a sample — J
 *          floats, C * I for dx — within 150 KB of LDS), IGCN_SPMM_ROWS_TILED (shorter lists, operand rows of at most
 *          1024 floats), IGCN_SPMM_WAVE / IGCN_SPMM_THREAD (the untiled kernels for what fits neither: long / short lists)
 *          DVAL: IGCN_SPMM_DVAL_LDS (`tile` samples' vectors in LDS per workgroup) or IGCN_SPMM_DVAL_GLOBAL (tile 0:
 *          one sample does not fit 120 KB, or the long side is x and C > 1)
 *   tile   DVAL: samples per workgroup (4, 3, 2, 1; 0 = global); FWD / DX: samples per workgroup of the tiled kernel (8),
 *          else 1
 *   lds_bytes   dynamic LDS of the launch (above 64 KB the kernel's limit is raised first)
 *   workgroups  of the launch (DVAL global: of its first kernel)
 * IGCN_SPMM_NO_LDS (igcn_configure) is honoured: the untiled kernels everywhere. */
enum { IGCN_SPMM_PASS_FWD = 0, IGCN_SPMM_PASS_DX = 1, IGCN_SPMM_PASS_DVAL = 2 };
enum { IGCN_SPMM_LONG_LDS = 0, IGCN_SPMM_ROWS_TILED = 1, IGCN_SPMM_WAVE = 2, IGCN_SPMM_THREAD = 3,
       IGCN_SPMM_DVAL_LDS = 4, IGCN_SPMM_DVAL_GLOBAL = 5 };
int igcn_spmm_route(int pass, int B, int C, int I, int J, int64_t nnz, int64_t* out);

/* ------------------------------------------------------------------------------------------------
 * GO attention-GCN encoder layer, all samples at once — replaces the dense transforms, the edge gathers
 * and the PER-SAMPLE python loop of go_model.py:226-244 (helper :182-186, attention_adj :173-180, gcn :170):
 *   x_in = W_inc x, x_s = W_s x                              (per node, fin -> fout)
 *   s_e  = exp(tanh(a_in[:fout].x_in[row_e] + a_in[fout:].x_in[col_e]))
 *   y[b,:,r] = sum_{e in row r} (s_e / sum_{e' in row r} s_e') x_in[col_e] + x_s[r] * sigmoid(a_s.x_s[r])
 * x [B,fin,N] and y [B,fout,N] channel-major.  Supported (fin,fout): (2,5) (5,5).
 */
int igcn_go_attn_fwd(int B, int N, int fin, int fout, const int32_t* row_ptr, const int32_t* col,
                     const float* x, const float* w_inc, const float* w_s, const float* a_in, const float* a_s,
                     float* y, void* stream);
/* The attention coefficients of that layer as an OUTPUT (go_model.py:226-244: attention_adj :173-180 forms them per
 * sample and the layer consumes them; igcn_go_attn_fwd keeps them in registers):
 *   alpha[b,e] = s_e / sum_{e' in row(e)} s_e'   [B,nnz], CSR order, nnz = row_ptr[N]
 *   beta[b,r]  = sigmoid(a_s.x_s[r])             [B,N]
 * by the forward's own device functions, thread -> node map and order of operations (the row sum in list order, the
 * quotient as s_e * rcp(sum)); rows longer than 64 entries are walked by a whole wave (their row sum is a fixed-tree
 * wave sum).  One writer per element, no atomics, bit-reproducible.  Same (fin,fout) as igcn_go_attn_fwd, any N. */
int igcn_go_attn_coeffs(int B, int N, int fin, int fout, const int32_t* row_ptr, const int32_t* col,
                        const float* x, const float* w_inc, const float* w_s, const float* a_in, const float* a_s,
                        float* alpha, float* beta, void* stream);
/* One step of the attention roll-out through the pooled hierarchy (go_model.py:219-251: the layer mixes a node with its
 * list and its self loop, :246-251 keeps nodes >= pool), on relevance kept channel-major like the activations:
 *   r_out[b,s,r-pool] = (sum_{e in row r} alpha[b,e] r_in[b,s,col_e] + beta[b,r] r_in[b,s,r])
 *                       / (sum_{e in row r} alpha[b,e] + beta[b,r])            for pool <= r < N
 * and r_out[b,s,r-pool] = r_in[b,s,r] for a row without a list.  r_in [B,S,N] with r_in_batch_stride elements between
 * samples (0: one [S,N] table shared by all samples — the encoding relevance of go_model.py:208-215), r_out
 * [B,S,N-pool].  A workgroup keeps igcn_go_rollout_chunk(N) relevance columns of one sample in LDS (8, 4, 2 or 1:
 * the most that fit 80 KB; 0 = N above 20 480 nodes, IGCN_ERR_UNSUPPORTED).  One writer per element, no atomics. */
int igcn_go_rollout_chunk(int N);
int igcn_go_rollout_layer(int B, int N, int S, int pool, const int32_t* row_ptr, const int32_t* col,
                          const float* alpha, const float* beta, const float* r_in, int64_t r_in_batch_stride,
                          float* r_out, void* stream);
/* Backward in O(nnz*f) (the reference's autograd forms a dense N x N product per sample and layer).
 * t_ptr/t_row: the transposed structure (for each column the rows that read it).
 * Outputs: dx [B,fin,N]; dparams float[ 2*fout*fin + 2*fout + fout ] = (dW_inc, dW_s, da_in, da_s).
 * Samples whose operands fit a CU's LDS ((fin+fout+4)*N*4 <= 160 KB, N <= 4096) run in an LDS-resident kernel, one
 * workgroup per sample; larger ones in global-memory kernels (hub columns walked by the whole wave).
 * scratch floats: igcn_go_attn_bwd_scratch_floats(B,N,fin,fout).  dparams is a FINAL reduction of block partials kept
 * in scratch: while igcn_reduce_defer is on it is performed by igcn_reduce_flush (scratch must stay alive until then). */
size_t igcn_go_attn_bwd_scratch_floats(int B, int N, int fin, int fout);
/* `walk_order` (device int32[igcn_go_attn_walk_slots(N, fin, fout)], or NULL = node order): the thread -> node map of
 * the LDS-resident kernel's column walks, from igcn_go_attn_walk_order(N, fin, fout, t_ptr on the HOST, order out on
 * the HOST) — structure-only, computed once per hierarchy and layer shape: nodes sorted by their number of readers and
 * dealt to the waves so that lanes walk lists of equal length and waves carry equal totals.  Results do not depend on
 * it.  igcn_go_attn_bwd_threads: the workgroup size the LDS-resident kernel runs with for that shape (512 when two
 * workgroups then fit a CU, else 1024) — the slot count is its multiple. */
int igcn_go_attn_bwd_threads(int N, int fin, int fout);
int igcn_go_attn_walk_slots(int N, int fin, int fout);
int igcn_go_attn_walk_order(int N, int fin, int fout, const int32_t* t_ptr_host, int32_t* order_host);
int igcn_go_attn_bwd(int B, int N, int fin, int fout, const int32_t* row_ptr, const int32_t* col,
                     const int32_t* t_ptr, const int32_t* t_row, const int32_t* walk_order,
                     const float* x, const float* w_inc, const float* w_s, const float* a_in, const float* a_s,
                     const float* dy, float* dx, float* dparams, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over the NODE axis + ReLU + node dropout + hierarchical pooling — go_model.py:246-251
 * (encoder) and :273-275 (decoder): for every (sample, channel) row of y [B,f,N]
 *   z = relu( (y-mean)/sqrt(var+eps) * gamma[n] + beta[n] ) * keep[b,n]      (keep may be NULL)
 * and only nodes n >= pool are written: z [B,f,N-pool].  Saves mean, rstd [B*f].
 */
int igcn_nodes_ln_fwd(int B, int f, int N, int pool, float eps, const float* y, const float* gamma,
                      const float* beta, const float* keep, float* z, float* mean, float* rstd, void* stream);
/* Outputs dy [B,f,N], dgb [2,N] (dgamma row then dbeta row).
 * scratch: igcn_nodes_ln_bwd_scratch_floats(B,f,N) floats. */
size_t igcn_nodes_ln_bwd_scratch_floats(int B, int f, int N);
int igcn_nodes_ln_bwd(int B, int f, int N, int pool, const float* y, const float* gamma, const float* beta,
                      const float* keep, const float* mean, const float* rstd, const float* dz,
                      float* dy, float* dgb, float* scratch, void* stream);
/* The same backward in two calls: the input gradient now, the affine gradients (d gamma | d beta: parameter gradients,
 * read by nobody before the optimiser) of up to four layers later, in ONE launch.  table [n][13] int64 =
 * {B, f, N, pool, y, gamma, beta, keep, mean, rstd, dz, scratch, dgb} per layer (pointers as integers). */
int igcn_nodes_ln_bwd_dy(int B, int f, int N, int pool, const float* y, const float* gamma, const float* beta,
                         const float* keep, const float* mean, const float* rstd, const float* dz, float* dy,
                         void* stream);
int igcn_nodes_ln_bwd_affine_multi(int n, const int64_t* table, void* stream);

/* A GO layer's backward WITH the backward of the LayerNorm block behind it (go_model.py:219-251 encoder,
 * :262-275 decoder: y = layer(x); z = dropout(relu(LN(y)))[.., pool:]).  The layer's LDS-resident backward holds one
 * sample per workgroup, so it forms d loss / d y from (y, dz, gamma, beta, keep, mean, rstd) while copying it in — the
 * LayerNorm's own dX launch and the d y tensor disappear — and leaves d gamma | d beta summed over the sample's channels
 * in part [B][2][N], reduced over samples by the (deferred) final reduction into dgb [2, N].  igcn_go_*_ln_fused_ok:
 * 1 when the sizes qualify (LDS-resident layer, N and pool multiples of 4, N / 4 <= workgroup size); otherwise use
 * igcn_nodes_ln_bwd* followed by igcn_go_attn_bwd / igcn_go_decode_bwd.  Every tensor 16-byte aligned.  dx, dparams and
 * scratch as the plain entry points; part: igcn_go_ln_part_floats(B, N) floats, alive until the reductions ran.
 * igcn_go_attn_ln_bwd's dz2 / dz3: when z feeds several consumers (the encoder output: two read-outs and the decoder) their
 * gradients are added while they are loaded, in that order — the sum igcn_sum_n would have written. */
int igcn_go_attn_ln_fused_ok(int N, int fin, int fout, int pool);
int igcn_go_decode_ln_fused_ok(int Nin, int Nout, int fin, int fout);
size_t igcn_go_ln_part_floats(int B, int N);
int igcn_go_attn_ln_bwd(int B, int N, int fin, int fout, const int32_t* row_ptr, const int32_t* col,
                        const int32_t* t_ptr, const int32_t* t_row, const int32_t* walk_order,
                        const float* x, const float* w_inc, const float* w_s, const float* a_in, const float* a_s,
                        int pool, const float* y, const float* gamma, const float* beta, const float* keep,
                        const float* mean, const float* rstd, const float* dz, const float* dz2 /*or NULL*/,
                        const float* dz3 /*or NULL*/, float* dx, float* dparams, float* dgb, float* scratch, float* part,
                        void* stream);
int igcn_go_decode_ln_bwd(int B, int Nin, int Nout, int fin, int fout, const int32_t* row_ptr,
                          const int32_t* t_ptr, const int32_t* t_row, const float* x, const float* w_out,
                          const float* w_sout, const float* y, const float* gamma, const float* beta,
                          const float* keep, const float* mean, const float* rstd, const float* dz, float* dx,
                          float* dparams, float* dgb, float* scratch, float* part, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GO decoder layer (mean aggregation down the hierarchy) — go_model.py:262-272, batch_mul :197-201:
 *   y[b,:,r] = (1/deg_r) sum_{e in row r} W_out x[b,:,col_e]  +  (r >= off ? W_sout x[b,:,r-off] : 0)
 * x [B,fin,Nin], y [B,fout,Nout], off = Nout-Nin.  Supported (fin,fout): (5,5) (5,2).
 */
int igcn_go_decode_fwd(int B, int Nin, int Nout, int fin, int fout, const int32_t* row_ptr, const int32_t* col,
                       const float* x, const float* w_out, const float* w_sout, float* y, void* stream);
/* Outputs dx [B,fin,Nin], dparams float[2*fout*fin] = (dW_out, dW_sout). */
size_t igcn_go_decode_bwd_scratch_floats(int B, int Nin, int fin, int fout);
int igcn_go_decode_bwd(int B, int Nin, int Nout, int fin, int fout, const int32_t* row_ptr,
                       const int32_t* t_ptr, const int32_t* t_row,
                       const float* x, const float* w_out, const float* w_sout, const float* dy,
                       float* dx, float* dparams, float* scratch, void* stream);
/* Which kernel the GO layer entry points launch for these sizes: the functions they run to choose it, as a query.  Host
 * only.  op: IGCN_GO_OP_ATTN_BWD (igcn_go_attn_bwd / igcn_go_attn_ln_bwd; Nin = Nout = N), IGCN_GO_OP_DECODE_FWD,
 * IGCN_GO_OP_DECODE_BWD (igcn_go_decode_bwd; with_ln != 0: igcn_go_decode_ln_bwd, whose LayerNorm rides along).
 * out [4] (host) = { route, threads, passes, lds_bytes }:
 *   route    IGCN_GO_ROUTE_LDS (one workgroup holds a sample in LDS) or IGCN_GO_ROUTE_GLOBAL (thread per node; for
 *            DECODE_BWD also whenever B < 128 and no LayerNorm rides along: that many samples do not fill the chip)
 *   threads  workgroup size (ATTN_BWD, DECODE_BWD: 512 or 1024 when LDS; DECODE_FWD: 1024 when LDS; 256 when global)
 *   passes   ATTN_BWD, LDS: passes of the workgroup over the nodes = the MAXIT instance (1..4); DECODE_FWD, LDS:
 *            workgroups per sample (3072 rows each); else 0
 *   lds_bytes  dynamic LDS of the LDS-resident launch (0 when global)
 * igcn_go_decode_fwd takes the LDS kernel only when x is 16-byte aligned as well: the probe sees no pointer and assumes
 * it is.  IGCN_GO_ATTN_CM (igcn_configure) is honoured: global everywhere. */
enum { IGCN_GO_OP_ATTN_BWD = 0, IGCN_GO_OP_DECODE_FWD = 1, IGCN_GO_OP_DECODE_BWD = 2 };
enum { IGCN_GO_ROUTE_LDS = 0, IGCN_GO_ROUTE_GLOBAL = 1 };
int igcn_go_route(int op, int B, int Nin, int Nout, int fin, int fout, int with_ln, int64_t* out);

/* ------------------------------------------------------------------------------------------------
 * Adam step over a flat fp32 parameter buffer — torch.optim.Adam(lr, weight_decay=0) at
 * kernel/train_eval_sgcn_img_snps.py:108,547.  `step` is a device int32 that the kernel's caller
 * increments (igcn_adam_step does it: one extra 1-thread kernel) so the call is graph-capturable.
 * `lr` is a DEVICE float[1] read by the kernel at run time: the reference's schedule
 * (`param_group['lr'] = lr_decay_factor * param_group['lr']`, kernel/train_eval_sgcn_img_snps.py:169-171) writes that
 * scalar, and a launch captured into a hipGraph sees the new rate at its next replay.
 * The update, with t = *step after the increment and g = grad * grad_scale (scaled BEFORE it is squared):
 *   m = beta1 m + (1 - beta1) g ;  v = beta2 v + (1 - beta2) g^2
 *   param -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * — eps is added AFTER the second moment's bias correction (torch.optim.Adam's placement), not to sqrt(v).  beta1, beta2,
 * eps and grad_scale are taken as given in float: 1 - beta2 is 1 - float(0.999), which moves exp_avg_sq by 1.3e-5 relative
 * and the update by at most 2e-5 of its scale from torch's double-valued betas (tests/test_adam_reference.py).  All forms
 * below compute this one expression in fp32 (tests/test_gpu_adam.py holds each to the fp64 evaluation of it).
 */
int igcn_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                   int32_t* step, const float* lr, float beta1, float beta2, float eps, float grad_scale,
                   void* stream);

/* Multi-tensor forms: `table` is a device array int64[n_tensors][4] = {param, grad, exp_avg, exp_avg_sq}
 * pointers, `numel` int64[n_tensors].  A zero grad pointer skips the tensor (torch's Adam skips parameters whose
 * .grad is None).  igcn_pack_grads copies the gradients (zeros where missing) to flat[offset[t]...] — the bucket of
 * the data-parallel all-reduce. */
int igcn_adam_step_multi(int n_tensors, const int64_t* table, const int64_t* numel, int32_t* step,
                         const float* lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
/* ..._ticked: `step` has been advanced already — by igcn_reduce_flush_tick, the launch that ends the backward — so
 * no one-thread counter launch goes in front. */
int igcn_adam_step_ticked(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t* step,
                          const float* lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
int igcn_adam_step_multi_ticked(int n_tensors, const int64_t* table, const int64_t* numel, int32_t* step,
                                const float* lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
/* igcn_adam_step_multi over a precomputed block list (the shapes of a model do not change between steps): block b covers
 * elements [blk_off[b], blk_off[b] + igcn_adam_chunk()) of tensor blk_tensor[b] — one workgroup per block instead of a
 * (96, n_tensors) grid whose workgroups mostly find nothing to do.  ticked != 0: `step` has been advanced already. */
int igcn_adam_chunk(void);
int igcn_adam_step_blocks(int n_blocks, const int64_t* table, const int64_t* numel, const int32_t* blk_tensor,
                          const int32_t* blk_off, int32_t* step, const float* lr, float beta1, float beta2, float eps,
                          float grad_scale, int ticked, void* stream);
int igcn_pack_grads(int n_tensors, const int64_t* table, const int64_t* numel, const int64_t* offset,
                    float* flat, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Deferred reductions of a backward pass.  About thirty kernels of the train step's backward end in a small "sum the
 * block partials" launch whose output is a parameter gradient that nothing reads before the optimiser (bias and
 * LayerNorm / BatchNorm affine gradients, split-K weight-gradient slabs, ...).  After igcn_reduce_defer(stream, 1)
 * those launches ON THAT STREAM are QUEUED instead (one queue per stream: trainers on different streams do not see each
 * other's partials; the partial buffers — the `scratch` arguments of the calls — must then stay alive until the
 * flush), and igcn_reduce_flush(stream) performs the stream's queued reductions in ONE launch, with the arithmetic
 * and summation order of the stand-alone kernels.  igcn_gemm_f32 / igcn_gemm_bf16 take part when bit 0x100 of `act`
 * marks their output as such a gradient.  Host-side state only: capturable like any other launch.
 * igcn_reduce_pending: queued entries over all streams. */
int igcn_reduce_defer(void* stream, int on);
int igcn_reduce_pending(void);
int igcn_reduce_flush(void* stream);
/* the flush + `*step_counter += 1` (device int32: the optimiser's step) by the same launch (a one-thread launch of its
 * own when nothing is queued) */
int igcn_reduce_flush_tick(void* stream, int32_t* step_counter);
/* out[j] = sum_r partial[r * ld + j] (j < n) as such a final reduction: queued while the stream defers, a launch of its own
 * otherwise — for the partial rows a kernel left behind for a parameter gradient (igcn_head_loss_fwd's wpart). */
int igcn_reduce_rows_final(const float* partial, int64_t rows, int64_t ld, int n, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient exchange of the data-parallel step (the reference has no multi-GPU code): one RCCL
 * communicator per process (one process per GPU), ONE all-reduce(sum) of the flat fp32 gradient bucket that
 * igcn_pack_grads fills, in place, enqueued on `stream` — i.e. on the launch stream between the pack kernel and
 * igcn_adam_step(grad_scale = 1/world_size), capturable into the step's hipGraph.  RCCL is resolved at run time
 * (the librccl already loaded in the process — PyTorch-ROCm's — else dlopen): IGCN_ERR_UNSUPPORTED when absent.
 *   rank 0: igcn_comm_get_unique_id(buf[igcn_comm_unique_id_bytes()]) -> host-side broadcast of the bytes (any
 *   channel: torch.distributed store, MPI, a file) -> every rank: igcn_comm_init(W, rank, bytes, &comm) with its
 *   GPU current.  These three calls are host-blocking set-up, not stream work; igcn_comm_allreduce never blocks. */
int igcn_comm_unique_id_bytes(void);
int igcn_comm_get_unique_id(void* out_bytes);
int igcn_comm_init(int world_size, int rank, const void* unique_id, void** comm_out);
int igcn_comm_allreduce(void* comm, float* buf, int64_t n, void* stream);
int igcn_comm_destroy(void* comm);

/* ------------------------------------------------------------------------------------------------
 * Loss head of train() — kernel/train_eval_sgcn_img_snps.py:525-543 — on the STACKED outputs of the batched sweep
 * (rows [0,B) = plain pass :521, rows [B,2B) = isExplain pass :523):
 *   terms[7] = {lam0*nll(logp[:B],y), lam0*nll(logp[B:],y), lam1*(mse_1+mse_2)/2, lam2*prob,
 *               lam3*(sse_1+sse_2)/2 (snps reconstruction), lam4*(consist_1+consist_2)/2, lam5*orth_1}
 *   loss = hp_ce*terms[0] + hp_mi*terms[1] + terms[2] + ... + terms[6]
 * logp [2B,C] log-probabilities, y int64 [B], reg [2B,NR], clin [B*NR], x_hat [2B,S], snps [B,S],
 * gram [2][2] = igcn_gram_loss_fwd outputs of the two passes, prob [1] = igcn_mask_reg_fwd output.
 * lam6 is a HOST array (read at call time).  Backward: gout [1] device scalar; dgram [4], dprob [1].
 * from_logits != 0: `logp` holds the raw class scores [2B,C]; F.log_softmax (kernel/sgcn_img_snp.py:305) is taken
 * inside and written to logp_out [2B,C]; the backward, given that logp, returns the gradient of the raw scores.
 * gram_rows / prob_rows > 1: gram [gram_rows][4] / prob [prob_rows] are the un-reduced partials of
 * igcn_gram_loss_fwd (out == NULL) / igcn_mask_reg_fwd (loss == NULL); their rows are summed here (the gradient of
 * every row is dgram / dprob).
 */
int igcn_loss_head_fwd(int B, int C, int NR, int S, const float* logp, int from_logits, float* logp_out,
                       const int64_t* y, const float* reg, const float* clin, const float* x_hat, const float* snps,
                       const float* gram, int gram_rows, const float* prob, int prob_rows, const float* lam6,
                       float hp_ce, float hp_mi, float* loss, float* terms, void* stream);
int igcn_loss_head_bwd(int B, int C, int NR, int S, const int64_t* y, const float* reg, const float* clin,
                       const float* x_hat, const float* snps, const float* logp, const float* lam6, float hp_ce,
                       float hp_mi, const float* gout, float* dlogp, float* dreg, float* dxhat, float* dgram,
                       float* dprob, void* stream);

/* THE OUTPUT HEADS AND THE LOSS HEAD OF A TRAIN STEP AS ONE LAUNCH (kernel/sgcn_img_snp.py:289-290,300-301,305 lin2 /
 * lin2_regr / log_softmax on the stacked sweep; train() :525-530 the cross-entropy, regression and reconstruction terms)
 * together with their BACKWARD for an upstream gradient of one: x1 / x2 [2B, K] = the heads' hidden features (keep1 / keep2
 * [2B, K]: dropout factors of those inputs, or NULL), W1 [C, K] + b1 = lin2, W2 [NR, K] + b2 = lin2_regr, y [B] int64, clin
 * [B, NR], x_hat [2B, S], snps [B, S]; K / 4 a power of two <= 64, C, NR <= 4 (igcn_head_loss_supported).  Outputs: logp_out
 * [2B, C] = log_softmax of the scores, reg_out [2B, NR]; dx1 / dx2 [2B, K] = d loss / d (x1, x2), dxhat [2B, S]; wpart
 * [blocks, C K + C + NR K + NR] = per-workgroup partial rows of (dW1 | db1 | dW2 | db2) for igcn_reduce_rows_final; dgram [4],
 * dprob [1] = d loss / d (Gram terms, regulariser); parts [blocks, 4] = partial sums of the four row-wise loss terms
 * (blocks = igcn_head_loss_blocks(B, K)).  Same arithmetic as igcn_small_linear_pair_fwd -> igcn_loss_head_fwd_grads ->
 * igcn_small_linear_pair_bwd.
 * igcn_loss_final: the loss VALUE from the partial sums of this launch, of igcn_gram_loss_fwd (gram [gram_rows, 4]) and of the
 * mask regulariser (prob [prob_rows]); wts [10] DEVICE floats = {lam[0..5], hp_ce, hp_mi, B, NR}; out [8] = loss, terms[7].
 * Nothing of the backward depends on it: while the stream defers its reductions (igcn_reduce_defer) it joins the flush as
 * one more workgroup, otherwise it is a launch of its own. */
int igcn_head_loss_supported(int K, int C, int NR);
int igcn_head_loss_blocks(int B, int K);
int igcn_head_loss_fwd(int B, int K, int C, int NR, int S, const float* x1, const float* keep1, const float* W1,
                       const float* b1, const float* x2, const float* keep2, const float* W2, const float* b2,
                       const int64_t* y, const float* clin, const float* x_hat, const float* snps,
                       const float* lam6 /*HOST [6]*/, float hp_ce, float hp_mi, float* logp_out, float* reg_out, float* dx1,
                       float* dx2, float* dxhat, float* parts, float* wpart, float* dgram, float* dprob, void* stream);
/* igcn_head_loss_fwd and igcn_gram_loss_fwd_rbf_unit(out = NULL: the row partials stay in gscratch [Bg, 2 groups]) as two
 * roles of ONE launch: the two read disjoint outputs of the launches in front of them and write disjoint buffers. */
int igcn_head_loss_gram_fwd(int B, int K, int C, int NR, int S, const float* x1, const float* keep1, const float* W1,
                            const float* b1, const float* x2, const float* keep2, const float* W2, const float* b2,
                            const int64_t* y, const float* clin, const float* x_hat, const float* snps,
                            const float* lam6 /*HOST [6]*/, float hp_ce, float hp_mi, float* logp_out, float* reg_out,
                            float* dx1, float* dx2, float* dxhat, float* parts, float* wpart, float* dgram, float* dprob,
                            int Bg, int RD, int groups, const float* G, const float* tsne, int T, float gamma,
                            float* lap_out, float* gscratch, const float* gout /*HOST [2 groups]*/, float* Ssym,
                            void* stream);
int igcn_loss_final(const float* parts, int nparts, const float* gram, int gram_rows, const float* prob, int prob_rows,
                    const float* wts, float* out, void* stream);
/* THE TWO CLASSIFICATION HEADS AND THE LOSS OF THE CLUSTER-LABEL TRAINER AS ONE LAUNCH (kernel/sgcn_img_snp_clusterlabel.py
 * :217-228 lin2_classify / lin2_cluster / both log_softmaxes on the stacked sweep; train() of
 * kernel/train_eval_sgcn_clusterlabel.py:376-393) with their BACKWARD for an upstream gradient of one — the sibling of
 * igcn_head_loss_fwd.  x1 / x2 [2B, K] = the heads' hidden features, pass-major (keep1 / keep2 [2B, K]: dropout factors, or
 * NULL), W1 [C1, K] + b1 = lin2_classify, W2 [C2, K] + b2 = lin2_cluster, y / clust_y [B] int64, x_hat [2B, S], snps [B, S];
 * K / 4 a power of two <= 64, C1, C2 <= 4 (igcn_cluster_head_loss_supported).
 *   loss = hp_ce (ce + ce_cluster)/2 + hp_mi (mi + mi_cluster)/2 + prob + lambda0 (sse_plain + sse_masked)/2
 *   predict_cluster == 0:  loss = hp_ce ce + hp_mi mi + prob + recon; logp2 is still written, dx2 and the W2 | b2 part of
 *   wpart are exact zeros.
 * Outputs: logp1 [2B, C1], logp2 [2B, C2]; dx1 / dx2 [2B, K], dxhat [2B, S]; parts [blocks, 5] = partial sums of (ce,
 * ce_cluster, mi, mi_cluster, sse); wpart [blocks, C1 K + C1 + C2 K + C2] = per-workgroup partial rows of (dW1 | db1 | dW2 |
 * db2) for igcn_reduce_rows_final; dprob [1]  (blocks = igcn_cluster_head_loss_blocks(B, K)).  No atomics, fixed-order sums.
 * A label outside its classes poisons its term with NaN (as igcn_head_loss_fwd).
 * igcn_cluster_loss_final: the loss VALUE from parts [nparts, 5] and the regulariser (prob [prob_rows], possibly the
 * un-reduced partials of igcn_mask_reg3_fwd); wts [5] DEVICE floats = {hp_ce, hp_mi, lambda0, B, predict_cluster}; out [8] =
 * loss, ce, ce_cluster, mi, mi_cluster, prob, recon, 0.  Joins the deferred flush exactly as igcn_loss_final does. */
int igcn_cluster_head_loss_supported(int K, int C1, int C2);
int igcn_cluster_head_loss_blocks(int B, int K);
int igcn_cluster_head_loss_fwd(int B, int K, int C1, int C2, int S, const float* x1, const float* keep1, const float* W1,
                               const float* b1, const float* x2, const float* keep2, const float* W2, const float* b2,
                               const int64_t* y, const int64_t* clust_y, const float* x_hat, const float* snps, float hp_ce,
                               float hp_mi, float lambda0, int predict_cluster, float* logp1, float* logp2, float* dx1,
                               float* dx2, float* dxhat, float* parts, float* wpart, float* dprob, void* stream);
int igcn_cluster_loss_final(const float* parts, int nparts, const float* prob, int prob_rows, const float* wts, float* out,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * The genetics-only trainer's head and loss (csrc/snps_head.hip; kernel/train_eval_snps.py:314-320 on the
 * ``classification`` module of kernel/go_model.py:148-157), one launch per direction:
 *   x = cat(latent [B, L], snps [B, S]) (two pointers, never materialised; K1 = L + S), a = relu(BatchNorm1d(K1)(x)) keep1,
 *   h = relu(a W1^T) keep2 (W1 [H, K1], no bias), y_hat = sigmoid(h W2^T + b2) (W2 [1, H]),
 *   class = sum BCELoss(y_hat, label), recon = lambda0 sum (x_hat - snps)^2, out [3] = {class + recon, class, recon}.
 * BCELoss is torch's on the probability: -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)), gradient
 * (p - y) / max(p (1 - p), 1e-12) p (1 - p); label [B] floats in [0, 1].  lambda0 == 0: recon and dx_hat are exact zeros.
 * keep1 [B, K1] / keep2 [B, H]: {0, 1/(1-p)} factors of igcn_dropout_masks or NULL; training mode only.
 * Training mode normalises with the batch statistics (biased variance, from centred values) and updates running_mean /
 * running_var with momentum m: (1 - m) running + m batch, the variance unbiased (B / (B - 1)); eval mode normalises with
 * the running statistics.
 * Supported (igcn_snps_head_supported; IGCN_ERR_UNSUPPORTED otherwise, nothing written): H == 16, L, S >= 1, L + S <= 96,
 * 1 <= B <= 1024; training mode needs B >= 2.  Both directions are ONE workgroup that loops over passes of 64 rows (the
 * batch statistics, the loss sums and the parameter gradients couple the rows); every sum runs in a fixed order, no
 * atomics.  label == NULL (eval mode only): y_hat alone for any 1 <= B <= 2^24 on a grid over the rows; x_hat, out, ws may be
 * NULL.
 * ws: caller-owned, igcn_snps_head_workspace_bytes, 16-byte aligned (as keep2 and W2): the statistics the forward
 * normalised with and the hidden activations, read by the backward.
 * igcn_snps_head_loss_bwd: the backward for the upstream gradient upstream[0] (a DEVICE scalar; NULL: one), from the same
 * inputs plus the forward's y_hat and ws.  Writes dlatent [B, L] (the SNP columns are data: no gradient), dx_hat [B, S] =
 * 2 lambda0 (x_hat - snps) upstream, dgamma / dbeta [K1], dW1 [H, K1], dW2 [H], db2 [1]. */
int igcn_snps_head_supported(int B, int L, int S, int H);
size_t igcn_snps_head_workspace_bytes(int B, int L, int S, int H);
int igcn_snps_head_loss_fwd(int B, int L, int S, int H, const float* latent, const float* snps, const float* bn_weight,
                            const float* bn_bias, float* running_mean, float* running_var, float momentum, float eps,
                            int training, const float* keep1, const float* keep2, const float* W1, const float* W2,
                            const float* b2, const float* label, const float* x_hat, float lambda0, float* y_hat,
                            float* out, void* ws, void* stream);
int igcn_snps_head_loss_bwd(int B, int L, int S, int H, int training, const float* latent, const float* snps,
                            const float* bn_weight, const float* bn_bias, const float* keep1, const float* keep2,
                            const float* W1, const float* W2, const float* label, const float* y_hat, const float* x_hat,
                            float lambda0, const float* upstream, const void* ws, float* dlatent, float* dx_hat,
                            float* dgamma, float* dbeta, float* dW1, float* dW2, float* db2, void* stream);
/* igcn_loss_head_fwd that also writes the gradients igcn_loss_head_bwd would return for gout = 1 (each element's gradient
 * is known where its forward term is computed): a train step, whose d loss / d loss is one, then has no backward launch
 * for the loss head.  dlogp [2B,C] (of the raw scores when from_logits), dreg [2B,NR], dxhat [2B,S], dgram [4], dprob [1]. */
int igcn_loss_head_fwd_grads(int B, int C, int NR, int S, const float* logp, int from_logits, float* logp_out,
                             const int64_t* y, const float* reg, const float* clin, const float* x_hat, const float* snps,
                             const float* gram, int gram_rows, const float* prob, int prob_rows, const float* lam6,
                             float hp_ce, float hp_mi, float* loss, float* terms, float* dlogp, float* dreg, float* dxhat,
                             float* dgram, float* dprob, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Graph-diffusion pre-transform + block-diagonal collation of B dense adjacencies A [B,R,R] (f32), on the device —
 * replaces, per graph, preprocess_diffusion_imgs_snps (util_gdc.py:71-86: get_ppr_matrix :7-15 with `alpha`,
 * get_top_k_matrix :25-31 with `k`, scipy coo_matrix) and the index offsetting of Batch.from_data_list
 * (batch.py:98-104).  fp64 arithmetic in LDS, one workgroup per graph; R <= igcn_gdc_topk_max_rois().
 *   edge_index int64 [2, B*R*k], edge_attr f32 [B*R*k]: graph g owns slots [g*R*k, (g+1)*R*k), its edges in
 *   (row, col) order with both endpoints offset by g*R, then (-1,-1,0) padding if fewer than R*k entries are
 *   non-zero; counts int32 [B] = edges of each graph.
 */
int igcn_gdc_topk_max_rois(void);
int igcn_gdc_topk(int B, int R, int k, double alpha, const float* A, int64_t* edge_index, float* edge_attr,
                  int32_t* counts, void* stream);
/* The same for a batch DRAWN from a resident dataset A [S,R,R]: graph g of the batch is matrix subject[g] (int64 [B],
 * device) — a per-step producer needs no gathered copy of the B matrices.  A subject[g] outside [0, n_subjects) is
 * not read: graph g comes out empty (counts[g] = 0, all its slots padding).
 * Both are igcn_gdc_diffuse(IGCN_GDC_PPR, IGCN_GDC_TOPK) under their first names, kept for callers of this interface;
 * the package's Python launches through igcn_gdc_diffuse alone. */
int igcn_gdc_topk_of(int B, int R, int k, double alpha, const float* A, int64_t n_subjects, const int64_t* subject,
                     int64_t* edge_index, float* edge_attr, int32_t* counts, void* stream);
/* All of util_gdc.py: either diffusion kernel with either sparsifier.
 *   kernel    IGCN_GDC_PPR   get_ppr_matrix  :7-14,  param = alpha in (0,1]
 *             IGCN_GDC_HEAT  get_heat_matrix :16-23, param = t in (0,64] (a condition of the interface; GDC uses
 *                            1-10): S = expm(-t (I - D^-1/2 A D^-1/2)) in fp64, scaling and squaring with the scaling
 *                            exponent chosen per graph from |t H|_1 (csrc/gdc.hip)
 *   sparsify  IGCN_GDC_TOPK       get_top_k_matrix   :25-31 with `k` (eps unused)
 *             IGCN_GDC_THRESHOLD  get_clipped_matrix :33-38 with `eps` (k unused): entries S[i][j] >= eps stay, each
 *                                 column is divided by the sum of what it kept (a sum <= 0 leaves it unscaled); a kept
 *                                 exact zero is not an edge, a column that keeps nothing has no edges
 * A need not be symmetric.  subject == NULL: graph g is matrix g of A [B,R,R]; otherwise graph g is matrix subject[g]
 * of A [n_subjects,R,R], and an index outside [0, n_subjects) is not read and yields an empty graph.
 * Output as igcn_gdc_topk with cap slots per column, cap = k (top-k) or R (threshold): edge_index int64 [2, B*R*cap],
 * edge_attr f32 [B*R*cap]; graph g owns slots [g*R*cap, (g+1)*R*cap): its edges in (row, col) order, both endpoints
 * offset by g*R, then (-1,-1,0) padding; counts int32 [B].  Every slot has one writer, no atomics on global memory:
 * the result is bit-reproducible.  igcn_gdc_diffuse(PPR, TOPK) equals igcn_gdc_topk bit for bit.
 * R <= igcn_gdc_max_rois(kernel), else IGCN_ERR_UNSUPPORTED (PPR: igcn_gdc_topk_max_rois(); heat: two R x R fp64
 * matrices, R padded to a multiple of 16, in LDS).
 * A matrix with a zero row sum is outside the contract of both kernels (the reference divides by zero there, :12 and
 * :21): the values are then unspecified, the writes still stay inside the graph's slots. */
enum { IGCN_GDC_PPR = 0, IGCN_GDC_HEAT = 1 };
enum { IGCN_GDC_TOPK = 0, IGCN_GDC_THRESHOLD = 1 };
int igcn_gdc_max_rois(int kernel);
int igcn_gdc_diffuse(int B, int R, int kernel, double param, int sparsify, int k, double eps, const float* A,
                     int64_t n_subjects, const int64_t* subject /* NULL: graph g = matrix g */, int64_t* edge_index,
                     float* edge_attr, int32_t* counts, void* stream);
/* The same transform for graphs beyond the LDS limit (csrc/gdc_tiled.hip): all of util_gdc.py — get_ppr_matrix :7-14,
 * get_heat_matrix :16-23, get_top_k_matrix :25-31, get_clipped_matrix :33-38, coo_matrix :82-86 — with every graph's
 * fp64 system in a caller-supplied global-memory workspace and the products on the fp64 matrix cores.  Arguments,
 * output layout, padding, counts and the subject list as igcn_gdc_diffuse; any R in [1, igcn_gdc_tiled_max_rois()].
 *   PPR   P = alpha (I - G)^-1 as prod_{j<J} (I + G^(2^j)), G = (1 - alpha) H, J = ceil(log2(ln 2^-60 / ln(1 - alpha)))
 *         (10 at alpha = 0.05, 8 at 0.15): 2 (J - 1) products.  alpha in [0.001, 1]: the smallest alpha with J <= 16.
 *   heat  the scheme of igcn_gdc_diffuse (degree-14 Taylor polynomial, s squarings, s per graph from |t H|_1); t in
 *         (0,64].  13 + smax products, smax = ceil(log2(2 t sqrt(R))) >= s for every symmetric A (|H|_1 <= sqrt(R)); a
 *         graph whose own s is smaller passes through the remaining launches unchanged.  For an A that is not symmetric
 *         s is capped at smax: beyond |t H|_1 = t sqrt(R) the Taylor remainder grows with the excess.
 * The results differ from igcn_gdc_diffuse in the last bits of the weights (another summation order), not in the
 * contract.  The library allocates nothing: `workspace` (device, 16-byte aligned) holds at least
 * igcn_gdc_tiled_workspace_bytes(B, R, kernel) bytes — per graph four (PPR) or three (heat) Rp x Rp fp64 matrices,
 * Rp = R rounded up to 64, plus 32 Rp + 80 bytes; linear in B, 0 for sizes outside the interface.  Its contents need no
 * initialisation and mean nothing afterwards.  A workspace that is too small: IGCN_ERR_UNSUPPORTED, the message names
 * the bytes needed; R above the limit: IGCN_ERR_UNSUPPORTED ("max R = 512").  B <= 65535 per call.
 * A matrix with a zero row sum is outside the contract exactly as for igcn_gdc_diffuse: the values are then
 * unspecified, the writes still stay inside the graph's slots and the workspace.
 * No atomics, one writer per element, fixed summation order: two runs give the same bits, and so does a batch
 * processed in several calls of fewer graphs. */
int igcn_gdc_tiled_max_rois(void);
size_t igcn_gdc_tiled_workspace_bytes(int B, int R, int kernel);
int igcn_gdc_diffuse_tiled(int B, int R, int kernel, double param, int sparsify, int k, double eps, const float* A,
                           int64_t n_subjects, const int64_t* subject /* NULL: graph g = matrix g */,
                           int64_t* edge_index, float* edge_attr, int32_t* counts, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Epoch evaluation on the device (csrc/eval.hip): replaces the per-batch host work of eval_loss :564-600, eval_acc
 * :551-561 and eval_scores :602-671 (kernel/train_eval_sgcn_img_snps.py) and the sklearn / scipy metrics of :633-667.
 * igcn_eval_collect: the last launch of one evaluation batch.  Reads the plain-pass rows [0, B) of logp [*, C], reg
 * [*, NR], out_lin [*, F], lin_f [*, H] (the stacked [2B, *] outputs of the batched sweep, or [B, *]), y [B] int64,
 * clin [B, NR], sbj [B] int64 and the batch loss (device scalar).  At row cursor c = state[0] it writes rows [c, c + B)
 * of the epoch buffers (rows_logp [cap, C], rows_pred = argmax(logp) [cap] int64, rows_y, rows_reg / rows_clin [cap, NR],
 * rows_out_lin [cap, F], rows_lin_f [cap, H], rows_sbj [cap] int64), adds loss * B to loss_sum[0] (fp64) and the correct
 * count to state[2], then advances the cursor.  If state[1] (overflow) is set or c + B > capacity it writes nothing and
 * sets state[1] = 1.  state int64 [3] and loss_sum are zeroed by the caller before the first batch.
 * igcn_eval_metrics: one call after the last batch, over the first n rows (1 <= n <= 65536 = IGCN_EVAL_MAX_ROWS;
 * C <= 16).  parts: int64 workspace of 2 * ceil(n / 256).  out [8 + 3 NR + C C] fp64 = {rows written (state[0]), overflow (state[1]), loss =
 * loss_sum / n, accuracy = correct / n, auc, weighted f1, sensitivity, specificity, corr[NR], r2[NR], rmse[NR],
 * confusion[C][C] (true-major counts)}.  auc / sensitivity / specificity only for C = 2 (else 0): auc is the Mann-Whitney
 * statistic of logp[:, 1] (ties 1/2; NaN when a class is absent, 0 when a score is NaN, as the reference's except
 * makes sklearn's error); sensitivity / specificity NaN on a zero denominator.  Per target: predictions' NaN -> 0,
 * pearsonr (NaN for a constant input), r2_score with force_finite, RMSE.  Integer counts and fixed-order fp64 sums:
 * bitwise reproducible. */
#define IGCN_EVAL_MAX_ROWS 65536
int igcn_eval_collect(int B, int C, int NR, int F, int H, const float* loss, const float* logp, const float* reg,
                      const float* out_lin, const float* lin_f, const int64_t* y, const float* clin, const int64_t* sbj,
                      int64_t capacity, int64_t* state, double* loss_sum, float* rows_logp, int64_t* rows_pred,
                      int64_t* rows_y, float* rows_reg, float* rows_clin, float* rows_out_lin, float* rows_lin_f,
                      int64_t* rows_sbj, void* stream);
int igcn_eval_metrics(int64_t n, int C, int NR, const float* logp, const int64_t* pred, const int64_t* y,
                      const float* reg, const float* clin, const int64_t* state, const double* loss_sum, int64_t* parts,
                      double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GUIDE_IMGSNP (csrc/guide.hip).  nn.PReLU() has one slope a (device float[1], read by the kernels so that a captured
 * step follows the optimiser): y = u > 0 ? u : a u; du = u > 0 ? dy : a dy; da = sum (u > 0 ? 0 : u dy), dy carrying the
 * dropout factor behind the activation.  da (dslope, float[1]) and the weight gradients are FINAL reductions of
 * per-row / per-column partials in a fixed order (queued while igcn_reduce_defer is on; scratch alive until the flush).
 *
 * LayerNorm over nodes + PReLU + node dropout + pooling: igcn_nodes_ln_fwd / igcn_nodes_ln_bwd with ReLU replaced by
 * PReLU — kernel/guide_go_model.py:246-251 (w_act, encoder) and :273-275 (w_act_out, decoder).  Arguments as there plus
 * the slope; dy [B,f,N], dgb [2,N], dslope [1].  scratch: igcn_nodes_ln_prelu_bwd_scratch_floats(B,f,N). */
int igcn_nodes_ln_prelu_fwd(int B, int f, int N, int pool, float eps, const float* y, const float* gamma,
                            const float* beta, const float* keep, const float* slope, float* z, float* mean,
                            float* rstd, void* stream);
size_t igcn_nodes_ln_prelu_bwd_scratch_floats(int B, int f, int N);
int igcn_nodes_ln_prelu_bwd(int B, int f, int N, int pool, const float* y, const float* gamma, const float* beta,
                            const float* keep, const float* slope, const float* mean, const float* rstd,
                            const float* dz, float* dy, float* dgb, float* dslope, float* scratch, void* stream);
/* BatchNorm1d(C) + PReLU (+ dropout keep [B,C], D == 1 only) with groups = 1, optionally behind a per-node linear:
 *   F == 0: the input is x [B,C] — kernel/guide_go_model.py:138-144 (latent: BN(32), PReLU, Dropout(0.5)),
 *           kernel/guide_img_snp.py:57-66 (decoder_i_N: BN(32) and BN(hidden_linear), PReLU, Dropout(0.4));
 *   F >= 1 (<= 8): x [B,F,C] channel-major, W [D,F], pre[b,c,d] = sum_f W[d,f] x[b,f,c] and BatchNorm1d(C) normalises
 *           each c over (batch, d) — :117-121 (conc_for_attention, D = dim_snps_atten), :123-128 (conc + B, D = 1),
 *           :130-136 (conc_D + B_D, D = 1).
 * y [B,C,D]; save_mean / save_rstd [C]; training != 0: batch statistics, running statistics updated (unbiased
 * variance over B D values).  Backward D == 1 only: dx as x, dW [F] (F >= 1), dgamma / dbeta [C], dslope [1];
 * scratch igcn_bn_prelu_bwd_scratch_floats(C, F). */
int igcn_bn_prelu_fwd(int B, int C, int F, int D, const float* x, const float* W, const float* gamma,
                      const float* beta, float* running_mean, float* running_var, int training, float momentum,
                      float eps, const float* keep, const float* slope, float* y, float* save_mean, float* save_rstd,
                      void* stream);
size_t igcn_bn_prelu_bwd_scratch_floats(int C, int F);
int igcn_bn_prelu_bwd(int B, int C, int F, int training, const float* x, const float* W, const float* gamma,
                      const float* beta, const float* slope, const float* save_mean, const float* save_rstd,
                      const float* dy, const float* keep, float* dx, float* dW, float* dgamma, float* dbeta,
                      float* dslope, float* scratch, void* stream);
/* The image gate and encoder_i_N of kernel/guide_img_snp.py:88-100,112 in one launch per direction (one workgroup per
 * sample).  img [B,K] (K = rois H_0), bias [K,2] (bias_n[0]), W1 [H,K], slope (the encoder's PReLU), keep [B,H] (its
 * Dropout(0.4)) or NULL, W2 [L,H]; latent [B,L]; imp1 [K] = softmax(bias_n[0], 1)[:, 1].  Temperature: tau (device
 * float[1]) or, when NULL, tau_value.
 * Training: per (b, k) logit_j = log softmax(bias[k])_j, s = softmax((logit + g) / tau), z1 = 1 iff s1 > s0 (ties: class
 * 0), taken as (z1 - s1) + s1 like gumbel_softmax(hard=True); gate [B,K,2] receives (z1, s0 s1).  Eval: z1 = 1, no draw.
 * The Gumbel noise g of element (b, k, j) sits at flat index i = 2 (b K + k) + j (the reference's [B K, 2] layout):
 * noise [B,K,2] when given, else drawn from the dropout generator's hash at state[0] = c — the 24-bit draw r(c, i) of
 * igcn_dropout_masks, u = (r + 1/2) 2^-24, g = -log(-log u) — after which the launch advances state[0] by one (state:
 * device uint64[igcn_dropout_state_words()], word 1 left at 0).  An eval forward or imposed noise draws nothing.
 * (u is exact: above 1/2 the kernel forms log u as log1p(-(2^24 - r - 1/2) 2^-24), so r = 2^24 - 1 gives a finite g.)
 * Backward: dimg [B,K] (written, not added), dparams [H K + L H + 2 K + 1] = (dW1, dW2, d bias [K,2], dslope); d bias is
 * the straight-through estimator (d z1 reaches s) plus, from dimp1 [K] when not NULL, the gradient reaching imp1.
 * Limits: igcn_guide_gate_supported(K, H, L) (K <= 1024, H <= 64, L <= 64); B >= 1.
 * scratch: igcn_guide_gate_bwd_scratch_floats(B, K, H, L). */
int igcn_guide_gate_supported(int K, int H, int L);
int igcn_guide_gate_fwd(int B, int K, int H, int L, int training, const float* img, const float* bias, const float* tau,
                        float tau_value, const float* noise, void* state, const float* W1, const float* slope,
                        const float* keep, const float* W2, float* latent, float* gate, float* imp1, void* stream);
size_t igcn_guide_gate_bwd_scratch_floats(int B, int K, int H, int L);
int igcn_guide_gate_bwd(int B, int K, int H, int L, int training, const float* img, const float* gate,
                        const float* bias, const float* tau, float tau_value, const float* dimp1, const float* W1,
                        const float* slope, const float* keep, const float* W2, const float* dlatent, float* dimg,
                        float* dparams, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-fold KNN imputation of the clinical scores (csrc/knn_impute.hip): util/tool.py:44-47 and :90-92
 * (KNNImputer(n_neighbors=k).fit_transform(train), .transform(val / test): sklearn's weights="uniform",
 * metric="nan_euclidean", NaN = not measured), :48-50 / :93-94 (scaler4score.transform as x * scale + shift) and :51-72 /
 * :95-110 (the [:, select_index] columns overwrite every subject's clini_score).
 * X [S, F] fp32 holds the demographics; rows_fit [n_fit] / rows_q [n_q] int64 name the training rows and the receivers
 * (NULL: all S rows in order), so a fold reads a resident dataset through its index vectors.  1 <= F <= 32, 1 <= k <= 32,
 * n_fit >= 1, n_q >= 0.
 * dist(q, t) = sqrt(sum over the columns P observed in both of (q_c - t_c)^2 / |P| * F), undefined for empty P.  A missing
 * entry (q, c) = the mean of column c over the min(k, #candidates) nearest candidates (training rows that observe c and
 * have a defined distance to q), ordered by (distance, position in rows_fit): equal distances go to the lower position,
 * the donors' values are added in that order in fp32 and divided once.  No candidate: means[c].  Observed entries pass
 * through bit-identical.  Exact fp32, no atomics, one writer per element.
 * igcn_knn_impute_stats: counts [F] int64 = observed training values per column (a column with 0 cannot be imputed: the
 * caller refuses it), means [F] = their mean (fp64 sum in a fixed order, rounded once).
 * igcn_knn_impute: any of the outputs may be NULL —
 *   out_full [n_q, F]    the imputed rows, unscaled;
 *   out_sel              imputed[:, sel[j]] * scale[sel[j]] + shift[sel[j]], j < n_sel (sel int32; scale / shift [F] or
 *                        NULL = 1 / 0): [n_q, n_sel] dense (scatter = 0), or row rows_q[i] of an [S, n_sel] destination
 *                        (scatter = 1: clini_score written in place, other rows untouched; rows_q must not repeat);
 *   donors [n_q, F, k]   int32 positions in rows_fit in selection order, -1 for unused slots and observed entries;
 *   status [1] int64     the number of entries filled by means[c] (required).
 * A row index outside [0, S) is never dereferenced: the row counts as all-missing, a scattered row is not written, and
 * it is reported — every count = -1 (stats), status = minus the number of such receivers (impute).
 * scratch: igcn_knn_impute_scratch_floats(n_q, n_fit). */
int igcn_knn_impute_stats(int64_t S, int F, const float* X, const int64_t* rows_fit, int64_t n_fit, int64_t* counts,
                          float* means, void* stream);
size_t igcn_knn_impute_scratch_floats(int64_t n_q, int64_t n_fit);
int igcn_knn_impute(int64_t S, int F, int k, const float* X, const int64_t* rows_fit, int64_t n_fit,
                    const int64_t* rows_q, int64_t n_q, const float* means, const float* scale, const float* shift,
                    const int32_t* sel, int n_sel, int scatter, float* out_full, float* out_sel, int32_t* donors,
                    int64_t* status, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cluster labels (csrc/tsne.hip, csrc/kmeans.hip): util/image_cluster.py:148-282 — sklearn's exact t-SNE of the image
 * features (tsne_fdim), KMeans on the embedding (clust_y) and the inertia curve (calculate_WSS), restated on fp32 device
 * tensors.  4 <= S <= 4096 subjects, 1 <= D <= 1024 features, 2 embedding dimensions; KMeans: 1 <= N <= 65536 points of
 * width 1 <= d <= 1024, 1 <= k <= 16 clusters (the IGCN_TSNE_* and IGCN_KMEANS_* limits below).  No atomics, one writer per
 * element, fixed-order reductions.
 * igcn_tsne_sqdist: dist [S, S] = squared Euclidean distances of X [S, D] by direct differences (fp32 fma chain in feature
 *   order; dist[i][j] and dist[j][i] hold the same bits, the diagonal is exactly 0).
 * igcn_tsne_joint_p: _binary_search_perplexity (fp64, at most 100 bisection steps on beta against log(perplexity),
 *   tolerance 1e-5, row sums floored at 1e-8) and _joint_probabilities (symmetrised, divided by the total, clamped at
 *   double epsilon, rounded once to fp32) -> P [S, S] with a zero diagonal, betas [S] fp64 (the beta each row's P was
 *   evaluated at), pstats [2] fp64 = (sum P log P, sum P) of the stored P.  scratch: igcn_tsne_joint_p_scratch_doubles(S).
 *   dist must be symmetric bit for bit (igcn_tsne_sqdist's is): the symmetrising pass reads d_ji as d_ij.
 * igcn_tsne_grad: rowacc [5, S] = per row i the sums over j of P_ij num_ij (y_i - y_j) (x, y), num_ij^2 (y_i - y_j) (x, y)
 *   and num_ij (j != i), num_ij = 1 / (1 + |y_i - y_j|^2), in fp32 from Y [S, 2].  want_kl: a second launch writes
 *   klpart [S] fp64 = sum_{j != i} P_ij log max(num_ij / Z, eps) with Z reduced from rowacc as the update reduces it.
 * igcn_tsne_update: grad = 4 (exaggeration attr - rep / Z) and sklearn's _gradient_descent step in place: gains + 0.2
 *   where update grad < 0, else x 0.8, floored at 0.01; update = momentum update - lr gains grad; Y += update.
 *   grad_out [S, 2] (or NULL) receives grad.  check: status [4] fp64 = (KL divergence of the exaggerated P, norm of
 *   gains grad, Z, status[3] + 1); requires klpart of a want_kl pass over the same Y and pstats.
 * igcn_kmeans_assign: labels [N] int64 = the nearest of centers [k, d] (direct differences; ties to the lower centre),
 *   mind [N] = the squared distance to it; counts [k] int64 and sums [k, d] fp64 (both or neither) per cluster, summed per
 *   workgroup of 64 points and combined in workgroup order; stats[0] = inertia, stats[1] = the number of labels that differ
 *   from what `labels` held on entry (stats: [4] fp64).  scratch: igcn_kmeans_scratch_floats(N, d, k), 8-byte aligned.
 * igcn_kmeans_update: centers <- sums / counts; clusters that came empty, in ascending order, take the points farthest
 *   from their own centre in descending order (ties: the lower point); sums is updated accordingly; a cluster left
 *   without points takes the centre of the largest one.  stats[2] = the total squared centre shift, stats[3] = 1 when
 *   the assignment before it changed a label (stats[1] != 0), else 0.
 * igcn_kmeanspp_step: one greedy k-means++ step from closest [N] (squared distance to the nearest chosen centre), pot [1]
 *   fp64 (their sum) and u [t] fp64 uniform numbers on the device, 1 <= t <= 8 (IGCN_KMEANSPP_MAX_TRIALS): candidates =
 *   left search of u_c pot in the fp64 inclusive scan of closest, clipped to N - 1; the candidate with the smallest new
 *   potential (ties: the first) is written to chosen [1], closest and pot are updated in place. */
#define IGCN_TSNE_MIN_S 4
#define IGCN_TSNE_MAX_S 4096
#define IGCN_TSNE_MAX_D 1024
#define IGCN_KMEANS_MAX_N 65536
#define IGCN_KMEANS_MAX_D 1024
#define IGCN_KMEANS_MAX_K 16
#define IGCN_KMEANSPP_MAX_TRIALS 8
int igcn_tsne_sqdist(int S, int D, const float* X, float* dist, void* stream);
size_t igcn_tsne_joint_p_scratch_doubles(int S);
int igcn_tsne_joint_p(int S, double perplexity, const float* dist, float* P, double* betas, double* pstats,
                      double* scratch, void* stream);
int igcn_tsne_grad(int S, int want_kl, const float* P, const float* Y, float* rowacc, double* klpart, void* stream);
int igcn_tsne_update(int S, float exaggeration, float momentum, float lr, int check, const float* rowacc,
                     const double* klpart, const double* pstats, float* Y, float* update, float* gains, float* grad_out,
                     double* status, void* stream);
size_t igcn_kmeans_scratch_floats(int64_t N, int d, int k);
int igcn_kmeans_assign(int64_t N, int d, int k, const float* X, const float* centers, int64_t* labels, float* mind,
                       int64_t* counts, double* sums, double* stats, float* scratch, void* stream);
int igcn_kmeans_update(int64_t N, int d, int k, const float* X, const int64_t* labels, const float* mind,
                       const int64_t* counts, double* sums, float* centers, double* stats, void* stream);
int igcn_kmeanspp_step(int64_t N, int d, int t, const float* X, const double* u, float* closest, double* pot,
                       int64_t* chosen, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Max-T permutation test of a two-group difference over the entries of a per-subject map table (csrc/perm_test.hip).
 * x [S_all, E] fp32 holds one map of E entries per subject; rows [S] lists the subjects of the two groups under test.
 * igcn_perm_prepare: per column over the listed rows, in fp64 and in list order: mean[e], the population sd[e] and
 *   constant[e] (1 when the column's max equals its min over the listed rows: an exact test).  z = fp32((x - mean) / sd),
 *   formed in fp64 and rounded once; z = 0 for a constant column; standardize = 0: z = x.  z is written as three bf16
 *   planes hi = bf16(z), mid = bf16(z - hi), lo = bf16(z - hi - mid) (round to nearest, every residual exact in fp32:
 *   hi + mid + lo == z for every z whose residuals stay normal), laid out [3][Ep][Sp] with the subject axis contiguous
 *   and zeros in the padding; igcn_perm_plane_dims writes dims = {Ep, Sp} (E rounded up to 64, S to 32) and
 *   igcn_perm_planes_bytes is 3 Ep Sp 2 (0 outside the limits).  A row index outside [0, S_all) reads as NaN.
 * igcn_perm_maxsum: G[p, e] = sum_s member[p, s] z[s, e] on v_mfma_f32_16x16x32_bf16 for member [P, S] uint8 with row
 *   stride ldm bytes (non-zero = 1; row p = group A of relabelling p), widened to bf16 0.0 / 1.0 while it is staged;
 *   the three planes accumulate into the same fp32 accumulators, so every product is exact and the only rounding is the
 *   fp32 accumulation.  G is never stored: maxabs[p] = max_e |G[p, e]| and, with g_obs [E] given,
 *   exceed[e] = #{p : |G[p, e]| >= |g_obs[e]|} (int32).  With g_obs NULL the call writes g [P, E] itself, for P <= 8
 *   (IGCN_PERM_MAX_G_ROWS; the observed pass, P = 1, through the same tile code), and exceed is not touched.  Rows of member that start 16-byte
 *   aligned (ldm % 16 == 0, aligned base: all ldm bytes of every row must then be readable) are staged with 16-byte
 *   loads; the result does not depend on it.
 *   Per-tile partials ([P, tiles_E] maxima, [tiles_P, E] counts) in `scratch` (device, 16-byte aligned,
 *   igcn_perm_maxsum_scratch_bytes(P, E); 0 outside the limits) are folded in tile order by two small kernels.  One
 *   writer per element, no atomics: two runs give the same bits, and a row's results do not depend on the tile, the
 *   launch or the chunk it sits in (the accumulation order along S is the same for every row).  The library allocates
 *   nothing.  Limits: 4 <= S <= 4096, 1 <= E <= 2^20, 1 <= P <= 65536 per launch
 *   (IGCN_PERM_MIN_S, IGCN_PERM_MAX_S, IGCN_PERM_MAX_E, IGCN_PERM_MAX_P). */
#define IGCN_PERM_MIN_S 4
#define IGCN_PERM_MAX_S 4096
#define IGCN_PERM_MAX_E 1048576
#define IGCN_PERM_MAX_P 65536
#define IGCN_PERM_MAX_G_ROWS 8
size_t igcn_perm_planes_bytes(int S, int E);
int igcn_perm_plane_dims(int S, int E, int* dims);
int igcn_perm_prepare(int64_t S_all, int S, int E, const float* x, const int64_t* rows, int standardize, double* mean,
                      double* sd, uint8_t* constant, void* planes, void* stream);
size_t igcn_perm_maxsum_scratch_bytes(int P, int E);
int igcn_perm_maxsum(int P, int S, int E, const uint8_t* member, int64_t ldm, const void* planes, const float* g_obs,
                     float* maxabs, int32_t* exceed, float* g, void* scratch, size_t scratch_bytes, void* stream);

/* Max-F permutation test of a difference between K = 2..5 groups (IGCN_PERM_MAX_GROUPS), on the planes of
 * igcn_perm_prepare.  labels [P, S] uint8 with row stride ldl bytes: byte g puts subject s in group g of relabelling p.
 * igcn_perm_maxf: for the K - 1 accumulated groups G_g[p, e] = sum_s (labels[p, s] == g) z[s, e], the indicator as bf16
 *   0.0 / 1.0 on v_mfma_f32_16x16x32_bf16 (exact products, fp32 accumulation, planes hi, mid, lo and subjects ascending
 *   for every row, as igcn_perm_maxsum; the label bytes stay raw in LDS and are widened in registers, and one read of a
 *   plane fragment feeds all groups).  The LAST group's sum is DEFINED as minus the sum of the others — the column sum of
 *   the fp32 z is zero only to rounding — so a label byte >= K - 1, whatever its value, counts for the last group.
 *   With weights [K] (a HOST array, copied into the launch; finite and > 0; 1 / n_g gives the between-groups sum of
 *   squares of a one-way ANOVA, of which F is one increasing function for every column)
 *     B[p, e] = sum_{g < K-1} w_g G_g^2 + w_{K-1} (sum_{g < K-1} G_g)^2      (fp32, g ascending, the last term last),
 *   maxstat[p] = max_e B[p, e] and, with b_obs [E] given, exceed[e] = #{p : B[p, e] >= b_obs[e]} (int32).  With b_obs
 *   NULL the call writes b [P, E] itself and, when g is not NULL, g [P, K-1, E], for P <= 8 (IGCN_PERM_MAX_G_ROWS: the
 *   observed pass through the same tile code, so a relabelling equal to the observed one ties exactly); exceed is not
 *   touched.  scratch, alignment, limits and the guarantees (one writer per element, no atomics, no allocation, same
 *   bits for any tile, launch or chunk) are those of igcn_perm_maxsum; scratch: igcn_perm_maxsum_scratch_bytes(P, E). */
#define IGCN_PERM_MAX_GROUPS 5
int igcn_perm_maxf(int P, int S, int E, int K, const uint8_t* labels, int64_t ldl, const void* planes,
                   const float* weights /* HOST, [K], copied into the launch */, const float* b_obs, float* maxstat,
                   int32_t* exceed, float* b, float* g /* or NULL */, void* scratch, size_t scratch_bytes, void* stream);

/* Network-based statistic (Zalesky, Fornito & Bullmore 2010) of a two-group difference over ROI x ROI connectivity maps,
 * on the planes of igcn_perm_prepare: threshold the edge-wise statistic, take the connected components of what is left,
 * correct with the permutation distribution of the largest component's extent.
 * igcn_perm_supra (csrc/perm_test.hip): the product, the tile and the accumulation order of igcn_perm_maxsum — the
 *   accumulators hold exactly the bits igcn_perm_maxsum writes to g — and ONE BIT per (relabelling, entry) leaves: with
 *   v = |G[p, e]| for tail 0, G for tail +1 and -G for tail -1, bit e & 31 of word e >> 5 of row p of bits (uint32
 *   [P, ldw], ldw >= Ep / 32 words, Ep = E rounded up to 64) is set iff tested[e] != 0 (uint8 [E], device) and v >= thr.
 *   |t| is one increasing function of |G| for every column, so a primary threshold t0 on t is the ONE threshold
 *   thr = sqrt(n_a n_b) t0 / sqrt(S - 2 + t0^2) on G.  Every word of every row below P is written, all-zero words and
 *   the words behind Ep / 32 included; bits at or behind E are 0.  A row's words are assembled from wave ballots: one
 *   writer per word, no atomics, no scratch, no fold launch.  thr finite and > 0, tail in {-1, 0, 1}, bits 16-byte
 *   aligned; the other limits and guarantees are those of igcn_perm_maxsum.
 * igcn_nbs_components (csrc/nbs.hip): row p of bits is the [R, R] entry set of relabelling p, row-major (entry i R + j:
 *   source row i, target column j; E = R R), 2 <= R <= 128 (IGCN_NBS_MAX_ROIS), ldw >= ceil(R R / 32), 1 <= P <= 65536.
 *   Nodes i != j are joined when bit (i, j) OR bit (j, i) is set (undirected; a diagonal bit joins nothing).  The extent
 *   of a component is the number of set bits whose source row lies in it: every set entry counts once, diagonal bits
 *   included, and with only the upper triangle tested every undirected edge counts once.  One wave per relabelling labels
 *   the graph by minimum-label propagation in LDS.  max_extent[p] is the largest extent (0 for an empty graph);
 *   label [P, R] (or NULL) the smallest node index of the node's component; extent [P, R] (or NULL) the extent of the
 *   node's component, 0 for a node without a set entry in its row and without a neighbour.  All int32; one writer per
 *   element; the extent sums are integer LDS atomics (one result in any order).  The library allocates nothing. */
#define IGCN_NBS_MAX_ROIS 128
int igcn_perm_supra(int P, int S, int E, const uint8_t* member, int64_t ldm, const void* planes, float thr, int tail,
                    const uint8_t* tested /* [E] */, void* bits /* uint32 [P, ldw] */, int64_t ldw, void* stream);
int igcn_nbs_components(int P, int R, const void* bits, int64_t ldw, int32_t* max_extent /* [P] */,
                        int32_t* label /* [P, R] or NULL */, int32_t* extent /* [P, R] or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IGCN_H */
