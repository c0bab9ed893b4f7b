// Graph-diffusion pre-transform for graphs beyond the LDS limit of csrc/gdc.hip (R <= 512): the same contract as
// igcn_gdc_diffuse — util_gdc.py:7-15 get_ppr_matrix, :16-23 get_heat_matrix, :25-31 get_top_k_matrix, :33-38
// get_clipped_matrix, :82-86 coo_matrix, batch.py:98-104 node offsets — with the fp64 system of every graph in a
// caller-supplied global-memory workspace instead of one workgroup's LDS.
//
// Both diffusion matrices are formed from fp64 matrix products with non-negative terms only (nothing cancels).
// H = D^-1/2 A D^-1/2, every matrix padded to Rp = R rounded up to GT_TILE with zero rows and columns: the padded block
// of either result is the identity and touches nothing else.
//   PPR   P = alpha (I - G)^-1, G = (1 - alpha) H.  G^n decays like (1 - alpha)^n, so
//             (I - G)^-1 = prod_{j<J} (I + G^(2^j)),   J = ceil(log2(ln 2^-60 / ln(1 - alpha)))     (gdct_ppr_terms)
//         as the recurrence Q <- G, P <- I + G; J - 1 times: Q <- Q Q, P <- P + P Q.   2 (J - 1) products.
//   heat  S = e^-t expm(t H): k_gdc_heat's scheme — X = t H / 2^s with s per graph the smallest s with |X|_1 <= 1/2, a
//         Taylor polynomial of degree 14 in Horner form, s squarings, e^-t applied where the matrix is read.
//         13 + smax products: the host launches smax = ceil(log2(2 t sqrt(R))) squarings (|H|_1 <= sqrt(R) for a
//         symmetric A) without reading anything back, and a graph whose own s is used up passes its matrix through.
// Launch sequence (all on one stream, no host read, no atomics, one writer per element, fixed summation order):
//   k_gdct_rowsum -> [k_gdct_colnorm] -> k_gdct_form -> k_gdct_gemm x (products) -> k_gdct_select -> k_gdct_rowcount
//   -> k_gdct_emit
#include <math.h>

#include "gdc_common.h"

#define GT_TILE 64                                     // output tile of a workgroup, and the padding unit of R
#define GT_BK 16                                       // k extent of one staged operand pair
#define GT_T 256                                       // 2 x 2 waves, each 2 x 2 MFMA tiles of 16 x 16
#define GT_LDA (GT_BK + 1)                             // odd leading dimensions (in doubles) of the staged operands
#define GT_LDB (GT_TILE + 1)
#define GT_MAX_R 512
#define GT_PPR_MAX_TERMS 16
#define GT_ALPHA_MIN 1e-3                              // J(1e-3) = 16

typedef double gdct_d4 __attribute__((ext_vector_type(4)));

struct GdctInfo {                                      // per graph, written by the set-up kernels
  double norm;                                         // |t H|_1 (heat; 0 for PPR)
  int s;                                               // squarings this graph needs (heat; 0 for PPR)
  int valid;                                           // 0: subject index outside the dataset -> empty graph
};

// where everything lives in the workspace; the ONLY place that knows how many matrices a kernel needs
struct GdctLayout {
  int Rp, nmat;
  size_t mat;                                          // doubles per matrix of one graph
  size_t o_mats, o_dinv, o_thrv, o_den, o_cmax, o_thri, o_rowcnt, o_info, bytes;
};

static GdctLayout gdct_layout(int B, int R, int kernel) {
  GdctLayout l;
  l.Rp = (R + GT_TILE - 1) / GT_TILE * GT_TILE;
  l.nmat = kernel == IGCN_GDC_PPR ? 4 : 3;             // PPR: Q, Q', P, P'.  heat: X, T, T'
  l.mat = (size_t)l.Rp * l.Rp;
  const size_t b = (size_t)B, rp = (size_t)l.Rp;
  size_t o = 0;
  l.o_mats = o;   o += b * l.nmat * l.mat * sizeof(double);
  l.o_dinv = o;   o += b * rp * sizeof(double);
  l.o_thrv = o;   o += b * rp * sizeof(double);
  l.o_den = o;    o += b * rp * sizeof(double);
  l.o_cmax = o;   o += b * (GT_MAX_R / GT_TILE) * sizeof(double);
  l.o_info = o;   o += b * sizeof(GdctInfo);
  l.o_thri = o;   o += b * rp * sizeof(int);
  l.o_rowcnt = o; o += b * rp * sizeof(int);
  l.bytes = o;
  return l;
}

static int gdct_ppr_terms(double alpha) {              // J: prod_{j<J} (I + G^(2^j)) leaves (1 - alpha)^(2^J) <= 2^-60
  if (alpha >= 1.0) return 1;
  const double n = (-60.0 * log(2.0)) / log(1.0 - alpha);
  const int j = (int)ceil(log2(n));
  return j < 1 ? 1 : j;
}

static int gdct_heat_max_squarings(double t, int R) {  // |t H|_1 <= t sqrt(R)  ->  s <= ceil(log2(2 t sqrt(R)))
  const int s = (int)ceil(log2(2.0 * t * sqrt((double)R)));
  return s < 0 ? 0 : s;
}

// ---- set-up ---------------------------------------------------------------------------------------------------------
// dinv[g][i] = 1 / sqrt(row sum i of graph g's matrix); one wave per row, lanes stride the row, fixed tree.
// Block (0, g) also records whether the graph is read at all.
__global__ void __launch_bounds__(64)
k_gdct_rowsum(int R, int Rp, const float* __restrict__ A, const int64_t* __restrict__ subject, int64_t n_subjects,
              double* __restrict__ dinv, GdctInfo* __restrict__ info) {
  const int i = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
  const int64_t sj = GDC_SUBJECT_OF(subject, g);
  const bool valid = !GDC_NOT_READ(subject, sj, n_subjects);
  if (i == 0 && lane == 0) {
    info[g].valid = valid ? 1 : 0;
    info[g].norm = 0.0;
    info[g].s = 0;
  }
  double s = 0.0;
  if (valid) {
    const float* a = A + (sj * R + i) * R;
    for (int j = lane; j < R; j += 64) s += (double)a[j];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) dinv[(size_t)g * Rp + i] = valid ? 1.0 / sqrt(s) : 0.0;
}

// heat: cmax[g][c] = largest column sum of |t H| among the columns of column block c (thread = column: a row of 64
// adjacent columns is one coalesced read)
__global__ void __launch_bounds__(GT_TILE)
k_gdct_colnorm(int R, int Rp, double t, const float* __restrict__ A, const int64_t* __restrict__ subject,
               const double* __restrict__ dinv, const GdctInfo* __restrict__ info, double* __restrict__ cmax) {
  const int g = blockIdx.y, j = blockIdx.x * GT_TILE + threadIdx.x;
  double s = 0.0;
  if (info[g].valid && j < R) {
    const float* a = A + GDC_SUBJECT_OF(subject, g) * R * R;
    const double* d = dinv + (size_t)g * Rp;
    const double dj = d[j];
    for (int i = 0; i < R; ++i) s += fabs(t * (d[i] * (double)a[(size_t)i * R + j] * dj));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = fmax(s, __shfl_xor(s, o, 64));
  if (threadIdx.x == 0) cmax[(size_t)g * (GT_MAX_R / GT_TILE) + blockIdx.x] = s;
}

// PPR:  M0 = G = (1 - alpha) H,  M1 = I + G.      heat:  M0 = X = t H / 2^s,  M1 = I + X / degree; info[g] = (|tH|_1, s)
// Both padded to Rp.  Every thread derives s for itself from the column-block maxima (the same value in all of them).
__global__ void __launch_bounds__(GT_T)
k_gdct_form(int R, int Rp, int kernel, double param, int smax, const float* __restrict__ A,
            const int64_t* __restrict__ subject, const double* __restrict__ dinv, const double* __restrict__ cmax,
            GdctInfo* __restrict__ info, double* __restrict__ M0, double* __restrict__ M1) {
  const int g = blockIdx.y;
  if (!info[g].valid) return;
  const float* a = A + GDC_SUBJECT_OF(subject, g) * R * R;    // (info.valid: the index is inside the dataset)
  const double* d = dinv + (size_t)g * Rp;
  double down = 1.0;
  if (kernel == IGCN_GDC_HEAT) {
    double nrm = 0.0;
    for (int c = 0; c < Rp / GT_TILE; ++c) nrm = fmax(nrm, cmax[(size_t)g * (GT_MAX_R / GT_TILE) + c]);
    const int s = gdc_scaling_exponent(nrm, smax);
    down = ldexp(1.0, -s);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      info[g].norm = nrm;
      info[g].s = s;
    }
  }
  const size_t base = (size_t)g * Rp * Rp;
  const int e = blockIdx.x * GT_T + threadIdx.x;        // (Rp * Rp is a multiple of GT_T)
  const int i = e / Rp, j = e - i * Rp;
  double x = 0.0;
  if (i < R && j < R) {
    const double av = (double)a[(size_t)i * R + j];
    x = kernel == IGCN_GDC_HEAT ? (param * (d[i] * av * d[j])) * down : (1.0 - param) * (d[i] * av * d[j]);
  }
  const double eye = i == j ? 1.0 : 0.0;
  M0[base + e] = x;
  M1[base + e] = kernel == IGCN_GDC_HEAT ? eye + x / (double)GDC_HEAT_DEGREE : eye + x;
}

// ---- batched fp64 GEMM on v_mfma_f64_16x16x4_f64 ----------------------------------------------------------------------
// C_g = epilogue(L_g * Rm_g), all [Rp][Rp] row-major with Rp a multiple of GT_TILE, matrix g at g * Rp * Rp.
// Grid (column tiles, row tiles, graphs).  C must be none of the inputs: other workgroups read them.
//   form 0: C = acc      form 1: C = I + mul * acc      form 2: C = Padd + acc
// sq_step >= 0 marks squaring number sq_step of the heat kernel: a graph whose s <= sq_step copies L through unchanged,
// so every graph ends on the same ping-pong buffer.  A graph that is not read (info.valid == 0) is skipped.
// Operands of the f64 MFMA: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15];
// C/D: col = lane & 15, row = (lane >> 4) + 4 reg.
enum { GT_FORM_PLAIN = 0, GT_FORM_EYE_MUL = 1, GT_FORM_ADD = 2 };

__global__ void __launch_bounds__(GT_T)
k_gdct_gemm(int Rp, const double* __restrict__ L, const double* __restrict__ Rm, const double* __restrict__ Padd,
            double* __restrict__ C, int form, double mul, int sq_step, const GdctInfo* __restrict__ info) {
  __shared__ double As[GT_TILE * GT_LDA];               // [row][k]
  __shared__ double Bs[GT_BK * GT_LDB];                 // [k][col]
  const int g = blockIdx.z, tid = threadIdx.x;
  if (!info[g].valid) return;                           // (uniform over the workgroup: no barrier has been reached yet)
  const size_t base = (size_t)g * Rp * Rp;
  const int bm = blockIdx.y * GT_TILE, bn = blockIdx.x * GT_TILE;
  L += base;
  Rm += base;
  C += base;
  if (sq_step >= 0 && sq_step >= info[g].s) {
    for (int e = tid; e < GT_TILE * GT_TILE; e += GT_T) {
      const int i = bm + e / GT_TILE, j = bn + (e & (GT_TILE - 1));
      C[(size_t)i * Rp + j] = L[(size_t)i * Rp + j];
    }
    return;
  }
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4;
  // staging: thread -> 4 consecutive doubles of the A tile [64][16] and of the B tile [16][64]
  const int ar = tid >> 2, ak = (tid & 3) * 4, bk = tid >> 4, bc = (tid & 15) * 4;
  const double* lp = L + (size_t)(bm + ar) * Rp + ak;
  const double* rp = Rm + (size_t)bk * Rp + bn + bc;
  gdct_d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = gdct_d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < Rp; k0 += GT_BK) {
    const double2 a0 = *reinterpret_cast<const double2*>(lp + k0);
    const double2 a1 = *reinterpret_cast<const double2*>(lp + k0 + 2);
    const double2 b0 = *reinterpret_cast<const double2*>(rp + (size_t)k0 * Rp);
    const double2 b1 = *reinterpret_cast<const double2*>(rp + (size_t)k0 * Rp + 2);
    __syncthreads();                                    // every wave has read the previous pair
    As[ar * GT_LDA + ak] = a0.x;
    As[ar * GT_LDA + ak + 1] = a0.y;
    As[ar * GT_LDA + ak + 2] = a1.x;
    As[ar * GT_LDA + ak + 3] = a1.y;
    Bs[bk * GT_LDB + bc] = b0.x;
    Bs[bk * GT_LDB + bc + 1] = b0.y;
    Bs[bk * GT_LDB + bc + 2] = b1.x;
    Bs[bk * GT_LDB + bc + 3] = b1.y;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GT_BK; kk += 4) {
      double fa[2], fb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) fa[a] = As[(wr * 32 + a * 16 + lr) * GT_LDA + kk + lk];
#pragma unroll
      for (int b = 0; b < 2; ++b) fb[b] = Bs[(kk + lk) * GT_LDB + wc * 32 + b * 16 + lr];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = bm + wr * 32 + a * 16 + lk + 4 * q, j = bn + wc * 32 + b * 16 + lr;
        const size_t at = (size_t)i * Rp + j;
        double v = acc[a][b][q];
        if (form == GT_FORM_EYE_MUL) v = (i == j ? 1.0 : 0.0) + v * mul;
        else if (form == GT_FORM_ADD) v = Padd[base + at] + v;
        C[at] = v;
      }
}

// ---- selection and emission from global memory (the contract: csrc/gdc_common.h) --------------------------------------
// What a column keeps is described by a pair (thrv, thri): entry (i, j) stays iff
//   v > thrv[j]  or  (v == thrv[j] and i >= thri[j]),        v = scale * M[i][j]
// top-k: (thrv, thri) is the k-th entry of the column in the order of preference; threshold: (eps, 0).  den[j] = sum of
// what the column kept, 1 where that sum is <= 0.
__device__ __forceinline__ double gdct_weight(double m, int i, double scale, double thrv, int thri, double den) {
  const double v = scale * m;
  const bool kept = v > thrv || (v == thrv && i >= thri);
  return kept ? v / den : 0.0;
}

// thread = column; the 64 columns of a block read every row as one coalesced segment
__global__ void __launch_bounds__(GT_TILE)
k_gdct_select(int R, int Rp, double scale, GdcSparsify sp, const double* __restrict__ M,
              const GdctInfo* __restrict__ info, double* __restrict__ thrv, int* __restrict__ thri,
              double* __restrict__ den) {
  const int g = blockIdx.y, j = blockIdx.x * GT_TILE + threadIdx.x;
  if (!info[g].valid || j >= R) return;
  const double* m = M + (size_t)g * Rp * Rp + j;
  double norm = 0.0, tv, pv = HUGE_VAL;
  int ti, pi = R;
  if (sp.mode == IGCN_GDC_THRESHOLD) {
    for (int i = 0; i < R; ++i) {
      const double v = scale * m[(size_t)i * Rp];
      if (v >= sp.eps) norm += v;
    }
    tv = sp.eps;
    ti = 0;
  } else {
    // sweep q finds the q-th entry in the order of preference: the best among those behind the previous one
    for (int q = 0; q < sp.k; ++q) {
      double best = 0.0;
      int bi = -1;
      for (int i = 0; i < R; ++i) {
        const double v = scale * m[(size_t)i * Rp];
        const bool behind = v < pv || (v == pv && i < pi);
        if (behind && (bi < 0 || v >= best)) { best = v; bi = i; }
      }
      if (bi < 0) break;                                // (only with values that do not compare: keep what was found)
      pv = best;
      pi = bi;
      norm += best;
    }
    tv = pv;
    ti = pi;
  }
  const size_t o = (size_t)g * Rp + j;
  thrv[o] = tv;
  thri[o] = ti;
  den[o] = norm <= 0.0 ? 1.0 : norm;
}

// one wave per row: rowcnt[g][i] = edges of row i
__global__ void __launch_bounds__(64)
k_gdct_rowcount(int R, int Rp, double scale, const double* __restrict__ M, const GdctInfo* __restrict__ info,
                const double* __restrict__ thrv, const int* __restrict__ thri, const double* __restrict__ den,
                int* __restrict__ rowcnt) {
  const int i = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
  int n = 0;
  if (info[g].valid) {
    const double* m = M + (size_t)g * Rp * Rp + (size_t)i * Rp;
    const size_t o = (size_t)g * Rp;
    for (int j = lane; j < R; j += 64) n += gdct_weight(m[j], i, scale, thrv[o + j], thri[o + j], den[o + j]) != 0.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane == 0) rowcnt[(size_t)g * Rp + i] = n;
}

// one wave per row: the row's edges behind those of the rows above it, in column order; the wave of row i also writes
// the padding slots total + i, total + i + R, ... and the wave of row 0 the count.
__global__ void __launch_bounds__(64)
k_gdct_emit(int R, int Rp, int cap, double scale, const double* __restrict__ M, const GdctInfo* __restrict__ info,
            const double* __restrict__ thrv, const int* __restrict__ thri, const double* __restrict__ den,
            const int* __restrict__ rowcnt, int64_t* __restrict__ ei_row, int64_t* __restrict__ ei_col,
            float* __restrict__ ew, int32_t* __restrict__ counts) {
  const int i = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
  const int* rc = rowcnt + (size_t)g * Rp;
  int start = 0, total = 0;
  for (int r = lane; r < R; r += 64) {
    const int c = rc[r];
    total += c;
    if (r < i) start += c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    start += __shfl_xor(start, o, 64);
    total += __shfl_xor(total, o, 64);
  }
  const int64_t slot0 = (int64_t)g * R * cap, off = (int64_t)g * R, slots = (int64_t)R * cap;
  if (info[g].valid) {                                  // (an unread graph has no edges: rowcnt is all zero)
    const double* m = M + (size_t)g * Rp * Rp + (size_t)i * Rp;
    const size_t o = (size_t)g * Rp;
    int before = start;
    for (int j0 = 0; j0 < R; j0 += 64) {                // (uniform trip count: the ballot sees the whole wave)
      const int j = j0 + lane;
      const double w = j < R ? gdct_weight(m[j], i, scale, thrv[o + j], thri[o + j], den[o + j]) : 0.0;
      const unsigned long long mask = __ballot(w != 0.0);
      if (w != 0.0) {
        const int64_t s2 = slot0 + before + __popcll(mask & ((1ull << lane) - 1ull));
        ei_row[s2] = off + i;
        ei_col[s2] = off + j;
        ew[s2] = (float)w;
      }
      before += __popcll(mask);
    }
  }
  for (int64_t p = (int64_t)total + i + (int64_t)lane * R; p < slots; p += (int64_t)64 * R) {
    ei_row[slot0 + p] = -1;
    ei_col[slot0 + p] = -1;
    ew[slot0 + p] = 0.f;
  }
  if (i == 0 && lane == 0) counts[g] = total;
}

// ---- host -------------------------------------------------------------------------------------------------------------
extern "C" int igcn_gdc_tiled_max_rois(void) { return GT_MAX_R; }

extern "C" size_t igcn_gdc_tiled_workspace_bytes(int B, int R, int kernel) {
  if (B <= 0 || R <= 0 || R > GT_MAX_R || (kernel != IGCN_GDC_PPR && kernel != IGCN_GDC_HEAT)) return 0;
  return gdct_layout(B, R, kernel).bytes;
}

extern "C" int igcn_gdc_diffuse_tiled(int B, int R, int kernel, double param, int sparsify, int k, double eps,
                                      const float* A, int64_t n_subjects, const int64_t* subject, int64_t* edge_index,
                                      float* edge_attr, int32_t* counts, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  const char* who = "gdc_diffuse_tiled";
  IGCN_REQUIRE(subject == nullptr || n_subjects > 0, "%s: a subject list needs n_subjects > 0", who);
  const int bad = gdc_check_args(who, B, R, kernel, param, sparsify, k, eps, GT_ALPHA_MIN, GT_PPR_MAX_TERMS, GT_MAX_R);
  if (bad != IGCN_OK) return bad;
  IGCN_REQUIRE(B <= 65535, "%s: B=%d graphs in one call (at most 65535)", who, B);
  if (B == 0) return IGCN_OK;
  const GdctLayout l = gdct_layout(B, R, kernel);
  if (workspace == nullptr || workspace_bytes < l.bytes) {
    igcn_set_error("%s: the workspace holds %zu bytes, B=%d R=%d needs %zu bytes", who,
                   workspace ? workspace_bytes : (size_t)0, B, R, l.bytes);
    return IGCN_ERR_UNSUPPORTED;
  }
  IGCN_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* mats = (double*)(ws + l.o_mats);
  auto matrix = [&](int m) { return mats + (size_t)m * B * l.mat; };          // matrix m of graph 0; graph g at + g * mat
  double* dinv = (double*)(ws + l.o_dinv);
  double* thrv = (double*)(ws + l.o_thrv);
  double* den = (double*)(ws + l.o_den);
  double* cmax = (double*)(ws + l.o_cmax);
  int* thri = (int*)(ws + l.o_thri);
  int* rowcnt = (int*)(ws + l.o_rowcnt);
  GdctInfo* info = (GdctInfo*)(ws + l.o_info);
  const int Rp = l.Rp, nt = Rp / GT_TILE;
  const GdcSparsify sp = gdc_sparsify(sparsify, k, eps, R);
  const int64_t slots = (int64_t)B * R * sp.cap;
  const int smax = kernel == IGCN_GDC_HEAT ? gdct_heat_max_squarings(param, R) : 0;

  hipLaunchKernelGGL(k_gdct_rowsum, dim3(R, B), dim3(64), 0, st, R, Rp, A, subject, n_subjects, dinv, info);
  if (kernel == IGCN_GDC_HEAT)
    hipLaunchKernelGGL(k_gdct_colnorm, dim3(nt, B), dim3(GT_TILE), 0, st, R, Rp, param, A, subject, dinv, info, cmax);
  hipLaunchKernelGGL(k_gdct_form, dim3(Rp * Rp / GT_T, B), dim3(GT_T), 0, st, R, Rp, kernel, param, smax, A, subject,
                     dinv, cmax, info, matrix(0), matrix(kernel == IGCN_GDC_HEAT ? 1 : 2));
  auto gemm = [&](const double* L, const double* Rm, const double* Padd, double* C, int form, double mul, int sq) {
    hipLaunchKernelGGL(k_gdct_gemm, dim3(nt, nt, B), dim3(GT_T), 0, st, Rp, L, Rm, Padd, C, form, mul, sq, info);
  };
  const double* result;
  double scale;
  if (kernel == IGCN_GDC_HEAT) {
    double* X = matrix(0);
    double* T[2] = {matrix(1), matrix(2)};
    int cur = 0;
    for (int j = GDC_HEAT_DEGREE - 1; j >= 1; --j, cur ^= 1)     // T_j = I + X T_(j+1) / j
      gemm(X, T[cur], nullptr, T[cur ^ 1], GT_FORM_EYE_MUL, 1.0 / (double)j, -1);
    for (int q = 0; q < smax; ++q, cur ^= 1) gemm(T[cur], T[cur], nullptr, T[cur ^ 1], GT_FORM_PLAIN, 1.0, q);
    result = T[cur];
    scale = exp(-param);
  } else {
    double* Q[2] = {matrix(0), matrix(1)};
    double* P[2] = {matrix(2), matrix(3)};
    int cur = 0;
    for (int j = 1; j < gdct_ppr_terms(param); ++j, cur ^= 1) {
      gemm(Q[cur], Q[cur], nullptr, Q[cur ^ 1], GT_FORM_PLAIN, 1.0, -1);                   // Q <- Q Q
      gemm(P[cur], Q[cur ^ 1], P[cur], P[cur ^ 1], GT_FORM_ADD, 1.0, -1);                  // P <- P + P Q
    }
    result = P[cur];
    scale = param;
  }
  hipLaunchKernelGGL(k_gdct_select, dim3(nt, B), dim3(GT_TILE), 0, st, R, Rp, scale, sp, result, info, thrv, thri, den);
  hipLaunchKernelGGL(k_gdct_rowcount, dim3(R, B), dim3(64), 0, st, R, Rp, scale, result, info, thrv, thri, den, rowcnt);
  hipLaunchKernelGGL(k_gdct_emit, dim3(R, B), dim3(64), 0, st, R, Rp, sp.cap, scale, result, info, thrv, thri, den,
                     rowcnt, edge_index, edge_index + slots, edge_attr, counts);
  IGCN_CHECK_LAUNCH(who);
  return IGCN_OK;
}
