// Max-T permutation test of a two-group difference over the E entries of a per-subject map table x [S_all, E]
// (include/igcn.h: igcn_perm_prepare, igcn_perm_maxsum).  For P relabellings of the S subjects under test the work is
//   G[p, e] = sum_s member[p, s] z[s, e],      member 0/1 (row p = group A of relabelling p), z the standardised column,
// a [P, S] x [S, E] product that is never stored: the epilogue keeps max_e |G[p, e]| per relabelling and, per entry, the
// number of relabellings with |G[p, e]| >= |g_obs[e]|.  After standardisation every column has the same sum of squares,
// so |t| is one increasing function of |G| for all columns and comparing |G| is comparing |t|.
//
// Exact operands on the bf16 matrix unit: z (fp32) is split into three bf16 planes hi = bf16(z), mid = bf16(z - hi),
// lo = bf16(z - hi - mid), every residual exact in fp32, so hi + mid + lo == z for every z whose residuals stay normal;
// member widens to bf16 0.0 / 1.0.  Every product is exact and the three planes accumulate into the SAME fp32
// accumulators: the only rounding is the fp32 accumulation.
//
// Layout of the planes: [3][Ep][Sp] bf16, Ep = E rounded up to PT_BN, Sp = S rounded up to PT_BK, the subject axis
// contiguous (the B fragment of v_mfma_f32_16x16x32_bf16 — col = lane & 15, k = 8 (lane >> 4) .. + 7 — is one 16-byte
// read of a row), zeros in the padding.
//
// Launch sequence of igcn_perm_maxsum: k_perm_maxsum (per-tile partials) -> k_perm_fold_max, k_perm_fold_cnt.
// One writer per element, no atomics, fixed order: the accumulation order along S of a row is k-steps ascending, planes
// hi, mid, lo inside a step, whichever tile or launch the row sits in.
//
// igcn_perm_maxf (k_perm_maxf, below the two-group kernels) is the same product for K = 2..5 groups: K - 1 indicator
// operands read off one label byte, one statistic B of which the one-way ANOVA F is an increasing function.
//
// igcn_perm_supra (k_perm_supra, below k_perm_maxsum) is the two-group product once more with an epilogue that keeps one
// bit per (relabelling, entry), |G| >= thr: the input of the network-based statistic (csrc/nbs.hip labels the graphs).
#include <math.h>

#include "common.h"

#define PT_BM 128                                      // relabellings per workgroup: 4 waves x 2 fragments of 16 rows
#define PT_BN 64                                       // map entries per workgroup: 4 fragments of 16 columns per wave
#define PT_BK 32                                       // subjects per step: one v_mfma_f32_16x16x32_bf16 deep
#define PT_LD (PT_BK + 8)                              // LDS row: 32 bf16 + 8 pad (80 B), as k_gemm_bf16 (csrc/gemm.hip)
#define PT_T 256

typedef __bf16 pt_bf16x8 __attribute__((ext_vector_type(8)));
typedef float pt_f32x4 __attribute__((ext_vector_type(4)));

static inline int pt_ep(int E) { return (E + PT_BN - 1) / PT_BN * PT_BN; }
static inline int pt_sp(int S) { return (S + PT_BK - 1) / PT_BK * PT_BK; }

// ---- prepare ----------------------------------------------------------------------------------------------------------
// Thread = column (adjacent threads read adjacent floats of a row); the listed rows in list order, fp64 throughout:
// the mean, then the centred sum of squares, then z.  A row index outside [0, S_all) reads as NaN (never out of bounds).
__device__ __forceinline__ unsigned short pt_bits(__bf16 v) { return __builtin_bit_cast(unsigned short, v); }

__global__ void __launch_bounds__(256)
k_perm_prepare(int64_t S_all, int S, int E, int Ep, int Sp, const float* __restrict__ x,
               const int64_t* __restrict__ rows, int standardize, double* __restrict__ mean, double* __restrict__ sd,
               uint8_t* __restrict__ constant, unsigned short* __restrict__ planes) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Ep) return;
  const size_t plane = (size_t)Ep * Sp;
  unsigned short* ph = planes + (size_t)e * Sp;
  if (e >= E) {                                         // a padded column: zeros in all three planes
    for (int s = 0; s < Sp; ++s) {
      ph[s] = 0;
      ph[plane + s] = 0;
      ph[2 * plane + s] = 0;
    }
    return;
  }
  const float nanf_ = __builtin_nanf("");
  auto at = [&](int s) -> float {
    const int64_t r = rows[s];
    return (r < 0 || r >= S_all) ? nanf_ : x[r * (int64_t)E + e];
  };
  double sum = 0.0;
  float lo = at(0), hi = lo;
  for (int s = 0; s < S; ++s) {
    const float v = at(s);
    sum += (double)v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  const double m = sum / (double)S;
  double ss = 0.0;
  for (int s = 0; s < S; ++s) {
    const double d = (double)at(s) - m;
    ss += d * d;
  }
  const double dev = sqrt(ss / (double)S);
  const bool is_const = hi == lo;
  mean[e] = m;
  sd[e] = dev;
  constant[e] = is_const ? 1 : 0;
  for (int s = 0; s < Sp; ++s) {
    float z = 0.f;
    if (s < S) {
      const float v = at(s);
      z = !standardize ? v : is_const ? 0.f : (float)(((double)v - m) / dev);
    }
    const __bf16 b0 = (__bf16)z;                        // round to nearest even
    const float r1 = z - (float)b0;                     // exact: the residual of an 8-bit rounding of a 24-bit value
    const __bf16 b1 = (__bf16)r1;
    const float r2 = r1 - (float)b1;                    // exact
    const __bf16 b2 = (__bf16)r2;
    ph[s] = pt_bits(b0);
    ph[plane + s] = pt_bits(b1);
    ph[2 * plane + s] = pt_bits(b2);
  }
}

// ---- the product and its epilogue --------------------------------------------------------------------------------------
// Grid (row tiles, column tiles): the workgroups in flight share the column tiles of the planes and all of member.
// Wave w owns rows 32 w .. 32 w + 31 of the tile (two A fragments) and all 64 columns (four B fragments):
//   acc[a][b][r] = G[m0 + 32 w + 16 a + 4 (lane >> 4) + r][n0 + 16 b + (lane & 15)]
// member is staged one row half (16 bytes) per thread: as one 16-byte load when every row of member starts 16-byte
// aligned (ldm % 16 == 0 and an aligned base; the bytes behind S of a row are then inside the row's stride), else byte
// by byte; both give the same LDS image.
struct PtStage {
  uint4 a;                                              // 16 member bytes
  uint4 b[3];                                           // 8 bf16 of each plane
};

__device__ __forceinline__ void pt_load(PtStage& st, const uint8_t* __restrict__ member, int64_t ldm, bool vec, int P,
                                        int S, int m0, const unsigned short* __restrict__ planes, size_t plane, int Sp,
                                        int n0, int k0, int tid) {
  const int ar = tid >> 1, ak = k0 + (tid & 1) * 16;
  const int p = m0 + ar;
  st.a = make_uint4(0u, 0u, 0u, 0u);
  if (p < P && ak < S) {
    const uint8_t* src = member + (int64_t)p * ldm + ak;
    if (vec) {
      st.a = *reinterpret_cast<const uint4*>(src);
    } else {
      unsigned w[4] = {0u, 0u, 0u, 0u};
      const int n = S - ak < 16 ? S - ak : 16;
      for (int j = 0; j < n; ++j) w[j >> 2] |= (unsigned)src[j] << (8 * (j & 3));
      st.a = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  const int br = tid >> 2, bk = k0 + (tid & 3) * 8;      // (Ep, Sp are whole tiles: no bound to check)
  const unsigned short* src = planes + (size_t)(n0 + br) * Sp + bk;
#pragma unroll
  for (int q = 0; q < 3; ++q) st.b[q] = *reinterpret_cast<const uint4*>(src + q * plane);
}

__device__ __forceinline__ void pt_store_planes(const PtStage& st, unsigned short (*Bs)[PT_BN][PT_LD], int tid) {
  const int br = tid >> 2, bk = (tid & 3) * 8;
#pragma unroll
  for (int q = 0; q < 3; ++q) *reinterpret_cast<uint4*>(&Bs[q][br][bk]) = st.b[q];
}

__device__ __forceinline__ void pt_store(const PtStage& st, unsigned short (*As)[PT_LD],
                                         unsigned short (*Bs)[PT_BN][PT_LD], int S, int k0, int tid) {
  const int ar = tid >> 1, ah = (tid & 1) * 16, ak = k0 + ah;
  const unsigned w[4] = {st.a.x, st.a.y, st.a.z, st.a.w};
  unsigned o[8];
#pragma unroll
  for (int j = 0; j < 16; j += 2) {                     // member byte -> bf16 0.0 / 1.0 (0x3F80); nothing behind S
    const unsigned lo = ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) && ak + j < S ? 0x3F80u : 0u;
    const unsigned hi = ((w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu) && ak + j + 1 < S ? 0x3F80u : 0u;
    o[j >> 1] = lo | (hi << 16);
  }
  uint4* ad = reinterpret_cast<uint4*>(&As[ar][ah]);
  ad[0] = make_uint4(o[0], o[1], o[2], o[3]);
  ad[1] = make_uint4(o[4], o[5], o[6], o[7]);
  pt_store_planes(st, Bs, tid);
}

__global__ void __launch_bounds__(PT_T)
k_perm_maxsum(int P, int S, int E, int Sp, const uint8_t* __restrict__ member, int64_t ldm, int vec,
              const unsigned short* __restrict__ planes, size_t plane, const float* __restrict__ g_obs,
              float* __restrict__ pmax, int tiles_e, int32_t* __restrict__ pcnt, float* __restrict__ g) {
  __shared__ __attribute__((aligned(16))) unsigned short As[2][PT_BM][PT_LD];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[2][3][PT_BN][PT_LD];
  __shared__ int cnt_s[PT_T / 64][PT_BN];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.x * PT_BM, n0 = blockIdx.y * PT_BN;

  pt_f32x4 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (pt_f32x4){0.f, 0.f, 0.f, 0.f};

  PtStage st;
  pt_load(st, member, ldm, vec != 0, P, S, m0, planes, plane, Sp, n0, 0, tid);
  pt_store(st, As[0], Bs[0], S, 0, tid);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < Sp; k0 += PT_BK) {
    const bool more = k0 + PT_BK < Sp;
    if (more) pt_load(st, member, ldm, vec != 0, P, S, m0, planes, plane, Sp, n0, k0 + PT_BK, tid);
    pt_bf16x8 fa[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) fa[a] = *reinterpret_cast<const pt_bf16x8*>(&As[buf][w * 32 + a * 16 + lr][lg * 8]);
#pragma unroll
    for (int q = 0; q < 3; ++q)                         // planes hi, mid, lo into the same accumulators
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const pt_bf16x8 fb = *reinterpret_cast<const pt_bf16x8*>(&Bs[buf][q][b * 16 + lr][lg * 8]);
#pragma unroll
        for (int a = 0; a < 2; ++a) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], fb, acc[a][b], 0, 0, 0);
      }
    if (more) pt_store(st, As[buf ^ 1], Bs[buf ^ 1], S, k0 + PT_BK, tid);
    __syncthreads();
    buf ^= 1;
  }

  // ---- epilogue: G stays in registers ----
  const int prow = m0 + w * 32 + lg * 4;                // + 16 a + r
  if (g_obs == nullptr) {                               // the observed pass: G itself, P <= IGCN_PERM_MAX_G_ROWS
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = prow + 16 * a + r, e = n0 + 16 * b + lr;
          if (p < P && e < E) g[(size_t)p * E + e] = acc[a][b][r];
        }
  }
  // maxabs partial: over the tile's real columns, for each of the lane's 8 rows; lanes of one 16-group hold the columns
  float mx[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = 0.f;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (n0 + 16 * b + lr < E) v = fmaxf(v, fabsf(acc[a][b][r]));
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
      mx[a][r] = v;
    }
  if (lr == 0) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = prow + 16 * a + r;
        if (p < P) pmax[(size_t)p * tiles_e + blockIdx.y] = mx[a][r];
      }
  }
  if (g_obs != nullptr) {                               // exceedance partial: over the tile's real rows, per column
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int e = n0 + 16 * b + lr;
      const float thr = e < E ? fabsf(g_obs[e]) : 0.f;
      int c = 0;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) c += (prow + 16 * a + r < P && fabsf(acc[a][b][r]) >= thr) ? 1 : 0;
      c += __shfl_xor(c, 16, 64);
      c += __shfl_xor(c, 32, 64);
      if (lg == 0) cnt_s[w][16 * b + lr] = c;
    }
    __syncthreads();
    if (tid < PT_BN && n0 + tid < E)
      pcnt[(size_t)blockIdx.x * E + n0 + tid] = cnt_s[0][tid] + cnt_s[1][tid] + cnt_s[2][tid] + cnt_s[3][tid];
  }
}

// ---- suprathreshold bits: the network-based statistic's first half ----------------------------------------------------------
// The tile and the main loop of k_perm_maxsum (the accumulators hold the bits igcn_perm_maxsum writes to g), and an
// epilogue that keeps ONE BIT per (relabelling, entry): bit e & 31 of word e >> 5 of row p is set iff tested[e] and
// v >= thr, v = |G| (tail 0), G (tail +1) or -G (tail -1).  For one accumulator register (a, b, r) a wave-wide ballot
// holds four 16-bit pieces, piece lane >> 4 the 16 columns of fragment b of row 16 a + 4 (lane >> 4) + r; the four b
// pieces of a row are the tile's two words.  Lane (lg, lr = 4 a + r) keeps them, so lanes lr < 8 store the wave's 32
// rows at once: one writer per word, no atomics, no scratch, and no LDS beyond the staging buffers.  The block of the
// last column tile also clears the words of its rows between Ep / 32 and ldw.
__global__ void __launch_bounds__(PT_T)
k_perm_supra(int P, int S, int E, int Sp, const uint8_t* __restrict__ member, int64_t ldm, int vec,
             const unsigned short* __restrict__ planes, size_t plane, float thr, int tail,
             const uint8_t* __restrict__ tested, unsigned* __restrict__ bits, int64_t ldw) {
  __shared__ __attribute__((aligned(16))) unsigned short As[2][PT_BM][PT_LD];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[2][3][PT_BN][PT_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.x * PT_BM, n0 = blockIdx.y * PT_BN;

  pt_f32x4 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (pt_f32x4){0.f, 0.f, 0.f, 0.f};

  PtStage st;
  pt_load(st, member, ldm, vec != 0, P, S, m0, planes, plane, Sp, n0, 0, tid);
  pt_store(st, As[0], Bs[0], S, 0, tid);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < Sp; k0 += PT_BK) {
    const bool more = k0 + PT_BK < Sp;
    if (more) pt_load(st, member, ldm, vec != 0, P, S, m0, planes, plane, Sp, n0, k0 + PT_BK, tid);
    pt_bf16x8 fa[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) fa[a] = *reinterpret_cast<const pt_bf16x8*>(&As[buf][w * 32 + a * 16 + lr][lg * 8]);
#pragma unroll
    for (int q = 0; q < 3; ++q)                         // planes hi, mid, lo into the same accumulators
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const pt_bf16x8 fb = *reinterpret_cast<const pt_bf16x8*>(&Bs[buf][q][b * 16 + lr][lg * 8]);
#pragma unroll
        for (int a = 0; a < 2; ++a) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], fb, acc[a][b], 0, 0, 0);
      }
    if (more) pt_store(st, As[buf ^ 1], Bs[buf ^ 1], S, k0 + PT_BK, tid);
    __syncthreads();
    buf ^= 1;
  }

  // ---- epilogue: G stays in registers, one bit of it leaves ----
  bool on[4];                                           // the lane's four columns: real and tested
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int e = n0 + 16 * b + lr;
    on[b] = e < E && tested[e] != 0;
  }
  const float sgn = (float)tail;                        // (+-1: the product is exact)
  unsigned w0 = 0u, w1 = 0u;                            // the two words of row 16 a + 4 lg + r, kept by lane lr = 4 a + r
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned piece[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float x = acc[a][b][r];
        const float v = tail == 0 ? fabsf(x) : sgn * x;
        const unsigned long long m = __ballot(on[b] && v >= thr);
        piece[b] = (unsigned)(m >> (16 * lg)) & 0xFFFFu;
      }
      if (lr == 4 * a + r) {
        w0 = piece[0] | (piece[1] << 16);
        w1 = piece[2] | (piece[3] << 16);
      }
    }
  const int p = m0 + w * 32 + 16 * (lr >> 2) + 4 * lg + (lr & 3);
  if (lr < 8 && p < P) {
    unsigned* row = bits + (int64_t)p * ldw;
    row[2 * blockIdx.y] = w0;
    row[2 * blockIdx.y + 1] = w1;
    if (blockIdx.y == gridDim.y - 1)
      for (int64_t x = 2 * (int64_t)gridDim.y; x < ldw; ++x) row[x] = 0u;
  }
}

// maxabs[p] = max_t pmax[p][t], tiles ascending
__global__ void __launch_bounds__(256)
k_perm_fold_max(int P, int tiles_e, const float* __restrict__ pmax, float* __restrict__ maxabs) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const float* src = pmax + (size_t)p * tiles_e;
  float v = 0.f;
  for (int t = 0; t < tiles_e; ++t) v = fmaxf(v, src[t]);
  maxabs[p] = v;
}

// exceed[e] = sum_t pcnt[t][e], tiles ascending
__global__ void __launch_bounds__(256)
k_perm_fold_cnt(int E, int tiles_p, const int32_t* __restrict__ pcnt, int32_t* __restrict__ exceed) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  int32_t c = 0;
  for (int t = 0; t < tiles_p; ++t) c += pcnt[(size_t)t * E + e];
  exceed[e] = c;
}

// ---- K groups: the max-F product and its epilogue ------------------------------------------------------------------------
// labels [P, S] uint8: byte g puts the subject in group g of the relabelling.  For the NG = K - 1 accumulated groups
//   G_g[p, e] = sum_s (labels[p, s] == g) z[s, e]
// on the same tile as k_perm_maxsum: wave w owns rows 32 w .. 32 w + 31 and all 64 columns, for every group,
//   acc[g][a][b][r] = G_g[m0 + 32 w + 16 a + 4 (lane >> 4) + r][n0 + 16 b + (lane & 15)].
// The label bytes stay RAW in LDS (PF_LDL bytes a row) and a lane widens the 8 bytes of its A fragment into NG
// fragments of bf16 0.0 / 1.0 in registers, so LDS does not grow with NG and every B fragment is read once for all
// 2 NG accumulators it feeds.  Rows behind P and bytes behind S are staged as PF_NONE, which is no group.
// The statistic, with the last group's sum DEFINED as minus the sum of the others (the column sum of the fp32 z is
// zero only to rounding):  B = sum_{g < NG} w_g G_g^2 + w_NG (sum_{g < NG} G_g)^2, in fp32, g ascending, the last term
// last.  With w_g = 1 / n_g this is the between-groups sum of squares, every column's total is S, and
// F = (B / (K - 1)) / ((S - B) / (S - K)) is ONE increasing function of B: comparing B is comparing F.
// maxstat[p] = max_e B[p, e] and exceed[e] = #{p : B[p, e] >= b_obs[e]} through the partials and folds of k_perm_maxsum.
#define PF_LDL 48                                      // LDS label row: 32 bytes + 16 pad (12 dwords: no bank conflicts)
#define PF_NONE 0xFFu

struct PfWeights {
  float w[IGCN_PERM_MAX_GROUPS];
};

__device__ __forceinline__ void pf_store(const PtStage& st, uint8_t (*Ls)[PF_LDL], unsigned short (*Bs)[PT_BN][PT_LD],
                                         bool row_ok, int S, int k0, int tid) {
  const int ar = tid >> 1, ah = (tid & 1) * 16;
  int n = row_ok ? S - (k0 + ah) : 0;                   // label bytes of this half that are real
  n = n < 0 ? 0 : n > 16 ? 16 : n;
  unsigned w[4] = {st.a.x, st.a.y, st.a.z, st.a.w};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int nv = n - 4 * d;
    const unsigned keep = nv >= 4 ? 0xFFFFFFFFu : nv <= 0 ? 0u : (1u << (8 * nv)) - 1u;
    w[d] = (w[d] & keep) | ~keep;                       // PF_NONE in every byte behind S
  }
  *reinterpret_cast<uint4*>(&Ls[ar][ah]) = make_uint4(w[0], w[1], w[2], w[3]);
  pt_store_planes(st, Bs, tid);
}

// the A fragment of group g from 8 label bytes: bf16 1.0 (0x3F80) where the byte is g
__device__ __forceinline__ pt_bf16x8 pf_widen(uint2 l, unsigned g) {
  const unsigned w[2] = {l.x, l.y};
  unsigned o[4];
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const unsigned lo = ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) == g ? 0x3F80u : 0u;
    const unsigned hi = ((w[j >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu) == g ? 0x3F80u : 0u;
    o[j >> 1] = lo | (hi << 16);
  }
  return __builtin_bit_cast(pt_bf16x8, make_uint4(o[0], o[1], o[2], o[3]));
}

template <int NG>
__global__ void __launch_bounds__(PT_T, 2)              // two waves a SIMD: NG = 4 then fits 208 registers, no spill
k_perm_maxf(int P, int S, int E, int Sp, const uint8_t* __restrict__ labels, int64_t ldl, int vec,
            const unsigned short* __restrict__ planes, size_t plane, PfWeights wt, const float* __restrict__ b_obs,
            float* __restrict__ pmax, int tiles_e, int32_t* __restrict__ pcnt, float* __restrict__ b,
            float* __restrict__ g) {
  __shared__ __attribute__((aligned(16))) uint8_t Ls[2][PT_BM][PF_LDL];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[2][3][PT_BN][PT_LD];
  __shared__ int cnt_s[PT_T / 64][PT_BN];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.x * PT_BM, n0 = blockIdx.y * PT_BN;
  const bool row_ok = m0 + (tid >> 1) < P;              // the row this thread stages

  pt_f32x4 acc[NG][2][4];
#pragma unroll
  for (int q = 0; q < NG; ++q)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[q][a][c] = (pt_f32x4){0.f, 0.f, 0.f, 0.f};

  PtStage st;
  pt_load(st, labels, ldl, vec != 0, P, S, m0, planes, plane, Sp, n0, 0, tid);
  pf_store(st, Ls[0], Bs[0], row_ok, S, 0, tid);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < Sp; k0 += PT_BK) {
    const bool more = k0 + PT_BK < Sp;
    if (more) pt_load(st, labels, ldl, vec != 0, P, S, m0, planes, plane, Sp, n0, k0 + PT_BK, tid);
    pt_bf16x8 fa[NG][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const uint2 l = *reinterpret_cast<const uint2*>(&Ls[buf][w * 32 + a * 16 + lr][lg * 8]);
#pragma unroll
      for (int q = 0; q < NG; ++q) fa[q][a] = pf_widen(l, (unsigned)q);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)                         // planes hi, mid, lo into the same accumulators
#pragma unroll
      for (int c = 0; c < 4; ++c) {                     // one read of a B fragment feeds all 2 NG accumulators
        const pt_bf16x8 fb = *reinterpret_cast<const pt_bf16x8*>(&Bs[buf][q][c * 16 + lr][lg * 8]);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi)
#pragma unroll
          for (int a = 0; a < 2; ++a)
            acc[gi][a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[gi][a], fb, acc[gi][a][c], 0, 0, 0);
      }
    if (more) pf_store(st, Ls[buf ^ 1], Bs[buf ^ 1], row_ok, S, k0 + PT_BK, tid);
    __syncthreads();
    buf ^= 1;
  }

  // ---- epilogue: the group sums and B stay in registers ----
  const int prow = m0 + w * 32 + lg * 4;                // + 16 a + r
  if (b_obs == nullptr && g != nullptr) {               // the observed pass: the sums themselves, g [P, NG, E]
#pragma unroll
    for (int gi = 0; gi < NG; ++gi)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int p = prow + 16 * a + r, e = n0 + 16 * c + lr;
            if (p < P && e < E) g[((size_t)p * NG + gi) * E + e] = acc[gi][a][c][r];
          }
  }
  pt_f32x4 bv[2][4];                                    // B: g ascending, the last group's term last
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sum = acc[0][a][c][r];
        float v = wt.w[0] * sum * sum;
#pragma unroll
        for (int gi = 1; gi < NG; ++gi) {
          const float x = acc[gi][a][c][r];
          v += wt.w[gi] * x * x;
          sum += x;
        }
        v += wt.w[NG] * sum * sum;
        bv[a][c][r] = v;
      }
  if (b_obs == nullptr) {                               // the observed pass: B itself, P <= IGCN_PERM_MAX_G_ROWS
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = prow + 16 * a + r, e = n0 + 16 * c + lr;
          if (p < P && e < E) b[(size_t)p * E + e] = bv[a][c][r];
        }
  }
  // max partial: over the tile's real columns, for each of the lane's 8 rows; lanes of one 16-group hold the columns
  float mx[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (n0 + 16 * c + lr < E) v = fmaxf(v, bv[a][c][r]);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
      mx[a][r] = v;
    }
  if (lr == 0) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = prow + 16 * a + r;
        if (p < P) pmax[(size_t)p * tiles_e + blockIdx.y] = mx[a][r];
      }
  }
  if (b_obs != nullptr) {                               // exceedance partial: over the tile's real rows, per column
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int e = n0 + 16 * c + lr;
      const float thr = e < E ? b_obs[e] : 0.f;
      int n = 0;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) n += (prow + 16 * a + r < P && bv[a][c][r] >= thr) ? 1 : 0;
      n += __shfl_xor(n, 16, 64);
      n += __shfl_xor(n, 32, 64);
      if (lg == 0) cnt_s[w][16 * c + lr] = n;
    }
    __syncthreads();
    if (tid < PT_BN && n0 + tid < E)
      pcnt[(size_t)blockIdx.x * E + n0 + tid] = cnt_s[0][tid] + cnt_s[1][tid] + cnt_s[2][tid] + cnt_s[3][tid];
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
static bool pt_sizes_ok(int S, int E) {
  return S >= IGCN_PERM_MIN_S && S <= IGCN_PERM_MAX_S && E >= 1 && E <= IGCN_PERM_MAX_E;
}

extern "C" size_t igcn_perm_planes_bytes(int S, int E) {
  if (!pt_sizes_ok(S, E)) return 0;
  return (size_t)3 * pt_ep(E) * pt_sp(S) * sizeof(unsigned short);
}

extern "C" int igcn_perm_plane_dims(int S, int E, int* dims) {
  IGCN_REQUIRE(dims != nullptr, "perm_plane_dims: dims is null");
  IGCN_REQUIRE(pt_sizes_ok(S, E), "perm_plane_dims: S=%d outside [%d,%d] or E=%d outside [1,%d]", S, IGCN_PERM_MIN_S,
               IGCN_PERM_MAX_S, E, IGCN_PERM_MAX_E);
  dims[0] = pt_ep(E);
  dims[1] = pt_sp(S);
  return IGCN_OK;
}

extern "C" int igcn_perm_prepare(int64_t S_all, int S, int E, const float* x, const int64_t* rows, int standardize,
                                 double* mean, double* sd, uint8_t* constant, void* planes, void* stream) {
  const char* who = "perm_prepare";
  IGCN_REQUIRE(S >= IGCN_PERM_MIN_S && S <= IGCN_PERM_MAX_S, "%s: S=%d subjects outside [%d,%d]", who, S, IGCN_PERM_MIN_S,
               IGCN_PERM_MAX_S);
  IGCN_REQUIRE(E >= 1 && E <= IGCN_PERM_MAX_E, "%s: E=%d map entries outside [1,%d]", who, E, IGCN_PERM_MAX_E);
  IGCN_REQUIRE(S_all >= 1, "%s: S_all=%lld rows in the table", who, (long long)S_all);
  IGCN_REQUIRE(x && rows && mean && sd && constant && planes, "%s: a null buffer", who);
  IGCN_REQUIRE(((uintptr_t)planes & 15) == 0, "%s: the planes must be 16-byte aligned", who);
  const int Ep = pt_ep(E), Sp = pt_sp(S);
  hipLaunchKernelGGL(k_perm_prepare, dim3((Ep + 255) / 256), dim3(256), 0, (hipStream_t)stream, S_all, S, E, Ep, Sp, x,
                     rows, standardize, mean, sd, constant, (unsigned short*)planes);
  IGCN_CHECK_LAUNCH(who);
  return IGCN_OK;
}

extern "C" size_t igcn_perm_maxsum_scratch_bytes(int P, int E) {
  if (P < 1 || P > IGCN_PERM_MAX_P || E < 1 || E > IGCN_PERM_MAX_E) return 0;
  const size_t tiles_p = (P + PT_BM - 1) / PT_BM, tiles_e = (E + PT_BN - 1) / PT_BN;
  return (size_t)P * tiles_e * sizeof(float) + tiles_p * (size_t)E * sizeof(int32_t);
}

extern "C" int igcn_perm_maxsum(int P, int S, int E, const uint8_t* member, int64_t ldm, const void* planes,
                                const float* g_obs, float* maxabs, int32_t* exceed, float* g, void* scratch,
                                size_t scratch_bytes, void* stream) {
  const char* who = "perm_maxsum";
  IGCN_REQUIRE(S >= IGCN_PERM_MIN_S && S <= IGCN_PERM_MAX_S, "%s: S=%d subjects outside [%d,%d]", who, S, IGCN_PERM_MIN_S,
               IGCN_PERM_MAX_S);
  IGCN_REQUIRE(E >= 1 && E <= IGCN_PERM_MAX_E, "%s: E=%d map entries outside [1,%d]", who, E, IGCN_PERM_MAX_E);
  IGCN_REQUIRE(P >= 1 && P <= IGCN_PERM_MAX_P, "%s: P=%d relabellings in one launch outside [1,%d]", who, P,
               IGCN_PERM_MAX_P);
  IGCN_REQUIRE(ldm >= S, "%s: member row stride %lld below S=%d", who, (long long)ldm, S);
  IGCN_REQUIRE(member && planes && maxabs && scratch, "%s: a null buffer", who);
  if (g_obs) {
    IGCN_REQUIRE(exceed != nullptr, "%s: g_obs without an exceed buffer", who);
  } else {
    IGCN_REQUIRE(g != nullptr && P <= IGCN_PERM_MAX_G_ROWS, "%s: without g_obs the call writes g itself, for P <= %d (P=%d)",
                 who, IGCN_PERM_MAX_G_ROWS, P);
  }
  IGCN_REQUIRE(((uintptr_t)planes & 15) == 0 && ((uintptr_t)scratch & 15) == 0,
               "%s: the planes and the scratch must be 16-byte aligned", who);
  const size_t need = igcn_perm_maxsum_scratch_bytes(P, E);
  if (scratch_bytes < need) {
    igcn_set_error("%s: the scratch holds %zu bytes, P=%d E=%d needs %zu bytes", who, scratch_bytes, P, E, need);
    return IGCN_ERR_UNSUPPORTED;
  }
  const int Ep = pt_ep(E), Sp = pt_sp(S);
  const int tiles_p = (P + PT_BM - 1) / PT_BM, tiles_e = Ep / PT_BN;
  float* pmax = (float*)scratch;
  int32_t* pcnt = (int32_t*)(pmax + (size_t)P * tiles_e);
  const int vec = (ldm % 16 == 0 && ((uintptr_t)member & 15) == 0) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_perm_maxsum, dim3(tiles_p, tiles_e), dim3(PT_T), 0, st, P, S, E, Sp, member, ldm, vec,
                     (const unsigned short*)planes, (size_t)Ep * Sp, g_obs, pmax, tiles_e, pcnt, g);
  hipLaunchKernelGGL(k_perm_fold_max, dim3((P + 255) / 256), dim3(256), 0, st, P, tiles_e, pmax, maxabs);
  if (g_obs)
    hipLaunchKernelGGL(k_perm_fold_cnt, dim3((E + 255) / 256), dim3(256), 0, st, E, tiles_p, pcnt, exceed);
  IGCN_CHECK_LAUNCH(who);
  return IGCN_OK;
}

extern "C" int igcn_perm_supra(int P, int S, int E, const uint8_t* member, int64_t ldm, const void* planes, float thr,
                               int tail, const uint8_t* tested, void* bits, int64_t ldw, void* stream) {
  const char* who = "perm_supra";
  IGCN_REQUIRE(S >= IGCN_PERM_MIN_S && S <= IGCN_PERM_MAX_S, "%s: S=%d subjects outside [%d,%d]", who, S, IGCN_PERM_MIN_S,
               IGCN_PERM_MAX_S);
  IGCN_REQUIRE(E >= 1 && E <= IGCN_PERM_MAX_E, "%s: E=%d map entries outside [1,%d]", who, E, IGCN_PERM_MAX_E);
  IGCN_REQUIRE(P >= 1 && P <= IGCN_PERM_MAX_P, "%s: P=%d relabellings in one launch outside [1,%d]", who, P,
               IGCN_PERM_MAX_P);
  IGCN_REQUIRE(ldm >= S, "%s: member row stride %lld below S=%d", who, (long long)ldm, S);
  IGCN_REQUIRE(member && planes && tested && bits, "%s: a null buffer", who);
  IGCN_REQUIRE(isfinite(thr) && thr > 0.f, "%s: the threshold is %g (finite and > 0)", who, (double)thr);
  IGCN_REQUIRE(tail >= -1 && tail <= 1, "%s: tail=%d (-1, 0 or 1)", who, tail);
  const int Ep = pt_ep(E), Sp = pt_sp(S);
  IGCN_REQUIRE(ldw >= Ep / 32, "%s: bits row stride %lld words below %d (E=%d rounded up to %d, 32 entries a word)", who,
               (long long)ldw, Ep / 32, E, PT_BN);
  IGCN_REQUIRE(((uintptr_t)planes & 15) == 0 && ((uintptr_t)bits & 15) == 0,
               "%s: the planes and the bits must be 16-byte aligned", who);
  const int tiles_p = (P + PT_BM - 1) / PT_BM, tiles_e = Ep / PT_BN;
  const int vec = (ldm % 16 == 0 && ((uintptr_t)member & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_perm_supra, dim3(tiles_p, tiles_e), dim3(PT_T), 0, (hipStream_t)stream, P, S, E, Sp, member, ldm,
                     vec, (const unsigned short*)planes, (size_t)Ep * Sp, thr, tail, tested, (unsigned*)bits, ldw);
  IGCN_CHECK_LAUNCH(who);
  return IGCN_OK;
}

template <int NG>
static void pf_launch(dim3 grid, hipStream_t st, int P, int S, int E, int Sp, const uint8_t* labels, int64_t ldl, int vec,
                      const unsigned short* planes, size_t plane, const PfWeights& wt, const float* b_obs, float* pmax,
                      int tiles_e, int32_t* pcnt, float* b, float* g) {
  hipLaunchKernelGGL(k_perm_maxf<NG>, grid, dim3(PT_T), 0, st, P, S, E, Sp, labels, ldl, vec, planes, plane, wt, b_obs,
                     pmax, tiles_e, pcnt, b, g);
}

extern "C" int igcn_perm_maxf(int P, int S, int E, int K, const uint8_t* labels, int64_t ldl, const void* planes,
                              const float* weights, const float* b_obs, float* maxstat, int32_t* exceed, float* b,
                              float* g, void* scratch, size_t scratch_bytes, void* stream) {
  const char* who = "perm_maxf";
  IGCN_REQUIRE(S >= IGCN_PERM_MIN_S && S <= IGCN_PERM_MAX_S, "%s: S=%d subjects outside [%d,%d]", who, S, IGCN_PERM_MIN_S,
               IGCN_PERM_MAX_S);
  IGCN_REQUIRE(E >= 1 && E <= IGCN_PERM_MAX_E, "%s: E=%d map entries outside [1,%d]", who, E, IGCN_PERM_MAX_E);
  IGCN_REQUIRE(P >= 1 && P <= IGCN_PERM_MAX_P, "%s: P=%d relabellings in one launch outside [1,%d]", who, P,
               IGCN_PERM_MAX_P);
  IGCN_REQUIRE(K >= 2 && K <= IGCN_PERM_MAX_GROUPS, "%s: K=%d groups outside [2,%d]", who, K, IGCN_PERM_MAX_GROUPS);
  IGCN_REQUIRE(ldl >= S, "%s: labels row stride %lld below S=%d", who, (long long)ldl, S);
  IGCN_REQUIRE(labels && planes && weights && maxstat && scratch, "%s: a null buffer", who);
  PfWeights wt = {};
  for (int k = 0; k < K; ++k) {
    IGCN_REQUIRE(isfinite(weights[k]) && weights[k] > 0.f, "%s: weight %d is %g (finite and > 0)", who, k,
                 (double)weights[k]);
    wt.w[k] = weights[k];
  }
  if (b_obs) {
    IGCN_REQUIRE(exceed != nullptr, "%s: b_obs without an exceed buffer", who);
  } else {
    IGCN_REQUIRE(b != nullptr && P <= IGCN_PERM_MAX_G_ROWS, "%s: without b_obs the call writes b itself, for P <= %d (P=%d)",
                 who, IGCN_PERM_MAX_G_ROWS, P);
  }
  IGCN_REQUIRE(((uintptr_t)planes & 15) == 0 && ((uintptr_t)scratch & 15) == 0,
               "%s: the planes and the scratch must be 16-byte aligned", who);
  const size_t need = igcn_perm_maxsum_scratch_bytes(P, E);
  if (scratch_bytes < need) {
    igcn_set_error("%s: the scratch holds %zu bytes, P=%d E=%d needs %zu bytes", who, scratch_bytes, P, E, need);
    return IGCN_ERR_UNSUPPORTED;
  }
  const int Ep = pt_ep(E), Sp = pt_sp(S);
  const int tiles_p = (P + PT_BM - 1) / PT_BM, tiles_e = Ep / PT_BN;
  float* pmax = (float*)scratch;
  int32_t* pcnt = (int32_t*)(pmax + (size_t)P * tiles_e);
  const int vec = (ldl % 16 == 0 && ((uintptr_t)labels & 15) == 0) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(tiles_p, tiles_e);
  const unsigned short* pl = (const unsigned short*)planes;
  const size_t plane = (size_t)Ep * Sp;
  switch (K - 1) {
    case 1: pf_launch<1>(grid, st, P, S, E, Sp, labels, ldl, vec, pl, plane, wt, b_obs, pmax, tiles_e, pcnt, b, g); break;
    case 2: pf_launch<2>(grid, st, P, S, E, Sp, labels, ldl, vec, pl, plane, wt, b_obs, pmax, tiles_e, pcnt, b, g); break;
    case 3: pf_launch<3>(grid, st, P, S, E, Sp, labels, ldl, vec, pl, plane, wt, b_obs, pmax, tiles_e, pcnt, b, g); break;
    default: pf_launch<4>(grid, st, P, S, E, Sp, labels, ldl, vec, pl, plane, wt, b_obs, pmax, tiles_e, pcnt, b, g); break;
  }
  hipLaunchKernelGGL(k_perm_fold_max, dim3((P + 255) / 256), dim3(256), 0, st, P, tiles_e, pmax, maxstat);
  if (b_obs)
    hipLaunchKernelGGL(k_perm_fold_cnt, dim3((E + 255) / 256), dim3(256), 0, st, E, tiles_p, pcnt, exceed);
  IGCN_CHECK_LAUNCH(who);
  return IGCN_OK;
}
