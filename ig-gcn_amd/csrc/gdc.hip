// Graph-diffusion pre-transform of a batch of dense brain adjacencies, on the device:
//   util_gdc.py:7-15   get_ppr_matrix     P = alpha * (I - (1-alpha) * D^-1/2 A D^-1/2)^-1,  D = diag(row sums of A)
//   util_gdc.py:25-31  get_top_k_matrix   the k largest entries of every column, the column divided by their sum
//   util_gdc.py:82-86  coo_matrix(A_res)  non-zeros in row-major order, edge_index = [row; col], edge_attr = f32
// plus the block-diagonal node offset of Batch.from_data_list (batch.py:98-104): graph g's indices are shifted by g*R.
// The other kernel and the other sparsifier of util_gdc.py share the selection and the emission (igcn_gdc_diffuse):
//   util_gdc.py:16-23  get_heat_matrix     S = expm(-t (I - D^-1/2 A D^-1/2))            -> k_gdc_heat, further down
//   util_gdc.py:33-38  get_clipped_matrix  the entries >= eps, the column divided by their sum (R slots, not k)
// What exactly is kept and how it is emitted is the contract both routes share: csrc/gdc_common.h.
//
// The PPR kernel (k_gdc_ppr):
// One workgroup per graph; the R x R system lives in LDS in fp64 (the reference computes in numpy float64 and the
// top-k SELECTION must not flip on rounding), inverted in place by Gauss-Jordan elimination with partial pivoting.
//
// The elimination is a chain of R dependent rank-1 updates: its time is instruction issue and barriers, not arithmetic.
// Round 3 kept the matrix in LDS and spent five barriers and ~45 dependent LDS read-modify-writes per thread on every
// pivot (6.5 us per pivot, 590 us per batch of 256 graphs).  Now:
//   * the matrix lives in REGISTERS for the whole elimination — thread = (row slice i0, column jc) holds the NR
//     consecutive rows i0 NR .. i0 NR + NR - 1 of its column;
//   * rows are never swapped (implicit pivoting): the pivot of column p is the largest entry among the rows that have
//     not been a pivot yet (lowest row on ties), the working matrix W ends as P^-1 A^-1 P^-1 and is written back to LDS
//     through the two index maps, so the selection phases read the inverse itself;
//   * a pivot costs two barriers and ~3 instructions per row: (A) every WAVE finds the pivot for itself — lane l looks
//     at the multipliers of rows l and l + 64 (in LDS), a six-step wave maximum and a ballot give the largest
//     magnitude and its lowest row — and the slice that owns row r stages it in LDS; (B) every thread updates its
//     registers with one fma per row — the thread of column p, whose registers ARE the multipliers, gets the in-place
//     inverse column from the same fma with the factor 1 + 1/pivot — and the thread of column p + 1 leaves the next
//     multipliers in LDS.
#include "gdc_common.h"

#define GDC_T 256

__device__ __forceinline__ int gdc_ld(int R) { return R | 1; }      // odd row stride (in doubles)

// reg[kr] with a wave-uniform kr: a scalar switch (one taken branch) instead of NR compare-selects per access
#define GDC_ROWS(X)                                                                                                \
  X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20)  \
  X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32) X(33) X(34) X(35) X(36) X(37) X(38) X(39)    \
  X(40) X(41) X(42) X(43) X(44) X(45) X(46) X(47) X(48) X(49) X(50) X(51) X(52) X(53) X(54) X(55) X(56) X(57) X(58)    \
  X(59) X(60) X(61) X(62) X(63)
#define GDC_GET(K) case K: if constexpr (K < NR) v = reg[K]; break;
#define GDC_SET(K) case K: if constexpr (K < NR) reg[K] = newp; break;

#ifdef GDC_PROBE_ON
// phase stamps of workgroup 0, wave 0 (tools/gdc_probe.py, IGCN_HIPCC_EXTRA=-DGDC_PROBE_ON)
__device__ long long gdc_probe_buf[16];
#define GDC_PROBE(i)                                                                    \
  do {                                                                                  \
    if (threadIdx.x == 0 && blockIdx.x == 0) gdc_probe_buf[i] = wall_clock64();         \
  } while (0)
// inside the pivot loop: time since the previous stamp, accumulated per stage (wave 0 of workgroup 0)
#define GDC_LAP(i)                                                                      \
  do {                                                                                  \
    const long long now_ = wall_clock64();                                              \
    lap_[i] += now_ - last_;                                                            \
    last_ = now_;                                                                       \
  } while (0)
#define GDC_LAP_BEGIN long long lap_[6] = {0, 0, 0, 0, 0, 0}, last_ = wall_clock64()
#define GDC_LAP_END                                                                     \
  do {                                                                                  \
    if (threadIdx.x == 0 && blockIdx.x == 0)                                            \
      for (int q_ = 0; q_ < 6; ++q_) gdc_probe_buf[9 + q_] = lap_[q_];                  \
  } while (0)
extern "C" int igcn_debug_gdc_probe(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(gdc_probe_buf), sizeof(long long) * 16);
}
#else
#define GDC_PROBE(i)
#define GDC_LAP(i)
#define GDC_LAP_BEGIN
#define GDC_LAP_END
#endif

// ---- shared by the PPR and the heat kernel: what is kept of the diffusion matrix, and its COO image -----------------
// a graph that is not read (subject index outside the dataset): all slots padding, count 0
__device__ __forceinline__ void gdc_emit_empty(int g, int R, int cap, int64_t* __restrict__ ei_row,
                                               int64_t* __restrict__ ei_col, float* __restrict__ ew,
                                               int32_t* __restrict__ counts) {
  const int tid = threadIdx.x;
  const int64_t s0 = (int64_t)g * R * cap;
  for (int64_t t = s0 + tid; t < s0 + (int64_t)R * cap; t += GDC_T) {
    ei_row[t] = -1;
    ei_col[t] = -1;
    ew[t] = 0.f;
  }
  if (tid == 0) counts[g] = 0;
}

// Selection per column, column normalisation and COO emission of graph g.  M [R][ld] (LDS, fp64) holds the diffusion
// matrix up to the factor `scale` and is complete (a barrier lies behind its last write); rowmask [128][2] is zero;
// rowcnt [R+2].  Called by all GDC_T threads.  The contract (tie rule, threshold, padding): csrc/gdc_common.h.
__device__ __forceinline__ void gdc_select_emit(double* M, int ld, int R, double scale, GdcSparsify sp,
                                                unsigned long long* rowmask, int* rowcnt, int g,
                                                int64_t* __restrict__ ei_row, int64_t* __restrict__ ei_col,
                                                float* __restrict__ ew, int32_t* __restrict__ counts) {
  const int tid = threadIdx.x, k = sp.k;
  // ---- per column (thread = column): the rows that stay as a bit set, their final weights in place --------------
  unsigned long long tk0 = 0ull, tk1 = 0ull;           // rows of this column that stay
  if (tid < R) {
    const int j = tid;
    double norm = 0.0;
    if (sp.mode == IGCN_GDC_THRESHOLD) {
      // util_gdc.py:33-38: entries below eps are zeroed, the column is divided by the sum of the rest (rows ascending)
      for (int i = 0; i < R; ++i) {
        const double v = scale * M[i * ld + j];
        if (v >= sp.eps) {
          norm += v;
          if (i < 64) tk0 |= 1ull << i; else tk1 |= 1ull << (i - 64);
        }
      }
    } else if (k <= 4) {
      // one sweep with the best four in registers: rows arrive in ascending order, so a newcomer beats an equal value
      double v0 = -HUGE_VAL, v1 = -HUGE_VAL, v2 = -HUGE_VAL, v3 = -HUGE_VAL;
      int b0 = -1, b1 = -1, b2 = -1, b3 = -1;
#pragma unroll 4
      for (int i = 0; i < R; ++i) {
        const double v = scale * M[i * ld + j];
        if (v >= v3) {
          if (v >= v2) {
            v3 = v2; b3 = b2;
            if (v >= v1) {
              v2 = v1; b2 = b1;
              if (v >= v0) { v1 = v0; b1 = b0; v0 = v; b0 = i; } else { v1 = v; b1 = i; }
            } else { v2 = v; b2 = i; }
          } else { v3 = v; b3 = i; }
        }
      }
      const double vs[4] = {v0, v1, v2, v3};
      const int bs[4] = {b0, b1, b2, b3};
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
        if (s2 < k && bs[s2] >= 0) {
          norm += vs[s2];
          if (bs[s2] < 64) tk0 |= 1ull << bs[s2]; else tk1 |= 1ull << (bs[s2] - 64);
        }
    } else {
      for (int s2 = 0; s2 < k && s2 < R; ++s2) {
        double best = 0.0;
        int bi = -1;
        for (int i = 0; i < R; ++i) {
          const double v = scale * M[i * ld + j];
          const bool taken = ((i < 64 ? tk0 >> i : tk1 >> (i - 64)) & 1ull) != 0;
          if (!taken && (bi < 0 || v >= best)) { best = v; bi = i; }
        }
        if (bi < 64) tk0 |= 1ull << bi; else tk1 |= 1ull << (bi - 64);
        norm += best;
      }
    }
    const double den = (norm <= 0.0) ? 1.0 : norm;
    for (int h = 0; h < 2; ++h) {
      unsigned long long m = h ? tk1 : tk0;
      while (m) {
        const int i = h * 64 + __ffsll((long long)m) - 1;
        m &= m - 1;
        const double w = (scale * M[i * ld + j]) / den;
        M[i * ld + j] = w;
        if (w != 0.0) atomicOr(rowmask + 2 * i + (j >> 6), 1ull << (j & 63));     // (a kept 0 is not an edge)
      }
    }
  }
  __syncthreads();
  GDC_PROBE(6);
  // ---- COO emission in row-major order: slot = row start + edges of the row in lower columns ---------------------
  if (tid < R) rowcnt[tid] = __popcll(rowmask[2 * tid]) + __popcll(rowmask[2 * tid + 1]);
  __syncthreads();
  GDC_PROBE(7);
  const int64_t slot0 = (int64_t)g * R * sp.cap, off = (int64_t)g * R;
  int total = 0;
  for (int t = 0; t < R; ++t) total += rowcnt[t];       // (every thread for itself: R independent LDS reads)
  if (tid < R) {
    const int j = tid;
    int start = 0, upto = 0;                            // edges in the rows below `upto` (the kept rows come ascending)
    for (int h = 0; h < 2; ++h) {
      unsigned long long m = h ? tk1 : tk0;
      while (m) {
        const int i = h * 64 + __ffsll((long long)m) - 1;
        m &= m - 1;
        const double w = M[i * ld + j];
        if (w == 0.0) continue;
        for (; upto < i; ++upto) start += rowcnt[upto];
        const unsigned long long m0 = rowmask[2 * i], m1 = rowmask[2 * i + 1];
        const int before = j < 64 ? __popcll(m0 & ((1ull << j) - 1ull))
                                  : __popcll(m0) + __popcll(m1 & ((1ull << (j - 64)) - 1ull));
        const int64_t s2 = slot0 + start + before;
        ei_row[s2] = off + i;
        ei_col[s2] = off + j;
        ew[s2] = (float)w;
      }
    }
  }
  if (tid == 0) counts[g] = total;
  // padding behind the last edge of the graph
  for (int64_t s2 = slot0 + total + tid; s2 < slot0 + (int64_t)R * sp.cap; s2 += GDC_T) {
    ei_row[s2] = -1;
    ei_col[s2] = -1;
    ew[s2] = 0.f;
  }
}

template <int NR>                                       // rows of its column a thread keeps: NR * (GDC_T / cw) >= R
__global__ void __launch_bounds__(GDC_T)
k_gdc_ppr(int R, GdcSparsify sp, double alpha, const float* __restrict__ A, int64_t* __restrict__ ei_row,
          int64_t* __restrict__ ei_col, float* __restrict__ ew, int32_t* __restrict__ counts,
          const int64_t* __restrict__ subject, int64_t n_subjects) {
  extern __shared__ double smem_d[];
  const int ld = gdc_ld(R), g = blockIdx.x, tid = threadIdx.x;
  const int cw = R <= 64 ? 64 : 128, nsl = GDC_T / cw;  // a wave lies inside one row slice
  double* colf = smem_d;                                // [2][128]  multipliers (column p) of the current / next pivot
  double* rowP = colf + 2 * 128;                        // [128]  the pivot row
  double* cand = rowP + 128;                            // [128]  scale factors d^-1/2
  unsigned long long* rowmask = (unsigned long long*)(cand + 128);   // [128][2]  edges of row i as a column bit set
  unsigned long long* wmax = rowmask + 256;             // [GDC_T / 64]  per-wave slot of the pivot search
  double* M = (double*)(wmax + GDC_T / 64);             // [R][ld]
  int* piv = (int*)(M + (size_t)R * ld);                // [R]  row chosen as the pivot of column p
  int* rinv = piv + R;                                  // [R]  step at which row w was the pivot
  int* rowcnt = rinv + R;                               // [R+2]
  const int64_t sj = GDC_SUBJECT_OF(subject, g);
  if (GDC_NOT_READ(subject, sj, n_subjects)) {          // (uniform over the workgroup: no barrier has been reached yet)
    gdc_emit_empty(g, R, sp.cap, ei_row, ei_col, ew, counts);
    return;
  }
  const float* a = A + sj * R * R;

  GDC_PROBE(0);
  // ---- H = D^-1/2 A D^-1/2, M = I - (1 - alpha) H -------------------------------------------------
  for (int t = tid; t < R * R; t += GDC_T) {            // coalesced: A enters LDS once
    const int i = t / R, j = t - i * R;
    M[i * ld + j] = (double)a[t];
  }
  for (int t = tid; t < 3 * 128; t += GDC_T) colf[t] = 0.0;          // multiplier buffers and the staged row, padded
  for (int t = tid; t < 256 + GDC_T / 64; t += GDC_T) rowmask[t] = 0ull;
  __syncthreads();
  GDC_PROBE(1);
  for (int i = tid; i < R; i += GDC_T) {
    double s = 0.0;
    for (int j = 0; j < R; ++j) s += M[i * ld + j];
    cand[i] = 1.0 / sqrt(s);
  }
  __syncthreads();
  GDC_PROBE(2);

  // ---- Gauss-Jordan inversion in registers, implicit partial pivoting -------------------------------
  const int jc = tid & (cw - 1), lane = tid & 63;
  const int i0 = __builtin_amdgcn_readfirstlane(tid / cw);          // wave-uniform: row predicates are scalar
  const int base = i0 * NR;
  const bool col_ok = jc < R;
  double reg[NR];
#pragma unroll
  for (int kk = 0; kk < NR; ++kk) {
    const int i = base + kk;
    double v = 0.0;
    if (col_ok && i < R) {
      const double h = cand[i] * M[i * ld + jc] * cand[jc];
      v = (i == jc ? 1.0 : 0.0) - (1.0 - alpha) * h;
    }
    reg[kk] = v;
  }
  // the thread of column c leaves its column — the multipliers of pivot c — in LDS (16 bytes per store)
  auto publish = [&](double* dst) {
#pragma unroll
    for (int kk = 0; kk < NR; kk += 2)
      *reinterpret_cast<double2*>(dst + base + kk) = make_double2(reg[kk], reg[kk + 1]);
  };
  if (jc == 0) publish(colf);
  // rows l and l + 64 of this lane: available as pivots while in range and not used yet
  bool free0 = lane < R, free1 = lane + 64 < R;
  __syncthreads();
  GDC_PROBE(3);
  GDC_LAP_BEGIN;
  for (int p = 0; p < R; ++p) {
    const double* cf = colf + (p & 1) * 128;            // column p: the multipliers of this pivot
    double* cn = colf + ((p + 1) & 1) * 128;            // column p + 1 after this pivot's update
    // (A) the pivot, found by every wave for itself: largest |.| among the free rows, lowest row on ties
    // (non-negative doubles order like their bit patterns: ONE LDS atomic maximum per lane on the wave's own slot
    // instead of a six-step shuffle chain; LDS operations of a wave complete in order, so no barrier is involved)
    const double a0 = free0 ? fabs(cf[lane]) : -1.0, a1 = free1 ? fabs(cf[lane + 64]) : -1.0;
    const double am = a0 >= a1 ? a0 : a1;
    unsigned long long* slot = wmax + (tid >> 6);
    if (am >= 0.0) atomicMax(slot, (unsigned long long)__double_as_longlong(am));
    const double wm = __longlong_as_double((long long)*(volatile unsigned long long*)slot);
    if (lane == 0) *(volatile unsigned long long*)slot = 0ull;      // (behind the read above: ready for the next pivot)
    const unsigned long long lo = __ballot(a0 == wm), hi = __ballot(a1 == wm);
    const int r = lo ? __ffsll((long long)lo) - 1 : 64 + __ffsll((long long)hi) - 1;       // (wave-uniform)
    free0 = free0 && lane != r;
    free1 = free1 && lane + 64 != r;
    const int own = r / NR, kr = r - own * NR;
    const bool mine = own == i0;                        // this slice holds the pivot row
    GDC_LAP(0);
    if (mine) {
      double v = 0.0;
      switch (kr) { GDC_ROWS(GDC_GET) default: break; }
      rowP[jc] = v;
    }
    if (tid == 0) { piv[p] = r; rinv[r] = p; }
    GDC_LAP(1);
    __syncthreads();
    GDC_LAP(2);
    // (B) one fma per row.  Column p's thread: its registers equal the multipliers, reg - c (1 + inv) = -c inv
    {
      const double inv = 1.0 / rowP[p];
      const double newp = ((jc == p) ? 1.0 : rowP[jc]) * inv;       // the scaled pivot row (stays in row r)
      const double fac = (jc == p) ? 1.0 + inv : newp;
#pragma unroll
      for (int k0 = 0; k0 < NR; k0 += 8) {
        double2 c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)                     // independent 16-byte LDS reads (same address in every lane)
          c[u] = *reinterpret_cast<const double2*>(cf + base + k0 + 2 * u);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          reg[k0 + 2 * u] = fma(-c[u].x, fac, reg[k0 + 2 * u]);
          reg[k0 + 2 * u + 1] = fma(-c[u].y, fac, reg[k0 + 2 * u + 1]);
        }
      }
      if (mine) switch (kr) { GDC_ROWS(GDC_SET) default: break; }   // the pivot row itself: the scaled row
      GDC_LAP(3);
      if (jc == p + 1) publish(cn);
    }
    GDC_LAP(4);
    __syncthreads();
    GDC_LAP(5);
  }
  GDC_LAP_END;
  GDC_PROBE(4);
  // the inverse to LDS: A^-1[i][j] = W[piv[i]][rinv[j]], i.e. W[w][c] belongs at (rinv[w], piv[c])
  if (col_ok) {
    const int cj = piv[jc];
#pragma unroll
    for (int kk = 0; kk < NR; ++kk)
      if (base + kk < R) M[rinv[base + kk] * ld + cj] = reg[kk];
  }
  __syncthreads();

  GDC_PROBE(5);
  gdc_select_emit(M, ld, R, alpha, sp, rowmask, rowcnt, g, ei_row, ei_col, ew, counts);
  GDC_PROBE(8);
}

// ---- heat kernel (util_gdc.py:16-23): S = expm(-t (I - H)) = e^-t expm(t H),  H = D^-1/2 A D^-1/2 ------------------------
// One workgroup per graph, two fp64 matrices in LDS: X = t H / 2^s and the running T, both Rp x (Rp | 1) with
// Rp = R rounded up to 16 by zero rows and columns (their block of expm is the identity and touches nothing else).
// Scaling and squaring of a Taylor polynomial in Horner form:
//     T_m = I + X / m,   T_j = I + X T_(j+1) / j  (j = m-1 .. 1),   expm(t H) = T_1 ^ (2^s)
//   * s is chosen PER GRAPH: the smallest s >= 0 with |X|_1 = |t H|_1 / 2^s <= 1/2 (|.|_1: largest column sum);
//   * m = GDC_HEAT_DEGREE = 14: with theta = |X|_1 <= 1/2 the remainder is
//         sum_{j>m} theta^j / j!  <=  theta^(m+1) / (m+1)! / (1 - theta / (m+2))  <=  2.4e-17,
//     and X >= 0 entrywise gives |expm(X)|_1 >= 1, so the remainder is below 2^-53 = 1.1e-16 of the result's norm
//     (m = 13 leaves 7.2e-16).  All terms are non-negative: nothing cancels, and the factor e^-t (the `scale` of the
//     selection, applied where the matrix is read) never meets a subtraction.
// The m - 1 + s products are the hot path: v_mfma_f64_16x16x4_f64, the 2 x 2 waves each owning every other 16 x 16 tile
// in both directions (3 x 3 tiles at Rp = 96: three A and three B fragments feed nine MFMAs per k-step).  A product
// accumulates in registers while T is only read; T is rewritten behind a barrier and read again behind a second one.
typedef double gdc_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int gdc_heat_pad(int R) { return (R + 15) & ~15; }

// acc[a][b] = tile (wr + 2a, wc + 2b) of L * Rm   (both [Rp][ld] in LDS; nt = Rp / 16 tiles a side)
// operands of the f64 MFMA: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]
__device__ __forceinline__ void gdc_heat_mm(const double* L, const double* Rm, int ld, int nt, int wr, int wc, int lane,
                                            gdc_d4 (&acc)[3][3]) {
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) acc[a][b] = gdc_d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < nt * 16; k0 += 4) {
    double fa[3], fb[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int tr = wr + 2 * a;                        // (wave-uniform)
      fa[a] = tr < nt ? L[(tr * 16 + lr) * ld + k0 + lk] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int tc = wc + 2 * b;
      fb[b] = tc < nt ? Rm[(k0 + lk) * ld + tc * 16 + lr] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        if (wr + 2 * a < nt && wc + 2 * b < nt)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
  }
}

// T = eye * I + acc * mul, through the f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 reg
__device__ __forceinline__ void gdc_heat_store(double* T, int ld, int nt, int wr, int wc, int lane,
                                               const gdc_d4 (&acc)[3][3], double eye, double mul) {
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int tr = wr + 2 * a, tc = wc + 2 * b;
      if (tr < nt && tc < nt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = tr * 16 + lk + 4 * q, j = tc * 16 + lr;
          T[i * ld + j] = (i == j ? eye : 0.0) + acc[a][b][q] * mul;
        }
      }
    }
}

__global__ void __launch_bounds__(GDC_T)
k_gdc_heat(int R, GdcSparsify sp, double t, double exp_mt, const float* __restrict__ A, int64_t* __restrict__ ei_row,
           int64_t* __restrict__ ei_col, float* __restrict__ ew, int32_t* __restrict__ counts,
           const int64_t* __restrict__ subject, int64_t n_subjects) {
  extern __shared__ double smem_d[];
  const int Rp = gdc_heat_pad(R), ld = gdc_ld(Rp), nt = Rp >> 4, g = blockIdx.x, tid = threadIdx.x;
  double* dinv = smem_d;                                // [128]  scale factors d^-1/2
  double* csum = dinv + 128;                            // [128]  column sums of |t H|
  unsigned long long* rowmask = (unsigned long long*)(csum + 128);   // [128][2]  edges of row i as a column bit set
  double* X = (double*)(rowmask + 256);                 // [Rp][ld]
  double* T = X + (size_t)Rp * ld;                      // [Rp][ld]
  int* rowcnt = (int*)(T + (size_t)Rp * ld);            // [R+2]
  const int64_t sj = GDC_SUBJECT_OF(subject, g);
  if (GDC_NOT_READ(subject, sj, n_subjects)) {          // (uniform over the workgroup: no barrier has been reached yet)
    gdc_emit_empty(g, R, sp.cap, ei_row, ei_col, ew, counts);
    return;
  }
  const float* a = A + sj * R * R;

  // ---- X = t D^-1/2 A D^-1/2 / 2^s, zero padded ------------------------------------------------------
  for (int e = tid; e < Rp * Rp; e += GDC_T) {
    const int i = e / Rp, j = e - i * Rp;
    X[i * ld + j] = (i < R && j < R) ? (double)a[i * R + j] : 0.0;
  }
  for (int e = tid; e < 256; e += GDC_T) rowmask[e] = 0ull;
  __syncthreads();
  for (int i = tid; i < R; i += GDC_T) {
    double s = 0.0;
    for (int j = 0; j < R; ++j) s += X[i * ld + j];
    dinv[i] = 1.0 / sqrt(s);
  }
  __syncthreads();
  for (int e = tid; e < R * R; e += GDC_T) {
    const int i = e / R, j = e - i * R;
    X[i * ld + j] = t * (dinv[i] * X[i * ld + j] * dinv[j]);
  }
  __syncthreads();
  for (int j = tid; j < R; j += GDC_T) {
    double s = 0.0;
    for (int i = 0; i < R; ++i) s += fabs(X[i * ld + j]);
    csum[j] = s;
  }
  __syncthreads();
  double nrm = 0.0;
  for (int j = 0; j < R; ++j) nrm = fmax(nrm, csum[j]); // (every thread for itself: the same value in all of them)
  const int s = __builtin_amdgcn_readfirstlane(gdc_scaling_exponent(nrm, 64));
  const double down = ldexp(1.0, -s);
  for (int e = tid; e < Rp * Rp; e += GDC_T) {
    const int i = e / Rp, j = e - i * Rp;
    const double x = X[i * ld + j] * down;              // (a power of two: exact)
    X[i * ld + j] = x;
    T[i * ld + j] = (i == j ? 1.0 : 0.0) + x / (double)GDC_HEAT_DEGREE;
  }
  __syncthreads();

  // ---- Horner steps, then s squarings ------------------------------------------------------------------
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1;
  gdc_d4 acc[3][3];
  for (int j = GDC_HEAT_DEGREE - 1; j >= 1; --j) {
    gdc_heat_mm(X, T, ld, nt, wr, wc, lane, acc);
    __syncthreads();                                    // every wave has read T
    gdc_heat_store(T, ld, nt, wr, wc, lane, acc, 1.0, 1.0 / (double)j);
    __syncthreads();
  }
  for (int q = 0; q < s; ++q) {
    gdc_heat_mm(T, T, ld, nt, wr, wc, lane, acc);
    __syncthreads();
    gdc_heat_store(T, ld, nt, wr, wc, lane, acc, 0.0, 1.0);
    __syncthreads();
  }
  gdc_select_emit(T, ld, R, exp_mt, sp, rowmask, rowcnt, g, ei_row, ei_col, ew, counts);
}

static int gdc_rows(int R) {                            // NR of the kernel instance that serves R
  const int nsl = GDC_T / (R <= 64 ? 64 : 128);
  const int rows = (R + nsl - 1) / nsl;
  for (int nr : {8, 16, 24, 32, 48, 64})
    if (rows <= nr) return nr;
  return 0;
}

static size_t gdc_lds_bytes(int R) {
  const size_t ld = (size_t)(R | 1);
  size_t b = ((size_t)R * ld + 4 * 128 + 256 + GDC_T / 64) * sizeof(double);
  b += ((size_t)R + R + R + 2) * sizeof(int);
  return (b + 15) & ~(size_t)15;
}

extern "C" int igcn_gdc_topk_max_rois(void) {
  int r = 8;
  while (r < 128 && gdc_lds_bytes(r + 1) <= IGCN_LDS_MAX_BYTES) ++r;  // (128: two row slices of 64 register rows)
  return r;
}

static size_t gdc_heat_lds_bytes(int R) {
  const size_t rp = (size_t)((R + 15) & ~15), ld = rp | 1;
  const size_t b = (2 * rp * ld + 2 * 128 + 256) * sizeof(double) + ((size_t)R + 2) * sizeof(int);
  return (b + 15) & ~(size_t)15;
}

extern "C" int igcn_gdc_max_rois(int kernel) {
  if (kernel == IGCN_GDC_PPR) return igcn_gdc_topk_max_rois();
  if (kernel != IGCN_GDC_HEAT) return 0;
  int r = 16;
  while (r < 128 && gdc_heat_lds_bytes(r + 1) <= IGCN_LDS_MAX_BYTES) ++r;  // (128: the selection's row bit set)
  return r;
}

// `who`: the entry point, for messages
static int gdc_diffuse(const char* who, int B, int R, int kernel, double param, int sparsify, int k, double eps,
                       const float* A, const int64_t* subject, int64_t n_subjects, int64_t* edge_index,
                       float* edge_attr, int32_t* counts, void* stream) {
  const int bad = gdc_check_args(who, B, R, kernel, param, sparsify, k, eps, 0.0, 0, igcn_gdc_max_rois(kernel));
  if (bad != IGCN_OK || B == 0) return bad;
  const GdcSparsify sp = gdc_sparsify(sparsify, k, eps, R);
  const int64_t slots = (int64_t)B * R * sp.cap;
  if (kernel == IGCN_GDC_HEAT) {
    IGCN_ALLOW_BIG_LDS(k_gdc_heat);
    hipLaunchKernelGGL(k_gdc_heat, dim3(B), dim3(GDC_T), gdc_heat_lds_bytes(R), (hipStream_t)stream, R, sp, param,
                       exp(-param), A, edge_index, edge_index + slots, edge_attr, counts, subject, n_subjects);
    IGCN_CHECK_LAUNCH(who);
    return IGCN_OK;
  }
  const size_t lds = gdc_lds_bytes(R);
#define GDC_LAUNCH(NR)                                                                                              \
  case NR:                                                                                                          \
    IGCN_ALLOW_BIG_LDS(k_gdc_ppr<NR>);                                                                              \
    hipLaunchKernelGGL(k_gdc_ppr<NR>, dim3(B), dim3(GDC_T), lds, (hipStream_t)stream, R, sp, param, A, edge_index,   \
                       edge_index + slots, edge_attr, counts, subject, n_subjects);                                 \
    break
  switch (gdc_rows(R)) {
    GDC_LAUNCH(8);
    GDC_LAUNCH(16);
    GDC_LAUNCH(24);
    GDC_LAUNCH(32);
    GDC_LAUNCH(48);
    GDC_LAUNCH(64);
  }
#undef GDC_LAUNCH
  IGCN_CHECK_LAUNCH(who);
  return IGCN_OK;
}

extern "C" int igcn_gdc_topk(int B, int R, int k, double alpha, const float* A, int64_t* edge_index, float* edge_attr,
                             int32_t* counts, void* stream) {
  return gdc_diffuse("gdc_topk", B, R, IGCN_GDC_PPR, alpha, IGCN_GDC_TOPK, k, 0.0, A, nullptr, B, edge_index,
                     edge_attr, counts, stream);
}

extern "C" int igcn_gdc_topk_of(int B, int R, int k, double alpha, const float* A, int64_t n_subjects,
                                const int64_t* subject, int64_t* edge_index, float* edge_attr, int32_t* counts,
                                void* stream) {
  IGCN_REQUIRE(subject != nullptr && n_subjects > 0, "gdc_topk_of: the subject list is missing");
  return gdc_diffuse("gdc_topk", B, R, IGCN_GDC_PPR, alpha, IGCN_GDC_TOPK, k, 0.0, A, subject, n_subjects,
                     edge_index, edge_attr, counts, stream);
}

extern "C" int igcn_gdc_diffuse(int B, int R, int kernel, double param, int sparsify, int k, double eps, const float* A,
                                int64_t n_subjects, const int64_t* subject, int64_t* edge_index, float* edge_attr,
                                int32_t* counts, void* stream) {
  IGCN_REQUIRE(subject == nullptr || n_subjects > 0, "gdc_diffuse: a subject list needs n_subjects > 0");
  return gdc_diffuse("gdc_diffuse", B, R, kernel, param, sparsify, k, eps, A, subject, n_subjects, edge_index,
                     edge_attr, counts, stream);
}
