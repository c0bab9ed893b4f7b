// Column sums of partial rows: the stand-alone reductions and the ONE launch that performs every deferred final
// reduction of a stream (igcn_reduce_flush) — both built from the same bodies, so that both give the same bits.  Which
// entries wait for a flush is pending.h's business; this file takes them out and launches them.
#include "common.h"
#include "loss_final.h"
#include "pending.h"

__global__ void k_reduce_rows(const float* __restrict__ partial, int64_t rows, int64_t ld, int n,
                              float* __restrict__ out, int accumulate) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  float t = 0.f;
#pragma unroll 8
  for (int64_t r = 0; r < rows; ++r) t += partial[r * ld + j];     // independent loads: several in flight
  out[j] = accumulate ? out[j] + t : t;
}

// many rows AND many columns (split-K / per-workgroup partial rows of wide gradients): a thread per column walking all
// rows is a chain of `rows` dependent-latency loads (128 rows: 16 batches of 8 = the whole 16 us of the launch).  Four
// row groups per column (rows r = g mod 4), combined in the fixed order ((s0 + s1) + s2) + s3: 64 columns x 4 groups per
// 256-thread workgroup.  Shared by the stand-alone and the deferred reduction so that both give the same bits.
#define RR_WIDE_ROWS 32
// Which form sums `rows` partial rows of n columns — ONE rule for the stand-alone launches, the deferred launch and its
// workgroup count.  0: a thread per column, rows in order (few rows).  Tall (> 32 rows): 1 = a wave per column
// (n < 16), 2 = 16 x 16 tiles (n <= 4096, or >= 256 rows whatever the width: with four row groups a thread would walk
// rows / 4 dependent-latency loads — 512 per-sample rows of a LayerNorm's affine partials = 16 batches of 8), 3 = four
// row groups per column (32 < rows < 256 and wide: fewer, fatter workgroups).
__host__ __device__ inline int rr_form(int64_t rows, int n) {
  if (!(rows > RR_WIDE_ROWS)) return 0;
  if (n < 16) return 1;
  return (n <= 4096 || rows >= 256) ? 2 : 3;
}
__device__ __forceinline__ void reduce_cols_grouped(const float* __restrict__ partial, int64_t rows, int64_t ld, int n,
                                                    float* __restrict__ out, int accumulate, int64_t block,
                                                    float (*lds)[64]) {
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t j = block * 64 + c;
  float t = 0.f;
  if (j < n) {
#pragma unroll 8
    for (int64_t r = g; r < rows; r += 4) t += partial[r * ld + j];
  }
  lds[g][c] = t;
  __syncthreads();
  if (g == 0 && j < n) {
    const float v = ((lds[0][c] + lds[1][c]) + lds[2][c]) + lds[3][c];
    out[j] = accumulate ? out[j] + v : v;
  }
}
__global__ void __launch_bounds__(256)
k_reduce_rows_grouped(const float* __restrict__ partial, int64_t rows, int64_t ld, int n, float* __restrict__ out,
                      int accumulate) {
  __shared__ float lds[4][64];
  reduce_cols_grouped(partial, rows, ld, n, out, accumulate, blockIdx.x, lds);
}

// many rows, few columns: one WAVE per column (four columns per 256-thread workgroup): lanes stride the rows, fixed
// xor tree — no LDS, no barrier.  [A workgroup per column with a block-wide tree: 5 000 one-load workgroups in the
// deferred launch of a train step, whose cost was their dispatch.]  Shared by the stand-alone and the deferred form.
__device__ __forceinline__ void reduce_col_wave(const float* __restrict__ partial, int64_t rows, int64_t ld, int n,
                                                float* __restrict__ out, int accumulate, int64_t block) {
  const int lane = threadIdx.x & 63;
  const int64_t j = block * 4 + (threadIdx.x >> 6);
  if (j >= n) return;                                 // wave-uniform
  float t = 0.f;
#pragma unroll 4
  for (int64_t r = lane; r < rows; r += 64) t += partial[r * ld + j];
  t = wave_sum(t);
  if (lane == 0) out[j] = accumulate ? out[j] + t : t;
}
__global__ void __launch_bounds__(256)
k_reduce_rows_par(const float* __restrict__ partial, int64_t rows, int64_t ld, int n, float* __restrict__ out,
                  int accumulate) {
  reduce_col_wave(partial, rows, ld, n, out, accumulate, blockIdx.x);
}

// many rows, 16..4096 columns: 16 columns x 16 row groups per 256-thread workgroup — a wave's load instruction covers
// 4 rows x 64 contiguous bytes (the wave-per-column form above touches 64 different cache lines per instruction and
// uses 4 bytes of each), a thread sums rows r = g mod 16 (8 loads in flight), the 16 group sums of a column are
// combined through LDS in a fixed pairwise tree.  Shared by the stand-alone and the deferred form.
// Which 16-column tile a workgroup takes.  A tile's rows are 64-byte segments, i.e. HALF of the 128-byte lines the L2
// fetches, and the hardware deals consecutive workgroups to the eight XCDs in turn: with tile = workgroup every line was
// fetched by two XCDs — k_multi_reduce read 92 MB for 53 MB of queued partials (PMC, profiles/r04_step_traffic_full.csv)
// at the HBM rate.  Within every 64 workgroups, the eight that land on XCD x (x, x + 8, ...) take eight CONSECUTIVE
// tiles: 7 of 8 shared lines now meet in one L2.  (Which workgroup sums a column does not change the sum.)
__device__ __forceinline__ int64_t tile16_of(int64_t block, int n) {
  const int64_t base = block & ~(int64_t)63, tiles = ((int64_t)n + 15) >> 4;
  if (base + 64 > tiles) return block;                  // the incomplete last group: as dealt
  const int o = (int)(block & 63);
  return base + ((o & 7) << 3) + (o >> 3);
}
__device__ __forceinline__ void reduce_cols_tile16(const float* __restrict__ partial, int64_t rows, int64_t ld, int n,
                                                   float* __restrict__ out, int accumulate, int64_t block,
                                                   float (*lds)[64]) {
  float* s = &lds[0][0];                               // [16 groups][16 columns]
  const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int64_t j = tile16_of(block, n) * 16 + c;
  float t = 0.f;
  if (j < n) {
#pragma unroll 8
    for (int64_t r = g; r < rows; r += 16) t += partial[r * ld + j];
  }
  s[g * 16 + c] = t;
  __syncthreads();
  if (g == 0 && j < n) {
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = s[k * 16 + c];
#pragma unroll
    for (int w = 1; w < 16; w *= 2)
#pragma unroll
      for (int k = 0; k < 16; k += 2 * w) v[k] += v[k + w];
    out[j] = accumulate ? out[j] + v[0] : v[0];
  }
}
__global__ void __launch_bounds__(256)
k_reduce_rows_tile16(const float* __restrict__ partial, int64_t rows, int64_t ld, int n, float* __restrict__ out,
                     int accumulate) {
  __shared__ float lds[4][64];
  reduce_cols_tile16(partial, rows, ld, n, out, accumulate, blockIdx.x, lds);
}

// gridDim.y independent sums of the same shape (the slab sums of a batched split-K product)
__global__ void __launch_bounds__(256)
k_reduce_rows_tile16_batched(const float* __restrict__ partial, int64_t rows, int64_t ld, int n, float* __restrict__ out,
                             int64_t p_batch, int64_t o_batch) {
  __shared__ float lds[4][64];
  reduce_cols_tile16(partial + (int64_t)blockIdx.y * p_batch, rows, ld, n, out + (int64_t)blockIdx.y * o_batch, 0,
                     blockIdx.x, lds);
}

int igcn_launch_reduce_rows_batched(const float* partial, int64_t rows, int64_t ld, int n, float* out, int batch,
                                    int64_t p_batch, int64_t o_batch, hipStream_t st) {
  if (n <= 0 || batch <= 0) return IGCN_OK;
  hipLaunchKernelGGL(k_reduce_rows_tile16_batched, dim3((unsigned)igcn_cdiv(n, 16), (unsigned)batch), dim3(256), 0, st,
                     partial, rows, ld, n, out, p_batch, o_batch);
  IGCN_CHECK_LAUNCH("reduce_rows_batched");
  return IGCN_OK;
}

// out[j] = sum_r partial[j * rows + r]: the summands of one output are CONTIGUOUS (coalesced), one block per output
__global__ void __launch_bounds__(1024)
k_reduce_contig(const float* __restrict__ partial, int64_t rows, float* __restrict__ out) {
  __shared__ float red[16];
  const float* p = partial + (int64_t)blockIdx.x * rows;
  float t = 0.f;
#pragma unroll 8
  for (int64_t r = threadIdx.x; r < rows; r += 1024) t += p[r];
  t = block_sum_all(t, red);
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}

int igcn_launch_reduce_contig(const float* partial, int64_t rows, int n, float* out, hipStream_t st) {
  if (n <= 0) return IGCN_OK;
  hipLaunchKernelGGL(k_reduce_contig, dim3((unsigned)n), dim3(1024), 0, st, partial, rows, out);
  IGCN_CHECK_LAUNCH("reduce_contig");
  return IGCN_OK;
}

int igcn_launch_reduce_rows(const float* partial, int64_t rows, int64_t ld, int n, float* out, int accumulate,
                            hipStream_t st) {
  if (n <= 0) return IGCN_OK;
  const int form = rr_form(rows, n);
  if (form == 1 || form == 2) {
    if (form == 2) {
      hipLaunchKernelGGL(k_reduce_rows_tile16, dim3((unsigned)igcn_cdiv(n, 16)), dim3(256), 0, st, partial, rows, ld, n,
                         out, accumulate);
      IGCN_CHECK_LAUNCH("reduce_rows_tile16");
      return IGCN_OK;
    }
    hipLaunchKernelGGL(k_reduce_rows_par, dim3((unsigned)igcn_cdiv(n, 4)), dim3(256), 0, st, partial, rows, ld, n, out,
                       accumulate);
    IGCN_CHECK_LAUNCH("reduce_rows_par");
    return IGCN_OK;
  }
  if (form == 3) {
    hipLaunchKernelGGL(k_reduce_rows_grouped, dim3((unsigned)igcn_cdiv(n, 64)), dim3(256), 0, st, partial, rows, ld, n,
                       out, accumulate);
    IGCN_CHECK_LAUNCH("reduce_rows_grouped");
    return IGCN_OK;
  }
  hipLaunchKernelGGL(k_reduce_rows, dim3((unsigned)igcn_cdiv(n, 64)), dim3(64), 0, st, partial, rows, ld, n, out,
                     accumulate);
  IGCN_CHECK_LAUNCH("reduce_rows");
  return IGCN_OK;
}

// ---- deferred reductions -------------------------------------------------------------------------------------
// A backward pass ends ~30 of its kernels with a small "sum the block partials" launch whose output is a parameter
// gradient that nothing reads before the optimiser.  With igcn_reduce_defer(1) those launches are queued (the
// partial buffers stay alive on the caller's side) and igcn_reduce_flush performs all of them in ONE launch whose
// table travels by value in the kernel arguments — same arithmetic and summation order as the stand-alone kernels.
#define MRQ_MAX 48
struct ReduceTable {                                 // (ReduceEntry: pending.h)
  ReduceEntry e[MRQ_MAX];
  int start[MRQ_MAX + 1];                            // first workgroup of every entry (flat grid: no idle workgroups)
  int count;
};

// the wide in-order form may take four columns per thread (same sums, column by column)
__host__ __device__ inline bool rq_wide_vec(const ReduceEntry& e) {
  return e.nptr == 0 && !(e.rows > 32) && e.n >= 1024 && (e.n & 3) == 0 && (e.ld & 3) == 0 &&
         (((uintptr_t)e.partial | (uintptr_t)e.out) & 15) == 0;
}

__global__ void __launch_bounds__(256) k_multi_reduce(ReduceTable t, int32_t* tick) {
  __shared__ float lds[4][64];
  if (tick && blockIdx.x == 0 && threadIdx.x == 0) *tick += 1;      // the optimiser's step counter (igcn_reduce_flush_tick)
  // flat grid: workgroup -> (entry, block inside the entry).  [A (max blocks) x (entries) grid launched 57 000
  // workgroups for 11 000 with work.]
  // entry = number of starts at or below blockIdx.x (start[] ascending, unused slots INT_MAX): the whole prefix table is
  // fetched from the kernel arguments in ONE batch of scalar loads and compared in registers.  [A binary search is six
  // DEPENDENT scalar loads before the entry itself can be fetched, a linear walk up to 40.]
  int ei = 0;
#pragma unroll
  for (int i = 1; i < MRQ_MAX; ++i) ei += (int)blockIdx.x >= t.start[i] ? 1 : 0;
  const ReduceEntry e = t.e[ei];
  const int64_t blk = (int64_t)blockIdx.x - t.start[ei];
  if (e.nptr == -2) {                                // the train step's loss value from its partial sums (loss_final.h):
    // partial = [rows][4] head-loss sums, more[0] = Gram partials [ld & 0xffffffff][4], more[1] = regulariser partials
    // [ld >> 32], more[2] = weights [10], out = loss | terms[7]; one workgroup
    loss_final_body(e.partial, (int)e.rows, e.more[0], (int)(e.ld & 0xffffffff), e.more[1], (int)(e.ld >> 32), e.more[2], e.out,
                    &lds[0][0]);
    return;
  }
  if (e.nptr < 0) {                                  // GO attention: parameter gradients from the block partials
    // (go_attn_finish_output, common.h — shared with go.hip's k_go_attn_bwd_finish; output j = blk, ld = FIN | FOUT << 8)
    go_attn_finish_output(e.partial, e.rows, (int)(e.ld & 255), (int)(e.ld >> 8), e.more[0], e.more[1], e.out, (int)blk,
                          &lds[0][0]);
    return;
  }
  if (e.nptr > 0) {                                  // a leaf's gradient = sum of its consumers' gradients (k_sum_n)
    const int64_t j4 = (blk * 256 + threadIdx.x) * 4;          // 16 bytes per lane (buffers 16-byte aligned)
    // more[] with CONSTANT indices only.  [A `for (k < nptr) ... e.more[k]` loop indexes the entry dynamically: the
    // compiler then keeps the whole entry addressable, and EVERY path of the kernel — the tiles, the row groups —
    // re-reads its fields around each load instead of holding them in registers: a 512 x 2400 tile sum took 13 us in
    // this launch and 4.7 us with this branch compiled out (tools/reduce_trace.py); same instructions otherwise.]
    const float* m0 = e.more[0];
    const float* m1 = e.more[1];
    const float* m2 = e.more[2];
    const int np = e.nptr;
    if (j4 + 3 < e.n) {
      float4 a = *reinterpret_cast<const float4*>(e.partial + j4);
      {
        const float4 b = *reinterpret_cast<const float4*>(m0 + j4);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      }
      if (np > 1) {
        const float4 b = *reinterpret_cast<const float4*>(m1 + j4);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      }
      if (np > 2) {
        const float4 b = *reinterpret_cast<const float4*>(m2 + j4);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      }
      *reinterpret_cast<float4*>(e.out + j4) = a;
    } else {
      for (int64_t j = j4; j < e.n; ++j) {
        float s = e.partial[j] + m0[j];
        if (np > 1) s += m1[j];
        if (np > 2) s += m2[j];
        e.out[j] = s;
      }
    }
    return;
  }
  const int form = rr_form(e.rows, e.n);
  if (form == 3) {                                   // tall and wide: grouped rows (k_reduce_rows_grouped)
    reduce_cols_grouped(e.partial, e.rows, e.ld, e.n, e.out, 0, blk, lds);
    return;
  }
  if (form != 0) {                                   // tall: 16 x 16 tiles (k_reduce_rows_tile16), or a wave per column
    if (form == 2) reduce_cols_tile16(e.partial, e.rows, e.ld, e.n, e.out, 0, blk, lds);
    else reduce_col_wave(e.partial, e.rows, e.ld, e.n, e.out, 0, blk);
  } else if (rq_wide_vec(e)) {                       // wide, 16-byte rows: four columns per thread, rows in order
    const int64_t j = (blk * 256 + threadIdx.x) * 4;
    if (j >= e.n) return;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int64_t r = 0; r < e.rows; ++r) {
      const float4 v = *reinterpret_cast<const float4*>(e.partial + r * e.ld + j);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(e.out + j) = s;
  } else {                                           // wide: one thread per column, rows in order (k_reduce_rows)
    const int64_t j = blk * 256 + threadIdx.x;
    if (j >= e.n) return;
    float s = 0.f;
#pragma unroll 8
    for (int64_t r = 0; r < e.rows; ++r) s += e.partial[r * e.ld + j];
    e.out[j] = s;
  }
}

__global__ void k_tick(int32_t* tick) { *tick += 1; }

// every entry waiting on `st`, in issue order, MRQ_MAX per launch; the stream's queue is empty afterwards whatever the
// launch check says
static int reduce_flush(hipStream_t st, int32_t* tick) {
  const std::vector<ReduceEntry> q = pending::take_reduce(st);
  if (igcn_opt(IGCN_OPT_DEBUG_REDUCE))
    for (const ReduceEntry& e : q)
      fprintf(stderr, "[igcn] deferred reduction: rows %lld x n %d (ld %lld)%s\n", (long long)e.rows, e.n,
              (long long)e.ld, e.nptr == -2 ? "  loss value" : e.nptr < 0 ? "  GO attention finish" : e.nptr > 0 ? "  separate buffers" : rr_form(e.rows, e.n) ? "  tree" : "  in-order");
  size_t done = 0;
  while (done < q.size()) {
    ReduceTable t = {};
    const int cnt = (int)(q.size() - done < MRQ_MAX ? q.size() - done : MRQ_MAX);
    int64_t total = 0;
    for (int i = 0; i < cnt; ++i) {
      const ReduceEntry& e = q[done + i];
      t.e[i] = e;
      const int64_t need = e.nptr == -2 ? 1 : e.nptr < 0 ? e.n : e.nptr > 0 ? igcn_cdiv(e.n, 1024)
                           : rr_form(e.rows, e.n) == 1 ? igcn_cdiv(e.n, 4)
                           : rr_form(e.rows, e.n) == 2 ? igcn_cdiv(e.n, 16)
                           : rr_form(e.rows, e.n) == 3 ? igcn_cdiv(e.n, 64)
                                                       : igcn_cdiv(e.n, rq_wide_vec(e) ? 1024 : 256);
      t.start[i] = (int)total;
      total += need;
    }
    for (int i = cnt; i <= MRQ_MAX; ++i) t.start[i] = 0x7fffffff;
    t.count = cnt;
    done += cnt;
    hipLaunchKernelGGL(k_multi_reduce, dim3((unsigned)total), dim3(256), 0, st, t, done == q.size() ? tick : nullptr);
    if (done == q.size()) tick = nullptr;
  }
  if (tick) hipLaunchKernelGGL(k_tick, dim3(1), dim3(1), 0, st, tick);          // nothing was queued: the tick alone
  IGCN_CHECK_LAUNCH("reduce_flush");
  return IGCN_OK;
}

extern "C" int igcn_reduce_flush(void* stream) { return reduce_flush((hipStream_t)stream, nullptr); }

// The flush that ends a train step's backward also advances the optimiser's step counter (int32, device) — the one-thread
// launch in front of igcn_adam_step_multi otherwise; pair with igcn_adam_step*_ticked.
extern "C" int igcn_reduce_flush_tick(void* stream, int32_t* tick) { return reduce_flush((hipStream_t)stream, tick); }

// out[j] = sum_r partial[r * ld + j], j < n, as a FINAL reduction: queued while the stream defers (igcn_reduce_defer),
// performed by a launch of its own otherwise — for partial rows a kernel left behind for a parameter gradient
extern "C" int igcn_reduce_rows_final(const float* partial, int64_t rows, int64_t ld, int n, float* out, void* stream) {
  IGCN_REQUIRE(partial && out && rows >= 1 && n >= 1 && ld >= n, "reduce_rows_final: bad arguments");
  return igcn_launch_reduce_rows_final(partial, rows, ld, n, out, (hipStream_t)stream);
}
extern "C" int igcn_debug_reduce_rows_final(const float* partial, int64_t rows, int64_t ld, int n, float* out, void* stream) {
  return igcn_launch_reduce_rows_final(partial, rows, ld, n, out, (hipStream_t)stream);
}
