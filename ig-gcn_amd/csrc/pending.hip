// The entry points that are about the library's host-side queues (contract: "HOST-SIDE QUEUES OF THE LIBRARY",
// include/igcn.h; the per-stream registry itself: pending.h).  Queueing and taking happen under the registry's lock;
// whatever is launched here is launched after the lock is released, by the launcher that lives with its kernel.
#include "pending.h"

#include "common.h"
#include "dropout.h"

// ---- deferred final reductions (the flush and its kernels: reduce.hip) ------------------------------------------------
extern "C" int igcn_reduce_defer(void* stream, int on) {
  pending::defer(stream, on != 0);
  return IGCN_OK;
}

extern "C" int igcn_reduce_pending(void) { return pending::count_reduce_all(); }

int igcn_launch_reduce_rows_final(const float* partial, int64_t rows, int64_t ld, int n, float* out,
                                  hipStream_t st) {
  if (n <= 0) return IGCN_OK;
  if (pending::queue_reduce(st, ReduceEntry{partial, out, rows, ld, n, 0, {nullptr, nullptr, nullptr}})) return IGCN_OK;
  return igcn_launch_reduce_rows(partial, rows, ld, n, out, 0, st);
}

int igcn_queue_loss_final(const float* parts, int nparts, const float* gram, int gram_rows, const float* prob,
                          int prob_rows, const float* wts, float* out, hipStream_t st) {
  return pending::queue_reduce(st, ReduceEntry{parts, out, (int64_t)nparts,
                                               (int64_t)gram_rows | ((int64_t)prob_rows << 32), 8, -2, {gram, prob, wts}});
}

int igcn_queue_go_finish(const float* gpart, int64_t parts, int fin, int fout, const float* w_inc, const float* w_s,
                         float* dparams, hipStream_t st) {
  if (fin > 64 || fout > 64) return 0;
  return pending::queue_reduce(st, ReduceEntry{gpart, dparams, parts, (int64_t)(fin | (fout << 8)),
                                               2 * fout * fin + 3 * fout, -1, {w_inc, w_s, nullptr}});
}

int igcn_queue_sum_final(const float* const* parts, int k, int64_t numel, float* out, hipStream_t st) {
  if (k < 2 || k > 4 || numel > 0x7fffffff) return 0;
  uintptr_t al = (uintptr_t)out;
  for (int i = 0; i < k; ++i) al |= (uintptr_t)parts[i];
  if (al & 15) return 0;
  ReduceEntry e = {parts[0], out, (int64_t)k, 0, (int)numel, k - 1, {nullptr, nullptr, nullptr}};
  for (int i = 1; i < k; ++i) e.more[i - 1] = parts[i];
  return pending::queue_reduce(st, e);
}

// ---- the dropout rider (carriers: plan.hip, sgcn_fused.hip, sgcn_dense.hip) --------------------------------------------
extern "C" int igcn_rider_dropout(void* stream, int64_t total, int n_segments, const int64_t* seg_end, const float* seg_p,
                                  void* state, float* out, int n_counters, int64_t* const* counters, int64_t counter_inc) {
  DropJob job;
  const int rc = igcn_dropout_job(job, "rider_dropout", total, n_segments, seg_end, seg_p, state, out, n_counters, counters,
                                  counter_inc);
  if (rc) return rc;
  IGCN_REQUIRE(pending::put_job(stream, job),
               "rider_dropout: this stream already has a job waiting (igcn_rider_flush it first)");
  return IGCN_OK;
}

bool igcn_rider_dropout_take(hipStream_t st, DropJob& job) { return pending::take_job(st, job); }

// a job still waiting on the stream is launched by itself; nothing waiting: nothing happens
extern "C" int igcn_rider_flush(void* stream) {
  DropJob job;
  return pending::take_job(stream, job) ? igcn_dropout_launch(job, (hipStream_t)stream) : IGCN_OK;
}

// ---- GEMM product riders (carrier: igcn_gemm_f32_grouped, gemm.hip) ----------------------------------------------------
extern "C" int igcn_gemm_rider(void* stream, int n, const int64_t* table) {
  IGCN_REQUIRE(n >= 1 && n <= GG_MAX && table != nullptr, "gemm_rider: 1..%d products", GG_MAX);
  IGCN_REQUIRE(pending::put_products(stream, n, table), "gemm_rider: more than %d products waiting on this stream",
               GG_MAX);
  return IGCN_OK;
}

extern "C" int igcn_gemm_rider_flush(void* stream) {
  const std::vector<int64_t> r = pending::take_products(stream);
  return r.empty() ? IGCN_OK : igcn_gemm_f32_grouped((int)(r.size() / 16), r.data(), stream);
}

// ---- all three ---------------------------------------------------------------------------------------------------------
// Forget every rider still waiting on the stream (mask job and products) WITHOUT launching it: for the start of a step
// that may follow one which failed between queueing a rider and the launch that would have carried it — the buffers it
// points at may be gone.
extern "C" int igcn_rider_cancel(void* stream) {
  pending::cancel_riders(stream);
  return IGCN_OK;
}

// Everything the library still holds for `stream` on the host side and has NOT launched: deferred reductions (entries),
// the dropout rider (0 / 1), product riders (products).  0 at the end of every step; see the header for each queue's
// ordering contract.
extern "C" int igcn_stream_pending(void* stream) { return pending::count(stream); }
