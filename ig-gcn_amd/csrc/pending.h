// The host-side queues of the library ("HOST-SIDE QUEUES OF THE LIBRARY", include/igcn.h): ONE record per stream holding
// the deferred final reductions, the dropout rider and the GEMM product riders, in ONE map under ONE lock — exactly
// these three kinds, with no way to register another.  Host only and free of HIP (tests/host/pending_check.cpp runs it
// under sanitizers without a device): the stream handle is an opaque key, never dereferenced.  Every operation takes and
// releases the lock itself and launches nothing: a flush takes the work out and launches it afterwards.
#pragma once
#include <stdint.h>

#include <map>
#include <mutex>
#include <vector>

#include "dropout_job.h"

// a deferred final reduction; travels by value inside ReduceTable in k_multi_reduce's kernel arguments (reduce.hip)
struct ReduceEntry {
  const float* partial;
  float* out;
  int64_t rows, ld;
  int n;
  int nptr;                                          // > 0: the rows are SEPARATE buffers (partial, more[0..nptr-1]),
  const float* more[3];                              //      summed in that order (igcn_sum_n_final)
};

#define GG_MAX 4                                     // products of one grouped GEMM launch = most that may wait

namespace pending {

// One record per STREAM: a backward pass defers on the stream it runs on (the autograd engine replays the forward's
// stream on its own thread, so the key is the stream, not the thread) and flushes that stream's entries only — several
// trainers in one process, each on a stream of its own, do not see each other's queues.
struct Stream {
  bool defer = false;
  std::vector<ReduceEntry> reduce;                   // in issue order
  bool has_job = false;
  DropJob job;
  std::vector<int64_t> products;                     // 16 words per product
  bool idle() const { return !defer && reduce.empty() && !has_job && products.empty(); }
};
inline std::mutex g_lock;
inline std::map<void*, Stream> g_streams;            // holds no idle record
inline void drop_if_idle(std::map<void*, Stream>::iterator it) {      // caller holds the lock
  if (it != g_streams.end() && it->second.idle()) g_streams.erase(it);
}

// ---- deferred final reductions ------------------------------------------------------------------------------------
// entries already queued survive defer(st, false) until the flush takes them
inline void defer(void* st, bool on) {
  std::lock_guard lk(g_lock);
  g_streams[st].defer = on;
  drop_if_idle(g_streams.find(st));
}
// queued if the stream defers (true), else not handled here
inline bool queue_reduce(void* st, const ReduceEntry& e) {
  std::lock_guard lk(g_lock);
  const auto it = g_streams.find(st);
  if (it == g_streams.end() || !it->second.defer) return false;
  it->second.reduce.push_back(e);
  return true;
}
inline std::vector<ReduceEntry> take_reduce(void* st) {
  std::vector<ReduceEntry> q;
  std::lock_guard lk(g_lock);
  const auto it = g_streams.find(st);
  if (it != g_streams.end()) q.swap(it->second.reduce);
  drop_if_idle(it);
  return q;
}

// ---- the dropout rider: at most one job per stream -------------------------------------------------------------------
inline bool put_job(void* st, const DropJob& job) {
  std::lock_guard lk(g_lock);
  Stream& s = g_streams[st];
  if (s.has_job) return false;
  s.has_job = true;
  s.job = job;
  return true;
}
inline bool take_job(void* st, DropJob& job) {
  std::lock_guard lk(g_lock);
  const auto it = g_streams.find(st);
  if (it == g_streams.end() || !it->second.has_job) return false;
  job = it->second.job;
  it->second.has_job = false;
  drop_if_idle(it);
  return true;
}

// ---- GEMM product riders: tables of 16 words, at most GG_MAX waiting -------------------------------------------------
inline bool put_products(void* st, int n, const int64_t* table) {
  std::lock_guard lk(g_lock);
  std::vector<int64_t>& q = g_streams[st].products;
  const bool room = q.size() / 16 + (size_t)n <= GG_MAX;
  if (room) q.insert(q.end(), table, table + 16 * n);
  drop_if_idle(g_streams.find(st));
  return room;
}
// A carrier takes them only whole, only with room for them, and only if it is a launch of the same operand type (word 15
// of the first waiting table against `bf16`); refused, they stay waiting.  The flush (no arguments) takes them all.
inline std::vector<int64_t> take_products(void* st, int room = GG_MAX, int bf16 = -1) {
  std::vector<int64_t> r;
  std::lock_guard lk(g_lock);
  const auto it = g_streams.find(st);
  if (it == g_streams.end() || it->second.products.empty()) return r;
  const std::vector<int64_t>& q = it->second.products;
  if ((int)(q.size() / 16) <= room && (bf16 < 0 || (q[15] != 0) == (bf16 != 0))) r.swap(it->second.products);
  drop_if_idle(it);
  return r;
}

// forget the riders (job and products) without launching them; reductions are left alone
inline void cancel_riders(void* st) {
  std::lock_guard lk(g_lock);
  const auto it = g_streams.find(st);
  if (it == g_streams.end()) return;
  it->second.has_job = false;
  it->second.products.clear();
  drop_if_idle(it);
}

// entries + job + products of ONE stream, as one snapshot
inline int count(void* st) {
  std::lock_guard lk(g_lock);
  const auto it = g_streams.find(st);
  if (it == g_streams.end()) return 0;
  const Stream& s = it->second;
  return (int)s.reduce.size() + (s.has_job ? 1 : 0) + (int)(s.products.size() / 16);
}
// deferred reductions of ALL streams
inline int count_reduce_all() {
  std::lock_guard lk(g_lock);
  size_t n = 0;
  for (const auto& kv : g_streams) n += kv.second.reduce.size();
  return (int)n;
}

}  // namespace pending
