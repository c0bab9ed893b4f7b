// Host-only check of the per-stream registry behind the library's three host-side queues (ig-gcn_amd/csrc/pending.h;
// contract: "HOST-SIDE QUEUES OF THE LIBRARY", include/igcn.h).  No HIP, no device: stream handles and entries are
// fabricated and no pointer is ever dereferenced.  Built and run under sanitizers by tests/test_pending_host.py.
// Prints one line per check; exits non-zero at the first failure.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>

#include "../../ig-gcn_amd/csrc/pending.h"

static void check(bool ok, const char* what) {
  printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok) exit(1);
}

static void* handle(uintptr_t v) { return reinterpret_cast<void*>(v); }
static ReduceEntry entry(int tag) {
  return ReduceEntry{reinterpret_cast<const float*>((uintptr_t)0x1000), reinterpret_cast<float*>((uintptr_t)0x2000), 4, 8,
                     tag, 0, {nullptr, nullptr, nullptr}};
}
static DropJob job_of(int tag) {
  DropJob j = {};
  j.total = tag;
  j.blocks = (unsigned)tag;
  return j;
}
// n product tables whose 16 words all carry `tag`, word 15 = operand type
static std::vector<int64_t> tables(int n, int64_t tag, bool bf16) {
  std::vector<int64_t> t((size_t)16 * n, tag);
  for (int i = 0; i < n; ++i) t[16 * i + 15] = bf16 ? 1 : 0;
  return t;
}

static void single_thread_checks() {
  void* A = handle(0xA0);
  void* B = handle(0xB0);

  // 3. a stream that does not defer queues nothing
  check(!pending::queue_reduce(A, entry(1)) && pending::count(A) == 0 && pending::g_streams.empty(),
        "3: a reduce entry on a stream that does not defer is not queued");
  // 1. defer off erases the record only if nothing is queued; entries survive until they are taken
  pending::defer(A, true);
  check(pending::g_streams.size() == 1, "1: defer on makes the stream's record");
  pending::defer(A, false);
  check(pending::g_streams.empty(), "1: defer off with nothing queued erases the record");
  pending::defer(A, true);
  check(pending::queue_reduce(A, entry(1)) && pending::queue_reduce(A, entry(2)) && pending::queue_reduce(A, entry(3)),
        "3: a deferring stream queues");
  pending::defer(A, false);
  check(pending::count(A) == 3 && pending::g_streams.size() == 1, "1: defer off keeps queued entries");
  check(!pending::queue_reduce(A, entry(4)) && pending::count(A) == 3, "1: ... and queues no more");
  {
    const std::vector<ReduceEntry> q = pending::take_reduce(A);
    check(q.size() == 3 && q[0].n == 1 && q[1].n == 2 && q[2].n == 3, "2: the flush takes the entries in issue order");
    check(pending::count(A) == 0 && pending::g_streams.empty(), "1: taking them erases a record that is off");
    check(pending::take_reduce(A).empty(), "2: nothing queued: nothing taken");
  }
  pending::defer(A, true);
  pending::queue_reduce(A, entry(5));
  check(pending::take_reduce(A).size() == 1 && pending::g_streams.size() == 1 && pending::queue_reduce(A, entry(6)),
        "1: taking them leaves a deferring stream deferring");
  check(pending::take_reduce(A).size() == 1, "   (drained)");
  pending::defer(A, false);

  // 4. the dropout rider: at most one job
  DropJob got = {};
  check(!pending::take_job(A, got), "4: no job waiting: nothing taken");
  check(pending::put_job(A, job_of(7)) && !pending::put_job(A, job_of(8)) && pending::count(A) == 1,
        "4: a second dropout job is refused");
  check(pending::take_job(A, got) && got.total == 7 && got.blocks == 7u && pending::count(A) == 0,
        "4: the first one is the one taken");
  check(pending::put_job(A, job_of(9)), "4: a taken job leaves the stream free");
  pending::cancel_riders(A);
  check(pending::count(A) == 0 && pending::put_job(A, job_of(10)), "4: a cancelled job leaves the stream free");
  check(pending::take_job(A, got) && got.total == 10 && pending::g_streams.empty(), "   (drained)");

  // 5. product riders
  check(pending::put_products(A, 3, tables(3, 11, false).data()) && pending::count(A) == 3, "5: three products wait");
  check(!pending::put_products(A, 2, tables(2, 12, false).data()) && pending::count(A) == 3,
        "5: more than GG_MAX waiting is refused");
  check(pending::put_products(A, 1, tables(1, 13, false).data()) && pending::count(A) == GG_MAX, "5: GG_MAX may wait");
  check(pending::take_products(A, 3, false).empty() && pending::count(A) == 4,
        "5: a carrier without room for all takes none, and they stay");
  check(pending::take_products(A, 4, true).empty() && pending::count(A) == 4,
        "5: a carrier of the other operand type takes none, and they stay");
  {
    const std::vector<int64_t> r = pending::take_products(A, 4, false);
    check(r.size() == 64 && r[0] == 11 && r[32] == 11 && r[48] == 13 && pending::count(A) == 0,
          "5: a carrier with room and the same type takes all, in order");
  }
  check(pending::put_products(A, 2, tables(2, 14, true).data()) && pending::take_products(A, 2, false).empty() &&
            pending::take_products(A, 2, true).size() == 32,
        "5: word 15 of the first waiting table decides the type");
  check(!pending::put_products(A, GG_MAX + 1, tables(GG_MAX + 1, 15, false).data()) && pending::g_streams.empty(),
        "5: a refused put on an idle stream leaves no record");
  check(pending::put_products(A, 1, tables(1, 16, true).data()) && pending::take_products(A).size() == 16 &&
            pending::take_products(A).empty() && pending::g_streams.empty(),
        "5: the flush takes them whatever their type");

  // 6. 7. 8. all three together, two streams
  pending::defer(A, true);
  pending::defer(B, true);
  pending::queue_reduce(A, entry(1));
  pending::queue_reduce(A, entry(2));
  pending::queue_reduce(B, entry(3));
  pending::put_job(A, job_of(1));
  pending::put_products(A, 1, tables(1, 1, false).data());
  pending::put_products(B, 2, tables(2, 2, false).data());
  check(pending::count(A) == 4 && pending::count(B) == 3 && pending::count(handle(0xC0)) == 0,
        "7: stream count = entries + job + products of that stream only");
  check(pending::count_reduce_all() == 3, "7: reduce count = entries of all streams");
  pending::cancel_riders(A);
  check(pending::count(A) == 2 && pending::count(B) == 3, "6: cancel forgets job and products of that stream only");
  check(!pending::take_job(A, got) && pending::take_products(A).empty(), "6: ... for good");
  check(pending::take_job(B, got) == false && pending::take_products(B, 4, false).size() == 32,
        "8: the other stream's riders are untouched");
  check(pending::take_reduce(A).size() == 2 && pending::count_reduce_all() == 1 && pending::take_reduce(B).size() == 1,
        "6: ... and never the reductions; 8: each stream flushes its own");
  pending::defer(A, false);
  pending::defer(B, false);
  check(pending::g_streams.empty(), "   nothing is left behind");
}

// An autograd thread and the main thread sharing a stream, times four: eight threads on two handles mix every
// operation.  Reductions are accounted exactly (cancel must never drop one); riders by what can be known without a
// log of the cancels: nothing is taken that was not put, and everything taken is whole.
static void threaded_checks() {
  const int THREADS = 8, ROUNDS = 4000;
  void* S[2] = {handle(0x51), handle(0x52)};
  std::atomic<long> queued{0}, flushed{0}, jobs_put{0}, jobs_taken{0}, prod_put{0}, prod_taken{0}, torn{0}, over{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < THREADS; ++t) {
    pool.emplace_back([&, t]() {
      unsigned x = 12345u + 977u * (unsigned)t;
      for (int r = 0; r < ROUNDS; ++r) {
        x = x * 1664525u + 1013904223u;
        void* st = S[(x >> 8) & 1];
        const int tag = t * ROUNDS + r + 1;
        switch ((x >> 16) % 12) {
          case 0: pending::defer(st, true); break;
          case 1: pending::defer(st, false); break;
          case 2: case 3: case 4:
            if (pending::queue_reduce(st, entry(tag))) ++queued;
            break;
          case 5: flushed += (long)pending::take_reduce(st).size(); break;
          case 6:
            if (pending::put_job(st, job_of(tag))) ++jobs_put;
            break;
          case 7: {
            DropJob j = {};
            if (pending::take_job(st, j)) {
              ++jobs_taken;
              if (j.total != (int64_t)j.blocks) ++torn;
            }
            break;
          }
          case 8: {
            const int n = 1 + (int)((x >> 24) % 3);
            if (pending::put_products(st, n, tables(n, tag, (x >> 30) & 1).data())) prod_put += n;
            break;
          }
          case 9: {
            const bool all = (x >> 24) & 1;
            const std::vector<int64_t> v = all ? pending::take_products(st) : pending::take_products(st, 2, (x >> 30) & 1);
            prod_taken += (long)(v.size() / 16);
            if (v.size() % 16 || v.size() / 16 > (size_t)(all ? GG_MAX : 2)) ++over;
            for (size_t i = 0; i + 16 <= v.size(); i += 16)
              for (int k = 1; k < 15; ++k)
                if (v[i + k] != v[i]) ++torn;
            break;
          }
          case 10: pending::cancel_riders(st); break;
          default:
            if (pending::count(st) < 0 || pending::count_reduce_all() < 0) ++over;
            break;
        }
      }
    });
  }
  for (std::thread& th : pool) th.join();
  long left = 0;
  for (void* st : S) {
    pending::defer(st, false);
    pending::cancel_riders(st);
    left += (long)pending::take_reduce(st).size();
  }
  printf("     queued %ld, flushed %ld + %ld at the end; jobs %ld put / %ld taken; products %ld put / %ld taken\n",
         queued.load(), flushed.load(), left, jobs_put.load(), jobs_taken.load(), prod_put.load(), prod_taken.load());
  check(queued > 0 && flushed > 0 && jobs_taken > 0 && prod_taken > 0, "threads: every kind of work went through");
  check(queued == flushed + left, "threads: every queued reduction was flushed exactly once, cancels or not");
  check(jobs_taken <= jobs_put && prod_taken <= prod_put, "threads: no rider was taken that had not been put");
  check(torn == 0 && over == 0, "threads: every job and every product table came out whole, within the limits");
  check(pending::g_streams.empty() && pending::count(S[0]) + pending::count(S[1]) == 0, "threads: nothing is left behind");
}

int main() {
  single_thread_checks();
  threaded_checks();
  printf("all checks passed\n");
  return 0;
}
