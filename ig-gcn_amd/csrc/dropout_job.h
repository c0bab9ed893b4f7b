// The plain structs of a dropout-mask job (dropout.h holds the device code that runs one).  No HIP here: the host-side
// registry (pending.h) keeps a waiting job by value and is compiled without a device.
#pragma once
#include <stdint.h>

#define DM_MAXSEG 32
struct DropSegs {
  int64_t end[DM_MAXSEG];
  float p[DM_MAXSEG];
  int n;
};
// int64 device counters the launch bumps by `inc` (BatchNorm's num_batches_tracked of the model's five BatchNorms: the
// masks are drawn once per training forward, which is exactly when those counters advance — a torch._foreach_add_
// launch less per step)
#define DM_MAXCNT 8
struct DropCounters {
  long long* c[DM_MAXCNT];
  int n;
  long long inc;
};

// one mask-generation job as the host hands it over (igcn_dropout_masks / igcn_rider_dropout)
struct DropJob {
  int64_t total;
  DropSegs sg;
  unsigned long long* state;
  float* out;
  DropCounters cnt;
  unsigned blocks;
};
