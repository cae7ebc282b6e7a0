// The argument structs of the Adam kernels (adam.h), plain data with no device code, so that a
// launcher's interface header (iqn_launch.h) can carry them by value.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "net.h"

// the kernel-layout ("shadow") weights a step re-emits into
struct ShadowPtrs {
  void* base;   // T elements, layout net::shadow()
  float* vecs;  // net::Vecs
  int A;
};

struct AdamArgs {
  float *params, *grads, *m, *v, *metrics;
  float* metrics_host;  // (or null) page-locked host copy of the step's metrics vector
  const float* sumsq_part;
  int n_part;
  const int64_t* step;
  const float* sc;  // [2] step size and sqrt(bias correction 2), written by reduce_grads
  double b1, b2;
  float eps, max_norm, inv_world;
  ShadowPtrs sp;
  net::Canon cn;
  net::Shadow sh;
};

// Where index i of the handle's own (Canon) order lies in the caller's flat buffers: the identity
// for the learners whose buffers are in Canon order; FlatGap for a net whose parameters() order has
// `ins` floats of another layer inserted at `gap` (the IQN net: Wq, bq between b3 and the LayerNorm).
struct FlatId {};
struct FlatGap {
  size_t gap, ins;
};
