// The fixed-order fp64 reduction behind every metric that sums per-block partials (K4 RMSE,
// K6 ranking metrics, K9 full-ranking metrics, K10 objective).
//
// Contract: the order of the additions depends on the number of blocks alone, so a sum is
// bitwise reproducible run to run.  With one block of 256 threads, per field:
//   1. thread t adds the partials of blocks t, t + 256, t + 512, ... in that (ascending)
//      order, starting from 0.0;
//   2. an LDS tree adds thread t's value and thread t + s's, for s = 128, 64, ... 1.
// Any change to that order changes the bits of every metric built on it.
#pragma once
#include "als_common.h"

namespace als {

// Tree sum of the 256 threads' values (thread t with t + s, s = 128 .. 1), returned to
// every thread.  sm: 256 doubles of LDS.
__device__ __forceinline__ double block_tree_sum(double mine, double* sm) {
  const int t = threadIdx.x;
  __syncthreads();  // sm may still be read from the previous field
  sm[t] = mine;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) sm[t] += sm[t + s];
    __syncthreads();
  }
  return sm[0];
}

// One block of 256 threads: out[f] = sum over the nb blocks of partial[block][f], f < NF, in
// the order of the contract above.
template <int NF>
__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ partial,
                                                           int64_t nb, double* __restrict__ out) {
  __shared__ double sm[256];
  for (int f = 0; f < NF; ++f) {
    double a = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += 256) a += partial[NF * b + f];
    a = block_tree_sum(a, sm);
    if (threadIdx.x == 0) out[f] = a;
  }
}

}  // namespace als
