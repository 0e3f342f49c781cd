// The per-workgroup LDS cache in front of an exact int32 histogram in memory, shared by the
// list exposure counts (K15, list_metrics.hip) and the co-rated counts (K19, co_rated.hip).
//
// kLxWindow int32 counters and as many tags, direct-mapped: key j lives in slot
// j mod kLxWindow, the first key to reach a slot claims it (one LDS compare-and-swap on the
// slot's tag), and from then on every entry naming that key is one LDS integer add.  A key
// that finds its slot taken by another goes to memory with one global integer add.  A flush
// adds every non-zero slot to counts[] once.  Every add is an integer add, so counts are
// exact and the same bits whatever order the adds land in.
#pragma once
#include "als_common.h"

namespace als {

constexpr int kLxWindow = 8192;  // LDS counters (and tags) per workgroup; a power of two

// Empty cache: every counter 0, every tag unclaimed.  All THREADS threads of the workgroup
// call it; a barrier must follow before the first lx_add.
template <int THREADS>
__device__ __forceinline__ void lx_clear(int32_t* __restrict__ scnt, int32_t* __restrict__ stag) {
  for (int s = threadIdx.x; s < kLxWindow; s += THREADS) {
    scnt[s] = 0;
    stag[s] = -1;
  }
}

// One entry of row `key`: an LDS add when the row owns (or can claim) its slot, a global add
// otherwise.  (One global add per entry, and this cache behind a per-wave fold of equal keys,
// were measured and are not kept: DESIGN.md section K15.)
__device__ __forceinline__ void lx_add(int32_t key, int32_t* __restrict__ scnt,
                                       int32_t* __restrict__ stag, int32_t* __restrict__ counts) {
  const int slot = key & (kLxWindow - 1);
  int32_t tag = __atomic_load_n(&stag[slot], __ATOMIC_RELAXED);
  if (tag < 0) {
    const int32_t old = atomicCAS(&stag[slot], -1, key);
    tag = old < 0 ? key : old;
  }
  if (tag == key) atomicAdd(&scnt[slot], 1);
  else atomicAdd(&counts[key], 1);
}

// Every non-zero slot to counts[], once.  All THREADS threads call it, after a barrier that
// follows the last lx_add.
template <int THREADS>
__device__ __forceinline__ void lx_flush(const int32_t* __restrict__ scnt,
                                         const int32_t* __restrict__ stag,
                                         int32_t* __restrict__ counts) {
  for (int s = threadIdx.x; s < kLxWindow; s += THREADS) {
    const int32_t c = scnt[s];
    if (c) atomicAdd(&counts[stag[s]], c);
  }
}

}  // namespace als
