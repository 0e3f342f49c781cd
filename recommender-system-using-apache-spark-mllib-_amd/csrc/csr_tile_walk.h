// K17 / K18 / K20 — the tile over the entries of a CSR side that merge_copy_kernel
// (csr_merge.hip), remove_mark_kernel (csr_remove.hip) and split_mark_kernel (split.hip) share:
// the tile geometry, the search for the row of a position, and the walk that gives every entry
// of a tile its row.  A kernel supplies what it keeps per row and what it does per entry.
#pragma once
#include "als_common.h"

namespace als {

constexpr int kTileThreads = 256;
constexpr int kTileItems = 8;
constexpr int kTile = kTileThreads * kTileItems;  // entries per workgroup
constexpr int kTileWaves = kTileThreads / 64;
constexpr int kTileWords = kTile / 64;            // keep_bits words per tile

static inline int64_t csr_tiles(int64_t nnz) { return (nnz + kTile - 1) / kTile; }

// The last r in [0, hi] with row_ptr[r] <= p; 0 when there is none.  `hi` is the caller's: n
// where row_ptr[n] = nnz > p keeps r below n, n - 1 where row n must never be the answer.
__device__ __forceinline__ int32_t csr_row_at(const int64_t* __restrict__ row_ptr, int32_t hi,
                                              int64_t p) {
  int32_t lo = 0;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo + 1) >> 1);
    if (row_ptr[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Entries [p0, p1) of one tile, p1 - p0 <= kTile, by a workgroup of kTileThreads, whichever rows
// they fall in.  row0 is the row of p0 (csr_row_at); from there the rows are walked 256 at a
// time.  load(r), called by every thread with r = row0 + threadIdx.x, stores the end of row r in
// s_end[threadIdx.x] (the end of the side for a row past the last: no entries) and whatever
// else the kernel keeps per row in LDS arrays of its own.  Every entry then finds its row among
// the batch's ends (8 steps in LDS) and entry(i, q, a, row) is called once for
// q = p0 + i * 256 + threadIdx.x: a is the row's index in the batch, row = row0 + a.  Thread t
// owns entries t, t + 256, ..., so along a run the loads and stores of a wavefront are
// consecutive words.  `done` only ever grows: a row pointer that decreases (outside the
// contract) cannot make the walk visit an entry twice, and for a non-decreasing one the guard
// never fires.
template <class Load, class Entry>
__device__ __forceinline__ void tile_row_walk(int64_t p0, int64_t p1, int64_t row0,
                                              const int64_t* s_end, Load load, Entry entry) {
  const int t = threadIdx.x;
  int64_t done = p0;  // entries below `done` have been visited
  while (done < p1) {
    load(row0 + t);
    __syncthreads();
    const int64_t batch_end = s_end[kTileThreads - 1];
    const int64_t stop = batch_end < p1 ? batch_end : p1;
#pragma unroll
    for (int i = 0; i < kTileItems; ++i) {
      const int64_t q = p0 + i * kTileThreads + t;
      if (q < done || q >= stop) continue;
      int a = 0, b = kTileThreads - 1;  // first row of the batch with end > q
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (s_end[mid] > q) b = mid; else a = mid + 1;
      }
      entry(i, q, a, row0 + a);
    }
    if (stop > done) done = stop;
    row0 += kTileThreads;
    __syncthreads();  // the next batch overwrites the LDS rows
  }
}

}  // namespace als
