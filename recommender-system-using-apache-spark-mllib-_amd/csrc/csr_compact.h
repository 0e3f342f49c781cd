// K18 / K20 — what the two producers of keep bits share: the tile geometry, the scan of the
// tiles' kept counts and the kept-entries-before-every-row pass.  als_csr_remove_mark
// (csr_remove.hip) and als_split_mark (split.hip) write keep_bits and per-tile counts with
// kernels of their own and finish with these two, so als_csr_remove_compact reads one format.
// The kernels are static: each translation unit that includes this header owns its copy.
#pragma once
#include "als_common.h"

namespace als {

constexpr int kRemoveThreads = 256;
constexpr int kRemoveItems = 8;
constexpr int kRemoveTile = kRemoveThreads * kRemoveItems;  // stored entries per workgroup
constexpr int kRemoveWaves = kRemoveThreads / 64;
constexpr int kRemoveWords = kRemoveTile / 64;              // keep_bits words per tile
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 4;

static inline int64_t remove_tiles(int64_t nnz_old) {
  return (nnz_old + kRemoveTile - 1) / kRemoveTile;
}

// tile_off = exclusive scan of tile_cnt, tile_off[tiles] = the total.  One workgroup walks
// the counts 4096 at a time with a running carry (tiles <= 2^20: at most 256 trips).
static __global__ __launch_bounds__(kScanThreads) void remove_scan_kernel(
    const int32_t* __restrict__ tile_cnt, int64_t tiles, int64_t* __restrict__ tile_off) {
  __shared__ int64_t s_wave[kScanThreads / 64];
  __shared__ int64_t s_carry;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < tiles; base += kScanThreads * kScanItems) {
    const int64_t j0 = base + (int64_t)t * kScanItems;
    int32_t c[kScanItems];
    int64_t mine = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      c[i] = j0 + i < tiles ? tile_cnt[j0 + i] : 0;
      mine += c[i];
    }
    int64_t incl = mine;  // inclusive scan of `mine` over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      int2 v = __builtin_bit_cast(int2, incl);
      v.x = __shfl_up(v.x, d);
      v.y = __shfl_up(v.y, d);
      if (lane >= d) incl += __builtin_bit_cast(int64_t, v);
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int64_t before = s_carry;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    int64_t run = before + incl - mine;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      if (j0 + i < tiles) tile_off[j0 + i] = run;
      run += c[i];
    }
    __syncthreads();  // every thread has read s_carry and s_wave
    if (t == kScanThreads - 1) s_carry = run;
    __syncthreads();
  }
  if (t == 0) tile_off[tiles] = s_carry;
}

// row_ptr_kept[r] = kept entries before row_ptr_old[r], r = 0 .. n_old: tile_off of the tile
// plus the popcount of that tile's words (at most 31 and a part of one) below the position.
static __global__ __launch_bounds__(256) void remove_row_ptr_kernel(
    const int64_t* __restrict__ row_ptr_old, int32_t n_old, int64_t nnz_old,
    const uint64_t* __restrict__ keep_bits, const int64_t* __restrict__ tile_off,
    int64_t* __restrict__ row_ptr_kept) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > n_old) return;
  int64_t p = row_ptr_old[r];
  p = p < 0 ? 0 : (p > nnz_old ? nnz_old : p);
  const int64_t tile = p / kRemoveTile;  // p == nnz_old on a tile edge: tile_off[tiles]
  int64_t kept = tile_off[tile];
  const int64_t w1 = p >> 6;
  for (int64_t w = tile * kRemoveWords; w < w1; ++w) kept += __popcll(keep_bits[w]);
  const int below = (int)(p & 63);  // > 0 implies p < 64 * n_words: the word exists
  if (below) kept += __popcll(keep_bits[w1] & ((uint64_t(1) << below) - 1));
  row_ptr_kept[r] = kept;
}

}  // namespace als
