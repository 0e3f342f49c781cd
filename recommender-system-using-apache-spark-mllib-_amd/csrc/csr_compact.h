// K18 / K20 — what the two producers of keep bits share beside the tile walk of
// csr_tile_walk.h: the tail of a mark kernel that turns a thread's keep flags into keep_bits
// words and the tile's kept count, the scan of the tiles' kept counts, the
// kept-entries-before-every-row pass and the host call that launches those two.
// als_csr_remove_mark (csr_remove.hip) and als_split_mark (split.hip) mark with kernels of
// their own and finish here, so als_csr_remove_compact reads one format.
// The kernels are static: each translation unit that includes this header owns its copy.
#pragma once
#include "als_common.h"
#include "csr_tile_walk.h"

namespace als {

constexpr int kScanThreads = 1024;
constexpr int kScanItems = 4;

// The end of a mark kernel, by the whole workgroup: bit i of `keep` says that entry
// p0 + i * 256 + threadIdx.x stays.  One ballot per item makes the words of keep_bits, and
// thread 0 writes the tile's kept count.  Entries at or past nnz never set a flag: the tail
// bits of the last word are 0.
__device__ __forceinline__ void tile_store_keep(uint32_t keep, int64_t p0, int64_t nnz,
                                                uint64_t* __restrict__ keep_bits,
                                                int32_t* __restrict__ tile_cnt, int32_t* s_cnt) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t n_words = (nnz + 63) >> 6;
  int32_t cnt = 0;
#pragma unroll
  for (int i = 0; i < kTileItems; ++i) {
    const uint64_t word = __ballot((keep >> i) & 1u);
    const int64_t w = (p0 >> 6) + i * kTileWaves + wave;
    if (lane == 0 && w < n_words) keep_bits[w] = word;
    cnt += __popcll(word);
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (t == 0) {
    int32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kTileWaves; ++w) sum += s_cnt[w];
    tile_cnt[blockIdx.x] = sum;
  }
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
      const int64_t up = shfl_up_64(incl, d);
      if (lane >= d) incl += up;
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
  const int64_t tile = p / kTile;  // p == nnz_old on a tile edge: tile_off[tiles]
  int64_t kept = tile_off[tile];
  const int64_t w1 = p >> 6;
  for (int64_t w = tile * kTileWords; w < w1; ++w) kept += __popcll(keep_bits[w]);
  const int below = (int)(p & 63);  // > 0 implies p < 64 * n_words: the word exists
  if (below) kept += __popcll(keep_bits[w1] & ((uint64_t(1) << below) - 1));
  row_ptr_kept[r] = kept;
}

// What follows every mark kernel on its stream: tile_cnt -> tile_off, then row_ptr_kept.
static inline int keep_finish(const int64_t* row_ptr, int32_t n_rows, int64_t nnz,
                              const uint64_t* keep_bits, const int32_t* tile_cnt,
                              int64_t* tile_off, int64_t* row_ptr_kept, hipStream_t st) {
  remove_scan_kernel<<<1, kScanThreads, 0, st>>>(tile_cnt, csr_tiles(nnz), tile_off);
  ALS_LAUNCH_CHECK();
  remove_row_ptr_kernel<<<(unsigned)(((int64_t)n_rows + 256) / 256), 256, 0, st>>>(
      row_ptr, n_rows, nnz, keep_bits, tile_off, row_ptr_kept);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // namespace als
