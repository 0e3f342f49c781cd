// K18 — drop listed (row, column) pairs from one CSR side without sorting it again.
//
// K17 lets a fitted model take new ratings; this is the opposite direction: un-rate a pair,
// forget a user, withdraw an item.  K1's layout makes removal as exact as it made the merge:
// dense rows are in ascending id order and a row keeps its ratings in input order, so the CSR
// K1 would build from the ratings with some filtered out is, row by row, the stored row with
// those entries dropped and the order kept.  That is a stream compaction in two passes:
//   mark     one bit per stored entry (a wave ballot per 64): kept unless its column is in
//            the row's ASCENDING delete list (binary search; a row with an empty list costs
//            one comparison of two words the row walk already has in LDS).  Per-tile kept
//            counts are scanned by one workgroup into tile_off, and row_ptr_kept[r] = kept
//            entries before row_ptr_old[r] = tile_off of the tile + popcounts below it.
//   compact  each kept entry goes to tile_off[tile] + its rank among the tile's kept entries,
//            its column through the other side's old-to-new row map, its value as bits.
// Work is split over stored ENTRIES, kTile per workgroup whichever rows they fall in: the tile
// and its row walk are csr_tile_walk.h's (shared with K17 and K20), the keep-bits tail, the
// scan and the row pass csr_compact.h's (shared with K20).
// Integer and copy work only; the one atomic (the optional per-pair hit count) is an integer
// add, so two calls give identical bytes.
#include "als_common.h"
#include "csr_compact.h"

namespace als {

// One tile of stored entries per workgroup, walked by tile_row_walk (csr_tile_walk.h) over
// row_ptr_old with the rows' delete ranges in LDS beside their ends.  Thread t owns entries t,
// t + 256, ...; its eight keep flags stay in a register until every row batch is done, then
// tile_store_keep (csr_compact.h) makes the words.
__global__ __launch_bounds__(kTileThreads) void remove_mark_kernel(
    const int64_t* __restrict__ row_ptr_old, const int32_t* __restrict__ col_old,
    int64_t nnz_old, int32_t n_old, const int64_t* __restrict__ row_ptr_del,
    const int32_t* __restrict__ col_del, int64_t nnz_del, uint64_t* __restrict__ keep_bits,
    int32_t* __restrict__ tile_cnt, int32_t* __restrict__ del_hits) {
  __shared__ int64_t s_end[kTileThreads];   // P[r + 1]
  __shared__ int64_t s_del0[kTileThreads];  // D[r]
  __shared__ int64_t s_del1[kTileThreads];  // D[r + 1]
  __shared__ int32_t s_cnt[kTileWaves];
  const int64_t p0 = (int64_t)blockIdx.x * kTile;
  const int64_t p1 = p0 + kTile < nnz_old ? p0 + kTile : nnz_old;
  const int t = threadIdx.x;
  uint32_t keep = 0;  // bit i: entry p0 + i * 256 + t stays
  // P[n_old] = nnz_old > p0, so the tile's first row is below n_old
  tile_row_walk(
      p0, p1, csr_row_at(row_ptr_old, n_old, p0), s_end,
      [&](int64_t r) {
        int64_t end = nnz_old, d0 = 0, d1 = 0;  // past the last row: no entries, no deletes
        if (r < n_old) {
          end = row_ptr_old[r + 1];
          if (row_ptr_del != nullptr) {
            d0 = row_ptr_del[r];
            d1 = row_ptr_del[r + 1];
          }
        }
        s_end[t] = end;
        s_del0[t] = d0;
        s_del1[t] = d1;
      },
      [&](int i, int64_t q, int a, int64_t) {
        int64_t dl = s_del0[a], dh = s_del1[a];
        bool stays = true;
        if (dl < dh) {  // the row has a delete list: is this entry's column in it?
          if (dl < 0) dl = 0;
          if (dh > nnz_del) dh = nnz_del;
          const int64_t top = dh;
          const int32_t c = col_old[q];
          while (dl < dh) {  // first listed column >= c
            const int64_t mid = dl + ((dh - dl) >> 1);
            if (col_del[mid] < c) dl = mid + 1; else dh = mid;
          }
          if (dl < top && col_del[dl] == c) {
            stays = false;
            if (del_hits != nullptr) atomicAdd(del_hits + dl, 1);
          }
        }
        if (stays) keep |= 1u << i;
      });
  tile_store_keep(keep, p0, nnz_old, keep_bits, tile_cnt, s_cnt);
}

// One tile per workgroup.  The first wave loads the tile's words and scans their popcounts;
// an entry's place is tile_off[tile] + kept entries of the words before its own + kept bits
// below it in its word.  Loads of a wavefront are consecutive words, and so are its stores.
__global__ __launch_bounds__(kTileThreads) void remove_compact_kernel(
    const int32_t* __restrict__ col_old, const uint32_t* __restrict__ val_old, int64_t nnz_old,
    const uint64_t* __restrict__ keep_bits, const int64_t* __restrict__ tile_off,
    const int32_t* __restrict__ new_of_old_col, int32_t n_cols_old,
    int32_t* __restrict__ col_out, uint32_t* __restrict__ val_out, int64_t nnz_out) {
  __shared__ uint64_t s_word[kTileWords];
  __shared__ int32_t s_before[kTileWords];
  const int64_t p0 = (int64_t)blockIdx.x * kTile;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t n_words = (nnz_old + 63) >> 6;
  if (wave == 0) {
    const int64_t w = (p0 >> 6) + lane;
    const uint64_t word = (lane < kTileWords && w < n_words) ? keep_bits[w] : 0;
    const int32_t c = __popcll(word);
    int32_t incl = c;
#pragma unroll
    for (int d = 1; d < kTileWords; d <<= 1) {
      const int32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane < kTileWords) {
      s_word[lane] = word;
      s_before[lane] = incl - c;
    }
  }
  __syncthreads();
  const int64_t out0 = tile_off[blockIdx.x];
#pragma unroll
  for (int i = 0; i < kTileItems; ++i) {
    const int64_t q = p0 + i * kTileThreads + t;
    const int wi = i * kTileWaves + wave;
    const uint64_t word = s_word[wi];
    if (q >= nnz_old || !((word >> lane) & 1)) continue;
    const int64_t dst = out0 + s_before[wi] + __popcll(word & ((uint64_t(1) << lane) - 1));
    if (dst < 0 || dst >= nnz_out) continue;  // tile_off does not belong to these bits
    int32_t c = col_old[q];
    if (new_of_old_col != nullptr) c = (c >= 0 && c < n_cols_old) ? new_of_old_col[c] : -1;
    col_out[dst] = c;
    val_out[dst] = val_old[q];
  }
}

}  // namespace als

using namespace als;

extern "C" {

int32_t als_csr_remove_tile(void) { return kTile; }

size_t als_csr_remove_scratch_bytes(int64_t nnz_old, int32_t n_old) {
  (void)n_old;  // the row pass needs no scratch; kept in the signature for a later layout
  if (nnz_old < 0) return 0;
  const int64_t tiles = csr_tiles(nnz_old);
  return align_up((size_t)(tiles > 0 ? tiles : 1) * sizeof(int32_t));
}

int als_csr_remove_mark(const int64_t* row_ptr_old, const int32_t* col_old, int64_t nnz_old,
                        int32_t n_old, const int64_t* row_ptr_del, const int32_t* col_del,
                        int64_t nnz_del, uint64_t* keep_bits, int64_t* tile_off,
                        int64_t* row_ptr_kept, int32_t* del_hits, void* scratch,
                        size_t scratch_bytes, void* stream) {
  ALS_REQUIRE(nnz_old >= 0 && nnz_del >= 0 && n_old >= 0, ALS_EINVAL,
              "als_csr_remove_mark: negative size");
  ALS_REQUIRE(nnz_old < (int64_t(1) << 31) && n_old < 0x7fffffff, ALS_EUNSUPPORTED,
              "als_csr_remove_mark: nnz_old >= 2^31 or n_old >= 2^31 - 1 (K1's limit)");
  ALS_REQUIRE(row_ptr_old && tile_off && row_ptr_kept, ALS_EINVAL,
              "als_csr_remove_mark: null row_ptr_old / tile_off / row_ptr_kept");
  ALS_REQUIRE(nnz_old == 0 || (col_old && keep_bits), ALS_EINVAL,
              "als_csr_remove_mark: null col_old / keep_bits with nnz_old > 0");
  ALS_REQUIRE(nnz_del == 0 || (row_ptr_del && col_del), ALS_EINVAL,
              "als_csr_remove_mark: null row_ptr_del / col_del with nnz_del > 0");
  ALS_REQUIRE(scratch != nullptr, ALS_EINVAL, "als_csr_remove_mark: null scratch");
  ALS_REQUIRE(scratch_bytes >= als_csr_remove_scratch_bytes(nnz_old, n_old), ALS_EWORKSPACE,
              "als_csr_remove_mark: scratch of %zu bytes, %zu needed", scratch_bytes,
              als_csr_remove_scratch_bytes(nnz_old, n_old));
  hipStream_t st = as_stream(stream);
  const int64_t tiles = csr_tiles(nnz_old);
  int32_t* tile_cnt = static_cast<int32_t*>(scratch);
  if (nnz_del == 0) row_ptr_del = nullptr;  // a plain copy: every bit set
  if (del_hits != nullptr && nnz_del > 0)
    ALS_HIP(hipMemsetAsync(del_hits, 0, (size_t)nnz_del * sizeof(int32_t), st));
  if (tiles > 0) {
    remove_mark_kernel<<<(unsigned)tiles, kTileThreads, 0, st>>>(
        row_ptr_old, col_old, nnz_old, n_old, row_ptr_del, col_del, nnz_del, keep_bits, tile_cnt,
        del_hits);
    ALS_LAUNCH_CHECK();
  }
  return keep_finish(row_ptr_old, n_old, nnz_old, keep_bits, tile_cnt, tile_off, row_ptr_kept, st);
}

int als_csr_remove_compact(const int32_t* col_old, const float* val_old, int64_t nnz_old,
                           const uint64_t* keep_bits, const int64_t* tile_off,
                           const int32_t* new_of_old_col, int32_t n_cols_old, int32_t* col_out,
                           float* val_out, int64_t nnz_out, void* stream) {
  ALS_REQUIRE(nnz_old >= 0 && nnz_out >= 0 && n_cols_old >= 0, ALS_EINVAL,
              "als_csr_remove_compact: negative size");
  ALS_REQUIRE(nnz_old < (int64_t(1) << 31), ALS_EUNSUPPORTED,
              "als_csr_remove_compact: nnz_old >= 2^31 (K1's limit)");
  ALS_REQUIRE(nnz_out <= nnz_old, ALS_EINVAL,
              "als_csr_remove_compact: nnz_out %lld > nnz_old %lld (entries only leave)",
              (long long)nnz_out, (long long)nnz_old);
  ALS_REQUIRE(tile_off != nullptr, ALS_EINVAL, "als_csr_remove_compact: null tile_off");
  ALS_REQUIRE(nnz_old == 0 || (col_old && val_old && keep_bits), ALS_EINVAL,
              "als_csr_remove_compact: null col_old / val_old / keep_bits with nnz_old > 0");
  ALS_REQUIRE(nnz_out == 0 || (col_out && val_out), ALS_EINVAL,
              "als_csr_remove_compact: null col_out / val_out with nnz_out > 0");
  if (nnz_out == 0) return ALS_OK;
  remove_compact_kernel<<<(unsigned)csr_tiles(nnz_old), kTileThreads, 0,
                          as_stream(stream)>>>(
      col_old, reinterpret_cast<const uint32_t*>(val_old), nnz_old, keep_bits, tile_off,
      new_of_old_col, n_cols_old, col_out, reinterpret_cast<uint32_t*>(val_out), nnz_out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // extern "C"
