// K17 — add a batch of ratings to one CSR side without sorting it again.
//
// The reference appends a new user's ratings to the training set and fits again
// (RecommenderSystem.py:207-247); with K1 alone that means a fresh radix sort of every
// rating.  K1's layout makes the sort unnecessary: dense rows are in ascending id order
// and a row keeps its ratings in input order, so the CSR of concat(old, batch) is, row by
// row, the old segment (columns renumbered where new ids shifted the other side's dense
// rows) followed by the batch's ratings of that row.  With
//   O = row_ptr_out, A = row_ptr_add, P = row_ptr_old, j(r) = old rows placed before r
// the row pointer needs no scan, O[r] = P[j(r)] + A[r], and an output entry q of row r is
//   old entry  q - A[r]                  when q - A[r] < P[j(r+1)] = O[r+1] - A[r+1]
//   add entry  q - (O[r+1] - A[r+1])     otherwise,
// so the copy kernel reads nothing but O and A to place an entry.  One streaming pass:
// integer and copy work only, no atomics, every output word written exactly once.
#include "als_common.h"
#include "csr_tile_walk.h"

namespace als {

// O[r] = P[j(r)] + A[r], j(r) = #{old rows whose new row is < r}: a lower bound in the
// strictly increasing new_of_old_row (NULL = identity: j(r) = min(r, n_old)).
__global__ __launch_bounds__(256) void merge_row_ptr_kernel(
    const int64_t* __restrict__ row_ptr_old, int32_t n_old,
    const int32_t* __restrict__ new_of_old_row, const int64_t* __restrict__ row_ptr_add,
    int32_t n_new, int64_t* __restrict__ row_ptr_out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > n_new) return;
  int32_t j;
  if (new_of_old_row == nullptr) {
    j = r < n_old ? (int32_t)r : n_old;
  } else {
    int32_t lo = 0, hi = n_old;  // first j with new_of_old_row[j] >= r
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (new_of_old_row[mid] < r) lo = mid + 1; else hi = mid;
    }
    j = lo;
  }
  row_ptr_out[r] = row_ptr_old[j] + row_ptr_add[r];
}

// One tile of kTile output entries per workgroup, walked by tile_row_walk (csr_tile_walk.h)
// over O: beside a row's end the two source offsets go to LDS, and an entry needs nothing else
// to find its source.
__global__ __launch_bounds__(kTileThreads) void merge_copy_kernel(
    const int32_t* __restrict__ col_old, const uint32_t* __restrict__ val_old, int64_t nnz_old,
    const int32_t* __restrict__ new_of_old_col, int32_t n_cols_old,
    const int64_t* __restrict__ row_ptr_add, const int32_t* __restrict__ col_add,
    const uint32_t* __restrict__ val_add, int64_t nnz_add, int32_t n_new,
    const int64_t* __restrict__ row_ptr_out, int32_t* __restrict__ col_out,
    uint32_t* __restrict__ val_out) {
  __shared__ int64_t s_end[kTileThreads];   // O[r + 1]
  __shared__ int64_t s_add0[kTileThreads];  // A[r]
  __shared__ int64_t s_old1[kTileThreads];  // O[r + 1] - A[r + 1] = P[j(r + 1)]
  const int64_t nnz_out = nnz_old + nnz_add;
  const int64_t p0 = (int64_t)blockIdx.x * kTile;
  const int64_t p1 = p0 + kTile < nnz_out ? p0 + kTile : nnz_out;
  const int t = threadIdx.x;
  // O[n_new] = nnz_out > p0, so the tile's first row is below n_new
  tile_row_walk(
      p0, p1, csr_row_at(row_ptr_out, n_new, p0), s_end,
      [&](int64_t r) {
        int64_t end = nnz_out, add0 = nnz_add, old1 = nnz_old;  // past the last row: no entries
        if (r < n_new) {
          end = row_ptr_out[r + 1];
          add0 = row_ptr_add[r];
          old1 = end - row_ptr_add[r + 1];
        }
        s_end[t] = end;
        s_add0[t] = add0;
        s_old1[t] = old1;
      },
      [&](int, int64_t q, int a, int64_t) {
        const int64_t src_old = q - s_add0[a], o1 = s_old1[a];
        int32_t c = -1;
        uint32_t v = 0;
        if (src_old < o1) {
          if (src_old >= 0 && src_old < nnz_old) {
            c = col_old[src_old];
            v = val_old[src_old];
            if (new_of_old_col != nullptr)
              c = (c >= 0 && c < n_cols_old) ? new_of_old_col[c] : -1;
          }
        } else {
          const int64_t src_add = q - o1;
          if (src_add >= 0 && src_add < nnz_add) {
            c = col_add[src_add];
            v = val_add[src_add];
          }
        }
        col_out[q] = c;
        val_out[q] = v;
      });
}

}  // namespace als

using namespace als;

extern "C" {

int32_t als_csr_merge_tile(void) { return kTile; }

int als_csr_merge(const int64_t* row_ptr_old, const int32_t* col_old, const float* val_old,
                  int64_t nnz_old, int32_t n_old, int32_t n_cols_old,
                  const int32_t* new_of_old_row, const int32_t* new_of_old_col,
                  const int64_t* row_ptr_add, const int32_t* col_add, const float* val_add,
                  int64_t nnz_add, int32_t n_new, int64_t* row_ptr_out, int32_t* col_out,
                  float* val_out, void* stream) {
  ALS_REQUIRE(nnz_old >= 0 && nnz_add >= 0 && n_old >= 0 && n_new >= 0 && n_cols_old >= 0,
              ALS_EINVAL, "als_csr_merge: negative size");
  ALS_REQUIRE(n_new >= n_old, ALS_EINVAL, "als_csr_merge: n_new %d < n_old %d (rows never leave)",
              n_new, n_old);
  ALS_REQUIRE(n_new < 0x7fffffff && nnz_old + nnz_add < (int64_t(1) << 31), ALS_EUNSUPPORTED,
              "als_csr_merge: n_new >= 2^31 - 1 or nnz_old + nnz_add >= 2^31 (K1's limit)");
  ALS_REQUIRE(row_ptr_old && row_ptr_add && row_ptr_out, ALS_EINVAL,
              "als_csr_merge: null row pointer");
  ALS_REQUIRE(nnz_old == 0 || (col_old && val_old), ALS_EINVAL,
              "als_csr_merge: null col_old / val_old with nnz_old > 0");
  ALS_REQUIRE(nnz_add == 0 || (col_add && val_add), ALS_EINVAL,
              "als_csr_merge: null col_add / val_add with nnz_add > 0");
  const int64_t nnz_out = nnz_old + nnz_add;
  ALS_REQUIRE(nnz_out == 0 || (col_out && val_out), ALS_EINVAL,
              "als_csr_merge: null col_out / val_out");
  ALS_REQUIRE(new_of_old_row != nullptr || n_new == n_old || n_old == 0, ALS_EINVAL,
              "als_csr_merge: n_new > n_old needs new_of_old_row");
  hipStream_t st = as_stream(stream);
  merge_row_ptr_kernel<<<(unsigned)(((int64_t)n_new + 256) / 256), 256, 0, st>>>(
      row_ptr_old, n_old, new_of_old_row, row_ptr_add, n_new, row_ptr_out);
  ALS_LAUNCH_CHECK();
  if (nnz_out > 0) {
    merge_copy_kernel<<<(unsigned)csr_tiles(nnz_out), kTileThreads, 0, st>>>(
        col_old, reinterpret_cast<const uint32_t*>(val_old), nnz_old, new_of_old_col, n_cols_old,
        row_ptr_add, col_add, reinterpret_cast<const uint32_t*>(val_add), nnz_add, n_new,
        row_ptr_out, col_out, reinterpret_cast<uint32_t*>(val_out));
    ALS_LAUNCH_CHECK();
  }
  return ALS_OK;
}

}  // extern "C"
