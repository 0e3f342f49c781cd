// The ranking key and the row filter shared by the ranking kernels: the top-k sweep
// (topk_sweep.h), the cosine neighbours (similar.hip) and the full-ranking positions
// (rank_positions.hip).
#pragma once
#include "als_common.h"

namespace als {

// Monotone key of a score that is not NaN: unsigned order = score order, -0 and +0 equal
// (the score's bits with the sign flipped).  NaN scores are never keys.
__device__ __forceinline__ uint32_t score_key(float sc) {
  const uint32_t u = __float_as_uint(sc + 0.f);  // -0 -> +0: equal scores, equal bits
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Lists hold (score, index) as one 64-bit key whose unsigned order is the ranking order:
// score descending, then index ascending.  High word = score_key, low word = ~index (a
// lower index ranks higher on equal scores).
__device__ __forceinline__ uint64_t rank_key(float sc, int id) {
  return ((uint64_t)score_key(sc) << 32) | (uint32_t)(~id);
}
__device__ __forceinline__ float rank_key_score(uint64_t key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ int rank_key_index(uint64_t key) { return (int)~(uint32_t)key; }
constexpr uint64_t kTkKeyOpen = 0;              // unfilled entry: any candidate ranks above it
constexpr uint64_t kTkKeySentinel = ~0ull;      // entries past `top`: nothing ranks above it

// Which table rows a query row may rank (als_topk_filtered, als_rank_positions): V row j is
// admissible for query row r only if bit j of `allow` is set (null: every row) and j is not
// in ex_col[ex_begin[r] .. ex_end[r]) (ascending, duplicates allowed; null: no exclusions).
// The arrays are indexed by the launch's query rows (the host offsets ex_begin / ex_end with
// Q for a sliced launch).
struct RowFilter {
  const int64_t* ex_begin;
  const int64_t* ex_end;
  const int32_t* ex_col;
  const uint32_t* allow;
};

__device__ __forceinline__ bool row_allowed(const RowFilter& f, int j) {
  return !f.allow || ((f.allow[j >> 5] >> (j & 31)) & 1u);
}

__device__ __forceinline__ bool row_excluded(const RowFilter& f, int64_t row, int j) {
  if (!f.ex_begin) return false;
  const int64_t end = f.ex_end[row];
  int64_t lo = f.ex_begin[row], hi = end;
  while (lo < hi) {  // lower bound of j in the row's range (one exit: no return inside)
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (f.ex_col[mid] < j) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && f.ex_col[lo] == j;
}

__device__ __forceinline__ bool row_admits(const RowFilter& f, int64_t row, int j) {
  return row_allowed(f, j) && !row_excluded(f, row, j);
}

// Host: the exclusion arrays come all null (no exclusions) or all set; `who` is the entry
// point named in the error text.
static inline int check_exclusion_args(const char* who, const int64_t* ex_begin,
                                       const int64_t* ex_end, const int32_t* ex_col) {
  const int n_ex = (ex_begin != nullptr) + (ex_end != nullptr) + (ex_col != nullptr);
  ALS_REQUIRE(n_ex == 0 || n_ex == 3, ALS_EINVAL,
              "%s: ex_begin, ex_end and ex_col must all be null or all be set", who);
  return ALS_OK;
}

}  // namespace als
