// K20 — per-user holdout and stratified folds: which stored entries of a built rating set are
// held out, decided on the device from (seed, user id, item id) alone.
//
// Every stored rating gets a 64-bit key, splitmix64 of (user id << 32 | item id) and the seed
// (external ids, so the key of a pair is the same on either CSR side and whatever the dense row
// numbering).  On the SELECTING side (users for a per-user holdout) the eligible entries of a
// row are ranked by the composite (key, column); the entries whose rank falls in the row's window
// [lo, hi) are held out.  With anchors, the entry with the smallest (key, column) of every row
// of the OTHER side is not eligible, so no row of that side loses its last rating.
//   anchor      one pass over the other side: per row the column of its smallest composite.  A
//               wavefront per row; a row of more than kSplitTask entries is cut at the absolute
//               positions that are multiples of kSplitTask (at most two long rows meet such a
//               tile, so two slots per tile hold their partial minima without a task scan), and
//               the row's wavefront merges its slots.  A minimum is exact and order-free.
//   eligible    one pass over the selecting side: per row the entries that are no anchor.
//   thresholds  the selection.  Rows of up to row_cap entries: a wavefront per row, four rows
//               per workgroup, the row's composites in LDS (12 bytes an entry), every lane
//               counts the composites below its own (the reads are wave-wide broadcasts) and the
//               smallest composite of rank >= lo and of rank >= hi comes out of a shuffle tree.
//               Longer rows are appended to a list (an integer atomic; the list's order changes
//               no result) and a workgroup per listed row selects by radix on the key's bytes,
//               most significant first, both ranks at once in two LDS histograms, then resolves
//               ties on (key, column) exactly.  No limit on the row length.
//   mark        the tile of csr_tile_walk.h over the stored entries of either side: the entry's
//               row from tile_row_walk, its key, its selecting-side row's two thresholds and
//               the anchor; one ballot per 64 entries.  keep_bits, tile_off and row_ptr_kept
//               are K18's (csr_compact.h finishes both), so als_csr_remove_compact reads them
//               unchanged.
// Integer work only.  The atomics are integer adds and minima on LDS words and one integer add
// on a list counter the call zeroes itself: two calls give identical bytes.
#include "als_common.h"
#include "csr_compact.h"
#include "csr_tile_walk.h"

namespace als {

constexpr int kSplitRowCap = 1024;   // als_split_row_cap(): longest row ranked in LDS
constexpr int kSplitRowWaves = 4;    // rows (wavefronts) per workgroup of the per-row kernels
constexpr int kSplitTask = 2048;     // entries per tile of a long row in als_split_anchor
constexpr int kSplitLongGrid = 2048; // workgroups dealt over the listed long rows
constexpr uint64_t kKeyEnd = ~uint64_t(0);
constexpr int32_t kColEnd = 0x7fffffff;  // (kKeyEnd, kColEnd): beyond the last composite

struct SplitSide {
  const int64_t* __restrict__ row_ptr;
  const int32_t* __restrict__ col;
  int64_t nnz;
  int32_t n_rows, n_cols;
  const int32_t* __restrict__ row_ids;
  const int32_t* __restrict__ col_ids;
  int rows_are_users;
  uint64_t add;  // (seed + 1) * 0x9E3779B97F4A7C15
};

struct Comp {
  uint64_t key;
  int32_t col;
};

__device__ __forceinline__ bool comp_less(const Comp& a, const Comp& b) {
  return a.key < b.key || (a.key == b.key && a.col < b.col);
}

// row < n_rows and 0 <= c < n_cols are the caller's to check
__device__ __forceinline__ uint64_t split_key(const SplitSide& s, int32_t row, int32_t c) {
  const uint64_t a = (uint32_t)s.row_ids[row], b = (uint32_t)s.col_ids[c];
  uint64_t z = (s.rows_are_users ? (a << 32) | b : (b << 32) | a) + s.add;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the smallest composite of the wavefront, in every lane
__device__ __forceinline__ Comp comp_wave_min(Comp a) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    Comp b;
    b.key = shfl_xor_64(a.key, m);
    b.col = __shfl_xor(a.col, m);
    if (comp_less(b, a)) a = b;
  }
  return a;
}

// Row bounds inside [0, nnz] and ordered, whatever row_ptr holds.
__device__ __forceinline__ void split_bounds(const SplitSide& s, int64_t row, int64_t& pb,
                                             int64_t& pe) {
  pb = s.row_ptr[row];
  pe = s.row_ptr[row + 1];
  if (pb < 0) pb = 0;
  if (pe > s.nnz) pe = s.nnz;
  if (pe < pb) pe = pb;
}

// the last row r in [0, n_rows) with row_ptr[r] <= p (n_rows >= 1)
__device__ __forceinline__ int32_t split_row_at(const SplitSide& s, int64_t p) {
  return csr_row_at(s.row_ptr, s.n_rows - 1, p);
}

__device__ __forceinline__ bool split_eligible(const int32_t* __restrict__ anchor, int32_t row,
                                               int32_t c) {
  return anchor == nullptr || anchor[c] != row;
}

// ---- anchor ----

// The smallest composite of entries [lo, hi) of `row`, by the whole workgroup, in every thread.
__device__ __forceinline__ Comp anchor_range_block(const SplitSide& s, int32_t row, int64_t lo,
                                                   int64_t hi, Comp* sm) {
  Comp best{kKeyEnd, kColEnd};
  for (int64_t q = lo + threadIdx.x; q < hi; q += 256) {
    const int32_t c = s.col[q];
    if (c < 0 || c >= s.n_cols) continue;
    const Comp x{split_key(s, row, c), c};
    if (comp_less(x, best)) best = x;
  }
  best = comp_wave_min(best);
  __syncthreads();  // sm may still be read from the previous range
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (comp_less(sm[w], best)) best = sm[w];
  return best;
}

// One workgroup per tile [p0, p0 + kSplitTask) of stored entries.  A row longer than a tile
// that holds p0 leaves its partial in slot 2 t, one that starts inside the tile in slot 2 t + 1;
// no third long row can meet the tile.  Tiles that meet no long row only search.
__global__ __launch_bounds__(256) void split_anchor_task_kernel(SplitSide s,
                                                                uint64_t* __restrict__ slot_key,
                                                                int32_t* __restrict__ slot_col) {
  __shared__ Comp sm[4];
  const int64_t p0 = (int64_t)blockIdx.x * kSplitTask;
  const int64_t p1 = p0 + kSplitTask < s.nnz ? p0 + kSplitTask : s.nnz;
  const int32_t r0 = split_row_at(s, p0);
  int64_t pb, pe;
  split_bounds(s, r0, pb, pe);
  if (pe - pb > kSplitTask) {
    const Comp m = anchor_range_block(s, r0, pb > p0 ? pb : p0, pe < p1 ? pe : p1, sm);
    if (threadIdx.x == 0) {
      slot_key[2 * (int64_t)blockIdx.x] = m.key;
      slot_col[2 * (int64_t)blockIdx.x] = m.col;
    }
  }
  const int32_t r1 = split_row_at(s, p1 - 1);
  if (r1 == r0) return;
  split_bounds(s, r1, pb, pe);
  if (pe - pb > kSplitTask) {
    const Comp m = anchor_range_block(s, r1, pb > p0 ? pb : p0, pe < p1 ? pe : p1, sm);
    if (threadIdx.x == 0) {
      slot_key[2 * (int64_t)blockIdx.x + 1] = m.key;
      slot_col[2 * (int64_t)blockIdx.x + 1] = m.col;
    }
  }
}

// A wavefront per row: a short row is read here, a long row's slots are merged here.
__global__ __launch_bounds__(64 * kSplitRowWaves) void split_anchor_rows_kernel(
    SplitSide s, const uint64_t* __restrict__ slot_key, const int32_t* __restrict__ slot_col,
    int64_t tiles, int32_t* __restrict__ anchor) {
  const int64_t row = (int64_t)blockIdx.x * kSplitRowWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= s.n_rows) return;
  int64_t pb, pe;
  split_bounds(s, row, pb, pe);
  Comp best{kKeyEnd, kColEnd};
  if (pe - pb <= kSplitTask) {
    for (int64_t q = pb + lane; q < pe; q += 64) {
      const int32_t c = s.col[q];
      if (c < 0 || c >= s.n_cols) continue;
      const Comp x{split_key(s, (int32_t)row, c), c};
      if (comp_less(x, best)) best = x;
    }
  } else {
    int64_t t1 = (pe - 1) / kSplitTask;
    if (t1 >= tiles) t1 = tiles - 1;
    for (int64_t t = pb / kSplitTask + lane; t <= t1; t += 64) {
      const int64_t slot = 2 * t + (t * kSplitTask >= pb ? 0 : 1);
      const Comp x{slot_key[slot], slot_col[slot]};
      if (comp_less(x, best)) best = x;
    }
  }
  best = comp_wave_min(best);
  if (lane == 0) anchor[row] = best.col == kColEnd ? -1 : best.col;
}

// ---- eligible ----

__global__ __launch_bounds__(64 * kSplitRowWaves) void split_eligible_kernel(
    SplitSide s, const int32_t* __restrict__ anchor, int32_t* __restrict__ eligible) {
  const int64_t row = (int64_t)blockIdx.x * kSplitRowWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= s.n_rows) return;
  int64_t pb, pe;
  split_bounds(s, row, pb, pe);
  int32_t n = 0;
  for (int64_t q = pb + lane; q < pe; q += 64) {
    const int32_t c = s.col[q];
    if (c >= 0 && c < s.n_cols && split_eligible(anchor, (int32_t)row, c)) ++n;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m);
  if (lane == 0) eligible[row] = n;
}

// ---- thresholds ----

struct SplitThr {
  uint64_t* __restrict__ lo_key;
  int32_t* __restrict__ lo_col;
  uint64_t* __restrict__ hi_key;
  int32_t* __restrict__ hi_col;
};

__device__ __forceinline__ int64_t split_window(const int32_t* __restrict__ w, int64_t row) {
  const int32_t k = w[row];
  return k < 0 ? 0 : k;
}

// A wavefront per row of at most `cap` entries; longer rows go to the list.
__global__ __launch_bounds__(64 * kSplitRowWaves) void split_thr_rows_kernel(
    SplitSide s, const int32_t* __restrict__ anchor, const int32_t* __restrict__ win_lo,
    const int32_t* __restrict__ win_hi, int32_t cap, SplitThr out,
    int32_t* __restrict__ long_count, int32_t* __restrict__ long_rows) {
  __shared__ uint64_t s_key[kSplitRowWaves][kSplitRowCap];
  __shared__ int32_t s_col[kSplitRowWaves][kSplitRowCap];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kSplitRowWaves + wave;
  const bool in_side = row < s.n_rows;
  int64_t pb = 0, pe = 0;
  if (in_side) split_bounds(s, row, pb, pe);
  const bool listed = pe - pb > cap;
  const int len = listed ? 0 : (int)(pe - pb);
  if (listed && lane == 0) {
    const int32_t at = atomicAdd(long_count, 1);
    if (at >= 0 && at < s.n_rows) long_rows[at] = (int32_t)row;
  }
  for (int j = lane; j < len; j += 64) {
    const int32_t c = s.col[pb + j];
    Comp x{kKeyEnd, kColEnd};  // not eligible: above every composite, never counted
    if (c >= 0 && c < s.n_cols && split_eligible(anchor, (int32_t)row, c))
      x = Comp{split_key(s, (int32_t)row, c), c};
    s_key[wave][j] = x.key;
    s_col[wave][j] = x.col;
  }
  __syncthreads();
  if (!in_side || listed) return;
  const int64_t k_lo = split_window(win_lo, row), k_hi = split_window(win_hi, row);
  Comp b_lo{kKeyEnd, kColEnd}, b_hi{kKeyEnd, kColEnd};
  for (int j = lane; j < len; j += 64) {
    const Comp x{s_key[wave][j], s_col[wave][j]};
    if (x.col == kColEnd) continue;
    int64_t rank = 0;
    for (int i = 0; i < len; ++i) rank += comp_less(Comp{s_key[wave][i], s_col[wave][i]}, x);
    if (rank >= k_lo && comp_less(x, b_lo)) b_lo = x;
    if (rank >= k_hi && comp_less(x, b_hi)) b_hi = x;
  }
  b_lo = comp_wave_min(b_lo);
  b_hi = comp_wave_min(b_hi);
  if (lane == 0) {
    out.lo_key[row] = b_lo.key;
    out.lo_col[row] = b_lo.col;
    out.hi_key[row] = b_hi.key;
    out.hi_col[row] = b_hi.col;
  }
}

struct LongShared {
  uint32_t hist[2][256];
  uint64_t prefix[2];
  int64_t k[2];
  int32_t done[2];
  unsigned long long m64;
  int32_t m32;
  int32_t cnt;
};

// f(key, col) for every eligible entry of the row, by the whole workgroup
template <class F>
__device__ __forceinline__ void long_scan(const SplitSide& s, const int32_t* __restrict__ anchor,
                                          int32_t row, int64_t pb, int64_t pe, F f) {
  for (int64_t q = pb + threadIdx.x; q < pe; q += 256) {
    const int32_t c = s.col[q];
    if (c >= 0 && c < s.n_cols && split_eligible(anchor, row, c)) f(split_key(s, row, c), c);
  }
}

// The smallest composite of rank >= k given the radix select's key (the key of the k-th
// eligible entry in sorted order) and `need`, the entries with that key that must lie below.
__device__ Comp long_resolve(const SplitSide& s, const int32_t* __restrict__ anchor, int32_t row,
                             int64_t pb, int64_t pe, uint64_t key, int64_t need, LongShared& sh) {
  int32_t cur = -1;
  int64_t below = 0;
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) sh.m32 = kColEnd;
    __syncthreads();
    long_scan(s, anchor, row, pb, pe, [&](uint64_t k, int32_t c) {
      if (k == key && c > cur) atomicMin(&sh.m32, c);
    });
    __syncthreads();
    const int32_t c0 = sh.m32;
    if (c0 == kColEnd) break;           // every entry of this key lies below rank k
    if (below >= need) return Comp{key, c0};
    __syncthreads();
    if (threadIdx.x == 0) sh.cnt = 0;
    __syncthreads();
    long_scan(s, anchor, row, pb, pe, [&](uint64_t k, int32_t c) {
      if (k == key && c == c0) atomicAdd(&sh.cnt, 1);
    });
    __syncthreads();
    below += sh.cnt;
    cur = c0;
  }
  // copies of one pair straddle rank k: the next key's smallest column, or the end
  __syncthreads();
  if (threadIdx.x == 0) sh.m64 = kKeyEnd;
  __syncthreads();
  long_scan(s, anchor, row, pb, pe, [&](uint64_t k, int32_t) {
    if (k > key) atomicMin(&sh.m64, (unsigned long long)k);
  });
  __syncthreads();
  const uint64_t next = sh.m64;
  __syncthreads();
  if (threadIdx.x == 0) sh.m32 = kColEnd;
  __syncthreads();
  long_scan(s, anchor, row, pb, pe, [&](uint64_t k, int32_t c) {
    if (k == next && k > key) atomicMin(&sh.m32, c);
  });
  __syncthreads();
  const int32_t c1 = sh.m32;
  return c1 == kColEnd ? Comp{kKeyEnd, kColEnd} : Comp{next, c1};
}

// A workgroup per listed row: eight histogram passes over the key's bytes for both ranks,
// then the tie resolve.
__global__ __launch_bounds__(256) void split_thr_long_kernel(
    SplitSide s, const int32_t* __restrict__ anchor, const int32_t* __restrict__ win_lo,
    const int32_t* __restrict__ win_hi, SplitThr out, const int32_t* __restrict__ long_count,
    const int32_t* __restrict__ long_rows) {
  __shared__ LongShared sh;
  int32_t n_long = *long_count;
  if (n_long > s.n_rows) n_long = s.n_rows;
  const int t = threadIdx.x;
  for (int32_t j = blockIdx.x; j < n_long; j += gridDim.x) {
    const int32_t row = long_rows[j];
    if (row < 0 || row >= s.n_rows) continue;
    int64_t pb, pe;
    split_bounds(s, row, pb, pe);
    __syncthreads();  // the previous row's state has been read
    if (t < 2) {
      sh.prefix[t] = 0;
      sh.k[t] = split_window(t == 0 ? win_lo : win_hi, row);
      sh.done[t] = 0;
    }
    for (int b = 7; b >= 0; --b) {
      __syncthreads();
      sh.hist[0][t] = 0;
      sh.hist[1][t] = 0;
      __syncthreads();
      const uint64_t pre0 = sh.prefix[0], pre1 = sh.prefix[1];
      const bool on0 = !sh.done[0], on1 = !sh.done[1];
      const int up = 8 * (b + 1);  // bits above this byte must match the prefix
      long_scan(s, anchor, row, pb, pe, [&](uint64_t k, int32_t) {
        const uint32_t d = (uint32_t)(k >> (8 * b)) & 255u;
        if (on0 && (b == 7 || (k >> up) == (pre0 >> up))) atomicAdd(&sh.hist[0][d], 1u);
        if (on1 && (b == 7 || (k >> up) == (pre1 >> up))) atomicAdd(&sh.hist[1][d], 1u);
      });
      __syncthreads();
      if (t < 2 && !sh.done[t]) {
        int64_t k = sh.k[t], cum = 0;
        int d = 0;
        for (; d < 256; ++d) {
          const int64_t h = sh.hist[t][d];
          if (k < cum + h) break;
          cum += h;
        }
        if (d == 256) {
          sh.done[t] = 1;  // the rank is past the last eligible entry
        } else {
          sh.prefix[t] |= (uint64_t)d << (8 * b);
          sh.k[t] = k - cum;
        }
      }
    }
    __syncthreads();
    Comp ans[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const bool done = sh.done[w] != 0;
      const uint64_t key = sh.prefix[w];
      const int64_t need = sh.k[w];
      ans[w] = done ? Comp{kKeyEnd, kColEnd}
                    : long_resolve(s, anchor, row, pb, pe, key, need, sh);
    }
    if (t == 0) {
      out.lo_key[row] = ans[0].key;
      out.lo_col[row] = ans[0].col;
      out.hi_key[row] = ans[1].key;
      out.hi_col[row] = ans[1].col;
    }
  }
}

// ---- mark ----

// The tile and row walk of csr_tile_walk.h and the keep-bits tail of csr_compact.h, as in K18's
// mark kernel, with the window predicate per entry and nothing but the row's end in LDS.
// selecting: the thresholds belong to this side's rows and the anchors to its columns; else
// the other way.
__global__ __launch_bounds__(kTileThreads) void split_mark_kernel(
    SplitSide s, int selecting, const uint64_t* __restrict__ lo_key,
    const int32_t* __restrict__ lo_col, const uint64_t* __restrict__ hi_key,
    const int32_t* __restrict__ hi_col, const int32_t* __restrict__ anchor,
    uint64_t* __restrict__ keep_bits, int32_t* __restrict__ tile_cnt) {
  __shared__ int64_t s_end[kTileThreads];  // P[r + 1]
  __shared__ int32_t s_cnt[kTileWaves];
  const int64_t p0 = (int64_t)blockIdx.x * kTile;
  const int64_t p1 = p0 + kTile < s.nnz ? p0 + kTile : s.nnz;
  uint32_t keep = 0;  // bit i: entry p0 + i * 256 + t stays
  tile_row_walk(
      p0, p1, split_row_at(s, p0), s_end,
      [&](int64_t r) {  // past the last row: no entries
        s_end[threadIdx.x] = r < s.n_rows ? s.row_ptr[r + 1] : s.nnz;
      },
      [&](int i, int64_t q, int, int64_t row) {
        const int32_t c = s.col[q];
        bool stays = true;
        if (row < s.n_rows && c >= 0 && c < s.n_cols) {
          const int32_t sel = selecting ? (int32_t)row : c;    // row of the selecting side
          const int32_t oth = selecting ? c : (int32_t)row;    // row of the other side
          if (anchor == nullptr || anchor[oth] != sel) {
            const Comp x{split_key(s, (int32_t)row, c), oth};
            const Comp lo{lo_key[sel], lo_col[sel]}, hi{hi_key[sel], hi_col[sel]};
            stays = comp_less(x, lo) || !comp_less(x, hi);
          }
        }
        if (stays) keep |= 1u << i;
      });
  tile_store_keep(keep, p0, s.nnz, keep_bits, tile_cnt, s_cnt);
}

static inline int64_t split_tasks(int64_t nnz) { return (nnz + kSplitTask - 1) / kSplitTask; }

static inline unsigned split_row_grid(int32_t n_rows) {
  return (unsigned)(((int64_t)n_rows + kSplitRowWaves - 1) / kSplitRowWaves);
}

static inline SplitSide split_side(const int64_t* row_ptr, const int32_t* col, int64_t nnz,
                                   int32_t n_rows, int32_t n_cols, const int32_t* row_ids,
                                   const int32_t* col_ids, int32_t rows_are_users, int64_t seed) {
  return SplitSide{row_ptr, col, nnz, n_rows, n_cols, row_ids, col_ids, rows_are_users != 0,
                   ((uint64_t)seed + 1) * 0x9E3779B97F4A7C15ull};
}

}  // namespace als

using namespace als;

// what every entry point checks of the side it is given
#define SPLIT_REQUIRE_SIDE(who)                                                                 \
  ALS_REQUIRE(nnz >= 0 && n_rows >= 0 && n_cols >= 0, ALS_EINVAL, who ": negative size");       \
  ALS_REQUIRE(nnz < (int64_t(1) << 31) && n_rows < 0x7fffffff && n_cols < 0x7fffffff,           \
              ALS_EUNSUPPORTED, who ": nnz >= 2^31 or a side of 2^31 - 1 rows (K1's limit)");   \
  ALS_REQUIRE(row_ptr != nullptr, ALS_EINVAL, who ": null row_ptr");                            \
  ALS_REQUIRE(nnz == 0 || (col && row_ids && col_ids && n_rows > 0), ALS_EINVAL,                \
              who ": null col / row_ids / col_ids, or no rows, with nnz > 0")

extern "C" {

int32_t als_split_row_cap(void) { return kSplitRowCap; }

size_t als_split_scratch_bytes(int64_t nnz, int32_t n_rows) {
  if (nnz < 0 || n_rows < 0) return 0;
  const int64_t tasks = split_tasks(nnz);
  ArenaSize anchor;
  anchor.take<uint64_t>((size_t)(tasks > 0 ? 2 * tasks : 1));
  anchor.take<int32_t>((size_t)(tasks > 0 ? 2 * tasks : 1));
  ArenaSize thr;
  thr.take<int32_t>(1);
  thr.take<int32_t>((size_t)(n_rows > 0 ? n_rows : 1));
  const size_t mark = als_csr_remove_scratch_bytes(nnz, n_rows);
  size_t need = anchor.off > thr.off ? anchor.off : thr.off;
  return need > mark ? need : mark;
}

int als_split_anchor(const int64_t* row_ptr, const int32_t* col, int64_t nnz, int32_t n_rows,
                     int32_t n_cols, const int32_t* row_ids, const int32_t* col_ids,
                     int32_t rows_are_users, int64_t seed, int32_t* anchor, void* scratch,
                     size_t scratch_bytes, void* stream) {
  SPLIT_REQUIRE_SIDE("als_split_anchor");
  ALS_REQUIRE(n_rows == 0 || anchor != nullptr, ALS_EINVAL, "als_split_anchor: null anchor");
  ALS_REQUIRE(scratch != nullptr, ALS_EINVAL, "als_split_anchor: null scratch");
  ALS_REQUIRE(scratch_bytes >= als_split_scratch_bytes(nnz, n_rows), ALS_EWORKSPACE,
              "als_split_anchor: scratch of %zu bytes, %zu needed", scratch_bytes,
              als_split_scratch_bytes(nnz, n_rows));
  if (n_rows == 0) return ALS_OK;
  hipStream_t st = as_stream(stream);
  const SplitSide s = split_side(row_ptr, col, nnz, n_rows, n_cols, row_ids, col_ids,
                                 rows_are_users, seed);
  const int64_t tasks = split_tasks(nnz);
  Arena arena(scratch, scratch_bytes);
  uint64_t* slot_key = arena.take<uint64_t>((size_t)(tasks > 0 ? 2 * tasks : 1));
  int32_t* slot_col = arena.take<int32_t>((size_t)(tasks > 0 ? 2 * tasks : 1));
  if (tasks > 0) {
    split_anchor_task_kernel<<<(unsigned)tasks, 256, 0, st>>>(s, slot_key, slot_col);
    ALS_LAUNCH_CHECK();
  }
  split_anchor_rows_kernel<<<split_row_grid(n_rows), 64 * kSplitRowWaves, 0, st>>>(
      s, slot_key, slot_col, tasks, anchor);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

int als_split_eligible(const int64_t* row_ptr, const int32_t* col, int64_t nnz, int32_t n_rows,
                       int32_t n_cols, const int32_t* anchor, int32_t* eligible, void* stream) {
  ALS_REQUIRE(nnz >= 0 && n_rows >= 0 && n_cols >= 0, ALS_EINVAL,
              "als_split_eligible: negative size");
  ALS_REQUIRE(nnz < (int64_t(1) << 31) && n_rows < 0x7fffffff && n_cols < 0x7fffffff,
              ALS_EUNSUPPORTED, "als_split_eligible: nnz >= 2^31 or a side of 2^31 - 1 rows");
  ALS_REQUIRE(row_ptr != nullptr && (nnz == 0 || col != nullptr), ALS_EINVAL,
              "als_split_eligible: null row_ptr / col");
  ALS_REQUIRE(n_rows == 0 || eligible != nullptr, ALS_EINVAL,
              "als_split_eligible: null eligible");
  if (n_rows == 0) return ALS_OK;
  const SplitSide s = split_side(row_ptr, col, nnz, n_rows, n_cols, nullptr, nullptr, 1, 0);
  split_eligible_kernel<<<split_row_grid(n_rows), 64 * kSplitRowWaves, 0, as_stream(stream)>>>(
      s, anchor, eligible);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

int als_split_thresholds(const int64_t* row_ptr, const int32_t* col, int64_t nnz, int32_t n_rows,
                         int32_t n_cols, const int32_t* row_ids, const int32_t* col_ids,
                         int32_t rows_are_users, int64_t seed, const int32_t* anchor,
                         const int32_t* win_lo, const int32_t* win_hi, int32_t row_cap,
                         uint64_t* thr_lo_key, int32_t* thr_lo_col, uint64_t* thr_hi_key,
                         int32_t* thr_hi_col, void* scratch, size_t scratch_bytes, void* stream) {
  SPLIT_REQUIRE_SIDE("als_split_thresholds");
  ALS_REQUIRE(row_cap >= 0 && row_cap <= kSplitRowCap, ALS_EINVAL,
              "als_split_thresholds: row_cap %d outside [0, %d]", row_cap, kSplitRowCap);
  ALS_REQUIRE(n_rows == 0 || (win_lo && win_hi && thr_lo_key && thr_lo_col && thr_hi_key &&
                              thr_hi_col),
              ALS_EINVAL, "als_split_thresholds: null window or threshold array");
  ALS_REQUIRE(scratch != nullptr, ALS_EINVAL, "als_split_thresholds: null scratch");
  ALS_REQUIRE(scratch_bytes >= als_split_scratch_bytes(nnz, n_rows), ALS_EWORKSPACE,
              "als_split_thresholds: scratch of %zu bytes, %zu needed", scratch_bytes,
              als_split_scratch_bytes(nnz, n_rows));
  if (n_rows == 0) return ALS_OK;
  hipStream_t st = as_stream(stream);
  const SplitSide s = split_side(row_ptr, col, nnz, n_rows, n_cols, row_ids, col_ids,
                                 rows_are_users, seed);
  Arena arena(scratch, scratch_bytes);
  int32_t* long_count = arena.take<int32_t>(1);
  int32_t* long_rows = arena.take<int32_t>((size_t)n_rows);
  const SplitThr out{thr_lo_key, thr_lo_col, thr_hi_key, thr_hi_col};
  ALS_HIP(hipMemsetAsync(long_count, 0, sizeof(int32_t), st));
  split_thr_rows_kernel<<<split_row_grid(n_rows), 64 * kSplitRowWaves, 0, st>>>(
      s, anchor, win_lo, win_hi, row_cap > 0 ? row_cap : kSplitRowCap, out, long_count,
      long_rows);
  ALS_LAUNCH_CHECK();
  const unsigned grid = (unsigned)(n_rows < kSplitLongGrid ? n_rows : kSplitLongGrid);
  split_thr_long_kernel<<<grid, 256, 0, st>>>(s, anchor, win_lo, win_hi, out, long_count,
                                              long_rows);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

int als_split_mark(const int64_t* row_ptr, const int32_t* col, int64_t nnz, int32_t n_rows,
                   int32_t n_cols, const int32_t* row_ids, const int32_t* col_ids,
                   int32_t rows_are_users, int64_t seed, int32_t selecting,
                   const uint64_t* thr_lo_key, const int32_t* thr_lo_col,
                   const uint64_t* thr_hi_key, const int32_t* thr_hi_col, const int32_t* anchor,
                   uint64_t* keep_bits, int64_t* tile_off, int64_t* row_ptr_kept, void* scratch,
                   size_t scratch_bytes, void* stream) {
  SPLIT_REQUIRE_SIDE("als_split_mark");
  ALS_REQUIRE(tile_off && row_ptr_kept, ALS_EINVAL,
              "als_split_mark: null tile_off / row_ptr_kept");
  ALS_REQUIRE(nnz == 0 || (keep_bits && thr_lo_key && thr_lo_col && thr_hi_key && thr_hi_col),
              ALS_EINVAL, "als_split_mark: null keep_bits or threshold array with nnz > 0");
  ALS_REQUIRE(scratch != nullptr, ALS_EINVAL, "als_split_mark: null scratch");
  ALS_REQUIRE(scratch_bytes >= als_split_scratch_bytes(nnz, n_rows), ALS_EWORKSPACE,
              "als_split_mark: scratch of %zu bytes, %zu needed", scratch_bytes,
              als_split_scratch_bytes(nnz, n_rows));
  hipStream_t st = as_stream(stream);
  const SplitSide s = split_side(row_ptr, col, nnz, n_rows, n_cols, row_ids, col_ids,
                                 rows_are_users, seed);
  const int64_t tiles = csr_tiles(nnz);
  int32_t* tile_cnt = static_cast<int32_t*>(scratch);
  if (tiles > 0) {
    split_mark_kernel<<<(unsigned)tiles, kTileThreads, 0, st>>>(
        s, selecting != 0, thr_lo_key, thr_lo_col, thr_hi_key, thr_hi_col, anchor, keep_bits,
        tile_cnt);
    ALS_LAUNCH_CHECK();
  }
  return keep_finish(row_ptr, n_rows, nnz, keep_bits, tile_cnt, tile_off, row_ptr_kept, st);
}

}  // extern "C"
