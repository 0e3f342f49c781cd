// K16 — rating statistics and bias baselines: per-row moments of one CSR side, the damped
// bias update and the mu + b_u + b_i predictor.
//
// Replaces the reference's getCountsAndAverages / "more than 500 reviews" filter
// (RecommenderSystem.py:49-86, an RDD groupByKey) and its training-mean baseline
// (RecommenderSystem.py:172-177); with a bias table it is the sweep behind Koren's damped
// baseline predictor.  Spark itself has neither.
//
// als_row_moments: over the terms e_j = (double)val_j - offset - (other ? other[col_j] : 0) of
// every row (a col_j outside [0, n_cols) takes 0 from `other` and is not dereferenced),
//   moments[row] = { n, sum, M2 = sum (e - mean_row)^2, min, max }   (fp64; min = max = NaN
//   when n = 0), and total[5] = the same five over all ratings of the side.
// Everything is accumulated in fp64.  M2 is never formed as sum e^2 - sum^2 / n: four
// consecutive ratings are folded two-pass (their sum, their mean, the squared deviations from
// it) and every further step is Chan's merge
//   d = mean_b - mean_a,  mean = mean_a + d n_b / n,  M2 = M2_a + M2_b + d^2 n_a n_b / n,
// as regression_metrics.hip merges; an empty side is the identity.  No atomics: the order of
// the additions is a function of row_ptr alone, so two calls give identical bytes.
//
// Layout.  Of the two models in the tree — the rating-span walk of objective.hip and the "long
// rows split into tasks" of nnls.hip — this file takes the second: the output here is per ROW,
// and a span walk would have to publish and later merge a partial for every row a span boundary
// cuts, short rows included; with row-relative tasks only rows longer than a task have
// partials, and a short row is finished by the lanes that read it.
//   quads   Ratings are read as QUADS, the four ratings 4 q .. 4 q + 3 of the side (absolute
//           positions, so a quad is 16-byte aligned whenever col / val are): one 16-byte load
//           of val, and of col when `other` is given, for a quad wholly inside the range being
//           read; a quad cut by the range's ends, or any quad of a misaligned table, is read
//           with up to four scalar loads.  Both forms give the same terms to the same lane in
//           the same order.  Without `other`, col is never read (4 bytes per rating).
//   rows    A 16-lane group per row, kRsGroupRows = 16 rows per 256-thread workgroup, so a
//           one-rating row costs a quarter of a wavefront and not a workgroup.  Lane l takes the
//           row's quads l, l + 16, ... in that order; the 16 lanes are merged by a shuffle tree
//           (lane l with l + s, s = 8 .. 1, the lower lane on the left).
//   tasks   A row of more than kRsTask = 1024 ratings is cut into 1024-rating tasks, numbered
//           by an exclusive scan of the rows' task counts (csr_build.hip's scan).  One
//           workgroup per task: a thread takes one quad (two when the task starts inside a
//           quad), the 64 lanes of a wavefront are merged by the same tree, the four wavefronts
//           in order, and the six numbers go to the task's slot in the scratch.  The row's
//           group then merges the row's slots in ascending task order.  Fewer than
//           2 nnz / kRsTask slots exist whatever the shape, which sizes the scratch.
//   total   From the moments table, rows in ascending order: a thread merges four consecutive
//           rows, a workgroup 1024, one final workgroup the per-workgroup partials (each thread
//           its partials ascending, then the tree).  n and sum, plain sums, go through
//           partial_sums.h.
// The `other` gather is the only irregular access; the table is n_cols doubles, a few MB at
// most, and stays in L2 / Infinity Cache while col and val stream past it.
//
// als_bias_update is its own entry point, not an optional output of the sweep: the sweep's
// ABI stays that of a statistics pass, and the update is one thread per row over a table the
// sweep has just written.  als_baseline_predict is one thread per pair.
#include <cmath>

#include "als_common.h"
#include "partial_sums.h"

namespace als {

constexpr int kRsTask = 1024;      // ratings per task of a long row (als_rating_stats_task)
constexpr int kRsGroupRows = 16;   // rows per workgroup (als_rating_stats_group_rows)
constexpr int kRsSlot = 6;         // doubles per task slot: n, sum, mean, M2, min, max
constexpr int kRsOut = 5;          // n, sum, M2, min, max
constexpr int kRsTotalRows = 1024;  // rows per workgroup of the total's first level
constexpr int kRsTotalPart = 5;    // n, mean, M2, min, max

struct RowMom {
  double n = 0.0, sum = 0.0, mean = 0.0, m2 = 0.0;
  double mn = INFINITY, mx = -INFINITY;
};

// Chan's rule, a on the left; an empty side is the identity (0 / 0 never formed).
__device__ __forceinline__ RowMom rs_merge(const RowMom& a, const RowMom& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  RowMom o;
  o.n = a.n + b.n;
  o.sum = a.sum + b.sum;
  const double w = b.n / o.n, d = b.mean - a.mean;
  o.mean = a.mean + d * w;
  o.m2 = a.m2 + b.m2 + d * d * (a.n * w);
  o.mn = fmin(a.mn, b.mn);
  o.mx = fmax(a.mx, b.mx);
  return o;
}

__device__ __forceinline__ RowMom rs_shfl_down(const RowMom& a, int s, int width) {
  RowMom o;
  o.n = __shfl_down(a.n, s, width);
  o.sum = __shfl_down(a.sum, s, width);
  o.mean = __shfl_down(a.mean, s, width);
  o.m2 = __shfl_down(a.m2, s, width);
  o.mn = __shfl_down(a.mn, s, width);
  o.mx = __shfl_down(a.mx, s, width);
  return o;
}

// Tree merge of W consecutive lanes (lane l with l + s, s = W / 2 .. 1); the first lane of
// the W holds the result.
template <int W>
__device__ __forceinline__ RowMom rs_lanes_merge(RowMom a) {
#pragma unroll
  for (int s = W / 2; s >= 1; s >>= 1) {
    const RowMom b = rs_shfl_down(a, s, W);
    a = rs_merge(a, b);  // lanes past W - s merge what the shuffle left them: never read
  }
  return a;
}

struct RsSide {
  const int32_t* __restrict__ col;
  const float* __restrict__ val;
  const double* __restrict__ other;
  int64_t nnz;
  int32_t n_cols;
  double offset;
  bool vec;  // col and val 16-byte aligned
};

__device__ __forceinline__ double rs_term(const RsSide& s, float v, int32_t c) {
  double e = (double)v - s.offset;
  if (s.other != nullptr && c >= 0 && c < s.n_cols) e -= s.other[c];
  return e;
}

// Quad q of the side restricted to [lo, hi), folded into acc.
__device__ __forceinline__ void rs_push_quad(const RsSide& s, int64_t q, int64_t lo, int64_t hi,
                                             RowMom& acc) {
  const int64_t base = 4 * q;
  double e[4];
  bool in[4];
  if (s.vec && base >= lo && base + 4 <= hi) {
    const float4 v = *reinterpret_cast<const float4*>(s.val + base);
    int4 c = make_int4(-1, -1, -1, -1);
    if (s.other != nullptr) c = *reinterpret_cast<const int4*>(s.col + base);
    e[0] = rs_term(s, v.x, c.x);
    e[1] = rs_term(s, v.y, c.y);
    e[2] = rs_term(s, v.z, c.z);
    e[3] = rs_term(s, v.w, c.w);
    in[0] = in[1] = in[2] = in[3] = true;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t p = base + j;
      in[j] = p >= lo && p < hi;
      e[j] = 0.0;
      if (in[j]) e[j] = rs_term(s, s.val[p], s.other != nullptr ? s.col[p] : -1);
    }
  }
  RowMom b;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (in[j]) {
      b.n += 1.0;
      b.sum += e[j];
      b.mn = fmin(b.mn, e[j]);
      b.mx = fmax(b.mx, e[j]);
    }
  }
  if (b.n == 0.0) return;
  b.mean = b.n == 4.0 ? b.sum * 0.25 : b.sum / b.n;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (in[j]) {
      const double d = e[j] - b.mean;
      b.m2 += d * d;
    }
  }
  acc = rs_merge(acc, b);
}

// The ratings [lo, hi) by `lanes` lanes: lane l the quads first + l, first + l + lanes, ...
__device__ __forceinline__ RowMom rs_range(const RsSide& s, int64_t lo, int64_t hi, int l,
                                           int lanes) {
  RowMom acc;
  const int64_t q1 = (hi + 3) >> 2;
  for (int64_t q = (lo >> 2) + l; q < q1; q += lanes) rs_push_quad(s, q, lo, hi, acc);
  return acc;
}

// Row bounds as the kernels use them: inside [0, nnz] and ordered, whatever row_ptr holds.
__device__ __forceinline__ void rs_bounds(const int64_t* __restrict__ row_ptr, int64_t row,
                                          int64_t nnz, int64_t& pb, int64_t& pe) {
  pb = row_ptr[row];
  pe = row_ptr[row + 1];
  if (pb < 0) pb = 0;
  if (pe > nnz) pe = nnz;
  if (pe < pb) pe = pb;
}

__device__ __forceinline__ void rs_store_slot(double* __restrict__ p, const RowMom& a) {
  p[0] = a.n, p[1] = a.sum, p[2] = a.mean, p[3] = a.m2, p[4] = a.mn, p[5] = a.mx;
}

__device__ __forceinline__ RowMom rs_load_slot(const double* __restrict__ p) {
  RowMom a;
  a.n = p[0], a.sum = p[1], a.mean = p[2], a.m2 = p[3], a.mn = p[4], a.mx = p[5];
  return a;
}

// ntasks[r] = tasks of row r (0 for a row of at most kRsTask ratings); ntasks[n_rows] = 0,
// where the exclusive scan leaves the total.
__global__ __launch_bounds__(256) void rs_ntasks_kernel(const int64_t* __restrict__ row_ptr,
                                                        int64_t n_rows, int64_t nnz,
                                                        int32_t* __restrict__ ntasks) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > n_rows) return;
  int32_t t = 0;
  if (r < n_rows) {
    int64_t pb, pe;
    rs_bounds(row_ptr, r, nnz, pb, pe);
    if (pe - pb > kRsTask) t = (int32_t)((pe - pb + kRsTask - 1) / kRsTask);
  }
  ntasks[r] = t;
}

// One workgroup per task of a long row -> slots[task].
__global__ __launch_bounds__(256) void rs_task_kernel(const int64_t* __restrict__ row_ptr,
                                                      int64_t n_rows, RsSide s,
                                                      const int32_t* __restrict__ slot_begin,
                                                      int64_t max_slots,
                                                      double* __restrict__ slots) {
  __shared__ double sm[4 * kRsSlot];
  int64_t total = slot_begin[n_rows];
  if (total > max_slots) total = max_slots;  // cannot happen for a row_ptr that sums to nnz
  for (int64_t task = blockIdx.x; task < total; task += gridDim.x) {
    // the row r with slot_begin[r] <= task < slot_begin[r + 1] (the same words in every thread)
    int64_t lo = 0, hi = n_rows;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)slot_begin[mid] > task) hi = mid; else lo = mid;
    }
    int64_t pb, pe;
    rs_bounds(row_ptr, lo, s.nnz, pb, pe);
    const int64_t tb = pb + (task - slot_begin[lo]) * kRsTask;
    const int64_t te = tb + kRsTask < pe ? tb + kRsTask : pe;
    RowMom acc = rs_range(s, tb, te, threadIdx.x, 256);
    acc = rs_lanes_merge<64>(acc);
    __syncthreads();  // sm may still be read from the previous task
    if ((threadIdx.x & 63) == 0) rs_store_slot(sm + kRsSlot * (threadIdx.x >> 6), acc);
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w) acc = rs_merge(acc, rs_load_slot(sm + kRsSlot * w));
      rs_store_slot(slots + kRsSlot * task, acc);
    }
  }
}

// A 16-lane group per row: a short row is read here, a long row's slots are merged here.
__global__ __launch_bounds__(256) void rs_rows_kernel(const int64_t* __restrict__ row_ptr,
                                                      int64_t n_rows, RsSide s,
                                                      const int32_t* __restrict__ slot_begin,
                                                      int64_t max_slots,
                                                      const double* __restrict__ slots,
                                                      double* __restrict__ moments) {
  const int64_t row = (int64_t)blockIdx.x * kRsGroupRows + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  RowMom acc;
  if (row < n_rows) {  // uniform across the group
    int64_t pb, pe;
    rs_bounds(row_ptr, row, s.nnz, pb, pe);
    if (pe - pb <= kRsTask) {
      acc = rs_range(s, pb, pe, l, 16);
    } else if (l == 0 && slot_begin != nullptr) {
      const int64_t first = slot_begin[row];
      int64_t last = first + (pe - pb + kRsTask - 1) / kRsTask;
      if (last > max_slots) last = max_slots;
      for (int64_t t = first; t < last; ++t) acc = rs_merge(acc, rs_load_slot(slots + kRsSlot * t));
    }
  }
  acc = rs_lanes_merge<16>(acc);  // every lane of the wavefront takes part in the shuffles
  if (row < n_rows && l == 0) {
    double* __restrict__ o = moments + kRsOut * row;
    o[0] = acc.n;
    o[1] = acc.sum;
    o[2] = acc.m2;
    o[3] = acc.n > 0.0 ? acc.mn : NAN;
    o[4] = acc.n > 0.0 ? acc.mx : NAN;
  }
}

__device__ __forceinline__ RowMom rs_load_row(const double* __restrict__ moments, int64_t row) {
  const double* __restrict__ p = moments + kRsOut * row;
  RowMom a;
  a.n = p[0];
  if (a.n > 0.0) a.sum = p[1], a.mean = p[1] / p[0], a.m2 = p[2], a.mn = p[3], a.mx = p[4];
  else a.n = 0.0;
  return a;
}

// Tree merge over the 256 threads of a workgroup: wavefront trees, then the four in order.
// The result is returned to thread 0.  sm: 4 * kRsSlot doubles.
__device__ __forceinline__ RowMom rs_block_merge(RowMom acc, double* sm) {
  acc = rs_lanes_merge<64>(acc);
  if ((threadIdx.x & 63) == 0) rs_store_slot(sm + kRsSlot * (threadIdx.x >> 6), acc);
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w) acc = rs_merge(acc, rs_load_slot(sm + kRsSlot * w));
  return acc;
}

// First level of the total: workgroup b merges rows 1024 b .. 1024 b + 1023, thread t four
// consecutive ones.  psum[2 b] = n, psum[2 b + 1] = sum (for sum_partials_kernel<2>);
// part[5 b] = n, mean, M2, min, max.
__global__ __launch_bounds__(256) void rs_total_rows_kernel(const double* __restrict__ moments,
                                                            int64_t n_rows,
                                                            double* __restrict__ psum,
                                                            double* __restrict__ part) {
  __shared__ double sm[4 * kRsSlot];
  RowMom acc;
  const int64_t r0 = (int64_t)blockIdx.x * kRsTotalRows + 4 * threadIdx.x;
  for (int j = 0; j < 4; ++j)
    if (r0 + j < n_rows) acc = rs_merge(acc, rs_load_row(moments, r0 + j));
  acc = rs_block_merge(acc, sm);
  if (threadIdx.x == 0) {
    psum[2 * blockIdx.x] = acc.n;
    psum[2 * blockIdx.x + 1] = acc.sum;
    double* __restrict__ o = part + (int64_t)kRsTotalPart * blockIdx.x;
    o[0] = acc.n, o[1] = acc.mean, o[2] = acc.m2, o[3] = acc.mn, o[4] = acc.mx;
  }
}

// Second level, one workgroup: total[2 .. 4] = M2, min, max (total[0 .. 1] come from
// sum_partials_kernel<2>).
__global__ __launch_bounds__(256) void rs_total_final_kernel(const double* __restrict__ part,
                                                             int64_t nb,
                                                             double* __restrict__ total) {
  __shared__ double sm[4 * kRsSlot];
  RowMom acc;
  for (int64_t b = threadIdx.x; b < nb; b += 256) {
    const double* __restrict__ p = part + kRsTotalPart * b;
    RowMom x;
    x.n = p[0], x.mean = p[1], x.m2 = p[2], x.mn = p[3], x.mx = p[4];
    acc = rs_merge(acc, x);
  }
  acc = rs_block_merge(acc, sm);
  if (threadIdx.x == 0) {
    total[2] = acc.m2;
    total[3] = acc.n > 0.0 ? acc.mn : NAN;
    total[4] = acc.n > 0.0 ? acc.mx : NAN;
  }
}

__global__ __launch_bounds__(256) void rs_bias_kernel(const double* __restrict__ moments,
                                                      int64_t n_rows, double damping,
                                                      double* __restrict__ bias) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const double n = moments[kRsOut * r], sum = moments[kRsOut * r + 1];
  bias[r] = n > 0.0 ? sum / (damping + n) : 0.0;
}

__global__ __launch_bounds__(256) void rs_predict_kernel(
    const int32_t* __restrict__ urow, const int32_t* __restrict__ irow, int64_t n, double mu,
    const double* __restrict__ bu, int32_t n_users, const double* __restrict__ bi,
    int32_t n_items, float* __restrict__ pred, uint8_t* __restrict__ known) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int32_t u = urow[e], i = irow[e];
  const bool ku = u >= 0 && u < n_users, ki = i >= 0 && i < n_items;
  double p = mu;
  if (ku && bu != nullptr) p += bu[u];
  if (ki && bi != nullptr) p += bi[i];
  pred[e] = (float)p;
  known[e] = (uint8_t)((ku ? 1 : 0) | (ki ? 2 : 0));
}

static inline int64_t rs_max_slots(int64_t nnz) {
  return nnz > kRsTask ? 2 * (nnz / kRsTask) + 2 : 0;
}
static inline int64_t rs_total_blocks(int64_t n_rows) {
  return (n_rows + kRsTotalRows - 1) / kRsTotalRows;
}

struct RsScratch {
  int32_t* ntasks;
  int32_t* slot_begin;
  char* scan_ws;
  size_t scan_bytes;
  double* slots;
  double* psum;
  double* part;
};

// One layout for the size function and the call.
template <class A>
static void rs_layout(A& a, int64_t nnz, int64_t n_rows, RsScratch* out) {
  const int64_t ms = rs_max_slots(nnz), nb = rs_total_blocks(n_rows);
  const size_t scan_bytes = ms > 0 ? scan_workspace_bytes(n_rows + 1) : 0;
  auto ntasks = a.template take<int32_t>(ms > 0 ? (size_t)n_rows + 1 : 0);
  auto slot_begin = a.template take<int32_t>(ms > 0 ? (size_t)n_rows + 1 : 0);
  auto scan_ws = a.template take<char>(scan_bytes);
  auto slots = a.template take<double>((size_t)ms * kRsSlot);
  auto psum = a.template take<double>((size_t)nb * 2);
  auto part = a.template take<double>((size_t)nb * kRsTotalPart);
  if (out) {
    out->ntasks = (int32_t*)ntasks;
    out->slot_begin = (int32_t*)slot_begin;
    out->scan_ws = (char*)scan_ws;
    out->scan_bytes = scan_bytes;
    out->slots = (double*)slots;
    out->psum = (double*)psum;
    out->part = (double*)part;
  }
}

// The layout arithmetic without memory (ArenaSize's take returns nothing to assign).
struct RsSizer {
  size_t off = 0;
  template <class T>
  T* take(size_t count) {
    off += align_up(count * sizeof(T));
    return nullptr;
  }
};

constexpr int64_t kRsMaxNnz = (int64_t)1 << 40;  // task numbers stay int32

}  // namespace als

using namespace als;

extern "C" {

int32_t als_rating_stats_task(void) { return kRsTask; }
int32_t als_rating_stats_group_rows(void) { return kRsGroupRows; }

size_t als_rating_stats_scratch_bytes(int64_t nnz, int64_t n_rows) {
  if (nnz < 0 || nnz >= kRsMaxNnz || n_rows < 0 || n_rows >= 0x7fffffff) return 0;
  RsSizer a;
  rs_layout(a, nnz, n_rows, nullptr);
  return a.off + 256;
}

int als_row_moments(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t nnz,
                    int32_t n_rows, int32_t n_cols, const double* other,
                    const double* offset_host, double* moments, double* total, void* ws,
                    size_t ws_bytes, void* stream) {
  ALS_REQUIRE(nnz >= 0 && n_rows >= 0 && n_cols >= 0, ALS_EINVAL,
              "als_row_moments: negative size");
  ALS_REQUIRE(nnz < kRsMaxNnz && n_rows < 0x7fffffff, ALS_EUNSUPPORTED,
              "als_row_moments: nnz >= 2^40 or n_rows >= 2^31 - 1");
  if (n_rows == 0) return ALS_OK;
  ALS_REQUIRE(row_ptr && moments && total, ALS_EINVAL, "als_row_moments: null pointer");
  ALS_REQUIRE(nnz == 0 || (val && (col || !other)), ALS_EINVAL,
              "als_row_moments: null col / val with nnz > 0");
  const double offset = offset_host ? *offset_host : 0.0;
  ALS_REQUIRE(ws && ws_bytes >= als_rating_stats_scratch_bytes(nnz, n_rows), ALS_EWORKSPACE,
              "als_row_moments: scratch %zu < %zu", ws_bytes,
              als_rating_stats_scratch_bytes(nnz, n_rows));
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(moments) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(total) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(other) & 7) == 0,
              ALS_EINVAL, "als_row_moments: scratch not 16-byte or fp64 table not 8-byte aligned");
  hipStream_t st = as_stream(stream);
  Arena ar(ws, ws_bytes);
  RsScratch sc;
  rs_layout(ar, nnz, n_rows, &sc);
  RsSide s;
  s.col = col, s.val = val, s.other = other, s.nnz = nnz, s.n_cols = n_cols, s.offset = offset;
  s.vec = (reinterpret_cast<uintptr_t>(val) & 15) == 0 &&
          (other == nullptr || (reinterpret_cast<uintptr_t>(col) & 15) == 0);
  const int64_t ms = rs_max_slots(nnz);
  if (ms > 0) {  // only then can a row be longer than a task
    rs_ntasks_kernel<<<(unsigned)(((int64_t)n_rows + 256) / 256), 256, 0, st>>>(row_ptr, n_rows,
                                                                                nnz, sc.ntasks);
    ALS_LAUNCH_CHECK();
    const int rc = scan_exclusive_i32(sc.ntasks, sc.slot_begin, (int64_t)n_rows + 1, sc.scan_ws,
                                      sc.scan_bytes, st);
    if (rc != ALS_OK) return rc;
    const int64_t grid = ms < (1 << 20) ? ms : (1 << 20);
    rs_task_kernel<<<(unsigned)grid, 256, 0, st>>>(row_ptr, n_rows, s, sc.slot_begin, ms,
                                                   sc.slots);
    ALS_LAUNCH_CHECK();
  }
  const int64_t nrb = ((int64_t)n_rows + kRsGroupRows - 1) / kRsGroupRows;
  rs_rows_kernel<<<(unsigned)nrb, 256, 0, st>>>(row_ptr, n_rows, s,
                                                ms > 0 ? sc.slot_begin : nullptr, ms, sc.slots,
                                                moments);
  ALS_LAUNCH_CHECK();
  const int64_t nb = rs_total_blocks(n_rows);
  rs_total_rows_kernel<<<(unsigned)nb, 256, 0, st>>>(moments, n_rows, sc.psum, sc.part);
  ALS_LAUNCH_CHECK();
  sum_partials_kernel<2><<<1, 256, 0, st>>>(sc.psum, nb, total);
  ALS_LAUNCH_CHECK();
  rs_total_final_kernel<<<1, 256, 0, st>>>(sc.part, nb, total);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

int als_bias_update(const double* moments, int32_t n_rows, const double* damping_host,
                    double* bias_out, void* stream) {
  ALS_REQUIRE(n_rows >= 0, ALS_EINVAL, "als_bias_update: n_rows < 0");
  const double damping = damping_host ? *damping_host : 0.0;
  ALS_REQUIRE(damping >= 0.0 && damping <= 1.79e308, ALS_EINVAL,
              "als_bias_update: damping must be finite and >= 0");
  if (n_rows == 0) return ALS_OK;
  ALS_REQUIRE(moments && bias_out, ALS_EINVAL, "als_bias_update: null pointer");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(moments) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(bias_out) & 7) == 0,
              ALS_EINVAL, "als_bias_update: tables not 8-byte aligned");
  rs_bias_kernel<<<(unsigned)(((int64_t)n_rows + 255) / 256), 256, 0, as_stream(stream)>>>(
      moments, n_rows, damping, bias_out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

int als_baseline_predict(const int32_t* urow, const int32_t* irow, int64_t n,
                         const double* mu_host, const double* bu, int32_t n_users,
                         const double* bi, int32_t n_items, float* pred, uint8_t* known,
                         void* stream) {
  ALS_REQUIRE(n >= 0 && n_users >= 0 && n_items >= 0, ALS_EINVAL,
              "als_baseline_predict: negative size");
  ALS_REQUIRE(n < ((int64_t)1 << 39), ALS_EUNSUPPORTED, "als_baseline_predict: n >= 2^39");
  if (n == 0) return ALS_OK;
  ALS_REQUIRE(urow && irow && pred && known, ALS_EINVAL, "als_baseline_predict: null pointer");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(bu) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(bi) & 7) == 0,
              ALS_EINVAL, "als_baseline_predict: bias tables not 8-byte aligned");
  const double mu = mu_host ? *mu_host : 0.0;
  rs_predict_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(
      urow, irow, n, mu, bu, n_users, bi, n_items, pred, known);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // extern "C"
