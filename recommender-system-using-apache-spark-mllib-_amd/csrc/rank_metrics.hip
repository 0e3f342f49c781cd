// K6 — ranking metrics over top-k lists: precision, recall, AP and NDCG at k.
//
// Replaces pyspark.mllib.evaluation.RankingMetrics (precisionAt, recallAt,
// meanAveragePrecisionAt, ndcgAt; upstream mllib/evaluation/RankingMetrics.scala, binary
// relevance) for lists that are already on the device: the [n_q, at] dense-row matrix
// als_topk / als_topk_filtered write, scored against per-row relevant sets given as
// ascending ranges of one shared column array (the form of the ex_* exclusion ranges).
//
// One wavefront per query row, four rows per 256-thread block, blocks striding over the
// row groups.  Lane l takes positions l, l + 64, ... (at <= 256: at most four passes),
// looks its listed row up in the row's range by binary search, and the pass's hits come
// back as one ballot mask.  The wave then walks the set bits of the mask in position
// order, so a row's AP and DCG are summed exactly as the definition reads, first
// position first; the ideal DCG is a prefix of the same terms summed in the same order
// (a table made once per call by a one-block launch), so a row whose first
// min(m, at) positions are all hits scores NDCG 1.0 exactly.  All arithmetic is fp64.
// Row values are added up per wave in row order, the four waves of a block in wave
// order, and the per-block partials by a single block in a fixed order (partial_sums.h):
// the sums are bitwise reproducible run to run.
#include "als_common.h"
#include "partial_sums.h"

namespace als {

constexpr int kRmMaxAt = 256;
constexpr int kRmRowsPerBlock = 4;   // one wavefront each
constexpr int kRmMaxBlocks = 4096;   // blocks stride over the row groups past this
constexpr int kRmSums = 6;

static inline int64_t rm_blocks(int64_t n_q) {
  const int64_t g = (n_q + kRmRowsPerBlock - 1) / kRmRowsPerBlock;
  return g < 1 ? 1 : (g > kRmMaxBlocks ? kRmMaxBlocks : g);
}

// tab[p] = d(p) = 1 / log2(p + 2); tab[256 + p] = d(0) + ... + d(p), summed in that order.
__global__ __launch_bounds__(kRmMaxAt) void rank_tables_kernel(double* __restrict__ tab) {
  __shared__ double sd[kRmMaxAt];
  const int p = threadIdx.x;
  const double d = 1.0 / log2((double)(p + 2));
  sd[p] = d;
  tab[p] = d;
  __syncthreads();
  if (p == 0) {
    double s = 0.0;
    for (int q = 0; q < kRmMaxAt; ++q) {
      s += sd[q];
      tab[kRmMaxAt + q] = s;
    }
  }
}

__global__ __launch_bounds__(256) void rank_metrics_kernel(
    const int32_t* __restrict__ idx, int64_t n_q, int idx_ld, int at,
    const int64_t* __restrict__ rel_begin, const int64_t* __restrict__ rel_end,
    const int32_t* __restrict__ rel_col, const double* __restrict__ tab,
    double* __restrict__ per_row, double* __restrict__ partial) {
  __shared__ double sd[kRmMaxAt], sideal[kRmMaxAt];
  __shared__ double swave[kRmRowsPerBlock][kRmSums];
  sd[threadIdx.x] = tab[threadIdx.x];
  sideal[threadIdx.x] = tab[kRmMaxAt + threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // every lane of a wave carries the same sums (all of the row arithmetic is wave-uniform)
  double s_prec = 0.0, s_rec = 0.0, s_ap = 0.0, s_ndcg = 0.0, s_rows = 0.0, s_hit = 0.0;
  const int64_t n_grp = (n_q + kRmRowsPerBlock - 1) / kRmRowsPerBlock;
  for (int64_t g = blockIdx.x; g < n_grp; g += gridDim.x) {
    const int64_t r = g * kRmRowsPerBlock + w;
    if (r >= n_q) continue;  // wave-uniform; no barrier inside the loop
    const int64_t beg = rel_begin[r], end = rel_end[r], m = end - beg;
    if (m <= 0) {
      if (per_row && lane < 4) per_row[r * 4 + lane] = 0.0;
      continue;
    }
    const int32_t* __restrict__ row = idx + r * (int64_t)idx_ld;
    int c = 0;  // hits so far
    double ap = 0.0, dcg = 0.0;
    for (int p0 = 0; p0 < at; p0 += 64) {
      const int p = p0 + lane;
      const int j = p < at ? row[p] : -1;
      bool hit = false;
      if (j >= 0) {
        int64_t lo = beg, hi = end;
        while (lo < hi) {  // lower bound of j in the row's range
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (rel_col[mid] < j) lo = mid + 1;
          else hi = mid;
        }
        hit = lo < end && rel_col[lo] == j;
      }
      uint64_t mask = __ballot(hit);
      while (mask) {  // the pass's hits in position order
        const int q = p0 + __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        ++c;
        ap += (double)c / (double)(q + 1);
        dcg += sd[q];
      }
    }
    const int n_ideal = m < at ? (int)m : at;
    const double prec = (double)c / (double)at;
    const double rec = (double)c / (double)m;
    const double apv = ap / (double)n_ideal;
    const double ndcg = dcg / sideal[n_ideal - 1];
    s_prec += prec;
    s_rec += rec;
    s_ap += apv;
    s_ndcg += ndcg;
    s_rows += 1.0;
    if (c > 0) s_hit += 1.0;
    if (per_row && lane == 0) {
      per_row[r * 4] = prec;
      per_row[r * 4 + 1] = rec;
      per_row[r * 4 + 2] = apv;
      per_row[r * 4 + 3] = ndcg;
    }
  }
  if (lane == 0) {
    swave[w][0] = s_prec;
    swave[w][1] = s_rec;
    swave[w][2] = s_ap;
    swave[w][3] = s_ndcg;
    swave[w][4] = s_rows;
    swave[w][5] = s_hit;
  }
  __syncthreads();
  if (threadIdx.x < kRmSums) {
    double a = 0.0;
    for (int i = 0; i < kRmRowsPerBlock; ++i) a += swave[i][threadIdx.x];
    partial[(int64_t)kRmSums * blockIdx.x + threadIdx.x] = a;
  }
}

}  // namespace als

using namespace als;

extern "C" {

size_t als_rank_metrics_workspace_bytes(int64_t n_q) {
  return align_up(sizeof(double) * 2 * kRmMaxAt) +
         align_up(sizeof(double) * kRmSums * (size_t)rm_blocks(n_q));
}

int als_rank_metrics(const int32_t* idx, int64_t n_q, int32_t idx_ld, int32_t at,
                     const int64_t* rel_begin, const int64_t* rel_end, const int32_t* rel_col,
                     double* sums_out, double* per_row_out, void* ws, size_t ws_bytes,
                     void* stream) {
  ALS_REQUIRE(at >= 1 && at <= kRmMaxAt, ALS_EUNSUPPORTED,
              "als_rank_metrics: at = %d outside [1, %d]", at, kRmMaxAt);
  ALS_REQUIRE(idx_ld >= at, ALS_EINVAL, "als_rank_metrics: idx_ld %d < at %d", idx_ld, at);
  ALS_REQUIRE(n_q >= 0, ALS_EINVAL, "als_rank_metrics: n_q < 0");
  hipStream_t st = as_stream(stream);
  if (n_q == 0) {
    if (sums_out) ALS_HIP(hipMemsetAsync(sums_out, 0, kRmSums * sizeof(double), st));
    return ALS_OK;
  }
  ALS_REQUIRE(idx && rel_begin && rel_end && rel_col && sums_out, ALS_EINVAL,
              "als_rank_metrics: null pointer");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, ALS_EINVAL,
              "als_rank_metrics: workspace not 16-byte aligned");
  ALS_REQUIRE(ws && ws_bytes >= als_rank_metrics_workspace_bytes(n_q), ALS_EWORKSPACE,
              "als_rank_metrics: workspace too small");
  Arena arena(ws, ws_bytes);
  double* tab = arena.take<double>(2 * kRmMaxAt);
  const int64_t nb = rm_blocks(n_q);
  double* partial = arena.take<double>(kRmSums * (size_t)nb);
  ALS_REQUIRE(tab && partial, ALS_EWORKSPACE, "als_rank_metrics: workspace too small");
  rank_tables_kernel<<<1, kRmMaxAt, 0, st>>>(tab);
  ALS_LAUNCH_CHECK();
  rank_metrics_kernel<<<(unsigned)nb, 256, 0, st>>>(idx, n_q, idx_ld, at, rel_begin, rel_end,
                                                    rel_col, tab, per_row_out, partial);
  ALS_LAUNCH_CHECK();
  sum_partials_kernel<kRmSums><<<1, 256, 0, st>>>(partial, nb, sums_out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // extern "C"
