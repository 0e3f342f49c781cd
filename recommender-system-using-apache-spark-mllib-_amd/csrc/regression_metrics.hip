// K8 — regression moments in one pass.
//
// Replaces the reductions behind pyspark.ml.evaluation.RegressionEvaluator /
// pyspark.mllib.evaluation.RegressionMetrics (upstream: a MultivariateOnlineSummarizer
// over (label, label - prediction) rows), the evaluation step of the reference's rank
// sweep and of its mean-rating baseline (RecommenderSystem.py:136-177).
//
// Two forms write the same 8 doubles
//   n, mean_label, M2_label, mean_pred, M2_pred, sse, sae, n_dropped
// (M2 = sum of squared deviations from the mean, sse / sae = sum of (label - pred)^2 and
// of |label - pred|):
//   fused   predictions are K4's fp64 gather-dot (pair_dot) of a rating list against the
//           factors; a pair with an unknown id is dropped and counted (computeError's
//           inner join);
//   columns two fp64 arrays, wherever the predictions came from.
//
// M2 is never formed as sum x^2 - (sum x)^2 / n.  Each 16-lane group (fused) or thread
// (columns) folds its own elements into (n, mean, M2) one at a time — Welford's update,
// Chan's merge with n_b = 1 — and partials are merged with Chan's rule
//   d = mean_b - mean_a,  mean = mean_a + d n_b / n,  M2 = M2_a + M2_b + d^2 n_a n_b / n
// in a fixed order: inside the block, then by one block over the per-block partials (each
// thread its partials in ascending order, then a tree over the 256 threads).  An empty
// partial is the identity.  No atomics: two calls give bit-identical output.
// The column form keeps its means relative to the first element of each column (when that
// is finite): the merge term d^2 n_a n_b / n inherits the rounding of the means, an ulp
// of |mean|, so data at 1e9 +- 1 would otherwise lose M2 at the 1e-9 level; the shifted
// means are of the size of the spread.  The final kernel adds the shift back.
// NaN needs no special case: it propagates through the means, M2, sse and sae.
#include "als_common.h"

namespace als {

constexpr int kRegPairsPerBlock = 256;   // fused: 16 groups x 16 passes
constexpr int kRegColsPerThread = 4;
constexpr int kRegColsPerBlock = 256 * kRegColsPerThread;
constexpr int kRegOut = 8;

struct Moments {
  double n = 0.0, ml = 0.0, m2l = 0.0, mp = 0.0, m2p = 0.0, sse = 0.0, sae = 0.0, drop = 0.0;
};

// One (label, prediction) row; sl / sp are the shifts the means are kept relative to.
__device__ __forceinline__ void mom_push(Moments& a, double l, double p, double sl, double sp) {
  a.n += 1.0;
  const double xl = l - sl, xp = p - sp;
  const double dl = xl - a.ml;
  a.ml += dl / a.n;
  a.m2l += dl * (xl - a.ml);
  const double dp = xp - a.mp;
  a.mp += dp / a.n;
  a.m2p += dp * (xp - a.mp);
  const double d = l - p;
  a.sse += d * d;
  a.sae += fabs(d);
}

// Chan's rule; an empty side is the identity (0 / 0 never formed).
__device__ __forceinline__ Moments mom_merge(const Moments& a, const Moments& b) {
  Moments o;
  o.sse = a.sse + b.sse;
  o.sae = a.sae + b.sae;
  o.drop = a.drop + b.drop;
  if (b.n == 0.0) {
    o.n = a.n, o.ml = a.ml, o.m2l = a.m2l, o.mp = a.mp, o.m2p = a.m2p;
  } else if (a.n == 0.0) {
    o.n = b.n, o.ml = b.ml, o.m2l = b.m2l, o.mp = b.mp, o.m2p = b.m2p;
  } else {
    o.n = a.n + b.n;
    const double w = b.n / o.n, c = a.n * b.n / o.n;
    const double dl = b.ml - a.ml, dp = b.mp - a.mp;
    o.ml = a.ml + dl * w;
    o.m2l = a.m2l + b.m2l + dl * dl * c;
    o.mp = a.mp + dp * w;
    o.m2p = a.m2p + b.m2p + dp * dp * c;
  }
  return o;
}

__device__ __forceinline__ void mom_store(double* __restrict__ p, int stride, const Moments& a) {
  p[0 * stride] = a.n;
  p[1 * stride] = a.ml;
  p[2 * stride] = a.m2l;
  p[3 * stride] = a.mp;
  p[4 * stride] = a.m2p;
  p[5 * stride] = a.sse;
  p[6 * stride] = a.sae;
  p[7 * stride] = a.drop;
}

__device__ __forceinline__ Moments mom_load(const double* __restrict__ p, int stride) {
  Moments a;
  a.n = p[0 * stride];
  a.ml = p[1 * stride];
  a.m2l = p[2 * stride];
  a.mp = p[3 * stride];
  a.m2p = p[4 * stride];
  a.sse = p[5 * stride];
  a.sae = p[6 * stride];
  a.drop = p[7 * stride];
  return a;
}

// Tree merge of the 256 threads' partials (thread t with t + s, s = 128 .. 1); the result
// is returned to thread 0.  sm: kRegOut x 256 doubles of LDS, field-major.
__device__ __forceinline__ Moments block_tree_merge(Moments mine, double* sm) {
  const int t = threadIdx.x;
  mom_store(sm + t, 256, mine);
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) {
      mine = mom_merge(mine, mom_load(sm + t + s, 256));
      mom_store(sm + t, 256, mine);
    }
    __syncthreads();
  }
  return mine;
}

__global__ __launch_bounds__(256) void regression_pairs_kernel(
    const int32_t* __restrict__ u, const int32_t* __restrict__ it, const float* __restrict__ r,
    int64_t n, const int32_t* __restrict__ umap, int32_t usz, const int32_t* __restrict__ imap,
    int32_t isz, const float* __restrict__ U, const float* __restrict__ V, int ld, int k,
    double* __restrict__ partial) {
  __shared__ double sm[kRegOut * 16];
  const int grp = threadIdx.x >> 4;
  Moments acc;  // every lane of a group carries the same values; lane 0 stores them
  for (int pass = 0; pass < kRegPairsPerBlock / 16; ++pass) {
    const int64_t e = (int64_t)blockIdx.x * kRegPairsPerBlock + pass * 16 + grp;
    const bool in = e < n;  // uniform across the 16-lane group
    bool known = false;
    const double p = pair_dot(in ? u[e] : -1, in ? it[e] : -1, umap, usz, imap, isz, U, V, ld, k,
                              known);
    if (in && known) mom_push(acc, (double)r[e], p, 0.0, 0.0);
    else if (in) acc.drop += 1.0;
  }
  if ((threadIdx.x & 15) == 0) mom_store(sm + grp, 16, acc);
  __syncthreads();
  if (threadIdx.x == 0) {
    Moments a = mom_load(sm, 16);
    for (int g = 1; g < 16; ++g) a = mom_merge(a, mom_load(sm + g, 16));
    mom_store(partial + (int64_t)kRegOut * blockIdx.x, 1, a);
  }
}

// The shift of one column: its first element when finite, else 0.
__device__ __forceinline__ double col_shift(const double* __restrict__ x) {
  const double s = x[0];
  return (s - s == 0.0) ? s : 0.0;
}

__global__ __launch_bounds__(256) void regression_cols_kernel(const double* __restrict__ label,
                                                              const double* __restrict__ pred,
                                                              int64_t n,
                                                              double* __restrict__ partial) {
  __shared__ double sm[kRegOut * 256];
  const double sl = col_shift(label), sp = col_shift(pred);
  Moments acc;
  for (int j = 0; j < kRegColsPerThread; ++j) {
    const int64_t e = (int64_t)blockIdx.x * kRegColsPerBlock + j * 256 + threadIdx.x;
    if (e < n) mom_push(acc, label[e], pred[e], sl, sp);
  }
  acc = block_tree_merge(acc, sm);
  if (threadIdx.x == 0) mom_store(partial + (int64_t)kRegOut * blockIdx.x, 1, acc);
}

// Single-block fixed-order merge of the per-block partials; label / pred: the columns
// whose first elements shifted the means (NULL = no shift).
__global__ __launch_bounds__(256) void regression_final_kernel(const double* __restrict__ partial,
                                                               int64_t nb,
                                                               const double* __restrict__ label,
                                                               const double* __restrict__ pred,
                                                               double* __restrict__ out) {
  __shared__ double sm[kRegOut * 256];
  Moments acc;
  for (int64_t b = threadIdx.x; b < nb; b += 256)
    acc = mom_merge(acc, mom_load(partial + kRegOut * b, 1));
  acc = block_tree_merge(acc, sm);
  if (threadIdx.x == 0) {
    if (acc.n > 0.0) {
      if (label) acc.ml += col_shift(label);
      if (pred) acc.mp += col_shift(pred);
    }
    mom_store(out, 1, acc);
  }
}

static inline int64_t reg_blocks(int64_t n, int per_block) {
  return n > 0 ? (n + per_block - 1) / per_block : 1;
}

}  // namespace als

using namespace als;

extern "C" {

size_t als_regression_moments_workspace_bytes(int64_t n) {
  // sized for the fused form, which has the most blocks
  return align_up(sizeof(double) * kRegOut * (size_t)reg_blocks(n, kRegPairsPerBlock)) + 256;
}

int als_regression_moments(const int32_t* u, const int32_t* i, const float* r, int64_t n,
                           const int32_t* umap, int32_t umap_size, const int32_t* imap,
                           int32_t imap_size, const float* U, const float* V, int32_t ld,
                           int32_t k, double* out, void* ws, size_t ws_bytes, void* stream) {
  ALS_REQUIRE(k >= 1 && ld >= k && ld % 4 == 0, ALS_EINVAL, "als_regression_moments: bad k/ld");
  ALS_REQUIRE(n >= 0, ALS_EINVAL, "als_regression_moments: n < 0");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    if (out) ALS_HIP(hipMemsetAsync(out, 0, kRegOut * sizeof(double), st));
    return ALS_OK;
  }
  ALS_REQUIRE(u && i && r && umap && imap && U && V && out, ALS_EINVAL,
              "als_regression_moments: null pointer");
  ALS_REQUIRE(umap_size >= 0 && imap_size >= 0, ALS_EINVAL,
              "als_regression_moments: negative map size");
  ALS_REQUIRE(ws && ws_bytes >= als_regression_moments_workspace_bytes(n), ALS_EWORKSPACE,
              "als_regression_moments: workspace too small");
  const int64_t nb = reg_blocks(n, kRegPairsPerBlock);
  ALS_REQUIRE(nb <= 0x7fffffff, ALS_EUNSUPPORTED, "als_regression_moments: n too large");
  double* partial = static_cast<double*>(ws);
  regression_pairs_kernel<<<(unsigned)nb, 256, 0, st>>>(u, i, r, n, umap, umap_size, imap,
                                                        imap_size, U, V, ld, k, partial);
  ALS_LAUNCH_CHECK();
  regression_final_kernel<<<1, 256, 0, st>>>(partial, nb, nullptr, nullptr, out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

int als_regression_moments_cols(const double* label, const double* pred, int64_t n, double* out,
                                void* ws, size_t ws_bytes, void* stream) {
  ALS_REQUIRE(n >= 0, ALS_EINVAL, "als_regression_moments_cols: n < 0");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    if (out) ALS_HIP(hipMemsetAsync(out, 0, kRegOut * sizeof(double), st));
    return ALS_OK;
  }
  ALS_REQUIRE(label && pred && out, ALS_EINVAL, "als_regression_moments_cols: null pointer");
  ALS_REQUIRE(ws && ws_bytes >= als_regression_moments_workspace_bytes(n), ALS_EWORKSPACE,
              "als_regression_moments_cols: workspace too small");
  const int64_t nb = reg_blocks(n, kRegColsPerBlock);
  ALS_REQUIRE(nb <= 0x7fffffff, ALS_EUNSUPPORTED, "als_regression_moments_cols: n too large");
  double* partial = static_cast<double*>(ws);
  regression_cols_kernel<<<(unsigned)nb, 256, 0, st>>>(label, pred, n, partial);
  ALS_LAUNCH_CHECK();
  regression_final_kernel<<<1, 256, 0, st>>>(partial, nb, label, pred, out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // extern "C"
