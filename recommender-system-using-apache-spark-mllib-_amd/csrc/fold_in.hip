// K7 — fold-in: factor rows for a few to a few thousand NEW rows against a fixed factor
// table, without a refit (als_fold_in, ABI 9).
//
// The reference serves a person the model has never seen by adding their dozen ratings to
// the training set and retraining everything (RecommenderSystem.py:211-218); Spark's ALS
// offers no other entry point.  The arithmetic needed is one row of one half-sweep
// (computeFactors + NormalEquation.add + CholeskySolver.solve for that row alone), and
// als_solve_half is the wrong tool for it: it needs a CSR schedule (three host syncs), its
// explicit PREP re-splits all of Y_src, and a serving-only core has no rating blocks.
//
// One 256-thread workgroup per row, one launch, no workspace, no pass over Y_src.  The
// gather, the Gram and the factorisation are row_system.h's, shared with K11 and K13:
//   gather   The row's ratings are taken 32 at a time.  Wave 0 reads (col, val) of the
//            batch, turns them into the weights of the two sums and counts the used ones;
//            then all four waves copy the 32 factor rows into LDS as float4 pieces,
//            columns >= k (padding, whatever it holds) and unknown items as zeros.
//   gram     The threads form a 16 x 16 grid: thread (a, b) owns the entries
//            (a + 16 p, b + 16 q), q <= p, of the lower triangle of A in registers — at most
//            36 fp64 accumulators at k = 128 — and thread t < k owns b[t].  Each rating
//            adds w_a * y_i * y_j and w_b * y_t in fp64, ratings in row order: the sums are
//            the oracle's to rounding and the same from call to call.
//   factor   The accumulators (plus YtY and reg * n on the diagonal) go to LDS as one
//            lower-packed (k + 1) x (k + 1) fp64 triangle whose last row is b: a
//            square-root-free LDL^T over the first k columns (one barrier per column)
//            then carries out the forward substitution in the same sweep.
//   solve    Thread i keeps z_i / d_i in a register; the back substitution broadcasts one
//            finished x_l per step through LDS.  The result is stored as fp32.
// A long row runs the same gather/gram loop serially; there is no chunked path.
#include <algorithm>

#include "row_system.h"

namespace als {

// Dynamic LDS of one block.  The packed triangle comes first; the gather buffer aliases
// its head (it is dead when the accumulators are written out) when the triangle is the
// larger of the two.
struct FiLds {
  int tri_doubles;  // (k + 1)(k + 2) / 2
  int head_bytes;   // max(triangle, gather buffer), 16-byte multiple
  int total_bytes;
};

__host__ __device__ static inline FiLds fi_lds(int k, int kp) {
  FiLds l;
  l.tri_doubles = (k + 1) * (k + 2) / 2;
  const int tri = (l.tri_doubles * 8 + 15) / 16 * 16;
  const int ybuf = kRowBatch * kp * 4;
  l.head_bytes = tri > ybuf ? tri : ybuf;
  // + x broadcast (kRowMaxRank doubles) + two weights per batch slot + col per slot + 4 ints
  l.total_bytes = l.head_bytes + kRowMaxRank * 8 + 2 * kRowBatch * 8 + kRowBatch * 4 + 16;
  return l;
}

// NB = k_pad / 16: thread (a, b) owns rows a + 16 p and columns b + 16 q, q <= p < NB.
template <int NB, bool IMPLICIT>
__global__ __launch_bounds__(kRowThreads) void fold_in_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t n_rows, const float* __restrict__ Y, int64_t n_src,
    int ld, int k, float reg, float alpha, const double* __restrict__ yty,
    float* __restrict__ X, int ld_out, int32_t* __restrict__ n_used_out,
    int32_t* __restrict__ status) {
  constexpr int KP = 16 * NB;
  constexpr int NACC = NB * (NB + 1) / 2;
  extern __shared__ float4 fi_smem[];  // 16-byte aligned
  const FiLds L = fi_lds(k, KP);
  double* const Ap = reinterpret_cast<double*>(fi_smem);        // packed triangle
  float* const ybuf = reinterpret_cast<float*>(fi_smem);        // [kRowBatch][KP], aliases Ap
  double* const sx = reinterpret_cast<double*>(reinterpret_cast<char*>(fi_smem) + L.head_bytes);
  double* const swa = sx + kRowMaxRank;   // weight of y y^T per batch slot
  double* const swb = swa + kRowBatch;    // weight of y in b
  int* const scol = reinterpret_cast<int*>(swb + kRowBatch);
  int* const scnt = scol + kRowBatch;     // [0] used entries, [1] used entries with r > 0

  const int t = threadIdx.x;
  const int ta = t >> 4, tb = t & 15;
  const int lane = t & 63;

  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const int64_t pb = row_ptr[row], pe = row_ptr[row + 1];
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    double bacc = 0.0;
    int n_used = 0, n_pos = 0;  // wave 0 only
    for (int64_t s0 = pb; s0 < pe; s0 += kRowBatch) {
      if (t < 64)
        row_weights<IMPLICIT>(s0, pe, col, val, n_src, alpha, lane, scol, swa, swb, n_used, n_pos);
      __syncthreads();
      row_gather<KP, KP>(Y, ld, k, scol, ybuf, t);
      __syncthreads();
      const int nb = pe - s0 < kRowBatch ? (int)(pe - s0) : kRowBatch;
      row_gram_batch<NB, KP, true>(ybuf, nb, swa, swb, acc, bacc);
      __syncthreads();  // the next batch (or the triangle) overwrites ybuf
    }
    if (t == 0) {
      scnt[0] = n_used;
      scnt[1] = n_pos;
    }
    __syncthreads();
    const int n_all = scnt[0];
    const double lam_n = (double)reg * (double)(IMPLICIT ? scnt[1] : n_all);
    float* const xr = X + row * (int64_t)ld_out;
    if (n_used_out && t == 0) n_used_out[row] = n_all;
    if (n_all == 0) {  // no used entry: a zero row, not an error
      for (int c = t; c < ld_out; c += kRowThreads) xr[c] = 0.f;
      __syncthreads();  // scnt is rewritten by the next row
      continue;
    }

    // accumulators -> the packed triangle (its diagonal as summed in sx), row k = b
#pragma unroll
    for (int p = 0; p < NB; ++p) {
#pragma unroll
      for (int q = 0; q <= p; ++q) {
        const int i = ta + 16 * p, j = tb + 16 * q;
        if (i < k && j <= i) {
          const int e = i * (i + 1) / 2 + j;
          double a = acc[p * (p + 1) / 2 + q];
          if (IMPLICIT) a += yty[e];
          if (i == j) {
            a += lam_n;
            sx[i] = a;  // the diagonal of A as summed: the scale of pivot i's rounding error
          }
          Ap[e] = a;
        }
      }
    }
    if (t < k) Ap[k * (k + 1) / 2 + t] = bacc;
    __syncthreads();

    // row k (= b) rides along, so that after column j its entry j holds (L^-1 b)_j
    if (!row_ldlt<true>(Ap, sx, k)) {
      if (t == 0) atomicCAS(status, 0, (int32_t)(row + 1));
      for (int c = t; c < ld_out; c += kRowThreads) xr[c] = 0.f;
      __syncthreads();
      continue;
    }

    // z = D^-1 L^-1 b in registers, then L^T x = z from the last row up
    double zi = 0.0, inv_di = 0.0;
    if (t < k) {
      inv_di = 1.0 / Ap[t * (t + 1) / 2 + t];
      zi = Ap[k * (k + 1) / 2 + t] * inv_di;
    }
    for (int l = k - 1; l >= 0; --l) {  // sx: the diagonal is no longer needed
      if (t == l) sx[l] = zi;
      __syncthreads();
      if (t < l) zi = fma(-(Ap[l * (l + 1) / 2 + t] * inv_di), sx[l], zi);
    }
    // k <= 128 < 256 threads: a column c < k is thread c's own
    for (int c = t; c < ld_out; c += kRowThreads) xr[c] = c < k ? (float)zi : 0.f;
    __syncthreads();  // Ap, sx and scnt are rewritten by the next row
  }
}

}  // namespace als

using namespace als;

extern "C" {

size_t als_fold_in_workspace_bytes(int64_t n_rows, int32_t k) {
  (void)n_rows;
  (void)k;
  return 0;  // every intermediate lives in registers and LDS
}

int als_fold_in(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows,
                const float* Y_src, int64_t n_src, int32_t ld, int32_t k, float reg, int implicit,
                float alpha, const double* yty_packed, float* X_out, int32_t ld_out,
                int32_t* n_used_out, int32_t* status_dev, void* ws, size_t ws_bytes,
                void* stream) {
  (void)ws;
  (void)ws_bytes;
  if (int rc = row_check_args("als_fold_in", k, ld, n_rows, n_src, reg, alpha, implicit,
                              yty_packed))
    return rc;
  ALS_REQUIRE(ld_out >= k && ld_out % 4 == 0, ALS_EINVAL,
              "als_fold_in: ld_out %d must be >= k and a multiple of 4", ld_out);
  if (n_rows == 0) return ALS_OK;
  ALS_REQUIRE(row_ptr && col && val && X_out && status_dev, ALS_EINVAL,
              "als_fold_in: null pointer");
  if (int rc = row_check_source("als_fold_in", n_src, Y_src, X_out)) return rc;
  hipStream_t st = as_stream(stream);
  const int nb = als_k_pad(k) / 16;
  const int lds = fi_lds(k, 16 * nb).total_bytes;
  const unsigned grid = (unsigned)std::min<int64_t>(n_rows, kRowMaxBlocks);
  return row_dispatch(nb, implicit, [&](auto nbc, auto imp) -> int {
    constexpr auto kernel = &fold_in_kernel<decltype(nbc)::value, decltype(imp)::value>;
    ALS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    kernel<<<grid, kRowThreads, lds, st>>>(row_ptr, col, val, n_rows, Y_src, n_src, ld, k, reg,
                                           alpha, yty_packed, X_out, ld_out, n_used_out,
                                           status_dev);
    ALS_LAUNCH_CHECK();
    return ALS_OK;
  });
}

}  // extern "C"
