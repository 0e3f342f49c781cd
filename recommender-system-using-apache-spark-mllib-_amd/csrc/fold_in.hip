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
// One 256-thread workgroup per row, one launch, no workspace, no pass over Y_src:
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

#include "als_common.h"

namespace als {

constexpr int kFiMaxRank = 128;
constexpr int kFiThreads = 256;
constexpr int kFiBatch = 32;         // ratings gathered per step
constexpr int kFiMaxBlocks = 65536;  // blocks stride over the rows past this
constexpr double kFiPivotEps = 0x1p-46;  // kFiMaxRank * 2^-53: see the factor step

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
  const int ybuf = kFiBatch * kp * 4;
  l.head_bytes = tri > ybuf ? tri : ybuf;
  // + x broadcast (kMaxRank doubles) + two weights per batch slot + col per slot + 4 ints
  l.total_bytes = l.head_bytes + kFiMaxRank * 8 + 2 * kFiBatch * 8 + kFiBatch * 4 + 16;
  return l;
}

// NB = k_pad / 16: thread (a, b) owns rows a + 16 p and columns b + 16 q, q <= p < NB.
template <int NB, bool IMPLICIT>
__global__ __launch_bounds__(kFiThreads) void fold_in_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t n_rows, const float* __restrict__ Y, int64_t n_src,
    int ld, int k, float reg, float alpha, const double* __restrict__ yty,
    float* __restrict__ X, int ld_out, int32_t* __restrict__ n_used_out,
    int32_t* __restrict__ status) {
  constexpr int KP = 16 * NB;
  constexpr int NACC = NB * (NB + 1) / 2;
  constexpr int P4 = KP / 4;                   // float4 pieces per gathered row
  constexpr int PIECES = kFiBatch * P4;        // per batch
  extern __shared__ float4 fi_smem[];  // 16-byte aligned
  const FiLds L = fi_lds(k, KP);
  double* const Ap = reinterpret_cast<double*>(fi_smem);        // packed triangle
  float* const ybuf = reinterpret_cast<float*>(fi_smem);        // [kFiBatch][KP], aliases Ap
  double* const sx = reinterpret_cast<double*>(reinterpret_cast<char*>(fi_smem) + L.head_bytes);
  double* const swa = sx + kFiMaxRank;   // weight of y y^T per batch slot
  double* const swb = swa + kFiBatch;    // weight of y in b
  int* const scol = reinterpret_cast<int*>(swb + kFiBatch);
  int* const scnt = scol + kFiBatch;     // [0] used entries, [1] used entries with r > 0

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

    for (int64_t s0 = pb; s0 < pe; s0 += kFiBatch) {
      if (t < 64) {  // wave 0: the batch's ids and weights
        bool used = false, pos = false;
        if (lane < kFiBatch) {
          const int64_t s = s0 + lane;
          int c = -1;
          double wa = 0.0, wb = 0.0;
          if (s < pe) {
            c = col[s];
            const double r = (double)val[s];
            used = c >= 0 && (int64_t)c < n_src;
            if (used) {
              pos = r > 0.0;
              if (IMPLICIT) {
                const double c1 = (double)alpha * fabs(r);
                wa = c1;
                wb = pos ? 1.0 + c1 : 0.0;
              } else {
                wa = 1.0;
                wb = r;
              }
            } else {
              c = -1;
            }
          }
          scol[lane] = c;
          swa[lane] = wa;
          swb[lane] = wb;
        }
        n_used += __popcll(__ballot(used));
        n_pos += __popcll(__ballot(pos));
      }
      __syncthreads();
      for (int g = t; g < PIECES; g += kFiThreads) {  // the batch's factor rows
        const int e = g / P4, c0 = (g % P4) * 4;
        const int c = scol[e];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c >= 0 && c0 < k) {  // c0 < k <= ld and ld % 4 == 0: the piece lies inside the row
          v = *reinterpret_cast<const float4*>(Y + (int64_t)c * ld + c0);
          if (c0 + 1 >= k) v.y = 0.f;
          if (c0 + 2 >= k) v.z = 0.f;
          if (c0 + 3 >= k) v.w = 0.f;
        }
        *reinterpret_cast<float4*>(ybuf + e * KP + c0) = v;
      }
      __syncthreads();
      const int nb = pe - s0 < kFiBatch ? (int)(pe - s0) : kFiBatch;
      for (int e = 0; e < nb; ++e) {
        const float* ye = ybuf + e * KP;
        const double wa = swa[e];
        double yj[NB], wyi[NB];
#pragma unroll
        for (int p = 0; p < NB; ++p) {
          wyi[p] = wa * (double)ye[ta + 16 * p];
          yj[p] = (double)ye[tb + 16 * p];
        }
#pragma unroll
        for (int p = 0; p < NB; ++p) {
#pragma unroll
          for (int q = 0; q <= p; ++q)
            acc[p * (p + 1) / 2 + q] = fma(wyi[p], yj[q], acc[p * (p + 1) / 2 + q]);
        }
        if (t < KP) bacc = fma(swb[e], (double)ye[t], bacc);
      }
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
      for (int c = t; c < ld_out; c += kFiThreads) xr[c] = 0.f;
      __syncthreads();  // scnt is rewritten by the next row
      continue;
    }

    // accumulators -> the packed triangle, row k = b
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

    // LDL^T, right-looking, column j left as l_ij d_j; row k (= b) rides along, so that
    // after column j its entry j holds (L^-1 b)_j
    // A pivot counts as positive only above kFiPivotEps of its diagonal entry of A: below
    // that it is rounding residue of the elimination (k * 2^-53 <= 2^-46 of a_jj), whose
    // sign is chance, so a rank-deficient A is reported whichever way it rounded.
    bool ok = true;
    for (int j = 0; j < k; ++j) {
      const double d = Ap[j * (j + 1) / 2 + j];
      if (!(d > kFiPivotEps * sx[j])) {  // the same words for every thread: a uniform exit
        ok = false;
        break;
      }
      const double inv_d = 1.0 / d;
      for (int i = j + 1 + ta; i <= k; i += 16) {
        const double cij = Ap[i * (i + 1) / 2 + j] * inv_d;
        const int lmax = i < k ? i : k - 1;
        for (int l = j + 1 + tb; l <= lmax; l += 16)
          Ap[i * (i + 1) / 2 + l] = fma(-cij, Ap[l * (l + 1) / 2 + j], Ap[i * (i + 1) / 2 + l]);
      }
      __syncthreads();
    }
    if (!ok) {
      if (t == 0) atomicCAS(status, 0, (int32_t)(row + 1));
      for (int c = t; c < ld_out; c += kFiThreads) xr[c] = 0.f;
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
    for (int c = t; c < ld_out; c += kFiThreads) xr[c] = c < k ? (float)zi : 0.f;
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
  ALS_REQUIRE(k >= 1 && k <= kFiMaxRank, ALS_EUNSUPPORTED, "als_fold_in: rank %d not in [1, %d]",
              k, kFiMaxRank);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL,
              "als_fold_in: ld %d must be >= k and a multiple of 4", ld);
  ALS_REQUIRE(ld_out >= k && ld_out % 4 == 0, ALS_EINVAL,
              "als_fold_in: ld_out %d must be >= k and a multiple of 4", ld_out);
  ALS_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31) - 1, ALS_EINVAL,
              "als_fold_in: n_rows outside [0, 2^31 - 1)");
  ALS_REQUIRE(n_src >= 0 && n_src < (int64_t(1) << 31), ALS_EINVAL,
              "als_fold_in: n_src outside [0, 2^31)");
  ALS_REQUIRE(reg >= 0.f && alpha >= 0.f, ALS_EINVAL, "als_fold_in: reg/alpha must be >= 0");
  ALS_REQUIRE(!implicit || yty_packed, ALS_EINVAL, "als_fold_in: implicit needs yty_packed");
  if (n_rows == 0) return ALS_OK;
  ALS_REQUIRE(row_ptr && col && val && X_out && status_dev, ALS_EINVAL,
              "als_fold_in: null pointer");
  ALS_REQUIRE(n_src == 0 || Y_src, ALS_EINVAL, "als_fold_in: null Y_src");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(Y_src) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(X_out) & 15) == 0,
              ALS_EINVAL, "als_fold_in: Y_src / X_out not 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int nb = als_k_pad(k) / 16;
  const int lds = fi_lds(k, 16 * nb).total_bytes;
  const unsigned grid = (unsigned)std::min<int64_t>(n_rows, kFiMaxBlocks);
#define ALS_FI_LAUNCH(NB, IMP)                                                                  \
  do {                                                                                          \
    ALS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fold_in_kernel<NB, IMP>),        \
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));              \
    fold_in_kernel<NB, IMP><<<grid, kFiThreads, lds, st>>>(                                     \
        row_ptr, col, val, n_rows, Y_src, n_src, ld, k, reg, alpha, yty_packed, X_out, ld_out,  \
        n_used_out, status_dev);                                                                \
  } while (0)
#define ALS_FI_MODE(NB)            \
  do {                             \
    if (implicit)                  \
      ALS_FI_LAUNCH(NB, true);     \
    else                           \
      ALS_FI_LAUNCH(NB, false);    \
  } while (0)
  switch (nb) {
    case 1: ALS_FI_MODE(1); break;
    case 2: ALS_FI_MODE(2); break;
    case 4: ALS_FI_MODE(4); break;
    default: ALS_FI_MODE(8); break;
  }
#undef ALS_FI_MODE
#undef ALS_FI_LAUNCH
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // extern "C"
