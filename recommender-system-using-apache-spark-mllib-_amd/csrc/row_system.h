// The per-row normal equations of K7 (fold_in.hip), K11 (explain.hip) and K13 (nnls.hip), in
// one place: A = sum_j wa_j y_j y_j^T (+ YtY) + reg * n I and b = sum_j wb_j y_j over a ragged
// row's ratings, formed by one 256-thread workgroup (the steps: fold_in.hip's head), and
// on the host the argument checks and the NB x IMPLICIT dispatch of the three entry points.
// Every device helper is inlined and takes the accumulators by reference, so they stay in
// registers.  The order of every floating-point operation is part of the contract:
// tests/test_gpu_row_kernel_bits.py pins the bits of all three kernels.
#pragma once
#include <type_traits>

#include "als_common.h"

namespace als {

constexpr int kRowThreads = 256;
constexpr int kRowBatch = 32;         // ratings gathered per step
constexpr int kRowMaxRank = 128;
constexpr int kRowMaxBlocks = 65536;  // blocks stride over the rows / tasks past this
// A pivot of the LDL^T counts as positive only above kRowPivotEps of its diagonal entry of A
// as summed: below that it is rounding residue of the elimination (k * 2^-53 <= 2^-46 of
// a_jj at k <= kRowMaxRank), whose sign is chance, so a rank-deficient A is reported
// whichever way it rounded.
constexpr double kRowPivotEps = 0x1p-46;

// Wave 0: ids and weights of the batch starting at s0; counts the used entries (n_used) and
// those with r > 0 (n_pos).  An item outside [0, n_src) is unknown: id -1, both weights 0.
template <bool IMPLICIT>
__device__ __forceinline__ void row_weights(int64_t s0, int64_t pe, const int32_t* __restrict__ col,
                                            const float* __restrict__ val, int64_t n_src,
                                            float alpha, int lane, int* scol, double* swa,
                                            double* swb, int& n_used, int& n_pos) {
  bool used = false, pos = false;
  if (lane < kRowBatch) {
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

// All threads: the batch's factor rows into LDS as float4 pieces, columns >= k and unknown
// items as zeros.  YS: the row stride of ybuf in floats (>= KP, a multiple of 4).
template <int KP, int YS>
__device__ __forceinline__ void row_gather(const float* __restrict__ Y, int ld, int k,
                                           const int* scol, float* ybuf, int t) {
  constexpr int P4 = KP / 4;  // float4 pieces per gathered row
  for (int g = t; g < kRowBatch * P4; g += kRowThreads) {
    const int e = g / P4, c0 = (g % P4) * 4;
    const int c = scol[e];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c >= 0 && c0 < k) {  // c0 < k <= ld and ld % 4 == 0: the piece lies inside the row
      v = *reinterpret_cast<const float4*>(Y + (int64_t)c * ld + c0);
      if (c0 + 1 >= k) v.y = 0.f;
      if (c0 + 2 >= k) v.z = 0.f;
      if (c0 + 3 >= k) v.w = 0.f;
    }
    *reinterpret_cast<float4*>(ybuf + e * YS + c0) = v;
  }
}

// The first nb gathered ratings into the accumulators, in order: acc[p (p + 1) / 2 + q] is
// entry (ta + 16 p, tb + 16 q) of A and, WITH_B, bacc is b[t] in the threads t < k_pad.
template <int NB, int YS, bool WITH_B>
__device__ __forceinline__ void row_gram_batch(const float* ybuf, int nb, const double* swa,
                                               const double* swb,
                                               double (&acc)[NB * (NB + 1) / 2], double& bacc) {
  const int t = threadIdx.x;
  const int ta = t >> 4, tb = t & 15;
  for (int e = 0; e < nb; ++e) {
    const float* ye = ybuf + e * YS;
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
    if constexpr (WITH_B) {
      if (t < 16 * NB) bacc = fma(swb[e], (double)ye[t], bacc);
    }
  }
}

// The Gram of the ratings [pb, pe) in the caller's accumulators, 32 ratings at a time: the
// batch loop of K13's two kernels.  (K7 and K11 write the same loop out around the three
// helpers above: as one helper it cost both about 3 % at rank 128.)  n_used / n_pos are
// valid in wave 0.  Ends on a barrier: scol, the weights and ybuf are free when it returns.
template <int NB, bool IMPLICIT>
__device__ __forceinline__ void row_gram(int64_t pb, int64_t pe, const int32_t* __restrict__ col,
                                         const float* __restrict__ val,
                                         const float* __restrict__ Y, int64_t n_src, int ld, int k,
                                         float alpha, int* scol, double* swa, double* swb,
                                         float* ybuf, double (&acc)[NB * (NB + 1) / 2],
                                         double& bacc, int& n_used, int& n_pos) {
  constexpr int KP = 16 * NB;
  const int t = threadIdx.x;
  for (int64_t s0 = pb; s0 < pe; s0 += kRowBatch) {
    if (t < 64)
      row_weights<IMPLICIT>(s0, pe, col, val, n_src, alpha, t & 63, scol, swa, swb, n_used, n_pos);
    __syncthreads();
    row_gather<KP, KP>(Y, ld, k, scol, ybuf, t);
    __syncthreads();
    const int nb = pe - s0 < kRowBatch ? (int)(pe - s0) : kRowBatch;
    row_gram_batch<NB, KP, true>(ybuf, nb, swa, swb, acc, bacc);
    __syncthreads();  // the next batch (or the caller) overwrites scol and ybuf
  }
}

// LDL^T of the packed triangle, right-looking, column j left as l_ij d_j, one barrier per
// column.  WITH_B: row k of the triangle holds a right-hand side b and rides along, so that
// its entry j is (L^-1 b)_j after column j; else rows up to k - 1 are eliminated.  sdiag: the
// diagonal of A as summed, the scale of each pivot's rounding error.  False when a pivot fails
// the kRowPivotEps test (the same words for every thread: a uniform exit).  Starts after
// the caller's barrier over Ap and sdiag.
template <bool WITH_B>
__device__ __forceinline__ bool row_ldlt(double* Ap, const double* sdiag, int k) {
  const int t = threadIdx.x;
  const int ta = t >> 4, tb = t & 15;
  bool ok = true;
  for (int j = 0; j < k; ++j) {
    const double d = Ap[j * (j + 1) / 2 + j];
    if (!(d > kRowPivotEps * sdiag[j])) {
      ok = false;
      break;
    }
    const double inv_d = 1.0 / d;
    for (int i = j + 1 + ta; WITH_B ? i <= k : i < k; i += 16) {
      const double cij = Ap[i * (i + 1) / 2 + j] * inv_d;
      const int lmax = WITH_B ? (i < k ? i : k - 1) : i;
      for (int l = j + 1 + tb; l <= lmax; l += 16)
        Ap[i * (i + 1) / 2 + l] = fma(-cij, Ap[l * (l + 1) / 2 + j], Ap[i * (i + 1) / 2 + l]);
    }
    __syncthreads();
  }
  return ok;
}

// ---- host side ----
// The argument checks the three entry points share, fn in front of every message: first
// the scalars (row_check_args), then, once the entry point has returned for n_rows == 0 and
// checked its own pointers, the source table (row_check_source).  X_out: the output table
// that shares Y_src's alignment rule, or nullptr for an entry point without one.
static inline int row_check_args(const char* fn, int k, int ld, int64_t n_rows, int64_t n_src,
                                 float reg, float alpha, int implicit, const double* yty_packed) {
  ALS_REQUIRE(k >= 1 && k <= kRowMaxRank, ALS_EUNSUPPORTED, "%s: rank %d not in [1, %d]", fn, k,
              kRowMaxRank);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL, "%s: ld %d must be >= k and a multiple of 4",
              fn, ld);
  ALS_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31) - 1, ALS_EINVAL,
              "%s: n_rows outside [0, 2^31 - 1)", fn);
  ALS_REQUIRE(n_src >= 0 && n_src < (int64_t(1) << 31), ALS_EINVAL, "%s: n_src outside [0, 2^31)",
              fn);
  ALS_REQUIRE(reg >= 0.f && alpha >= 0.f, ALS_EINVAL, "%s: reg/alpha must be >= 0", fn);
  ALS_REQUIRE(!implicit || yty_packed, ALS_EINVAL, "%s: implicit needs yty_packed", fn);
  return ALS_OK;
}

static inline int row_check_source(const char* fn, int64_t n_src, const float* Y_src,
                                   const float* X_out) {
  ALS_REQUIRE(n_src == 0 || Y_src, ALS_EINVAL, "%s: null Y_src", fn);
  ALS_REQUIRE(((reinterpret_cast<uintptr_t>(Y_src) | reinterpret_cast<uintptr_t>(X_out)) & 15) == 0,
              ALS_EINVAL, "%s: %s not 16-byte aligned", fn, X_out ? "Y_src / X_out" : "Y_src");
  return ALS_OK;
}

// f(integral_constant<int, NB>, bool_constant<IMPLICIT>) for nb = k_pad / 16 in {1, 2, 4, 8}.
template <class F>
static inline int row_dispatch(int nb, bool implicit, F&& f) {
  auto mode = [&](auto n) {
    return implicit ? f(n, std::true_type{}) : f(n, std::false_type{});
  };
  switch (nb) {
    case 1: return mode(std::integral_constant<int, 1>{});
    case 2: return mode(std::integral_constant<int, 2>{});
    case 4: return mode(std::integral_constant<int, 4>{});
    default: return mode(std::integral_constant<int, 8>{});
  }
}

}  // namespace als
