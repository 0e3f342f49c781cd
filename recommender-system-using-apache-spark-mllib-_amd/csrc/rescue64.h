// The fp64 re-solve of the rows on the rescue list: rescue64_kernel.
#pragma once

#include "solve_config.h"
#include "solve_guards.h"

namespace als {

// Rescue launch: every row the fp32-grade path did not solve to the 1e-4 bar — its
// operands missed the split window (window_miss), its LDL^T pivots spread beyond
// kCondMax, or a pivot was not positive / the solution not finite — is re-solved with
// Spark's own arithmetic: the normal equations accumulated in fp64 from the fp32 factor
// rows (NormalEquation.add's dspr / daxpy: products of fp32 values are exact in fp64),
// implicit YtY merged in fp64, lambda * numExplicits on the diagonal, and a fp64
// Cholesky (dppsv) of the packed lower triangle in LDS.  A pivot that is not positive
// in fp64 either is Spark's failure: status = row + 1.  One 256-thread workgroup per
// listed row (a few hundred workgroups walk the list; an empty list costs one launch).
constexpr int kRescueThreads = 256;
constexpr int kRescueBatch = 32;  // ratings staged per step

// (i, j), i >= j, of lower-packed entry e (e = i (i + 1) / 2 + j).
__device__ __forceinline__ void packed_ij(int e, int& i, int& j) {
  int r = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= e) ++r;
  while (r * (r + 1) / 2 > e) --r;
  i = r;
  j = e - r * (r + 1) / 2;
}

template <bool IMPLICIT>
__global__ __launch_bounds__(kRescueThreads) void rescue64_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, const float* __restrict__ Y, int ld, int k, float reg,
    float alpha, const double* __restrict__ yty, float* __restrict__ X,
    int32_t* __restrict__ status, RescueList rl) {
  constexpr int NPMAX = kMaxRank * (kMaxRank + 1) / 2;
  __shared__ double Ap[NPMAX];  // lower-packed A
  __shared__ double bs[kMaxRank];
  __shared__ float ys[kRescueBatch][kMaxRank + 1];
  __shared__ double wa[kRescueBatch], wb[kRescueBatch];
  __shared__ int npos_s;
  __shared__ int fail_s;
  const int tid = threadIdx.x;
  const int np = k * (k + 1) / 2;
  const unsigned n_app = *rl.cnt;
  const unsigned n_list = n_app < rl.cap ? n_app : rl.cap;
  if (n_app > rl.cap && blockIdx.x == 0 && tid == 0)
    atomicExch(status, -1);  // appended past the list: the phases ran out of order
  for (unsigned it = blockIdx.x; it < n_list; it += gridDim.x) {
    const int row = rl.list[it];
    const int64_t pb = row_ptr[row], pe = row_ptr[row + 1];
    for (int e = tid; e < np; e += kRescueThreads) Ap[e] = IMPLICIT ? yty[e] : 0.0;
    for (int d = tid; d < k; d += kRescueThreads) bs[d] = 0.0;
    if (tid == 0) {
      npos_s = 0;
      fail_s = 0;
    }
    __syncthreads();
    int npos = 0;
    for (int64_t base = pb; base < pe; base += kRescueBatch) {
      const int nb = (int)(pe - base < kRescueBatch ? pe - base : kRescueBatch);
      if (tid < kRescueBatch) {
        const bool v = tid < nb;
        const double r = v ? (double)val[base + tid] : 0.0;
        if (IMPLICIT) {
          const double c1 = (double)alpha * fabs(r);
          wa[tid] = v ? c1 : 0.0;
          wb[tid] = (v && r > 0.0) ? 1.0 + c1 : 0.0;
          npos += (v && r > 0.0) ? 1 : 0;
        } else {
          wa[tid] = v ? 1.0 : 0.0;
          wb[tid] = r;
        }
      }
      for (int x = tid; x < kRescueBatch * k; x += kRescueThreads) {
        const int jr = x / k, d = x - jr * k;
        ys[jr][d] = jr < nb ? Y[(int64_t)col[base + jr] * ld + d] : 0.f;
      }
      __syncthreads();
      for (int e = tid; e < np; e += kRescueThreads) {
        int i, j;
        packed_ij(e, i, j);
        double acc = 0.0;
        for (int jr = 0; jr < nb; ++jr)
          acc = fma(wa[jr], (double)ys[jr][i] * (double)ys[jr][j], acc);
        Ap[e] += acc;
      }
      for (int d = tid; d < k; d += kRescueThreads) {
        double acc = 0.0;
        for (int jr = 0; jr < nb; ++jr) acc = fma(wb[jr], (double)ys[jr][d], acc);
        bs[d] += acc;
      }
      __syncthreads();
    }
    if (IMPLICIT && tid < kRescueBatch) atomicAdd(&npos_s, npos);
    __syncthreads();
    const double lam = (double)reg * (double)(IMPLICIT ? npos_s : (int)(pe - pb));
    for (int d = tid; d < k; d += kRescueThreads) Ap[d * (d + 1) / 2 + d] += lam;
    __syncthreads();
    // Cholesky A = L L^T (right-looking, packed lower, in place)
    for (int jc = 0; jc < k; ++jc) {
      const int dj = jc * (jc + 1) / 2 + jc;
      const double dd = Ap[dj];
      if (!(dd > 0.0)) {  // uniform: every thread reads the same value
        if (tid == 0) fail_s = 1;
        break;
      }
      const double l = sqrt(dd);
      __syncthreads();
      if (tid == 0) Ap[dj] = l;
      for (int i = jc + 1 + tid; i < k; i += kRescueThreads) Ap[i * (i + 1) / 2 + jc] /= l;
      __syncthreads();
      const int m = k - jc - 1;  // trailing block, lower-packed entries (a, c), c <= a
      for (int t = tid; t < m * (m + 1) / 2; t += kRescueThreads) {
        int a, c;
        packed_ij(t, a, c);
        const int ia = jc + 1 + a, ic = jc + 1 + c;
        Ap[ia * (ia + 1) / 2 + ic] -= Ap[ia * (ia + 1) / 2 + jc] * Ap[ic * (ic + 1) / 2 + jc];
      }
      __syncthreads();
    }
    __syncthreads();
    float* xrow = X + (int64_t)row * ld;
    if (fail_s) {
      if (tid == 0) atomicCAS(status, 0, row + 1);  // Spark: dppsv info > 0
      for (int d = tid; d < ld; d += kRescueThreads) xrow[d] = 0.f;
    } else {
      // L y = b (forward), L^T x = y (backward), column-oriented
      for (int jc = 0; jc < k; ++jc) {
        const double yj = bs[jc] / Ap[jc * (jc + 1) / 2 + jc];
        __syncthreads();
        if (tid == 0) bs[jc] = yj;
        for (int i = jc + 1 + tid; i < k; i += kRescueThreads) bs[i] -= Ap[i * (i + 1) / 2 + jc] * yj;
        __syncthreads();
      }
      for (int jc = k - 1; jc >= 0; --jc) {
        const double xj = bs[jc] / Ap[jc * (jc + 1) / 2 + jc];
        __syncthreads();
        if (tid == 0) bs[jc] = xj;
        for (int i = tid; i < jc; i += kRescueThreads) bs[i] -= Ap[jc * (jc + 1) / 2 + i] * xj;
        __syncthreads();
      }
      for (int d = tid; d < ld; d += kRescueThreads) xrow[d] = d < k ? (float)bs[d] : 0.f;
    }
    __syncthreads();  // LDS reused by the next listed row
  }
  // the list is consumed: the last block to finish (every block read the count before
  // its increment) empties it for the next LAUNCH1 of this workspace.  rl.cnt[1] is
  // the finished-block counter (zeroed with the count by the prep, reset here).  No
  // fence: a block's read of the count returned before its increment was issued (the
  // loop bound depends on it), and nothing else in this launch reads what it wrote.
  __syncthreads();
  if (tid == 0) {
    if (atomicAdd(rl.cnt + 1, 1u) == gridDim.x - 1) {
      rl.cnt[0] = 0u;
      rl.cnt[1] = 0u;
    }
  }
}

}  // namespace als
