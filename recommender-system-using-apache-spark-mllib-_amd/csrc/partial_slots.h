// Partial sums of a heavy row's chunks (and of the YtY tasks): the slot layout, its
// store / add helpers, and launch 2a, the kernels that sum a heavy row's chunk slots
// (heavy_sum_f64_kernel at rank <= 64, heavy_sum_w1_kernel at rank 65-128).  Used by
// the four solve kernels and the YtY kernels.
#pragma once

#include "solve_config.h"
#include "gram_accumulate.h"
#include "w1_solve.h"

namespace als {

// Partial-sum slot of one task: N tiles x 4 accumulator rows, NRA rhs values and
// the positive-rating count, each as 64 lane-contiguous values of SlotT: fp64 for the
// YtY tasks, fp32 for the chunk tasks of the k <= 64 heavy rows (a chunk task's sums are
// fp32 anyway: storing them as fp64 only doubled the launch-1 write and launch-2a read
// bytes).
template <int N, int NRA>
struct Slot {
  static constexpr int SIZE = (N * 4 + NRA + 1) * 64;
};

template <int N, int NRA, class AccT, class SlotT>
__device__ __forceinline__ void store_slot(SlotT* __restrict__ slot, const AccT (&tot)[N][4],
                                           const AccT (&bt)[NRA], float npos) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < N; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) slot[(t * 4 + r) * 64 + lane] = (SlotT)tot[t][r];
#pragma unroll
  for (int c = 0; c < NRA; ++c) slot[(N * 4 + c) * 64 + lane] = (SlotT)bt[c];
  slot[(N * 4 + NRA) * 64 + lane] = (SlotT)npos;
}

template <int N, int NRA, class SlotT>
__device__ __forceinline__ void add_slot(const SlotT* __restrict__ slot, double (&a64)[N][4],
                                         double (&b64)[NRA], int& npos) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < N; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) a64[t][r] += (double)slot[(t * 4 + r) * 64 + lane];
#pragma unroll
  for (int c = 0; c < NRA; ++c) b64[c] += (double)slot[(N * 4 + c) * 64 + lane];
  npos += (int)slot[(N * 4 + NRA) * 64 + lane];
}

template <int N, int NRA, class AccT>
__device__ __forceinline__ void zero_acc(AccT (&tot)[N][4], AccT (&bt)[NRA]) {
#pragma unroll
  for (int t = 0; t < N; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) tot[t][r] = AccT(0);
#pragma unroll
  for (int c = 0; c < NRA; ++c) bt[c] = AccT(0);
}

// Launch 2a (k <= 64): a heavy row's fp32 chunk slots summed element-wise in fp64 (one
// thread per slot element, four interleaved partial sums in a fixed order), rounded
// once to fp32 into its first slot; each thread reads and writes only its own element.
// Explicit: the last 64 entries (each chunk's scaled max |rating|) take the max.
// The partial slots of heavy row h: [slot_begin[h], slot_begin[h+1]) and, for a
// two-segment schedule (slot_begin2 != null: the sharded engine's pipelined item
// side, whose rows have an early and a late rating segment), [slot_begin2[h],
// slot_begin2[h+1]).  The first slot of the union is the row's home slot, where
// launch 2a leaves the sum.
struct SlotRange {
  int s0, n1, t0, n;
  __device__ __forceinline__ int at(int i) const { return i < n1 ? s0 + i : t0 + (i - n1); }
  __device__ __forceinline__ int home() const { return at(0); }
};
__device__ __forceinline__ SlotRange slot_range(const int32_t* __restrict__ sb,
                                                const int32_t* __restrict__ sb2, int h) {
  SlotRange r;
  r.s0 = sb[h];
  r.n1 = sb[h + 1] - r.s0;
  r.t0 = sb2 ? sb2[h] : 0;
  r.n = r.n1 + (sb2 ? sb2[h + 1] - r.t0 : 0);
  return r;
}

template <int SLOT, bool IMPLICIT>
__global__ __launch_bounds__(256) void heavy_sum_f64_kernel(const int32_t* __restrict__ slot_begin,
                                                            const int32_t* __restrict__ slot_begin2,
                                                            float* __restrict__ slots) {
  const int h = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= SLOT) return;
  const SlotRange sr = slot_range(slot_begin, slot_begin2, h);
  if (sr.n <= 1) return;
  const int64_t home = (int64_t)sr.home() * SLOT + e;
  if (!IMPLICIT && e >= SLOT - 64) {
    float mx = 0.f;
    for (int i = 0; i < sr.n; ++i) mx = fmaxf(mx, slots[(int64_t)sr.at(i) * SLOT + e]);
    slots[home] = mx;
    return;
  }
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int i = 0;
  for (; i + 4 <= sr.n; i += 4) {
    a0 += (double)slots[(int64_t)sr.at(i) * SLOT + e];
    a1 += (double)slots[(int64_t)sr.at(i + 1) * SLOT + e];
    a2 += (double)slots[(int64_t)sr.at(i + 2) * SLOT + e];
    a3 += (double)slots[(int64_t)sr.at(i + 3) * SLOT + e];
  }
  for (; i < sr.n; ++i) a0 += (double)slots[(int64_t)sr.at(i) * SLOT + e];
  slots[home] = (float)((a0 + a1) + (a2 + a3));
}

// Launch 2a: the fp32 chunk slots of every heavy row summed in fp64 (element-wise,
// one thread per slot element; fixed order: four interleaved partial sums),
// the implicit YtY added in fp64, then rounded once to fp32 into the row's first
// slot (each thread reads and writes only its own element: in place is safe).
// Four consecutive elements per thread (16-B loads and stores: the slots are
// 16-B aligned and kW1Slot is a multiple of 4), each with the same four partial
// sums in the same order as one element per thread.
template <bool IMPLICIT>
__global__ __launch_bounds__(256) void heavy_sum_w1_kernel(const int32_t* __restrict__ slot_begin,
                                                           const int32_t* __restrict__ slot_begin2,
                                                           float* __restrict__ slots,
                                                           const double* __restrict__ yty) {
  constexpr int CN = 8, NT = kW1NT, NE = (NT * 4 + CN + 1) * 64;
  static_assert(NE % 4 == 0 && kW1Slot % 4 == 0, "heavy_sum_w1: float4 elements");
  const int h = blockIdx.y;
  const int e = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (e >= NE) return;
  const SlotRange sr = slot_range(slot_begin, slot_begin2, h);
  auto ld4 = [&](int i) -> float4 {
    return *reinterpret_cast<const float4*>(slots + (int64_t)sr.at(i) * kW1Slot + e);
  };
  double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
  double a2[4] = {0.0, 0.0, 0.0, 0.0}, a3[4] = {0.0, 0.0, 0.0, 0.0};
  auto add = [](double (&a)[4], const float4& x) {
    a[0] += (double)x.x;
    a[1] += (double)x.y;
    a[2] += (double)x.z;
    a[3] += (double)x.w;
  };
  int i = 0;
  for (; i + 4 <= sr.n; i += 4) {
    const float4 x0 = ld4(i), x1 = ld4(i + 1), x2 = ld4(i + 2), x3 = ld4(i + 3);
    add(a0, x0);
    add(a1, x1);
    add(a2, x2);
    add(a3, x3);
  }
  for (; i < sr.n; ++i) add(a0, ld4(i));
  const int ent = e >> 6;  // e .. e + 3 share one entry (64 elements per entry)
  float o[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = (float)((a0[c] + a1[c]) + (a2[c] + a3[c]));
  if (!IMPLICIT && ent == NT * 4 + CN) {  // the chunks' scaled max |rating|: max, not sum
    float mx[4] = {0.f, 0.f, 0.f, 0.f};
    for (i = 0; i < sr.n; ++i) {
      const float4 x = ld4(i);
      mx[0] = fmaxf(mx[0], x.x);
      mx[1] = fmaxf(mx[1], x.y);
      mx[2] = fmaxf(mx[2], x.z);
      mx[3] = fmaxf(mx[3], x.w);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = mx[c];
  }
  if (IMPLICIT && ent < NT * 4) {
    const int t = ent >> 2, r = ent & 3;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int lane = (e + c) & 63;
      const int ii = (4 * (lane >> 4) + r) * CN + FullTiles<CN>::l1(t);
      const int jj = (lane & 15) * CN + FullTiles<CN>::l2(t);
      const int hi = ii > jj ? ii : jj, lo = ii > jj ? jj : ii;
      o[c] = (float)(((a0[c] + a1[c]) + (a2[c] + a3[c])) + yty[hi * (hi + 1) / 2 + lo]);
    }
  }
  *reinterpret_cast<float4*>(slots + (int64_t)sr.home() * kW1Slot + e) =
      make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace als
