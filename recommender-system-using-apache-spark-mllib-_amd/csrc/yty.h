// K2b, YtY of one factor matrix: the partial and reduce kernels (one wavefront per task at
// rank <= 64, one workgroup of four at rank 65-128) and slot_sum_kernel between them.
#pragma once

#include "solve_config.h"
#include "gram_accumulate.h"
#include "partial_slots.h"

namespace als {

// Scatter the MFMA-layout matrix into the packed lower triangle P (type T) in LDS.
template <int CN, class T>
__device__ __forceinline__ void pack_gram(const double (&a64)[Cfg<CN>::NT][4], T* __restrict__ P) {
  int tt = 0;
#pragma unroll
  for (int c1 = 0; c1 < CN; ++c1) {
#pragma unroll
    for (int c2 = c1; c2 < CN; ++c2) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i, j;
        tile_ij<CN>(c1, c2, r, i, j);
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        P[hi * (hi + 1) / 2 + lo] = (T)a64[tt][r];
      }
      ++tt;
    }
  }
}

// K2b: YtY partial Grams over row chunks of Y (unweighted, identity gather), fp64.
template <int CN>
__global__ __launch_bounds__(64, 2) void yty_partial_kernel(const float* __restrict__ Y, int64_t n,
                                                            int ld, int k,
                                                            double* __restrict__ slots) {
  constexpr int NT = Cfg<CN>::NT;
  double a64[NT][4], b64[CN];
  zero_acc<NT, CN, double>(a64, b64);
  int npos = 0;
  const int64_t chunk = yty_chunk(n);
  const int64_t pb = (int64_t)blockIdx.x * chunk;
  const int64_t pe = pb + chunk < n ? pb + chunk : n;
  gram_accumulate<CN, false, true, double>(nullptr, nullptr, pb, pe, Y, ld, k, 0.f, a64, b64,
                                           npos);
  store_slot<NT, CN, double>(slots + (int64_t)blockIdx.x * Cfg<CN>::SLOT, a64, b64, (float)npos);
}

template <int CN>
__global__ __launch_bounds__(64) void yty_reduce_kernel(const double* __restrict__ slots,
                                                        int nslots, double* __restrict__ out) {
  constexpr int NT = Cfg<CN>::NT, NP = Cfg<CN>::NP;
  __shared__ double P[NP];
  double a64[NT][4], b64[CN];
  zero_acc<NT, CN, double>(a64, b64);
  int npos = 0;
  for (int s = 0; s < nslots; ++s) add_slot<NT, CN>(slots + (int64_t)s * Cfg<CN>::SLOT, a64, b64, npos);
  pack_gram<CN, double>(a64, P);
  __syncthreads();
  for (int e = threadIdx.x; e < NP; e += 64) out[e] = P[e];
}

// ---------------------------------------------------------------------------
// K2b at 64 < k <= 128: one workgroup of 4 wavefronts per YtY task, wave R
// accumulating the tiles of WgTiles<R> (10/10/8/8 of the 36 upper tiles).
// ---------------------------------------------------------------------------
constexpr int kWgNB = 8;
constexpr int kWgSub = Slot<10, 4>::SIZE;  // doubles per wave sub-slot (max over roles)
constexpr int kWgSlot = 4 * kWgSub;

template <int R>
__device__ __forceinline__ void wg_yty_partial_task(const float* __restrict__ Y, int64_t n, int ld,
                                                    int k, double* __restrict__ slots) {
  typedef WgTiles<R> TS;
  double a64[TS::N][4], b64[TS::NRA];
  zero_acc<TS::N, TS::NRA, double>(a64, b64);
  int npos = 0;
  const int64_t chunk = yty_chunk(n);
  const int64_t pb = (int64_t)blockIdx.x * chunk;
  const int64_t pe = pb + chunk < n ? pb + chunk : n;
  gram_accumulate<kWgNB, false, true, double, TS>(nullptr, nullptr, pb, pe, Y, ld, k, 0.f, a64,
                                                  b64, npos);
  store_slot<TS::N, TS::NRA, double>(slots + (int64_t)blockIdx.x * kWgSlot + R * kWgSub, a64, b64,
                                     (float)npos);
}

template <int R>
__device__ __forceinline__ void wg_yty_reduce_task(const double* __restrict__ slots, int nslots,
                                                   double* __restrict__ out) {
  typedef WgTiles<R> TS;
  double a64[TS::N][4], b64[TS::NRA];
  zero_acc<TS::N, TS::NRA, double>(a64, b64);
  int npos = 0;
  for (int s = 0; s < nslots; ++s)
    add_slot<TS::N, TS::NRA>(slots + (int64_t)s * kWgSlot + R * kWgSub, a64, b64, npos);
  static_for<TS::N>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    constexpr int c1 = TS::g1(t), c2 = TS::g2(t);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i, j;
      tile_ij<kWgNB>(c1, c2, r, i, j);
      // a diagonal tile holds both (i, j) and (j, i): store the lower one only
      if (c1 < c2 || i >= j) {
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        out[hi * (hi + 1) / 2 + lo] = a64[t][r];
      }
    }
  });
}

// The workgroup kernels: wave index -> role (wave-uniform branch).
#define ALS_WG_ROLES(CALL) \
  do {                                                                    \
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      \
    if (wv == 0) CALL(0);                                                 \
    else if (wv == 1) CALL(1);                                            \
    else if (wv == 2) CALL(2);                                            \
    else CALL(3);                                                         \
  } while (0)

// Element-wise fp64 sum of the YtY task slots, so the final reduce reads one slot.
// A workgroup owns 64 consecutive elements (one per lane, coalesced) and 16
// wavefronts: wave w sums slots w, w + 16, ... (8 loads in flight per round),
// then wave 0 adds the 16 partials in wave order — a fixed order, so the result
// is deterministic.  (One thread per element over every slot left a few dozen
// workgroups waiting on one load round trip per 4 slots: 43 us at 318 slots.)
constexpr int kSlotSumWaves = 16;
__global__ __launch_bounds__(64 * kSlotSumWaves) void slot_sum_kernel(
    const double* __restrict__ slots, int nslots, int64_t slot_len, double* __restrict__ out) {
  __shared__ double part[kSlotSumWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * 64 + lane;
  double s = 0.0;
  if (e < slot_len) {
    constexpr int kBatch = 8;
    int i = w;
    for (; i + kSlotSumWaves * (kBatch - 1) < nslots; i += kSlotSumWaves * kBatch) {
      double v[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) v[j] = slots[(int64_t)(i + kSlotSumWaves * j) * slot_len + e];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) s += v[j];
    }
    for (; i < nslots; i += kSlotSumWaves) s += slots[(int64_t)i * slot_len + e];
  }
  part[w][lane] = s;
  __syncthreads();
  if (w == 0 && e < slot_len) {
    double t = part[0][lane];
#pragma unroll
    for (int j = 1; j < kSlotSumWaves; ++j) t += part[j][lane];
    out[e] = t;
  }
}

__global__ __launch_bounds__(256, 2) void yty_partial_wg_kernel(const float* __restrict__ Y,
                                                                int64_t n, int ld, int k,
                                                                double* __restrict__ slots) {
#define CALL(R) wg_yty_partial_task<R>(Y, n, ld, k, slots)
  ALS_WG_ROLES(CALL);
#undef CALL
}

__global__ __launch_bounds__(256) void yty_reduce_wg_kernel(const double* __restrict__ slots,
                                                            int nslots, double* __restrict__ out) {
#define CALL(R) wg_yty_reduce_task<R>(slots, nslots, out)
  ALS_WG_ROLES(CALL);
#undef CALL
}
#undef ALS_WG_ROLES

}  // namespace als
