// Shared by every header of the ALS solve (gram_solve.hip): launch constants, Cfg<CN>
// (tile and slot counts of a padded rank), the vector typedefs, the MFMA tile layout
// (tile_ij, tile_index) and the wave-level primitives (static_for, LDS ordering, DPP,
// reciprocal, row loads).  Used by all kernels of gram_solve.hip.
#pragma once

#include "als_common.h"
#include <utility>

namespace als {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef _Float16 half8v __attribute__((ext_vector_type(8)));
typedef float float2v __attribute__((ext_vector_type(2)));

// src rows per YtY task: a multiple of 32 sized for ~kYtyTasks tasks (two resident
// workgroups per CU, so every task runs in one round: at 512-row tasks a 162k-row
// side left 62 CUs with two tasks and 194 with one, a 59k-row side 140 CUs idle)
constexpr int kYtyTasks = 512;
__host__ __device__ inline int64_t yty_chunk(int64_t n) {
  const int64_t c = (n + kYtyTasks - 1) / kYtyTasks;
  return c < 32 ? 32 : (c + 31) / 32 * 32;
}
// workgroups walking the rescue list (rescue64_kernel).  64, not 256: an empty list (the
// usual case) still costs one finished-block atomic per workgroup on one word; configs[1]
// LAUNCH2 + RESCUE phases 3 us shorter per half-sweep (profiles/r05/ab_rescue_grid.jsonl).
constexpr int kRescueGrid = 64;
// Largest LDL^T pivot spread (max / min pivot of the real dims, a lower bound on
// cond(A)) the fp32 solve keeps: beyond it the row is re-solved in fp64.  Regularised
// rating data (lambda 0.1) spread far less (pivots lie in [lambda_min, lambda_max] and
// the diagonal stays within a few times lambda n); implicit confidences spanning six
// decades spread by 1e3-1e5 and reach 1e-3 errors in fp32.
constexpr float kCondMax = 32.f;
// The same limit for the implicit rows of the rank 65-128 (W1) solve, which has no
// iterative refinement (ranks <= 64 refine every implicit row against Spark's fp64
// residual): implicit counts 1..1e6 at rank 128 left rows with spreads in (8, 32] at
// 4.9e-6..5.6e-6 against the fp64 oracle; at 8 every row of that test is within 8.4e-8
// (the rows beyond it re-solved in fp64) and configs[2] re-solves none (its item rows
// spread 2-4, user rows < 2): 9.01 / 9.09 ms/iter at 32 / 8, profiles/r06/ab_cond_implicit.txt.
constexpr float kCondMaxImplicit = 8.f;
constexpr int kMaxRank = 128;

template <int CN>
struct Cfg {
  static constexpr int KP = 16 * CN;                  // padded rank
  static constexpr int NT = CN * (CN + 1) / 2;        // upper 16x16 tiles
  static constexpr int NP = KP * (KP + 1) / 2;        // packed lower entries
  static constexpr int SLOT = (NT * 4 + CN + 1) * 64; // doubles per partial slot
};

static inline int cn_for_k(int k) { return k <= 16 ? 1 : (k <= 32 ? 2 : (k <= 64 ? 4 : 8)); }

// Compile-time loop over 0..N-1 (indices are constant expressions in the body,
// so register arrays indexed through constexpr tables stay in registers).
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// Wave-local LDS ordering (lanes of one wave exchanging values through LDS).
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// Compiler-only ordering of one wave's LDS accesses: the LDS executes a wave's DS
// instructions in issue order, so a read issued after a write (any lane) returns
// the written data without draining lgkmcnt; the compiler inserts the waits for
// the loaded values where they are used.
__device__ __forceinline__ void wave_lds_order() { asm volatile("" ::: "memory"); }

template <int CN>
__device__ __forceinline__ void load_dims(const float* __restrict__ p, float (&y)[CN]) {
  if constexpr (CN == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
  } else if constexpr (CN == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    y[0] = v.x; y[1] = v.y;
  } else {
    y[0] = *p;
  }
}

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL,
                                                               0xF, 0xF, false));
}

__device__ __forceinline__ float rcp_t(float d) { return __builtin_amdgcn_rcpf(d); }
__device__ __forceinline__ double rcp_t(double d) {
  double y = __builtin_amdgcn_rcp(d);  // v_rcp_f64 estimate + two Newton steps
  y = fma(fma(-d, y, 1.0), y, y);
  return fma(fma(-d, y, 1.0), y, y);
}
__device__ __forceinline__ float readlane_t(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ double readlane_t(double v, int l) { return readlane_f64(v, l); }

// (i, j) of register r of upper tile tt for this lane (MFMA 16x16 C layout:
// row = 4q + r, col = m; dims interleaved as d = 16-index * CN + tile-index).
template <int CN>
__device__ __forceinline__ void tile_ij(int c1, int c2, int r, int& i, int& j) {
  const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
  i = (4 * q + r) * CN + c1;
  j = m * CN + c2;
}

__host__ __device__ constexpr int tile_index(int nb, int i, int j) {
  // upper tiles in (c1, c2 >= c1) row order, as the Gram accumulates them
  return i * nb - i * (i - 1) / 2 + (j - i);
}

}  // namespace als
