// The tests that send a row to the fp64 rescue instead of the fp32-grade solve: split
// window, rank-deficient short rows, and the rescue list itself.  Used by the four solve
// kernels, gram_solve_dual_kernel and rescue64_kernel.
#pragma once

#include "solve_config.h"

namespace als {

// Largest value over the wave (every lane gets it; v >= 0, NaN ignored).
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_f<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_f<0x141>(v));  // row_half_mirror
  v = fmaxf(v, dpp_f<0x140>(v));  // row_mirror
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  float c = fmaxf(a, b), d = c;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(c), "+v"(d));
  return fmaxf(c, d);
}

__device__ __forceinline__ float absmax4(const floatx4& x) {
  return fmaxf(fmaxf(__builtin_fabsf(x[0]), __builtin_fabsf(x[1])),
               fmaxf(__builtin_fabsf(x[2]), __builtin_fabsf(x[3])));
}

// ---------------------------------------------------------------------------
// Split window guard.  The explicit Gram and rhs use ONE power-of-two scale per
// launch (max |Y_src| -> [2^14, 2^15), max |rating| likewise), so the f16 lo half
// of an operand t goes subnormal once |t| < 2^-3 and its relative precision then
// degrades towards 2^-24 / |t|.  A row whose own operands all sit that far below
// the launch maxima (a user-supplied U0, a loaded model, ratings spanning many
// decades) would silently lose precision.  Each explicit task therefore checks
// its scaled operands against a window T = 2^-4 (precision of its largest
// operand >= 2^-20, 16x inside the fp32-grade split):
//   max diag(G) < n T^2  (covers every row whose largest |t| < T: diag <= n max t^2)
//   or 0 < max |r| < T   (the row's ratings, scaled by the launch's rating scale).
// A row that misses the window is not solved here: it is appended to the rescue
// list and re-solved in fp64 by rescue64_kernel (as are rows whose fp32 LDL^T pivots
// spread beyond kCondMax, or fail).  Implicit rows need no window test: their A
// includes YtY (>= the largest row's square) and b is fp32.
// ---------------------------------------------------------------------------
constexpr float kWindowT = 0.0625f;  // 2^-4, in scaled units (launch max in [2^14, 2^15))

// Largest diagonal entry of an upper-tile set in the MFMA C layout (this lane's).
// (Lane (q, m) holds a diagonal entry of each diagonal tile iff r = m - 4q is in [0, 4):
// one select per tile, not a compare-and-select per (tile, r) — 4 CN + 1 VALU instead
// of ~4 x 4 CN.)
template <int CN>
__device__ __forceinline__ float diag_max_lane(const floatx4 (&A)[CN * (CN + 1) / 2]) {
  const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
  const int r = m - 4 * q;
  float d = 0.f;
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    const floatx4& t = A[tile_index(CN, c, c)];
    d = fmaxf(d, r == 0 ? t[0] : (r == 1 ? t[1] : (r == 2 ? t[2] : t[3])));
  }
  return (r >= 0 && r < 4) ? d : 0.f;
}

// Sum of the diagonal entries of real dims (dims < k) of an upper-tile set in the C
// layout, summed over the wave (every lane gets it).
template <int CN>
__device__ __forceinline__ float diag_trace(const floatx4 (&A)[CN * (CN + 1) / 2], int k) {
  const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
  float t = 0.f;
#pragma unroll
  for (int c = 0; c < CN; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * q + r == m && m * CN + c < k) t += A[tile_index(CN, c, c)][r];
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  return t;
}

// Very short explicit rows on the primal path (n <= k / 4 ratings; at k > 32 such rows
// take the dual path unless it is off): A = G + lambda n I with G of rank n << k has
// lambda_min = lambda n and lambda_max ~ tr(G) + lambda n, so cond(A) ~ 1 + tr(G) /
// (lambda n), which the LDL^T pivots do not show (they stay within (tr(G) / k + lambda
// n) / (lambda n)).  The fp32 solve's error there grows as that bound (measured ~1.5e-6
// x tr(G) / (lambda n) at n <= 16, k 65-128, lambda 1e-3 / 1e-4; at n > k / 4 the
// measured errors stay ~1e-5 and below, e.g. 8.8e-7 on the configs[3] users of 97-255
// ratings).  Beyond kCondRankDef the row is re-solved in fp64.  tr_scaled: tr(G) in the
// Gram's scale (x 1/inv2).
constexpr float kCondRankDef = 64.f;
template <int CN>
__device__ __forceinline__ bool rank_deficient_illcond(const floatx4 (&acc)[CN * (CN + 1) / 2],
                                                       float inv2, int64_t n, int k, float reg) {
  if (4 * n > (int64_t)k) return false;  // uniform: the trace only for very short rows
  return diag_trace<CN>(acc, k) * inv2 > (kCondRankDef - 1.f) * reg * (float)n;
}

// Wave-uniform: do the scaled operands of a task with n terms miss the window?
// (max over lanes < x <=> no lane at or above x: ballots, no reduction)
__device__ __forceinline__ bool window_miss(float diag_lane, float n_terms, float rmax_lane) {
  const bool dmiss = __ballot(diag_lane >= n_terms * (kWindowT * kWindowT)) == 0 &&
                     __ballot(diag_lane > 0.f) != 0;
  const bool rmiss = __ballot(rmax_lane >= kWindowT) == 0 && __ballot(rmax_lane > 0.f) != 0;
  return dmiss || rmiss;
}

// The rescue list of one als_solve_half call: count word (scale word 2), the list
// (cap = the call's rows) in the workspace.
struct RescueList {
  unsigned* cnt;
  int32_t* list;
  unsigned cap;
};

// Append `row` to the rescue list (one lane).  Each row is appended at most once per
// LAUNCH1..RESCUE sequence; a caller that runs the launches twice without the RESCUE
// phase between them overflows the count, which is never written past `cap`:
// rescue64_kernel walks min(count, cap) entries and reports the overflow (status -1).
__device__ __forceinline__ void rescue_append(const RescueList& rl, int row) {
  if ((threadIdx.x & 63) == 0) {
    const unsigned i = atomicAdd(rl.cnt, 1u);
    if (i < rl.cap) rl.list[i] = row;
  }
}

}  // namespace als
