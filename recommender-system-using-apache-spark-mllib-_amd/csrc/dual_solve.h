// Short explicit rows at rank 33-128 through their n x n dual system:
// gram_solve_dual_kernel and its row solve.
#pragma once

#include "solve_config.h"
#include "gram_accumulate.h"
#include "solve_guards.h"
#include "w1_solve.h"

namespace als {

// ---------------------------------------------------------------------------
// Short explicit rows at 64 < k <= 128: the n x n dual system.
// For a row with n <= 96 ratings r_j on the factor rows y_j (Y_S = n x k):
//   x = (Y_S^T Y_S + lambda n I)^-1 Y_S^T r  =  Y_S^T (Y_S Y_S^T + lambda n I)^-1 r
// (push-through identity (Y^T Y + c I) Y^T = Y^T (Y Y^T + c I); both systems are
// SPD for lambda n > 0).  So x is the solution of Spark's CholeskySolver on the
// k x k normal equations, obtained through an n x n system: for n < k the
// k(k+1)/2-entry Gram and the k^3/3 factorisation become n(n+1)/2 k-dim inner
// products and an n^3/3 one (n = 64, k = 128: 1/2 the Gram, 1/8 the solve).
// Variables: rating j <-> (block c = j % NB, index i = j / NB) — the dim
// permutation of the primal kernels — so w1_solve_x consumes the Gram tiles as
// the MFMAs leave them and pads ratings j >= n the way it pads dims.
//  * Gram G = 2^2ey Y_S Y_S^T on v_mfma_f32_16x16x32_f16 from the split table
//    (hi | lo words of 2^ey Y): MFMA K = dims, 4 k-steps of 32 dims, streamed
//    (step s+1's gathers in flight during step s's MFMAs); operand (c, s) on lane
//    (q, m) = dims 32s + 8q .. +7 of rating m * NB + c; hi.hi + hi.lo + lo.hi per
//    tile per k-step (fp32-grade products, as the primal Gram).
//  * solve: w1_solve_x<NB> (fp32 MFMA tile products), z_j on the lanes of block c.
//  * x = Y_S^T z from the same rows re-gathered (L2-hot): a split word is the f16
//    pair (hi, lo) of one entry, so v_dot2_f32_f16 against (z_hi, z_hi) and
//    (z_lo, z_lo) (z split after a power-of-two scale) accumulates (hi + lo) z in
//    fp32; summed over the 16 lanes of a row group.
// NB = 2 (n <= 32), 4 (n <= 64), 6 (n <= 96): a wave-uniform branch of one kernel.
// 32 < k <= 64 (KP = 64 split words per row): n <= 32 only (NB = 2 against the primal
// NB = 4: a quarter of the k x k Gram tiles, half the block sweeps; for 32 < n <= 64
// the dual system is as large as the primal one).
constexpr int kDualMaxRatings = 96;
constexpr int kDualMaxRatings64 = 32;

// The 8 split words of dims 32s + 8q .. +7 of each operand block's rating.
template <int NB, int KP>
__device__ __forceinline__ void dual_gather_step(uint32_t (&w)[NB][8], const int (&cc)[NB], int s,
                                                 const uint32_t* __restrict__ Ysp) {
  const int q = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const uint32_t* p = Ysp + (uint64_t)(uint32_t)cc[c] * (uint32_t)KP + 32 * s + 8 * q;
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    const uint4 b = *reinterpret_cast<const uint4*>(p + 4);
    w[c][0] = a.x; w[c][1] = a.y; w[c][2] = a.z; w[c][3] = a.w;
    w[c][4] = b.x; w[c][5] = b.y; w[c][6] = b.z; w[c][7] = b.w;
  }
}

template <int NB, int KP>
__device__ __forceinline__ void dual_row(int row, int n, const int (&cj)[2],
                                         const float (&rj)[2], const uint32_t* __restrict__ Ysp,
                                         int ey, float reg, float* __restrict__ xrow, int ld,
                                         float* __restrict__ lds, int32_t* __restrict__ status,
                                         RescueList rl) {
  constexpr int NT = NB * (NB + 1) / 2;
  constexpr int NS = KP / 32;  // k-steps of 32 dims
  typedef FullTiles<NB> TS;
  const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
  // operand block c of lane (q, m) is rating j = m * NB + c (held by lane j % 64 in
  // register j / 64 of the staging pair)
  int cc[NB];
  float rc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const int j = m * NB + c;
    const int c0 = __shfl(cj[0], j & 63);
    const float r0 = __shfl(rj[0], j & 63);
    if constexpr (NB * 16 > 64) {
      const int c1 = __shfl(cj[1], j & 63);
      const float r1 = __shfl(rj[1], j & 63);
      cc[c] = j < 64 ? c0 : c1;
      rc[c] = j < 64 ? r0 : r1;
    } else {
      cc[c] = c0;
      rc[c] = r0;
    }
  }
  floatx4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  // NB <= 4: step s+1's gathers in flight during step s; NB = 6: one step of
  // registers (the two waves per SIMD overlap each other's gathers instead)
  constexpr int NBUF = NB <= 4 ? 2 : 1;
  uint32_t w[NBUF][NB][8];
  dual_gather_step<NB, KP>(w[0], cc, 0, Ysp);
  static_for<NS>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int cur = s % NBUF;
    if constexpr (NBUF == 2 && s + 1 < NS)
      dual_gather_step<NB, KP>(w[(s + 1) % NBUF], cc, s + 1, Ysp);
    if constexpr (NBUF == 1 && s > 0) dual_gather_step<NB, KP>(w[0], cc, s, Ysp);
    uint32_t hi[NB][4], lo[NB][4];
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        hi[c][p] = __builtin_amdgcn_perm(w[cur][c][2 * p + 1], w[cur][c][2 * p], 0x05040100u);
        lo[c][p] = __builtin_amdgcn_perm(w[cur][c][2 * p + 1], w[cur][c][2 * p], 0x07060302u);
      }
    static_for<NT>([&](auto ti) {
      constexpr int t = decltype(ti)::value;
      constexpr int a = TS::l1(t), b = TS::l2(t);
      const half8v ha = as_h8(hi[a]), hb = as_h8(hi[b]);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, as_h8(lo[b]), acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_h8(lo[a]), hb, acc[t], 0, 0, 0);
    });
  });
  // split window guard: G_jj = |t_j|^2 <= KP max_d t_jd^2 (ratings are not split here)
  if (window_miss(diag_max_lane<NB>(acc), (float)KP, 0.f)) {
    rescue_append(rl, row);
    return;
  }
  // (2^2ey G + 2^2ey lambda n I) z = 2^2ey r; ratings j >= n: identity rows, rhs 0
  const float inv = ldexpf(1.f, 2 * ey);
  const float lam = (float)((double)reg * (double)n) * inv;
  static_for<NT>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    constexpr int c1 = TS::l1(t), c2 = TS::l2(t);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i, j;
      tile_ij<NB>(c1, c2, r, i, j);
      const bool pad = (i >= n) | (j >= n);
      float v = pad ? 0.f : acc[t][r];
      if constexpr (c1 == c2) v = (i == j) ? (pad ? 1.f : v + lam) : v;
      acc[t][r] = v;
    }
  });
  float bcol[NB], z[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) bcol[c] = rc[c] * inv;
  const bool ok = w1_solve_x<NB, false>(acc, bcol, lds, n, z);
  if (!ok) {  // re-solved in fp64 (the primal k x k system)
    rescue_append(rl, row);
    return;
  }
  // x = Y_S^T z: z split into f16 hi + lo after a power-of-two scale
  float zm = 0.f;
#pragma unroll
  for (int c = 0; c < NB; ++c) zm = fmaxf(zm, __builtin_fabsf(z[c]));
  const int ez = split_exponent(wave_max(zm));
  const float sz = ldexpf(1.f, ez);
  half2v zh2[NB], zl2[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const float t = z[c] * sz;
    const _Float16 h = (_Float16)t;
    const _Float16 l = (_Float16)(t - (float)h);
    zh2[c] = half2v{h, h};
    zl2[c] = half2v{l, l};
  }
  float px[NS][8];
  dual_gather_step<NB, KP>(w[0], cc, 0, Ysp);
  static_for<NS>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr int cur = s % NBUF;
    if constexpr (NBUF == 2 && s + 1 < NS)
      dual_gather_step<NB, KP>(w[(s + 1) % NBUF], cc, s + 1, Ysp);
    if constexpr (NBUF == 1 && s > 0) dual_gather_step<NB, KP>(w[0], cc, s, Ysp);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        const half2v hl = __builtin_bit_cast(half2v, w[cur][c][t]);
        a = __builtin_amdgcn_fdot2(hl, zh2[c], a, false);
        a = __builtin_amdgcn_fdot2(hl, zl2[c], a, false);
      }
      px[s][t] = reduce_lanes16(a);
    }
  });
  // lane (q, 0) holds dims 32s + 8q .. +7; (2^ey y)(2^ez z) -> x
  const float un = ldexpf(1.f, -ey - ez);
  if (m == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int d = 32 * s + 8 * q + 4 * h;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = ok ? px[s][4 * h + e] * un : 0.f;
        if (d < ld) *reinterpret_cast<float4*>(xrow + d) = make_float4(o[0], o[1], o[2], o[3]);
      }
  }
  // ld past k_pad (any ld >= k is allowed): columns [KP, ld) are written as zero too
  for (int d = KP + lane; d < ld; d += 64) xrow[d] = 0.f;
}

// One wavefront per short light row (the tail of the longest-first light list: every
// row with <= kDualMaxRatings ratings at k in (64, 128], KP = 128; <= kDualMaxRatings64
// at k in (32, 64], KP = 64), explicit, regParam > 0.  (Three waves per SIMD: 27
// spilled registers, configs[3] dual launch 64.8 -> 67.8 ms, profiles/r05/ab_occupancy.jsonl.)
template <int KP>
__global__ __launch_bounds__(64, 2) void gram_solve_dual_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, const int32_t* __restrict__ rows, float* __restrict__ X, int ld,
    float reg, int32_t* __restrict__ status, const float* __restrict__ scal,
    const uint32_t* __restrict__ Ysp, int32_t zero_row, RescueList rl) {
  static_assert(KP == 64 || KP == 128, "dual: k_pad 64 or 128");
  constexpr int NMAX = KP == 128 ? kDualMaxRatings : kDualMaxRatings64;
  __shared__ __attribute__((aligned(16))) float lds[W1LdsT<KP == 128 ? 6 : 2>::SIZE];
  const int lane = threadIdx.x & 63;
  const int row = rows[blockIdx.x];
  const int64_t pb = row_ptr[row];
  const int n = (int)(row_ptr[row + 1] - pb);
  const int ey = split_exponent(scal[0]);
  float* xrow = X + (int64_t)row * ld;
  if (n > NMAX) {  // schedule contract broken: report the row, leave it zero
    if (lane == 0) atomicCAS(status, 0, row + 1);
    return;
  }
  // ratings j = lane and j = lane + 64 (missing ones point at the zero row)
  int cj[2];
  float rj[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int j = lane + 64 * h;
    cj[h] = j < n ? col[pb + j] : zero_row;
    rj[h] = j < n ? val[pb + j] : 0.f;
  }
  if constexpr (KP == 64) {
    dual_row<2, 64>(row, n, cj, rj, Ysp, ey, reg, xrow, ld, lds, status, rl);
  } else {
    if (n <= 32)
      dual_row<2, 128>(row, n, cj, rj, Ysp, ey, reg, xrow, ld, lds, status, rl);
    else if (n <= 64)
      dual_row<4, 128>(row, n, cj, rj, Ysp, ey, reg, xrow, ld, lds, status, rl);
    else
      dual_row<6, 128>(row, n, cj, rj, Ysp, ey, reg, xrow, ld, lds, status, rl);
  }
}

}  // namespace als
