// The three Gram accumulators of one wavefront and their tile-set policies: fp32 VALU/MFMA
// (gram_accumulate: the YtY kernels), split in registers (gram_accumulate_split: the implicit
// solve kernels), pre-split table (gram_accumulate_pre / _pre2, rhs_from_tiles: the explicit
// solve kernels), and split_table_kernel, which writes that table.
#pragma once

#include "solve_config.h"

namespace als {

// Tile-set policy: which 16x16 Gram tiles a wavefront accumulates.
//   N tiles; tile t is block (g1(t), g2(t)), g1 <= g2, in dims-block units
//   (block c holds dims d = 16-index * CN + c).
//   NC dims-blocks are gathered per rating ("local columns"; gcol(lc) = block),
//   l1(t), l2(t) are tile t's local columns; NR rhs blocks = local columns 0..NR-1
//   (NRA = max(NR, 1), the register array size).
//   load(p, y, d0, k): this lane's NC values of one factor row (p = row + d0),
//   zero for dims >= k (never reads past the row: ld % 4 == 0, k <= ld).
// FullTiles<CN>: all CN(CN+1)/2 upper tiles (one wavefront per system, k <= 64).
template <int CN>
struct FullTiles {
  static constexpr int N = CN * (CN + 1) / 2, NC = CN, NR = CN, NRA = CN;
  __host__ __device__ static constexpr int l1(int t) {
    int a = 0;
    while (t >= CN - a) { t -= CN - a; ++a; }
    return a;
  }
  __host__ __device__ static constexpr int l2(int t) {
    int a = 0;
    while (t >= CN - a) { t -= CN - a; ++a; }
    return a + t;
  }
  __host__ __device__ static constexpr int gcol(int c) { return c; }
  __host__ __device__ static constexpr int g1(int t) { return l1(t); }
  __host__ __device__ static constexpr int g2(int t) { return l2(t); }
  __device__ static __forceinline__ void load(const float* __restrict__ p, float (&y)[NC], int d0,
                                              int k) {
    if (d0 < k) {
      load_dims<CN>(p, y);
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c) y[c] = 0.f;
    }
  }
  // Unconditional load of this lane's dims from row `row` (offsets clamped into
  // [0, ld): lanes whose dims are >= k read real dims, masked out after the Gram).
  __device__ static __forceinline__ void load_clamped(const float* __restrict__ row,
                                                      float (&y)[NC], int d0, int ld) {
    if constexpr (CN == 8) {
      auto cl = [&](int o) { return o + 4 <= ld ? o : ld - 4; };
      const float4 a = *reinterpret_cast<const float4*>(row + cl(d0));
      const float4 b = *reinterpret_cast<const float4*>(row + cl(d0 + 4));
      y[0] = a.x; y[1] = a.y; y[2] = a.z; y[3] = a.w;
      y[4] = b.x; y[5] = b.y; y[6] = b.z; y[7] = b.w;
    } else {
      load_dims<CN>(row + (d0 + CN <= ld ? d0 : ld - CN), y);
    }
  }
  // This lane's NC words of a pre-split row (p = row + m*CN; rows are kp = 16*CN wide).
  __device__ static __forceinline__ void load_pre(const uint32_t* __restrict__ p,
                                                  uint32_t (&w)[NC]) {
    if constexpr (CN == 1) {
      w[0] = p[0];
    } else if constexpr (CN == 2) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      w[0] = v.x; w[1] = v.y;
    } else if constexpr (CN == 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
      static_assert(CN == 8, "pre-split rows: CN in {1, 2, 4, 8}");
      const uint4 a = *reinterpret_cast<const uint4*>(p);
      const uint4 b = *reinterpret_cast<const uint4*>(p + 4);
      w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
      w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    }
  }
};

// WgTiles<R>: wavefront R of the 4-wave workgroup that owns one k <= 128 system
// (CN = 8, blocks H0 = 0..3, H1 = 4..7).  R0: upper(H0) 10 tiles + rhs H0;
// R1: upper(H1) 10 tiles + rhs H1; R2: {0,1} x H1, 8 tiles; R3: {2,3} x H1.
// Each wave gathers only the dims its tiles need (16 or 24 B per lane).
template <int R>
struct WgTiles {
  static_assert(R >= 0 && R < 4, "4 waves");
  static constexpr int N = R < 2 ? 10 : 8, NC = R < 2 ? 4 : 6, NR = R < 2 ? 4 : 0,
                       NRA = R < 2 ? 4 : 1;
  __host__ __device__ static constexpr int gcol(int c) {
    return R == 0 ? c : (R == 1 ? 4 + c : (c < 2 ? 2 * (R - 2) + c : c + 2));
  }
  __host__ __device__ static constexpr int l1(int t) { return R < 2 ? FullTiles<4>::l1(t) : t / 4; }
  __host__ __device__ static constexpr int l2(int t) {
    return R < 2 ? FullTiles<4>::l2(t) : 2 + t % 4;
  }
  __host__ __device__ static constexpr int g1(int t) { return gcol(l1(t)); }
  __host__ __device__ static constexpr int g2(int t) { return gcol(l2(t)); }
  __device__ static __forceinline__ void load(const float* __restrict__ p, float (&y)[NC], int d0,
                                              int k) {
#pragma unroll
    for (int c = 0; c < NC; ++c) y[c] = 0.f;
    if constexpr (R < 2) {
      if (d0 + 4 * R < k) {
        const float4 v = *reinterpret_cast<const float4*>(p + 4 * R);
        y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
      }
    } else {
      constexpr int o = 2 * (R - 2);
      if (d0 + o < k) {
        const float2 v = *reinterpret_cast<const float2*>(p + o);
        y[0] = v.x; y[1] = v.y;
      }
      if (d0 + 4 < k) {
        const float4 v = *reinterpret_cast<const float4*>(p + 4);
        y[2] = v.x; y[3] = v.y; y[4] = v.z; y[5] = v.w;
      }
    }
  }
  __device__ static __forceinline__ void load_clamped(const float* __restrict__ row,
                                                      float (&y)[NC], int d0, int ld) {
    auto cl = [&](int o, int w) { return o + w <= ld ? o : ld - w; };
    if constexpr (R < 2) {
      const float4 v = *reinterpret_cast<const float4*>(row + cl(d0 + 4 * R, 4));
      y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
    } else {
      const float2 u = *reinterpret_cast<const float2*>(row + cl(d0 + 2 * (R - 2), 2));
      const float4 v = *reinterpret_cast<const float4*>(row + cl(d0 + 4, 4));
      y[0] = u.x; y[1] = u.y;
      y[2] = v.x; y[3] = v.y; y[4] = v.z; y[5] = v.w;
    }
  }
  __device__ static __forceinline__ void load_pre(const uint32_t* __restrict__ p,
                                                  uint32_t (&w)[NC]) {
    if constexpr (R < 2) {
      const uint4 v = *reinterpret_cast<const uint4*>(p + 4 * R);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
      const uint2 u = *reinterpret_cast<const uint2*>(p + 2 * (R - 2));
      const uint4 v = *reinterpret_cast<const uint4*>(p + 4);
      w[0] = u.x; w[1] = u.y;
      w[2] = v.x; w[3] = v.y; w[4] = v.z; w[5] = v.w;
    }
  }
};

// Gather the factor rows of one half-block (32 ratings = 8 MFMA steps) into
// registers: step t, lane (q, m) gets its TS dims among m*CN .. m*CN+CN-1 of
// rating 4t+q.
template <int CN, class TS>
__device__ __forceinline__ void gather_half(float (&y)[8][TS::NC], int ci, int base, int nrem,
                                            const float* __restrict__ Y, int ld, int d0, int k) {
  const int q = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int src = base + 4 * t + q;
    const int s = __shfl(ci, src);
    if (src < nrem) {
      TS::load(Y + (int64_t)s * ld + d0, y[t], d0, k);
    } else {
#pragma unroll
      for (int c = 0; c < TS::NC; ++c) y[t][c] = 0.f;
    }
  }
}

// MFMA over one gathered half-block: acc[tile] += (w_a y)(y)^T over the tiles of
// TS, and bf += w_b y over its rhs blocks.
template <class TS, bool IMPLICIT>
__device__ __forceinline__ void mfma_half(const float (&y)[8][TS::NC], float rv, int base,
                                          int nrem, float alpha, floatx4 (&acc)[TS::N],
                                          float (&bf)[TS::NRA]) {
  const int q = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    if (base + 16 * g < nrem) {  // wave-uniform: skip empty 16-rating groups
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = 4 * g + j;
        const float r = __shfl(rv, base + 4 * t + q);
        float ya[TS::NC];
        float wb;
        if constexpr (IMPLICIT) {
          const float c1 = alpha * fabsf(r);
          wb = r > 0.f ? 1.f + c1 : 0.f;
#pragma unroll
          for (int c = 0; c < TS::NC; ++c) ya[c] = c1 * y[t][c];
        } else {
          wb = r;
#pragma unroll
          for (int c = 0; c < TS::NC; ++c) ya[c] = y[t][c];
        }
        static_for<TS::N>([&](auto ti) {
          constexpr int tt = decltype(ti)::value;
          constexpr int a = TS::l1(tt), b = TS::l2(tt);
          acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ya[a], y[t][b], acc[tt], 0, 0, 0);
        });
#pragma unroll
        for (int c = 0; c < TS::NR; ++c) bf[c] = fmaf(wb, y[t][c], bf[c]);
      }
    }
  }
}

// Accumulate the (weighted) Gram and rhs of ratings [pb, pe) of one row.
// tot[t][r]: this lane's 4 accumulator rows of upper tile t (MFMA C layout),
// summed over 64-rating blocks in AccT (each block's own sum is an exact-product
// fp32 MFMA chain of <= 16 steps); btot[c]: partial rhs for dim m*CN+c over this
// lane's rating slot q (summed over q by the caller); npos: #ratings > 0.
// Software pipeline: the row gathers of half-block h+1 are in flight while the
// MFMAs of half-block h run; rating indices are loaded one 64-block ahead.
template <int CN, bool IMPLICIT, bool IDENT, class AccT, class TS = FullTiles<CN>>
__device__ __forceinline__ void gram_accumulate(const int32_t* __restrict__ col,
                                                const float* __restrict__ val, int64_t pb,
                                                int64_t pe, const float* __restrict__ Y, int ld,
                                                int k, float alpha, AccT (&tot)[TS::N][4],
                                                AccT (&btot)[TS::NRA], int& npos) {
  constexpr int NT = TS::N;
  const int lane = threadIdx.x & 63, m = lane & 15;
  const int d0 = m * CN;  // dims in [k, ld) are zero by contract (see als_hip.h)
  if (pe <= pb) return;
  auto load_idx = [&](int64_t base, int& ci, float& rv) {
    ci = 0;
    rv = 0.f;
    if (base + lane < pe) {
      ci = IDENT ? (int)(base + lane) : col[base + lane];
      rv = IDENT ? 1.f : val[base + lane];
    }
  };
  int ci_c, ci_n;
  float rv_c, rv_n;
  load_idx(pb, ci_c, rv_c);
  load_idx(pb + 64, ci_n, rv_n);
  float yA[8][TS::NC], yB[8][TS::NC];
  int nrem = (int)((pe - pb) < 64 ? (pe - pb) : 64);
  gather_half<CN, TS>(yA, ci_c, 0, nrem, Y, ld, d0, k);
  for (int64_t base = pb; base < pe; base += 64) {
    const int64_t nbase = base + 64;
    const int nrem_n = nbase < pe ? (int)((pe - nbase) < 64 ? (pe - nbase) : 64) : 0;
    if (32 < nrem) gather_half<CN, TS>(yB, ci_c, 32, nrem, Y, ld, d0, k);
    floatx4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    float bf[TS::NRA];
#pragma unroll
    for (int c = 0; c < TS::NRA; ++c) bf[c] = 0.f;
    mfma_half<TS, IMPLICIT>(yA, rv_c, 0, nrem, alpha, acc, bf);
    if (nrem_n > 0) gather_half<CN, TS>(yA, ci_n, 0, nrem_n, Y, ld, d0, k);
    if (32 < nrem) mfma_half<TS, IMPLICIT>(yB, rv_c, 32, nrem, alpha, acc, bf);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) tot[t][r] += (AccT)acc[t][r];
    }
#pragma unroll
    for (int c = 0; c < TS::NR; ++c) btot[c] += (AccT)bf[c];
    if constexpr (IMPLICIT) npos += __popcll(__ballot(lane < nrem && rv_c > 0.f));
    ci_c = ci_n;
    rv_c = rv_n;
    nrem = nrem_n;
    if (nrem_n > 0) load_idx(nbase + 64, ci_n, rv_n);
  }
}

// ---------------------------------------------------------------------------
// Row Grams on the f16 matrix cores with fp32-grade products ("split" Gram).
//
// v_mfma_f32_16x16x4_f32 runs at the fp32 VECTOR rate on gfx950 and occupies
// the VALU issue port, so an fp32-MFMA Gram leaves nothing for the solves of
// the other waves.  Here every gathered value t = w*y (w = per-launch power-of-
// two scale, times sqrt(alpha |r|) for implicit) is split into
//   t = hi + lo,  hi = f16_rn(t),  lo = f16_rn(t - hi)   (~22 significant bits)
// and the Gram tile is  sum hi_a hi_b + hi_a lo_b + lo_a hi_b  — three
// v_mfma_f32_16x16x32_f16 per tile per 32 ratings (16x the fp32-MFMA rate,
// so 5.3x fewer matrix cycles), exact f16 products accumulated in fp32.  The
// dropped lo*lo term and the two roundings are ~2^-21 relative per product:
// the Gram matches an fp32 one to within its own accumulation error.
// The scale keeps |t| in [2^14, 2^15) for the largest entry, so hi never
// overflows and lo stays normal for entries within ~2^17 of the largest.
// MFMA K dimension = rating index: lane (q, m) holds ratings 8q..8q+7 of a
// 32-rating step and dims m*CN .. m*CN+CN-1, exactly the dim permutation of
// the fp32 path, so the C layout (and the solve that consumes it) is unchanged.
// rhs b = sum coef * y stays an fp32 VALU FMA on the unscaled values.
// ---------------------------------------------------------------------------

// The split of two weighted values w0 y0, w1 y1 straight from the fp32 operands:
// hi = f16(w y) and lo = f16(w y - hi), each one v_fma_mix (the product and the
// residual formed inside one fp32 fma; lo also keeps the product's own fp32 rounding
// error), 4 VALU per pair instead of a multiply, a packed convert, two converts back,
// a subtract and a packed convert (round 5): configs[2] 9.11 -> 9.06 ms/iter,
// profiles/r06/ab_fma_mix_split.jsonl.
__device__ __forceinline__ void split_pair_w(float y0, float w0, float y1, float w1, uint32_t& hi,
                                             uint32_t& lo) {
  uint32_t h, l;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "=v"(h) : "v"(y0), "v"(w0));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "+v"(h) : "v"(y1), "v"(w1));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]"
      : "=v"(l) : "v"(y0), "v"(w0), "v"(h));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "+v"(l) : "v"(y1), "v"(w1), "v"(h));
  hi = h;
  lo = l;
}

__device__ __forceinline__ half8v as_h8(const uint32_t (&v)[4]) {
  return __builtin_bit_cast(half8v, make_uint4(v[0], v[1], v[2], v[3]));
}

// Power-of-two scale for the split: the largest |w y| lands in [2^14, 2^15).
__device__ __forceinline__ int split_exponent(float m) {
  if (!(m > 0.f) || !(m < 3.0e38f)) return 0;
  int e = 14 - ilogbf(m);
  return e < -60 ? -60 : (e > 60 ? 60 : e);
}

// Per-step register set of the split Gram: 8 ratings x NC dims of this lane
// (unscaled).  The per-rating weights stay in the LDS staging block until the
// step is consumed: w = Gram weight (implicit: sc sqrt(alpha |r|)), b = rhs
// weight (implicit: (1 + alpha |r|) [r > 0]), both 0 for missing ratings.
template <int NC>
struct SplitStep {
  float y[8][NC];
};

// Split Gram staging: columns, Gram weights and rhs weights of one 64-rating
// block (computed once per rating here instead of once per lane of its group).
template <bool IMPLICIT>
__device__ __forceinline__ void stage_weights(int* __restrict__ st_c, float* __restrict__ st_w,
                                              float* __restrict__ st_b, int ci, float rv, float sc,
                                              float alpha) {
  const int lane = threadIdx.x & 63;
  const bool v = ci >= 0;
  float w, b;
  if constexpr (IMPLICIT) {
    const float c1 = alpha * fabsf(rv);
    w = v ? sc * __builtin_sqrtf(c1) : 0.f;
    b = (v && rv > 0.f) ? 1.f + c1 : 0.f;
  } else {
    w = v ? sc : 0.f;
    b = v ? rv : 0.f;
  }
  st_c[lane] = ci;
  st_w[lane] = w;
  st_b[lane] = b;
}

// Issue the gathers of one 32-rating step (half h of the staged block).
template <int CN, class TS>
__device__ __forceinline__ void split_issue(SplitStep<TS::NC>& s, const int* __restrict__ st_c,
                                            int h, const float* __restrict__ Y, int ld, int d0,
                                            int k) {
  const int q = (threadIdx.x & 63) >> 4;
  const int o = 32 * h + 8 * q;
  const int4 c0 = *reinterpret_cast<const int4*>(st_c + o);
  const int4 c1 = *reinterpret_cast<const int4*>(st_c + o + 4);
  const int ids[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
  for (int j = 0; j < 8; ++j)
    TS::load_clamped(Y + (int64_t)(ids[j] >= 0 ? ids[j] : 0) * ld, s.y[j], d0, ld);
}

// Consume one step, part 1 (VALU): rhs FMAs and the hi/lo split of w*y.
template <class TS, bool IMPLICIT>
__device__ __forceinline__ void split_prepare(const SplitStep<TS::NC>& s,
                                              const float* __restrict__ st_w,
                                              const float* __restrict__ st_b, int h,
                                              uint32_t (&hi)[TS::NC][4], uint32_t (&lo)[TS::NC][4],
                                              float (&bf)[TS::NRA]) {
  const int o = 32 * h + 8 * ((threadIdx.x & 63) >> 4);
  const float4 w0 = *reinterpret_cast<const float4*>(st_w + o);
  const float4 w1 = *reinterpret_cast<const float4*>(st_w + o + 4);
  const float4 b0 = *reinterpret_cast<const float4*>(st_b + o);
  const float4 b1 = *reinterpret_cast<const float4*>(st_b + o + 4);
  const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
  for (int c = 0; c < TS::NR; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) bf[c] = fmaf(b[j], s.y[j][c], bf[c]);
#pragma unroll
  for (int c = 0; c < TS::NC; ++c)
#pragma unroll
    for (int p = 0; p < 4; ++p)
      split_pair_w(s.y[2 * p][c], w[2 * p], s.y[2 * p + 1][c], w[2 * p + 1], hi[c][p], lo[c][p]);
}

// Part 2 (matrix cores): 3 f16 MFMAs per tile.
template <class TS>
__device__ __forceinline__ void split_mfma(const uint32_t (&hi)[TS::NC][4],
                                           const uint32_t (&lo)[TS::NC][4],
                                           floatx4 (&acc)[TS::N]) {
  static_for<TS::N>([&](auto ti) {
    constexpr int tt = decltype(ti)::value;
    constexpr int a = TS::l1(tt), b = TS::l2(tt);
    const half8v ha = as_h8(hi[a]), hb = as_h8(hi[b]);
    acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, acc[tt], 0, 0, 0);
    acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, as_h8(lo[b]), acc[tt], 0, 0, 0);
    acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_h8(lo[a]), hb, acc[tt], 0, 0, 0);
  });
}

// Gram + rhs of ratings [pb, pe) of one row with the split f16 MFMA.
// acc: scaled Gram tiles (x sc^2), bf: per-lane partial rhs (unscaled, summed
// over the 4 rating slots q by the caller), npos: #ratings > 0 (implicit).
// Pipeline: the gathers of step s+1 are in flight while step s is consumed;
// the (column, rating) pairs of the next 64-block are prefetched into registers
// and staged in LDS (`st`, 128 words, wave-private) when that block starts.
template <int CN, bool IMPLICIT, class TS = FullTiles<CN>>
__device__ __forceinline__ void gram_accumulate_split(
    const int32_t* __restrict__ col, const float* __restrict__ val, int64_t pb, int64_t pe,
    const float* __restrict__ Y, int ld, int k, float alpha, float sc,
    floatx4 (&acc)[TS::N], float (&bf)[TS::NRA], int& npos, int* __restrict__ st) {
  const int lane = threadIdx.x & 63, m = lane & 15;
  const int d0 = m * CN;
  int* st_c = st;  // 192 words: columns, Gram weights, rhs weights
  float* st_w = reinterpret_cast<float*>(st + 64);
  float* st_b = reinterpret_cast<float*>(st + 128);
  if (pe <= pb) return;
  auto load_idx = [&](int64_t base, int& ci, float& rv) {
    ci = -1;
    rv = 0.f;
    if (base + lane < pe) {
      ci = col[base + lane];
      rv = val[base + lane];
    }
  };
  const int64_t n = pe - pb;
  const int nsteps = (int)((n + 31) >> 5);
  int ci_n, ci_c;
  float rv_n, rv_c;
  load_idx(pb, ci_c, rv_c);
  load_idx(pb + 64, ci_n, rv_n);
  stage_weights<IMPLICIT>(st_c, st_w, st_b, ci_c, rv_c, sc, alpha);
  if constexpr (IMPLICIT) npos += __popcll(__ballot(ci_c >= 0 && rv_c > 0.f));
  wave_lds_sync();
  // One register set for the gathered rows: step s is split into its f16
  // operands, then the gathers of step s+1 are issued into the same registers,
  // then step s's MFMAs run while those loads are in flight.
  SplitStep<TS::NC> sA;
  split_issue<CN, TS>(sA, st_c, 0, Y, ld, d0, k);
  // rhs: fp32 partials per lane over 64-rating blocks, summed into bf
  float bp[TS::NRA];
#pragma unroll
  for (int c = 0; c < TS::NRA; ++c) bp[c] = 0.f;
  for (int s = 0; s < nsteps; ++s) {
    uint32_t hi[TS::NC][4], lo[TS::NC][4];
    split_prepare<TS, IMPLICIT>(sA, st_w, st_b, s & 1, hi, lo, bp);
    const int s1 = s + 1;
    if (s1 < nsteps) {
      // step s1 uses block s1>>1, half s1&1; a new block is staged from the
      // pairs prefetched one block earlier
      if ((s1 & 1) == 0) {
        stage_weights<IMPLICIT>(st_c, st_w, st_b, ci_n, rv_n, sc, alpha);
        if constexpr (IMPLICIT) npos += __popcll(__ballot(ci_n >= 0 && rv_n > 0.f));
        wave_lds_sync();
        load_idx(pb + 64 * (int64_t)((s1 >> 1) + 1), ci_n, rv_n);
      }
      split_issue<CN, TS>(sA, st_c, s1 & 1, Y, ld, d0, k);
    }
    split_mfma<TS>(hi, lo, acc);
    if (s & 1) {
#pragma unroll
      for (int c = 0; c < TS::NRA; ++c) {
        bf[c] += bp[c];
        bp[c] = 0.f;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < TS::NRA; ++c) bf[c] += bp[c];
}

// ---------------------------------------------------------------------------
// Explicit feedback: the Gram is unweighted, so every factor row is split once
// per half-sweep into a table (split_table_kernel): Ysp[row][d] = f16 hi |
// f16 lo << 16 of 2^ey * Y[row][d] (padding dims and the extra row n_src zero).
// The Gram loop then gathers 4 B per dim (as for fp32) and forms its f16
// operands with v_perm_b32 alone.  Ratings are split the same way (2^er * r)
// when a 64-rating block is staged, and the rhs b = sum r y runs on the matrix
// cores too: B operand column 0 = hi(r), column 1 = lo(r), all other columns 0,
// so C[i][0] + C[i][1] = sum (hi_y + lo_y)(hi_r + lo_r).  Ratings past the end
// of the row point at the zero row and add nothing.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t split_word(float t) {
  const _Float16 h = (_Float16)t;  // round to nearest
  const _Float16 l = (_Float16)(t - (float)h);
  return (uint32_t)__builtin_bit_cast(unsigned short, h) |
         ((uint32_t)__builtin_bit_cast(unsigned short, l) << 16);
}

template <int NC>
struct PreStep {
  uint32_t w[8][NC];  // split words: rating j of this lane's slot, its NC dims
  uint32_t r[8];      // split words of those ratings
};

template <class TS>
__device__ __forceinline__ void pre_issue(PreStep<TS::NC>& s, const int* __restrict__ st_c,
                                          const uint32_t* __restrict__ st_r, int h,
                                          const uint32_t* __restrict__ base, uint32_t kp) {
  const int q = (threadIdx.x & 63) >> 4;
  const int o = 32 * h + 8 * q;
  const int4 c0 = *reinterpret_cast<const int4*>(st_c + o);
  const int4 c1 = *reinterpret_cast<const int4*>(st_c + o + 4);
  const uint4 r0 = *reinterpret_cast<const uint4*>(st_r + o);
  const uint4 r1 = *reinterpret_cast<const uint4*>(st_r + o + 4);
  const int ids[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  s.r[0] = r0.x; s.r[1] = r0.y; s.r[2] = r0.z; s.r[3] = r0.w;
  s.r[4] = r1.x; s.r[5] = r1.y; s.r[6] = r1.z; s.r[7] = r1.w;
#pragma unroll
  for (int j = 0; j < 8; ++j) TS::load_pre(base + (uint64_t)(uint32_t)ids[j] * kp, s.w[j]);
}

// How the pre path keeps its rhs sums.  ONE = false: one tile per dims-block c, the
// rating words as the MFMA's column operand (column 0 = hi(r), column 1 = lo(r)):
// C_c[i][0] + C_c[i][1] = b[i * CN + c].  ONE = true: one tile for all dims-blocks,
// the rating words as the row operand in rows 2c (hi(r)) and 2c + 1 (lo(r)) of
// dims-block c's two MFMAs and exact zeros in the other rows: C[2c][i] + C[2c+1][i]
// = b[i * CN + c].  Every entry receives the same products in the same order as
// with ONE = false (plus exact zeros), so the sums are bit-identical; NR - 1 fewer
// accumulator tiles stay live through the Gram loop.
template <class TS, bool ONE>
struct RhsTiles {
  static_assert(!ONE || (TS::NR >= 1 && 2 * TS::NR <= 16), "rows 2c, 2c + 1 of one tile");
  static constexpr int N = ONE ? 1 : TS::NRA;
};

// f16 operands of one step: ratings (2p, 2p+1) share a dword, hi halves and lo
// halves; rhs operand by lane index m: hi(r) on m = 0, lo(r) on m = 1, else 0
// (rsel of the caller; one rhs tile: hi(r) on even m, lo(r) on odd m < 2 NR).
template <class TS>
__device__ __forceinline__ void pre_operands(const PreStep<TS::NC>& s, uint32_t rsel,
                                             uint32_t (&hi)[TS::NC][4], uint32_t (&lo)[TS::NC][4],
                                             uint32_t (&rb)[4]) {
#pragma unroll
  for (int c = 0; c < TS::NC; ++c)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      hi[c][p] = __builtin_amdgcn_perm(s.w[2 * p + 1][c], s.w[2 * p][c], 0x05040100u);
      lo[c][p] = __builtin_amdgcn_perm(s.w[2 * p + 1][c], s.w[2 * p][c], 0x07060302u);
    }
#pragma unroll
  for (int p = 0; p < 4; ++p) rb[p] = __builtin_amdgcn_perm(s.r[2 * p + 1], s.r[2 * p], rsel);
}

// Keep the operands where they are formed: otherwise the scheduler sinks the
// v_perm next to their MFMAs, past the next step's loads into the same
// registers, and the loop then carries copies of the step (waiting for its
// loads early).
template <class TS>
__device__ __forceinline__ void pin_operands(uint32_t (&hi)[TS::NC][4], uint32_t (&lo)[TS::NC][4],
                                             uint32_t (&rb)[4]) {
#pragma unroll
  for (int c = 0; c < TS::NC; ++c)
#pragma unroll
    for (int p = 0; p < 4; ++p) asm volatile("" : "+v"(hi[c][p]), "+v"(lo[c][p]));
  if constexpr (TS::NR > 0) {
#pragma unroll
    for (int p = 0; p < 4; ++p) asm volatile("" : "+v"(rb[p]));
  }
  asm volatile("" ::: "memory");
}

template <class TS, bool ONE = false>
__device__ __forceinline__ void pre_mfma(const uint32_t (&hi)[TS::NC][4],
                                         const uint32_t (&lo)[TS::NC][4], const uint32_t (&rb)[4],
                                         floatx4 (&acc)[TS::N],
                                         floatx4 (&accb)[RhsTiles<TS, ONE>::N]) {
  split_mfma<TS>(hi, lo, acc);
  if constexpr (ONE) {
    const int m = threadIdx.x & 15;
#pragma unroll
    for (int c = 0; c < TS::NR; ++c) {
      uint32_t rc[4];  // the rating words in rows 2c, 2c + 1 only
#pragma unroll
      for (int p = 0; p < 4; ++p) rc[p] = (m >> 1) == c ? rb[p] : 0u;
      const half8v a = as_h8(rc);
      accb[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, as_h8(hi[c]), accb[0], 0, 0, 0);
      accb[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, as_h8(lo[c]), accb[0], 0, 0, 0);
    }
  } else {
    const half8v b = as_h8(rb);
#pragma unroll
    for (int c = 0; c < TS::NR; ++c) {
      accb[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_h8(hi[c]), b, accb[c], 0, 0, 0);
      accb[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_h8(lo[c]), b, accb[c], 0, 0, 0);
    }
  }
}

// Byte selector of this lane's rhs operand words (pre_operands).
template <class TS, bool ONE>
__device__ __forceinline__ uint32_t pre_rsel() {
  const int m = threadIdx.x & 15;
  if constexpr (ONE)
    return m >= 2 * TS::NR ? 0x0C0C0C0Cu : ((m & 1) ? 0x07060302u : 0x05040100u);
  else
    return m == 0 ? 0x05040100u : (m == 1 ? 0x07060302u : 0x0C0C0C0Cu);
}

// Gram tiles (acc, x 2^2ey) and rhs tiles (accb, x 2^(ey+er)) of ratings
// [pb, pe) from the split table.  d0 = this lane's first dim (m * CN); st: 128
// words of wave-private LDS staging.  Pipeline as gram_accumulate_split; the
// gathers of the step after the last one read the zero row (never consumed).
template <class TS, bool ONE = false>
__device__ __forceinline__ void gram_accumulate_pre(
    const int32_t* __restrict__ col, const float* __restrict__ val, int64_t pb, int64_t pe,
    const uint32_t* __restrict__ Ysp, uint32_t kp, int zero_row, float sr, int d0,
    floatx4 (&acc)[TS::N], floatx4 (&accb)[RhsTiles<TS, ONE>::N], int* __restrict__ st,
    float& rmax) {
  const int lane = threadIdx.x & 63;
  int* st_c = st;
  uint32_t* st_r = reinterpret_cast<uint32_t*>(st + 64);
  if (pe <= pb) return;
  const uint32_t rsel = pre_rsel<TS, ONE>();
  const uint32_t* base = Ysp + d0;
  auto load_idx = [&](int64_t b, int& ci, float& rv) {
    ci = zero_row;
    rv = 0.f;
    if (b + lane < pe) {
      ci = col[b + lane];
      rv = val[b + lane];
    }
  };
  auto stage = [&](int ci, float rv) {
    st_c[lane] = ci;
    st_r[lane] = split_word(sr * rv);
    rmax = fmaxf(rmax, __builtin_fabsf(rv));
    wave_lds_sync();
  };
  const int nsteps = (int)((pe - pb + 31) >> 5);
  int ci, ci_n;
  float rv, rv_n;
  load_idx(pb, ci, rv);
  load_idx(pb + 64, ci_n, rv_n);
  stage(ci, rv);
  PreStep<TS::NC> s;
  pre_issue<TS>(s, st_c, st_r, 0, base, kp);
  for (int t = 0; t < nsteps; ++t) {
    uint32_t hi[TS::NC][4], lo[TS::NC][4], rb[4];
    pre_operands<TS>(s, rsel, hi, lo, rb);
    pin_operands<TS>(hi, lo, rb);
    // step t+1 = block (t+1)>>1, half (t+1)&1; a new block is staged from the
    // pairs prefetched one block earlier
    if (t & 1) {
      stage(ci_n, rv_n);
      load_idx(pb + 64 * (int64_t)((t >> 1) + 2), ci_n, rv_n);
    }
    pre_issue<TS>(s, st_c, st_r, (t + 1) & 1, base, kp);
    pre_mfma<TS, ONE>(hi, lo, rb, acc, accb);
  }
}

// Two steps of gathers in flight (W1 explicit light rows and chunks, one wave per
// SIMD: a step's MFMAs alone do not cover an HBM gather latency).  Register sets
// s0 / s1 hold steps t+1 and t+2 while step t's operands are formed; the rating
// indices are staged in LDS one block further ahead, in two block slots.
template <class TS>
__device__ __forceinline__ void gram_accumulate_pre2(
    const int32_t* __restrict__ col, const float* __restrict__ val, int64_t pb, int64_t pe,
    const uint32_t* __restrict__ Ysp, uint32_t kp, int zero_row, float sr, int d0,
    floatx4 (&acc)[TS::N], floatx4 (&accb)[TS::NRA], int* __restrict__ st, float& rmax) {
  const int lane = threadIdx.x & 63;
  // slot b % 2: 64 column indices then 64 split rating words
  if (pe <= pb) return;
  const uint32_t rsel = pre_rsel<TS, false>();
  const uint32_t* base = Ysp + d0;
  auto load_idx = [&](int64_t b, int& ci, float& rv) {
    ci = zero_row;
    rv = 0.f;
    if (b + lane < pe) {
      ci = col[b + lane];
      rv = val[b + lane];
    }
  };
  auto stage = [&](int slot, int ci, float rv) {
    st[128 * slot + lane] = ci;
    reinterpret_cast<uint32_t*>(st + 128 * slot + 64)[lane] = split_word(sr * rv);
    rmax = fmaxf(rmax, __builtin_fabsf(rv));
    wave_lds_sync();
  };
  auto issue = [&](PreStep<TS::NC>& s, int step) {
    const int slot = (step >> 1) & 1;
    pre_issue<TS>(s, st + 128 * slot, reinterpret_cast<const uint32_t*>(st + 128 * slot + 64),
                  step & 1, base, kp);
  };
  const int nsteps = (int)((pe - pb + 31) >> 5);
  int ci0, ci1, ci_n;
  float rv0, rv1, rv_n;
  load_idx(pb, ci0, rv0);
  load_idx(pb + 64, ci1, rv1);
  load_idx(pb + 128, ci_n, rv_n);
  stage(0, ci0, rv0);
  stage(1, ci1, rv1);
  PreStep<TS::NC> s0, s1;
  issue(s0, 0);
  issue(s1, 1);
  // step t: operands from s[t % 2]; that set then loads step t + 2 (block (t >> 1) + 1);
  // after an odd step the slot of block t >> 1 (fully issued) takes block (t >> 1) + 2
  auto body = [&](PreStep<TS::NC>& s, int t) {
    uint32_t hi[TS::NC][4], lo[TS::NC][4], rb[4];
    pre_operands<TS>(s, rsel, hi, lo, rb);
    pin_operands<TS>(hi, lo, rb);
    if (t & 1) {
      stage((t >> 1) & 1, ci_n, rv_n);
      load_idx(pb + 64 * (int64_t)((t >> 1) + 3), ci_n, rv_n);
    }
    issue(s, t + 2);  // past the last step: the zero row's words (never consumed)
    pre_mfma<TS>(hi, lo, rb, acc, accb);
  };
  for (int t = 0; t < nsteps; t += 2) {
    body(s0, t);
    if (t + 1 < nsteps) body(s1, t + 1);
  }
}

// rhs from the pre path's tiles: b[i*CN + gcol(c)] = C[i][0] + C[i][1] of
// accb[c], returned in the layout of the split path's partials (lane (0, m)
// holds dim m*CN + gcol(c), lanes with q > 0 hold 0), times `scale`.
// (One rhs tile: rows 2c and 2c + 1, i.e. registers (2c) % 4 and (2c) % 4 + 1 of
// lane (c / 2, m).)
template <class TS, bool ONE = false>
__device__ __forceinline__ void rhs_from_tiles(const floatx4 (&accb)[RhsTiles<TS, ONE>::N],
                                               float scale, float (&bt)[TS::NRA]) {
  const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
  if constexpr (ONE) {
#pragma unroll
    for (int c = 0; c < TS::NRA; ++c) {
      const float x = __shfl(accb[0][(2 * c) & 3] + accb[0][((2 * c) & 3) + 1], m + 16 * (c >> 1));
      bt[c] = (c < TS::NR && q == 0) ? x * scale : 0.f;
    }
    return;
  }
  const int src = (m >> 2) << 4;
  const int rr = m & 3;
#pragma unroll
  for (int c = 0; c < TS::NRA; ++c) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = __shfl(accb[c][r] + __shfl_xor(accb[c][r], 1), src);
    const float x = rr == 0 ? v[0] : (rr == 1 ? v[1] : (rr == 2 ? v[2] : v[3]));
    bt[c] = (c < TS::NR && q == 0) ? x * scale : 0.f;
  }
}

// Split table of one half-sweep's source factors (explicit only): one uint4
// (4 dims) per thread; rows of kp = 4 << kp4_shift words; row n_src is zero.
__global__ __launch_bounds__(256) void split_table_kernel(const float* __restrict__ Y,
                                                          int64_t n_src, int ld, int k,
                                                          int kp4_shift,
                                                          const float* __restrict__ scal,
                                                          uint4* __restrict__ Ysp) {
  const float sy = ldexpf(1.f, split_exponent(scal[0]));
  const int64_t total = (n_src + 1) << kp4_shift;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * 256) {
    const int64_t row = i >> kp4_shift;
    const int d = 4 * (int)(i & ((1 << kp4_shift) - 1));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n_src && d + 4 <= ld) v = *reinterpret_cast<const float4*>(Y + row * ld + d);
    uint4 w;
    w.x = d + 0 < k ? split_word(sy * v.x) : 0u;
    w.y = d + 1 < k ? split_word(sy * v.y) : 0u;
    w.z = d + 2 < k ? split_word(sy * v.z) : 0u;
    w.w = d + 3 < k ? split_word(sy * v.w) : 0u;
    Ysp[i] = w;
  }
}

}  // namespace als
