// Rank <= 64 row solve of one wavefront: the column-per-lane panel LDL^T, the iterative
// refinement of the implicit rows, and finish_and_solve (normal equations completed, then
// solved).  Used by gram_solve_kernel and reduce_solve_kernel.
#pragma once

#include "solve_config.h"
#include "solve_guards.h"

namespace als {

// ---------------------------------------------------------------------------
// Block LDL^T on a column-per-lane panel (k <= 64, one wavefront per system).
//
// The regularised Gram arrives as fp32 16x16 tiles in the MFMA C layout
// (A[t] = tile (I, J), I <= J; block I holds dims d = 16-index * CN + I).  Any
// symmetric permutation is a valid pivot order, so A = U^T D U (U unit upper)
// is factored in that block order.  For block row K, lane t holds column t of
// the 16 x 16(NB-K) panel [B_KK | B_K,K+1 | ...] (16 registers) plus one rhs
// value (b of the dim that column stands for).  Because B_KK is symmetric, its
// columns are its rows, and the 16-pivot elimination of the diagonal block, the
// TRSM of the off-diagonal panel (W = L^-1 B) and the forward substitution of
// the rhs — including the rhs trailing update b_J -= U_KJ^T D z_K — are ONE
// instruction stream over all lanes:
//   pivot p: d = R_p[p], f_t = R_t[p] / d (= U[p][t]),
//            R_t[i] -= R_p[i] * f_t (i > p),  rb_t -= f_t * rb_p
// (R_p[i] and rb_p broadcast from lane p by v_readlane).  The trailing tiles
// B_IJ -= U_KI^T D_K U_KJ (K < I <= J) run on the matrix cores from the U
// columns in LDS.  Back substitution x_K = U_KK^-1 (z_K / D_K - sum_J U_KJ x_J)
// on 16 lanes (DPP row broadcasts).
// LDS (floats): tile slots NT x 288 (16 columns, stride 18: 8-B aligned, at
// most 2-way conflicts on the MFMA operand reads) | z, d, x 3 x 16 NB.
// ---------------------------------------------------------------------------
template <int CN>
struct PanelLds {
  static constexpr int NB = CN, NT = CN * (CN + 1) / 2, CS = 18;  // column stride
  static constexpr int T = 0, Z = NT * 16 * CS, D = Z + 16 * NB, X = D + 16 * NB,
                       SIZE = X + 16 * NB;
};

// ata[ii] += lambda (explicit, fp32 tiles); padded dims get an identity row.
template <int CN>
__device__ __forceinline__ void regularise_f32(floatx4 (&A)[Cfg<CN>::NT], float lam, int k) {
  int tt = 0;
#pragma unroll
  for (int c1 = 0; c1 < CN; ++c1) {
#pragma unroll
    for (int c2 = c1; c2 < CN; ++c2) {
      if (c1 == c2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int i, j;
          tile_ij<CN>(c1, c2, r, i, j);
          if (i == j) A[tt][r] = (i < k) ? A[tt][r] + lam : 1.f;
        }
      }
      ++tt;
    }
  }
}

// x on lanes above P, 0 on lanes <= P.  The lane mask comes from the scalar
// unit (all-ones shifted left by P + 1), so the gate costs one VALU op.
template <int P>
__device__ __forceinline__ float gate_above(float x) {
  float r;
  uint64_t m;
  asm volatile("s_lshl_b64 %1, -1, %2\n\ts_nop 0\n\tv_cndmask_b32_e64 %0, 0, %3, %1"
               : "=v"(r), "=&s"(m)
               : "i"(P + 1), "v"(x));
  return r;
}

// Lane P of v replaced by the uniform value s (one v_writelane; the s_nop
// covers an SGPR just written by v_readlane).
template <int P>
__device__ __forceinline__ float put_lane(float v, float s) {
  asm volatile("s_nop 1\n\tv_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(s), "i"(P));
  return v;
}

// Pivot p's broadcasts from lane p: a[i] = R_p[i] for i >= p (a[p] = the pivot
// d) and bp = rb_p.  The uniform-index ds_bpermute becomes one v_readlane per
// value (measured: the LDS round trip on this serial chain is slower); all are
// issued before their FMAs, into distinct SGPRs, so no SGPR-hazard s_nop pads
// the updates, which then run two rows per v_pk_fma_f32 with an SGPR pair.
template <int N>
__device__ __forceinline__ void pivot_broadcast(const float (&R)[N], float rb, int p,
                                                float (&a)[N], float& bp) {
  const int addr = p << 2;
#pragma unroll
  for (int i = p; i < N; ++i)
    a[i] = __builtin_bit_cast(float,
                              __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, R[i])));
  bp = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, rb)));
}

// R[i] -= a[i] * f for i > p, two rows per v_pk_fma_f32 (for even p the pair
// (p, p+1) is updated too; the caller then overwrites R[p]).
template <int N>
__device__ __forceinline__ void pivot_update(float (&R)[N], const float (&a)[N], int p, float f) {
  const float2v nf = {-f, -f};
#pragma unroll
  for (int i = (p + 1) & ~1; i < N; i += 2) {
    const float2v r = __builtin_elementwise_fma((float2v){a[i], a[i + 1]}, nf,
                                                (float2v){R[i], R[i + 1]});
    R[i] = r[0];
    R[i + 1] = r[1];
  }
}

template <int P>
__device__ __forceinline__ float newbcast(float v) {  // lane P of each 16-lane row
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v),
                                                                0x150 + P, 0xF, 0xF, false));
}

// Block back substitution x_K = U_KK^-1 (z_K / D_K - sum_{J>K} U_KJ x_J) on lanes
// 0..15 (lanes 16.. mirror), K = NB-1 .. 0, from the U columns in the tile slots
// (column-major, stride CS; the U_KK columns hold 0 on and below the diagonal, so
// no masks are needed).  Runtime block loops keep the LDS address arithmetic
// out of the registers of the unrolled solve.
template <int CS>
__device__ __forceinline__ void block_back_subst(int NB, const float* __restrict__ tiles,
                                                 const float* __restrict__ Zv,
                                                 const float* __restrict__ Dv,
                                                 float* __restrict__ Xv) {
  const int lane = threadIdx.x & 63, i = lane & 15;
  for (int K = NB - 1; K >= 0; --K) {
    float v = Zv[K * 16 + i] * rcp_t(Dv[K * 16 + i]);
    for (int J = K + 1; J < NB; ++J) {
      const float* U = tiles + tile_index(NB, K, J) * 16 * CS + i;
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4) {
        const float4 xj = *reinterpret_cast<const float4*>(Xv + J * 16 + 4 * j4);
        v = fmaf(-U[(4 * j4 + 0) * CS], xj.x, v);
        v = fmaf(-U[(4 * j4 + 1) * CS], xj.y, v);
        v = fmaf(-U[(4 * j4 + 2) * CS], xj.z, v);
        v = fmaf(-U[(4 * j4 + 3) * CS], xj.w, v);
      }
    }
    const float* Ukk = tiles + tile_index(NB, K, K) * 16 * CS + i;
    float u[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) u[j] = Ukk[j * CS];
    static_for<16>([&](auto jr) {
      constexpr int j = 15 - decltype(jr)::value;
      v = fmaf(-u[j], newbcast<j>(v), v);
    });
    if (lane < 16) Xv[K * 16 + i] = v;
    wave_lds_sync();
  }
}

// x (permuted block layout Xv[K*16 + i] = dim i*CN + K) -> xrow (natural order, 0 past k
// and everywhere when !ok).
template <int CN>
__device__ __forceinline__ void panel_store_x(const float* __restrict__ Xv, int k, bool ok,
                                              float* __restrict__ xrow, int ld) {
  for (int d = threadIdx.x & 63; d < ld; d += 64) {
    const float x = d < 16 * CN ? Xv[(d % CN) * 16 + d / CN] : 0.f;
    xrow[d] = (d < k && ok) ? x : 0.f;
  }
}

// SPREAD: the pivot spread test (explicit rows; the implicit rows are checked a
// posteriori by iterative refinement instead).  STORE: write x to xrow here.
template <int CN, bool SPREAD = true, bool STORE = true>
__device__ __forceinline__ bool panel_ldl_solve(floatx4 (&A)[Cfg<CN>::NT], const float (&bq)[CN],
                                                float* __restrict__ lds, int k,
                                                float* __restrict__ xrow, int ld) {
  typedef PanelLds<CN> Lo;
  constexpr int NB = CN, CS = Lo::CS;
  const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
  float* Zv = lds + Lo::Z;
  float* Dv = lds + Lo::D;
  float* Xv = lds + Lo::X;
  auto slot = [&](int I, int J) { return lds + Lo::T + tile_index(NB, I, J) * 16 * CS; };
  // rhs of this lane's panel column at K = 0: dim m*CN + (block q)
  float rb = 0.f;
#pragma unroll
  for (int c = 0; c < CN; ++c)
    if (q == c) rb = bq[c];
  bool okl = true;  // this lane: every pivot of its diagonal lane was > 0
  float pmin = 3.0e38f, pmax = 0.f;  // this lane's pivots (lanes < 16)
  static_for<NB>([&](auto Kc) {
    constexpr int K = decltype(Kc)::value;
    constexpr int NCOL = 16 * (NB - K);
    // (a) block row K: C layout -> column-major tile slots (column m, rows 4q..4q+3)
    static_for<NB - K>([&](auto jc) {
      constexpr int J = K + decltype(jc)::value;
      const floatx4 v = A[tile_index(NB, K, J)];
      float2* dst = reinterpret_cast<float2*>(slot(K, J) + m * CS + 4 * q);
      dst[0] = make_float2(v[0], v[1]);
      dst[1] = make_float2(v[2], v[3]);
    });
    wave_lds_sync();
    const bool col_ok = lane < NCOL;
    const int Jl = K + (col_ok ? q : 0);
    float* colp = slot(K, Jl) + m * CS;
    float R[16];
#pragma unroll
    for (int c2 = 0; c2 < 8; ++c2) {
      const float2 v = *reinterpret_cast<const float2*>(colp + 2 * c2);
      R[2 * c2] = v.x; R[2 * c2 + 1] = v.y;
    }
    // (b) 16 pivots over the whole panel (diag LDL^T + TRSM + rhs forward)
    float myd = 1.f;
    static_for<16>([&](auto pc) {
      constexpr int p = decltype(pc)::value;
      float a[16];
      float bp;
      pivot_broadcast<16>(R, rb, p, a, bp);
      const float d = a[p];
      const float rd = rcp_t(d);
      const float f = gate_above<p>(R[p] * rd);  // U[p][t]; 0 below the diagonal
      rb = fmaf(-f, bp, rb);
      pivot_update<16>(R, a, p, f);
      R[p] = f;
      myd = put_lane<p>(myd, d);
    });
    okl = okl && (myd > 0.f);  // lanes >= 16 keep myd = 1; NaN pivots fail
    if (lane < 16 && lane * CN + K < k) {  // pivots of real dims
      pmin = fminf(pmin, myd);
      pmax = fmaxf(pmax, myd);
    }
    // (c) U columns -> tile slots (block row K); z_K, D_K
    if (col_ok) {
#pragma unroll
      for (int c2 = 0; c2 < 8; ++c2)
        *reinterpret_cast<float2*>(colp + 2 * c2) = make_float2(R[2 * c2], R[2 * c2 + 1]);
    }
    if (lane < 16) {
      Zv[K * 16 + lane] = rb;
      Dv[K * 16 + lane] = myd;
    }
    if constexpr (K + 1 < NB) {
      rb = __shfl(rb, (lane + 16) & 63);  // next block row's rhs: columns shift by 16
      wave_lds_sync();
      // (d) trailing update B_IJ -= (D_K U_KI)^T U_KJ on the matrix cores
      float dq[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) dq[s4] = -Dv[K * 16 + 4 * s4 + q];
      static_for<NB - 1 - K>([&](auto ic) {
        constexpr int I = K + 1 + decltype(ic)::value;
        float ua[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) ua[s4] = dq[s4] * slot(K, I)[m * CS + 4 * s4 + q];
        static_for<NB - I>([&](auto jc) {
          constexpr int J = I + decltype(jc)::value;
          floatx4 acc = A[tile_index(NB, I, J)];
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[s4], slot(K, J)[m * CS + 4 * s4 + q],
                                                        acc, 0, 0, 0);
          A[tile_index(NB, I, J)] = acc;
        });
      });
    }
  });
  wave_lds_sync();
  // pivot spread (lower bound on cond(A)) within what fp32 holds to the 1e-4 bar
  for (int o = 32; o > 0; o >>= 1) {
    pmin = fminf(pmin, __shfl_xor(pmin, o));
    pmax = fmaxf(pmax, __shfl_xor(pmax, o));
  }
  const bool ok = __ballot(!okl) == 0 && (!SPREAD || pmax <= kCondMax * pmin);
  // (e) back substitution
  block_back_subst<CS>(NB, lds + Lo::T, Zv, Dv, Xv);
  // (f) un-permute: dim d = i*CN + K  <->  Xv[K*16 + i]
  if constexpr (STORE) panel_store_x<CN>(Xv, k, ok, xrow, ld);
  return ok;
}

// Forward substitution U^T z = r for a new right-hand side (U unit upper from the
// panel factorisation: tile slot (J, K) column i holds U_JK[p][i], p = 0..15, and the
// diagonal tiles hold 0 on and below the diagonal), block row by block row on lanes
// 0..15 (lanes 16.. mirror).  Rv, Zv in the permuted block layout.
template <int CS>
__device__ __forceinline__ void block_fwd_subst(int NB, const float* __restrict__ tiles,
                                                const float* __restrict__ Rv,
                                                float* __restrict__ Zv) {
  const int lane = threadIdx.x & 63, i = lane & 15;
  for (int K = 0; K < NB; ++K) {
    float v = Rv[K * 16 + i];
    for (int J = 0; J < K; ++J) {  // v -= U_JK^T z_J: column i of tile (J, K)
      const float* U = tiles + tile_index(NB, J, K) * 16 * CS + i * CS;
#pragma unroll
      for (int p4 = 0; p4 < 4; ++p4) {
        const float4 zj = *reinterpret_cast<const float4*>(Zv + J * 16 + 4 * p4);
        v = fmaf(-U[4 * p4 + 0], zj.x, v);
        v = fmaf(-U[4 * p4 + 1], zj.y, v);
        v = fmaf(-U[4 * p4 + 2], zj.z, v);
        v = fmaf(-U[4 * p4 + 3], zj.w, v);
      }
    }
    const float* Ukk = tiles + tile_index(NB, K, K) * 16 * CS + i * CS;
    float u[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) u[p] = Ukk[p];  // U_KK[p][i]: 0 for p >= i
    static_for<16>([&](auto pc) {  // z_i = v_i - sum_{p < i} U_KK[p][i] z_p
      constexpr int p = decltype(pc)::value;
      v = fmaf(-u[p], newbcast<p>(v), v);
    });
    if (lane < 16) Zv[K * 16 + i] = v;
    wave_lds_sync();
  }
}

// ---------------------------------------------------------------------------
// Iterative refinement of the implicit rows' panel solutions (k <= 64).
//
// The fp32-grade Gram (split-f16 products, fp32 sums) and the fp32 LDL^T each
// perturb A by ~2^-21..2^-24 relative, which the condition of an implicit system
// (confidences 1 + alpha |r| spanning decades) amplifies: emulated at ranks 16-64 on
// counts 1..1e6, 1e-4..4e-3 relative errors, half from each source.  Mixed-precision
// refinement removes both: r = b - A x with A's own terms in Spark's fp64 arithmetic
// (NormalEquation.add: products of fp32 values, exact in fp64; YtY; lambda n), the
// correction A d = r solved with the kept fp32 factorisation, x += d.  Each step
// contracts the error by ~cond(A) 2^-21, and |d| estimates the error it removed, so
// the loop is its own a-posteriori test: done when |d| <= kIrConv |x| (the error left
// is then ~(|d| / |x|)^2 |x| <= 1e-7 |x|), and a row that has not converged within
// kIrSteps, or whose correction exceeds kIrDiverge |x| (contraction not reliable), is
// re-solved in fp64 (rescue64_kernel).
// ---------------------------------------------------------------------------
constexpr int kIrSteps = 3;
constexpr float kIrConv = 3e-4f;
constexpr float kIrDiverge = 0.1f;

// The implicit row's ratings and source factors (for the residual pass).
struct IrArgs {
  const int32_t* col;
  const float* val;
  const float* Y;
  int64_t pb, pe;
  float alpha;
};

// LDS after the panel (floats): x in fp64 (natural order, 64) | batch weights g
// (64 doubles) | their columns (64 ints) | residual rhs, correction (permuted, 16 NB).
template <int CN>
struct IrLds {
  static constexpr int XS = PanelLds<CN>::SIZE, GS = XS + 128, CC = GS + 128, RV = CC + 64,
                       DX = RV + 16 * CN, SIZE = DX + 16 * CN;
  static_assert(XS % 4 == 0, "fp64 alignment");
};

// r_d = b_d - ((G + YtY + lambda n I) x)_d for an implicit row, lane d < k (fp64).
// Batches of 64 ratings: lane j forms g_j = [r_j > 0](1 + c_j) - c_j (y_j . x), then
// lane d accumulates sum_j g_j y_jd (coalesced row reads, L2-hot after the Gram pass).
__device__ __forceinline__ double implicit_residual(const IrArgs& a, int ld, int k,
                                                    const double* __restrict__ yty, double lam_n,
                                                    const double* __restrict__ xs,
                                                    double* __restrict__ gs, int* __restrict__ cc) {
  const int lane = threadIdx.x & 63;
  double r = 0.0;
  for (int64_t base = a.pb; base < a.pe; base += 64) {
    const int nb = (int)(a.pe - base < 64 ? a.pe - base : 64);
    double g = 0.0;
    int c = 0;
    if (lane < nb) {
      c = a.col[base + lane];
      const double rv = (double)a.val[base + lane];
      const float* y = a.Y + (int64_t)c * ld;
      double s0 = 0.0, s1 = 0.0;
      for (int d = 0; d < k; d += 4) {  // xs is zero past k (< ld, ld % 4 == 0)
        const float4 v = *reinterpret_cast<const float4*>(y + d);
        s0 = fma((double)v.x, xs[d], s0);
        s1 = fma((double)v.y, xs[d + 1], s1);
        s0 = fma((double)v.z, xs[d + 2], s0);
        s1 = fma((double)v.w, xs[d + 3], s1);
      }
      const double c1 = (double)a.alpha * fabs(rv);
      g = (rv > 0.0 ? 1.0 + c1 : 0.0) - c1 * (s0 + s1);
    }
    gs[lane] = g;
    cc[lane] = c;
    wave_lds_sync();
    if (lane < k) {
#pragma unroll 8
      for (int j = 0; j < nb; ++j) r = fma(gs[j], (double)a.Y[(int64_t)cc[j] * ld + lane], r);
    }
    wave_lds_sync();
  }
  if (lane < k) {
    for (int e = 0; e < k; ++e) {
      const int hi = lane > e ? lane : e, lo = lane > e ? e : lane;
      r = fma(-yty[hi * (hi + 1) / 2 + lo], xs[e], r);
    }
    r = fma(-lam_n, xs[lane], r);
  }
  return r;
}

// Refine the panel solution in Xv (permuted layout) in place; true once converged.
template <int CN>
__device__ __forceinline__ bool panel_refine(float* __restrict__ lds, const IrArgs& a, int ld,
                                             int k, const double* __restrict__ yty,
                                             double lam_n) {
  typedef PanelLds<CN> Lo;
  typedef IrLds<CN> Ir;
  float* Xv = lds + Lo::X;
  float* Zv = lds + Lo::Z;
  const float* Dv = lds + Lo::D;
  double* xs = reinterpret_cast<double*>(lds + Ir::XS);
  double* gs = reinterpret_cast<double*>(lds + Ir::GS);
  int* cc = reinterpret_cast<int*>(lds + Ir::CC);
  float* Rv = lds + Ir::RV;
  float* DX = lds + Ir::DX;
  const int lane = threadIdx.x & 63;
  const int pl = (lane % CN) * 16 + lane / CN;  // permuted slot of natural dim `lane`
  bool conv = false;
  for (int it = 0; it < kIrSteps; ++it) {
    xs[lane] = lane < k ? (double)Xv[pl] : 0.0;  // k <= 64: one dim per lane
    wave_lds_sync();
    const double r = implicit_residual(a, ld, k, yty, lam_n, xs, gs, cc);
    if (lane < 16 * CN) Rv[pl] = lane < k ? (float)r : 0.f;
    wave_lds_sync();
    block_fwd_subst<Lo::CS>(CN, lds + Lo::T, Rv, Zv);
    block_back_subst<Lo::CS>(CN, lds + Lo::T, Zv, Dv, DX);
    float nd = 0.f, nx = 0.f;
    if (lane < 16 * CN) {
      const float dx = DX[lane];
      const float xn = Xv[lane] + dx;
      Xv[lane] = xn;
      nd = dx * dx;
      nx = xn * xn;
    }
    wave_lds_sync();
    for (int o = 32; o > 0; o >>= 1) {
      nd += __shfl_xor(nd, o);
      nx += __shfl_xor(nx, o);
    }
    if (nd <= (kIrConv * kIrConv) * nx) {
      conv = true;
      break;
    }
    if (!(nd <= (kIrDiverge * kIrDiverge) * nx)) break;  // (NaN included)
  }
  return conv;
}

__device__ __forceinline__ float shfl_xor_t(float v, int m) { return __shfl_xor(v, m); }
__device__ __forceinline__ double shfl_xor_t(double v, int m) { return shfl_xor_f64(v, m); }

// Shared tail of a row: rhs reduce over the 4 rating slots, complete the normal
// equations (Spark CholeskySolver.solve: ata[ii] += lambda * numExplicits;
// implicit: ls.merge(YtY), added in fp64 before the single rounding to fp32),
// then the block LDL^T on the matrix cores.  fp32 factorisation: the systems are
// regularised (cond ~ (lambda + |y|^2)/lambda, measured <= 240 for implicit
// alpha = 40 at k = 128), fp32 error ~2e-6 vs the 1e-4 parity bar.
template <int CN, bool IMPLICIT, class AccT>
__device__ __forceinline__ void finish_and_solve(AccT (&tot)[Cfg<CN>::NT][4], AccT (&bt)[CN],
                                                 int64_t n_reg, unsigned char* smem, int k,
                                                 float reg, const double* __restrict__ yty,
                                                 float* __restrict__ xrow, int ld, int row,
                                                 RescueList rl, const IrArgs& ir) {
  constexpr int NT = Cfg<CN>::NT;
  float bq[CN];
  const int m = threadIdx.x & 15;
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    AccT v = bt[c];
    v += shfl_xor_t(v, 16);
    v += shfl_xor_t(v, 32);
    bq[c] = m * CN + c < k ? (float)v : 0.f;  // padded dims: rhs 0
  }
  floatx4 A[NT];
  int tt = 0;
#pragma unroll
  for (int c1 = 0; c1 < CN; ++c1) {
#pragma unroll
    for (int c2 = c1; c2 < CN; ++c2) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (IMPLICIT) {
          int i, j;
          tile_ij<CN>(c1, c2, r, i, j);
          const int hi = i > j ? i : j, lo = i > j ? j : i;
          A[tt][r] = (float)((double)tot[tt][r] + yty[hi * (hi + 1) / 2 + lo]);
        } else {
          A[tt][r] = (float)tot[tt][r];
        }
        int i, j;
        tile_ij<CN>(c1, c2, r, i, j);
        if (i >= k || j >= k) A[tt][r] = 0.f;  // padded dims: rows/columns of the identity
      }
      ++tt;
    }
  }
  regularise_f32<CN>(A, (float)((double)reg * (double)n_reg), k);
  float* lds = reinterpret_cast<float*>(smem);
  if constexpr (IMPLICIT) {
    // pivots checked here, accuracy a posteriori by the refinement
    bool ok = panel_ldl_solve<CN, false, false>(A, bq, lds, k, xrow, ld);
    if (ok) ok = panel_refine<CN>(lds, ir, ld, k, yty, (double)reg * (double)n_reg);
    panel_store_x<CN>(lds + PanelLds<CN>::X, k, ok, xrow, ld);
    if (!ok) rescue_append(rl, row);  // re-solved in fp64
  } else {
    const bool ok = panel_ldl_solve<CN>(A, bq, lds, k, xrow, ld);
    if (!ok) rescue_append(rl, row);  // re-solved in fp64
  }
}

}  // namespace als
