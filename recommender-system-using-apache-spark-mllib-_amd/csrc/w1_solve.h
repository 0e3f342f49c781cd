// The W1 block elimination of one wavefront (16 x 16 diagonal inverses by the sweep
// operator, Pm and Schur products on the matrix cores): NB = 8 for rank 65-128
// (gram_solve_w1_kernel, reduce_solve_w1_kernel), 4 for explicit rank 33-64
// (gram_solve_kernel), 2 / 4 / 6 for the dual systems (gram_solve_dual_kernel); the W1
// slot, table and LDS constants; w1_finish_and_solve.
#pragma once

#include "solve_config.h"
#include "gram_accumulate.h"
#include "solve_guards.h"

namespace als {

// ---------------------------------------------------------------------------
// k in (64, 128]: ONE wavefront per system ("W1"), block Gaussian elimination
// with explicit inverses of the 16 x 16 diagonal blocks (NB = 8 block rows).
//
// The Gram's 36 upper tiles stay in the MFMA C layout (lane (q, m): rows
// 4q..4q+3 of column m).  For two tiles X, Y in that layout, the products
//   C += X^T Y  =  sum_s4 mfma_16x16x4_f32(X.reg[s4], Y.reg[s4])
// need no data movement (the MFMA's k index is permuted to 4q + s4), so the
// whole right-looking elimination runs on registers:
//   for K = 0..7:
//     Gm   = -(B_KK)^-1            sweep operator on the diagonal block (VALU,
//                                  column per lane, lane-p broadcasts by DPP)
//     Pm_J = Gm B_KJ   (J > K)     = -B_KK^-1 B_KJ, on the matrix cores
//     B_IJ += B_KI^T Pm_J (K < I <= J)   Schur complement, matrix cores
//     b_J  += Pm_J^T b_K,  z_K = -Gm b_K
//     tile (K, J) <- Pm_J           (kept for the back substitution)
//   x_K = z_K + sum_{J>K} Pm_KJ x_J,  K = 7..0.
// The sweep's pivots are the LDL^T pivots of B (all must be > 0: Spark's dppsv
// fails otherwise).  Same solution as Spark's Cholesky dppsv, fp32 arithmetic
// with exact-product fp32 MFMA; no barrier, no LDS beyond one 16 x 16
// transposition buffer per wave.
// rhs layouts: "column" = lane m (any q) holds element m of a 16-block;
// "row" = lanes of row-group q hold elements 4q..4q+3.
// ---------------------------------------------------------------------------
template <int NB>
struct W1LdsT {
  static constexpr int CS = 20;                     // floats per column (16 + pad, 16-B aligned)
  // transposition buffer | rhs vector | Pm tiles of the back substitution (NB(NB-1)/2 x 256)
  static constexpr int COL = 0, VEC = 16 * CS, PM = VEC + 16,
                       SIZE = PM + NB * (NB - 1) / 2 * 256;
};

constexpr int kW1NB = 8;
using W1Lds = W1LdsT<kW1NB>;

template <int NB>
__host__ __device__ constexpr int w1_tile(int i, int j) { return tile_index(NB, i, j); }

// v on lanes with (lane & 15) == P, else w (mask from the scalar unit).
template <int P>
__device__ __forceinline__ float sel_lane16(float v, float w) {
  float r;
  const uint64_t msk = 0x0001000100010001ull << P;
  asm volatile("v_cndmask_b32_e64 %0, %2, %1, %3" : "=v"(r) : "v"(v), "v"(w), "s"(msk));
  return r;
}

// Sum over the four 16-lane row groups (every lane gets the total): two VALU
// row swaps (v_permlane16_swap: rows 0<->1, 2<->3; v_permlane32_swap: rows
// {0,1}<->{2,3}), no LDS crossbar on the dependency chain.
// (Inline asm: this compiler's __builtin_amdgcn_permlane*_swap loses the second
// result when both are consumed — measured, it emitted v_add v1, v1, v1.)
__device__ __forceinline__ float reduce_rows4(float v) {
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  float c = a + b, d = c;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(c), "+v"(d));
  return c + d;
}

// Sum over the 16 lanes of each row group (every lane of the group gets it).
// Lane P of each 16-lane row, as a DPP source the combiner folds into the user
// (bound_ctrl set, old undefined: v_fmac_f32_dpp / v_rcp_f32_dpp row_newbcast:P).
template <int P>
__device__ __forceinline__ float bcast16(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x150 + P,
                                                            0xF, 0xF, true));
}

// r += (lane P's r, same 16-lane row) * nf: one v_fmac_f32_dpp row_newbcast:P.
template <int P>
__device__ __forceinline__ void fmac_bcast16(float& r, float nf) {
  asm volatile("v_fmac_f32_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf"
               : "+v"(r)
               : "v"(nf), "i"(P));
}

__device__ __forceinline__ float reduce_lanes16(float v) {
  v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);  // row_half_mirror
  v += dpp_f<0x140>(v);  // row_mirror
  return v;
}

// Sweep operator over all 16 pivots of a symmetric 16 x 16 block held column per
// lane (R[i] = B[i][m], replicated in the four row groups): R <- -(B^-1) column m.
// Pivot p: d = B[p][p]; B[i][j] -= B[i][p] B[p][j] / d; row/column p scaled by
// 1/d; B[p][p] = -1/d.  The pivot column's 1/d scaling is DEFERRED: lane p keeps
// its column unscaled (multiplier 0 at its own pivot) and every column is scaled
// by 1/(its pivot) once at the end.  The stored values then follow the generic
// update for every lane (the multiplier -B[p][m]/d does not depend on a column's
// pending scale), and no lane ever forms 1 - 1/d (which cancels for large d).
// Returns the smallest pivot (> 0 for an SPD block; NaN propagates as "not > 0").
// hook(p) runs after pivot p: the caller interleaves independent matrix-core work
// there (the asm statements fix the instruction order).
template <class Hook>
__device__ __forceinline__ float sweep16(float (&R)[16], Hook&& hook, float& dself_out) {
  float dmin = 3.0e38f;  // NaN pivots are not seen here: they make the solution NaN
  float dself = 1.f;     // this lane's own pivot (its column's deferred scale is 1/dself)
  // pivot p's broadcast pivot, reciprocal and multipliers; for p > 0 they are formed
  // inside pivot p-1, right after row p's update, so their latency (DPP, v_rcp)
  // hides behind that pivot's remaining row updates
  float d = bcast16<0>(R[0]);
  float rd = rcp_t(d);
  float f = R[0] * rd;
  float nf = sel_lane16<0>(0.f, -f);
  static_for<16>([&](auto pc) {
    constexpr int p = decltype(pc)::value;
    dmin = fminf(dmin, d);
    // R[i] += (lane p's R[i]) * nf as ONE v_fmac_f32_dpp per row (the compiler only
    // folds DPP into untied VOP2 ops); s_nop 1 covers the VALU-write -> DPP-read
    // hazard of the previous pivot's last writes.
    asm volatile("s_nop 1" ::: "memory");
    float dn = 0.f, rdn = 0.f, fn = 0.f, nfn = 0.f;
    auto row = [&](auto ic) {
      constexpr int i = decltype(ic)::value;
      if constexpr (i != p) fmac_bcast16<p>(R[i], nf);
      if constexpr (i == p + 1) {  // row p+1 is final for pivot p+1: start it now
        asm volatile("s_nop 1" ::: "memory");
        dn = bcast16<p + 1>(R[p + 1]);
        rdn = rcp_t(dn);
        fn = R[p + 1] * rdn;
        nfn = sel_lane16<p + 1>(0.f, -fn);
      }
    };
    // row p+1 first, then the others
    if constexpr (p + 1 < 16) row(std::integral_constant<int, p + 1>{});
    static_for<16>([&](auto ic) {
      constexpr int i = decltype(ic)::value;
      if constexpr (i != p + 1) row(ic);
    });
    R[p] = sel_lane16<p>(-1.f, f);
    dself = sel_lane16<p>(d, dself);
    hook(pc);
    d = dn; rd = rdn; f = fn; nf = nfn;
  });
  const float s = rcp_t(dself);
#pragma unroll
  for (int i = 0; i < 16; ++i) R[i] *= s;
  dself_out = dself;
  return dmin;
}

// x of row group G broadcast to all four row groups: one ds_bpermute (the LDS
// crossbar, not the VALU).  The sweep is bound by VALU issue, not by its pivot chain's
// latency (three waves per SIMD hide it): two v_permlane*_swap plus their operand
// copies (five VALU instructions per pivot) measured 0.06 ms slower on the configs[1]
// user launch (A/B round 5, profiles/r05/ab_sweep_lean.jsonl).
template <int G>
__device__ __forceinline__ float rowgroup_bcast(float x) {
  const int src = (16 * G + (threadIdx.x & 15)) << 2;
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, x)));
}

// v on lanes with (lane & 15) == P, else -w.
template <int P>
__device__ __forceinline__ float sel_lane16_n(float v, float w) {
  float r;
  const uint64_t msk = 0x0001000100010001ull << P;
  asm volatile("v_cndmask_b32_e64 %0, -%2, %1, %3" : "=v"(r) : "v"(v), "v"(w), "s"(msk));
  return r;
}

// v on the lanes of 64-bit mask M (a constant), else w.
template <uint64_t M>
__device__ __forceinline__ float sel_mask(float v, float w) {
  float r;
  asm volatile("v_cndmask_b32_e64 %0, %2, %1, %3" : "=v"(r) : "v"(v), "v"(w), "s"(M));
  return r;
}

// The sweep of sweep16 on a symmetric 16 x 16 block held in the MFMA C layout (lane
// (q, m): B[4q + r][m], r = 0..3) instead of column per lane: per pivot p, row p is
// broadcast from row group p/4 to all four (rowgroup_bcast), and a lane's four column-p
// entries come from lane p of its own row group (v_fmac_f32_dpp row_newbcast:p), so a
// lane updates its four entries, not sixteen replicated ones, and the block never goes
// through LDS (the result is already in the C layout the Pm / Schur MFMAs read).  Every
// entry sees the same fp32 operations, in the same order, as in sweep16 (deferred
// pivot-column scaling, look-ahead of the next pivot).  Per pivot the VALU issues the
// four row updates, the pivot broadcast, its reciprocal, one multiply and the selects
// (the multiplier's negation rides in a select's source modifier); positivity of the
// pivots is checked by the caller from the spread test's minimum (dself_out), so the
// returned minimum is not tracked here (+inf).  A 2 x 2-pivot form (8 sequential steps
// instead of 16) measured slower: the same updates plus a 2 x 2 inverse per pair, and
// the sweep is issue-bound, not chain-bound (A/B round 5, profiles/r05/ab_pair_pivots.jsonl)
// — at two or more waves per SIMD.  LA (the one-wave-per-SIMD W1 kernels, NB = 8): the
// next pivot row's broadcast is issued one pivot earlier, before the current pivot's
// update, and brought up to date on the copy by one more DPP fmac (the same fp32
// operation as on its register, so the results are bit-identical): the ds_bpermute
// latency leaves the pivot chain for one VALU more per pivot.  A/B round 5
// (profiles/r05/ab_lookahead.jsonl): configs[3] W1 user rows 96.6 -> 95.2 ms, 271.9 ->
// 270.1 ms/iter; slower where other waves hide the chain (k <= 64: user launch +0.7 %,
// dual rows +2.5 %).  Round 6: two rows ahead (row p+2's copy is brought up to date after
// the pivot's row updates, so each ds_bpermute has a whole pivot to land; one DPP fmac
// more per pivot, still bit-identical): W1 user rows 94.9 -> 93.0 ms, 273.4 -> 271.0
// ms/iter at 4096-rating tasks (profiles/r06/ab_lookahead2.jsonl).
//
// LEAN (the full-rank 33-64 explicit launch, where the VALU is the busiest unit): two
// VALU instructions fewer per pivot, every entry's operations as before.  The pivot's
// own-lane copy comes from the broadcast row (lane p of it IS the pivot, the same bits
// as its row_newbcast copy d), so d feeds the reciprocal alone and rides in its DPP
// operand; and row p's write (f off the pivot, -1 on it, row group p/4 only) is one
// v_cndmask_b32_dpp whose row_mask keeps the other row groups' register.
template <int P>
__device__ __forceinline__ void put_pivot_row(float& b, float f, float neg1) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the VOP2 DPP select takes its lane mask from vcc (a scalar move, no VALU)
  const uint64_t msk = 0x0001000100010001ull << P;
  asm volatile("s_mov_b64 vcc, %3\n\t"
               "v_cndmask_b32_dpp %0, %1, %2, vcc quad_perm:[0,1,2,3] row_mask:%4 bank_mask:0xf"
               : "+v"(b)
               : "v"(f), "v"(neg1), "s"(msk), "i"(1 << (P >> 2))
               : "vcc");
#endif
}

template <bool LA = false, bool LEAN = false, class Hook>
__device__ __forceinline__ float sweep16c(floatx4& Bv, Hook&& hook, float& dself_out) {
  static_assert(!(LA && LEAN), "the lean form keeps the pivot row's broadcast, not its look-ahead copy");
  // Bv was just written by the matrix cores (the pivot block's Schur update) and is
  // read below by inline DPP asm, which the hazard recognizer does not see: the XDL
  // write -> VALU read wait states by hand (tests/test_isa_hazards.py checks the rest)
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  float B[4] = {Bv[0], Bv[1], Bv[2], Bv[3]};
  float dmin = 3.0e38f;
  float dself = 1.f;
  float rowp = rowgroup_bcast<0>(B[0]);
  float pre = 0.f;   // LA: the next pivot row's broadcast copy
  float pre2 = 0.f;  // LA: the one after it (its ds_bpermute has a whole pivot to land)
  if constexpr (LA) {
    pre = rowgroup_bcast<0>(B[1]);   // row 1 before pivot 0
    pre2 = rowgroup_bcast<0>(B[2]);  // row 2 before pivot 0
  }
  float d = bcast16<0>(rowp);
  float rd = rcp_t(d);
  float f = rowp * rd;
  float nf = sel_lane16_n<0>(0.f, f);
  float rowc = rowp;  // LEAN: the current pivot's broadcast row
  const float neg1 = -1.f;
  static_for<16>([&](auto pc) {
    constexpr int p = decltype(pc)::value;
    constexpr int qp = p >> 2, rp = p & 3, rn = (p + 1) & 3;
    asm volatile("s_nop 1" ::: "memory");
    float dn = 0.f, rdn = 0.f, fn = 0.f, nfn = 0.f, rowcn = 0.f;
    if constexpr (LA) {
      if constexpr (p + 1 < 16) {  // row p+1 after pivot p, on its broadcast copy
        fmac_bcast16<p>(pre, nf);
        dn = bcast16<p + 1>(pre);
        rdn = rcp_t(dn);
        fn = pre * rdn;
        nfn = sel_lane16_n<p + 1>(0.f, fn);
      }
      static_for<4>([&](auto rc) { fmac_bcast16<p>(B[decltype(rc)::value], nf); });
      // row p+2's copy (broadcast two pivots ago) after pivot p, after this pivot's row
      // updates so its ds_bpermute has had them to land; row p+3's broadcast (after
      // pivots <= p) is issued now and consumed two pivots on
      if constexpr (p + 2 < 16) fmac_bcast16<p>(pre2, nf);
      if constexpr (p + 3 < 16) {
        constexpr int q3 = (p + 3) / 4, r3 = (p + 3) % 4;
        pre = pre2;
        pre2 = rowgroup_bcast<q3>(B[r3]);
      } else {
        pre = pre2;
      }
    } else {
      // the register holding row p+1 first: then pivot p+1's row is final
      fmac_bcast16<p>(B[rn], nf);
      if constexpr (p + 1 < 16) {
        constexpr int qn = (p + 1) >> 2;
        const float rown = rowgroup_bcast<qn>(B[rn]);
        dn = bcast16<p + 1>(rown);
        rdn = rcp_t(dn);
        fn = rown * rdn;
        nfn = sel_lane16_n<p + 1>(0.f, fn);
        rowcn = rown;
      }
      static_for<4>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        if constexpr (r != rn) fmac_bcast16<p>(B[r], nf);
      });
    }
    // row p (row group qp): f off the pivot, -1 on it (scaled by 1/d at the end)
    if constexpr (LEAN) {
      put_pivot_row<p>(B[rp], f, neg1);
      dself = sel_lane16<p>(rowc, dself);
    } else {
      B[rp] = sel_mask<0xFFFFull << (16 * qp)>(sel_lane16<p>(-1.f, f), B[rp]);
      dself = sel_lane16<p>(d, dself);
    }
    hook(pc);
    d = dn; rd = rdn; f = fn; nf = nfn; rowc = rowcn;
  });
  const float s = rcp_t(dself);
#pragma unroll
  for (int r = 0; r < 4; ++r) Bv[r] = B[r] * s;
  dself_out = dself;
  return dmin;
}

// Schur tiles of step K, I-major: u = 0 is (K+1, K+1), the next pivot block.
template <int NB>
__host__ __device__ constexpr int schur_n(int K) { return (NB - 1 - K) * (NB - K) / 2; }
template <int NB>
__host__ __device__ constexpr int schur_I(int K, int u) {
  int I = K + 1;
  while (u >= NB - I) { u -= NB - I; ++I; }
  return I;
}
template <int NB>
__host__ __device__ constexpr int schur_J(int K, int u) {
  int I = K + 1;
  while (u >= NB - I) { u -= NB - I; ++I; }
  return I + u;
}

// Schur complement and Pm products of the W1 elimination.  Both operands of
// C += X^T Y are 16 x 16 tiles in the C layout, so each product is a handful of
// MFMAs with no data movement: on v_mfma_f32_16x16x32_f16 lane (q, m) supplies
// k = 8q..8q+7, i.e. its four C-layout values twice (hi and lo halves).
// Split f16 (default): the operands are scaled by powers of two and split into
// f16 hi + lo; [Xh|Xl]^T [Yh|Yh] + [Xh|Xl]^T [Yl|Yl] = (Xh + Xl)^T (Yh + Yl) is
// two MFMAs (32 cycles; the fp32 form, four v_mfma_f32_16x16x4_f32, takes 128).
// For the Schur update the two scales cancel (X 2^a, Pm 2^-a, a balancing the
// two maxima), so the MFMAs accumulate straight into the fp32 tile: no VALU
// touches the 36 system tiles during the elimination.  The system is first
// scaled by a power of two (largest diagonal entry -> [2^13, 2^14)), which bounds
// every Schur complement entry and keeps the scaled operands inside the f16
// range; pieces are exact to ~2^-22 relative, and entries far below their tile's
// maximum lose precision only below the fp32 rounding floor of the elimination.
// Where it is used (measured, ML-25M shape): the implicit rank-128 light-row
// kernel (configs[2] 11.0 -> 9.4 ms/iter) and the heavy-row solve.  Not for
// NB = 4 (rank 33-64: 10 Schur tiles per system, too few to pay for the scaling
// and splitting) and not in the explicit rank-128 light-row kernel, whose
// pre-split Gram leaves no registers for the split operands (it spills; 7.8 ->
// 8.1 ms/iter measured).
template <int NB>
constexpr bool kW1SplitSchur = NB == 8;
// Diagonal blocks swept in the MFMA C layout (sweep16c: 4 entries per lane instead of
// 16 replicated) in every elimination but the split-Schur one.  With the row-group
// pivot broadcast as one ds_bpermute (round 5) it pays in the NB = 8 fp32 kernels too,
// which round 4 (two permlane swaps per pivot) had measured slower: A/B round 5,
// `profiles/r05/ab_sweepc_nb.jsonl`, configs[3] 287.4 -> 280.1 ms/iter (explicit
// rank-128 user launch 101.5 -> 96.3 ms, dual systems 65.6 -> 64.7 ms), configs[1]
// 2.043 -> 2.032.  In the split-Schur form (implicit rank-128 light rows, heavy-row
// solves) it is slower: configs[2] 9.32 -> 10.99 ms/iter (user launch 5.48 -> 6.66), and
// still with the pivot lookahead of the W1 sweep: 9.12 -> 10.75 (ab_sweepc_split_lookahead.jsonl).
template <int NB, bool SPLIT>
constexpr bool kSweepC = !SPLIT;
// Measured round 4 (A/B at configs[1] / configs[3]): the split form in the explicit
// k <= 64 solve (2.33 vs 2.26 ms/iter), the explicit rank-128 light rows (user launch
// 112 vs 102 ms) and the n x n dual systems (76 vs 70 ms) is slower: fp32 stays there.

// fp32 form: acc += X^T Y (the MFMA's k index is permuted to 4q + s4).
__device__ __forceinline__ floatx4 tile_xty(const floatx4& X, const floatx4& Y, floatx4 acc) {
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(X[s4], Y[s4], acc, 0, 0, 0);
  return acc;
}

// [hi | lo] f16 halves of s * x (s a power of two): hi = f16(s x) and
// lo = f16(s x - hi), each one v_fma_mix (the fp32 fma inside is exact).
__device__ __forceinline__ half8v split_hl(const floatx4& x, float s) {
  uint32_t h01, h23, l01, l23;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "=v"(h01) : "v"(x[0]), "v"(s));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "+v"(h01) : "v"(x[1]), "v"(s));
  asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "=v"(h23) : "v"(x[2]), "v"(s));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "+v"(h23) : "v"(x[3]), "v"(s));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]"
      : "=v"(l01) : "v"(x[0]), "v"(s), "v"(h01));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "+v"(l01) : "v"(x[1]), "v"(s), "v"(h01));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]"
      : "=v"(l23) : "v"(x[2]), "v"(s), "v"(h23));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "+v"(l23) : "v"(x[3]), "v"(s), "v"(h23));
  return __builtin_bit_cast(half8v, make_uint4(h01, h23, l01, l23));
}
__device__ __forceinline__ half8v dup_hi(const half8v& v) {
  return __builtin_shufflevector(v, v, 0, 1, 2, 3, 0, 1, 2, 3);
}
__device__ __forceinline__ half8v dup_lo(const half8v& v) {
  return __builtin_shufflevector(v, v, 4, 5, 6, 7, 4, 5, 6, 7);
}

// NB = 8 (rank 65-128, W1 kernels), 4 (rank 33-64, explicit gram_solve_kernel) or
// 2 / 4 (the n x n dual systems of short rows, gram_solve_dual_kernel).  Returns
// whether every pivot was positive and the solution finite; xcol[c] on lane (q, m)
// = solution entry of variable (block c, index m), every row group q.
// FULL: k == 16 NB is known at compile time (no padded dims: every test of a dim against k
// folds away) and the diagonal blocks take the lean sweep.
template <int NB, bool SPLIT = kW1SplitSchur<NB>, bool FULL = false>
__device__ __forceinline__ bool w1_solve_x(floatx4 (&A)[NB * (NB + 1) / 2], float (&bcol)[NB],
                                           float* __restrict__ lds, int k, float (&xcol)[NB],
                                           float cond_max = kCondMax) {
  using L = W1LdsT<NB>;
  constexpr int CS = L::CS;
  const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
  float* col = lds + L::COL;
  float* vec = lds + L::VEC;
  float zcol[NB];
  float dmin = 3.0e38f;
  // this lane's pivots of real dims (its column m of every block: dim m * NB + K < k)
  float rmin = 3.0e38f, rmax = 0.f;
  auto track_pivot = [&](float ds, bool real) {
    rmin = real ? fminf(rmin, ds) : rmin;
    rmax = real ? fmaxf(rmax, ds) : rmax;
  };
  if constexpr (SPLIT) {
    // scale the system by 2^g: largest diagonal entry (= largest entry) -> [2^13, 2^14)
    float dm = 0.f;
    static_for<NB>([&](auto cc) { dm = fmaxf(dm, absmax4(A[w1_tile<NB>(cc, cc)])); });
    const float sg = ldexpf(1.f, split_exponent(wave_max(dm)) - 1);
#pragma unroll
    for (int t = 0; t < NB * (NB + 1) / 2; ++t) A[t] *= sg;
#pragma unroll
    for (int c = 0; c < NB; ++c) bcol[c] *= sg;
    if (k < NB * 16) {
      // padded dims' identity rows -> 2^13 I: a unit pivot far below the scaled
      // system would put -1/pivot at the top of Gm's range and flush its real
      // entries out of the split (x_pad stays 0: b_pad = 0, no coupling)
      static_for<NB>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * q + r == m && m * NB + c >= k) A[w1_tile<NB>(c, c)][r] = 8192.f;
      });
    }
  }
  // bcol[J] for J > 0 holds per-row-group partial sums (summed over the groups when
  // block J becomes the pivot block): start with the full b_J in row group 0
#pragma unroll
  for (int c = 1; c < NB; ++c) bcol[c] = q == 0 ? bcol[c] : 0.f;
  // Sweep block K from its tile (C layout -> column per lane through LDS), running
  // `hook` between pivots; then Gm_K (C layout) and b_K (row layout).
  floatx4 Gm, bk;
  auto pivot_block = [&](auto Kc, auto&& hook) {
    constexpr int K = decltype(Kc)::value;
    if constexpr (kSweepC<NB, SPLIT>) {
      // swept in the C layout: Gm comes out where the MFMAs read it
      Gm = A[w1_tile<NB>(K, K)];
      float ds;
      dmin = fminf(dmin, sweep16c<NB == 8, FULL>(Gm, hook, ds));
      track_pivot(ds, FULL || m * NB + K < k);
      const float bK = K == 0 ? bcol[0] : reduce_rows4(bcol[K]);  // partials -> b_K[m]
      if (q == 0) vec[m] = bK;
      wave_lds_order();
      bk = *reinterpret_cast<const floatx4*>(vec + 4 * q);  // row layout
      wave_lds_order();
      return;
    }
    *reinterpret_cast<floatx4*>(col + m * CS + 4 * q) = A[w1_tile<NB>(K, K)];
    wave_lds_order();
    float R[16];
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      const floatx4 v = *reinterpret_cast<const floatx4*>(col + m * CS + 4 * c4);
      R[4 * c4] = v[0]; R[4 * c4 + 1] = v[1]; R[4 * c4 + 2] = v[2]; R[4 * c4 + 3] = v[3];
    }
    float ds;
    dmin = fminf(dmin, sweep16(R, hook, ds));
    track_pivot(ds, m * NB + K < k);
    wave_lds_order();
    const float bK = K == 0 ? bcol[0] : reduce_rows4(bcol[K]);  // partials -> b_K[m]
    if (q == 0) {
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4)
        *reinterpret_cast<floatx4*>(col + m * CS + 4 * c4) =
            floatx4{R[4 * c4], R[4 * c4 + 1], R[4 * c4 + 2], R[4 * c4 + 3]};
      vec[m] = bK;
    }
    wave_lds_order();
    Gm = *reinterpret_cast<const floatx4*>(col + m * CS + 4 * q);  // C layout
    bk = *reinterpret_cast<const floatx4*>(vec + 4 * q);           // row layout
    wave_lds_order();
  };
  // step-K operands of the split form: block row K ([hi|lo] of sK A_KJ), Pm halves
  half8v XK[NB], Ph[NB], Pl[NB];
  auto schur = [&](auto Kc, auto uc, const floatx4 (&Pm)[NB]) {
    constexpr int K = decltype(Kc)::value, u = decltype(uc)::value;
    constexpr int I = schur_I<NB>(K, u), J = schur_J<NB>(K, u);
    floatx4& C = A[w1_tile<NB>(I, J)];
    if constexpr (SPLIT) {
      // C += (2^a X)^T (2^-a Pm): lo halves of Pm first, then the hi halves
      C = __builtin_amdgcn_mfma_f32_16x16x32_f16(XK[I - K - 1], Pl[J - K - 1], C, 0, 0, 0);
      C = __builtin_amdgcn_mfma_f32_16x16x32_f16(XK[I - K - 1], Ph[J - K - 1], C, 0, 0, 0);
    } else {
      C = tile_xty(A[w1_tile<NB>(K, I)], Pm[J - K - 1], C);
    }
  };
  pivot_block(std::integral_constant<int, 0>{}, [](auto) {});
  static_for<NB>([&](auto Kc) {
    constexpr int K = decltype(Kc)::value;
    // z_K = -Gm b_K  (Gm symmetric: (Gm b)[i] = sum_k Gm[k][i] b[k])
    zcol[K] = -reduce_rows4(Gm[0] * bk[0] + Gm[1] * bk[1] + Gm[2] * bk[2] + Gm[3] * bk[3]);
    if constexpr (K + 1 < NB) {
      // Pm_J = Gm B_KJ;  b_J += Pm_J^T b_K (per-row-group partials)
      floatx4 Pm[NB];
      if constexpr (SPLIT) {
        // block row K's scale; Pm_J = Gm^T A_KJ on split f16
        float mx = 0.f;
        static_for<NB - 1 - K>([&](auto jc) {
          mx = fmaxf(mx, absmax4(A[w1_tile<NB>(K, K + 1 + decltype(jc)::value)]));
        });
        const int eX = split_exponent(wave_max(mx));
        float mp = 0.f;
        static_for<NB - 1 - K>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          XK[j] = split_hl(A[w1_tile<NB>(K, K + 1 + j)], ldexpf(1.f, eX));
        });
        const int eG = split_exponent(wave_max(absmax4(Gm)));
        const half8v g = split_hl(Gm, ldexpf(1.f, eG));
        const half8v gh = dup_hi(g), gl = dup_lo(g);
        const float invGX = ldexpf(1.f, -eG - eX);
        static_for<NB - 1 - K>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          // Gm^T X = [Gl|Gl]^T [Xh|Xl] + [Gh|Gh]^T [Xh|Xl]
          floatx4 acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(gl, XK[j],
                                                              floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh, XK[j], acc, 0, 0, 0) * invGX;
          Pm[j] = acc;
          bcol[K + 1 + j] += acc[0] * bk[0] + acc[1] * bk[1] + acc[2] * bk[2] + acc[3] * bk[3];
          mp = fmaxf(mp, absmax4(acc));
        });
        // Schur operands 2^a X and 2^-a Pm: a balances the two maxima (both at
        // 2^((x + p) / 2)), clamped so neither exceeds 2^15
        const int eP = split_exponent(wave_max(mp));
        const int a = min(max((eX - eP) >> 1, -eP), eX);
        static_for<NB - 1 - K>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          XK[j] = split_hl(A[w1_tile<NB>(K, K + 1 + j)], ldexpf(1.f, a));
          const half8v p = split_hl(Pm[j], ldexpf(1.f, -a));
          Ph[j] = dup_hi(p);
          Pl[j] = dup_lo(p);
        });
      } else {
        static_for<NB - 1 - K>([&](auto jc) {
          constexpr int J = K + 1 + decltype(jc)::value;
          const floatx4 acc = tile_xty(Gm, A[w1_tile<NB>(K, J)], floatx4{0.f, 0.f, 0.f, 0.f});
          Pm[decltype(jc)::value] = acc;
          bcol[J] += acc[0] * bk[0] + acc[1] * bk[1] + acc[2] * bk[2] + acc[3] * bk[3];
        });
      }
      // Pm of block row K -> LDS for the back substitution (lane-private slots)
      static_for<NB - 1 - K>([&](auto jc) {
        constexpr int J = K + 1 + decltype(jc)::value;
        *reinterpret_cast<floatx4*>(lds + L::PM + (w1_tile<NB>(K, J) - (K + 1)) * 256 + 4 * lane) =
            Pm[decltype(jc)::value];
      });
      // the next pivot block's Schur update first, then its sweep with the rest of
      // step K's Schur updates (independent of it) issued between the pivots
      schur(Kc, std::integral_constant<int, 0>{}, Pm);
      pivot_block(std::integral_constant<int, K + 1>{}, [&](auto pc) {
        constexpr int p = decltype(pc)::value;
        static_for<schur_n<NB>(K) - 1>([&](auto vc) {
          constexpr int u = 1 + decltype(vc)::value;
          if constexpr ((u - 1) % 16 == p) schur(Kc, std::integral_constant<int, u>{}, Pm);
        });
      });
    }
  });
  // back substitution x_K = z_K + sum_{J>K} Pm_KJ x_J (column layout)
  xcol[NB - 1] = zcol[NB - 1];
  static_for<NB - 1>([&](auto kc) {
    constexpr int K = NB - 2 - decltype(kc)::value;
    float pr[4] = {0.f, 0.f, 0.f, 0.f};
    static_for<NB - 1 - K>([&](auto jc) {
      constexpr int J = K + 1 + decltype(jc)::value;
      const floatx4 pm = *reinterpret_cast<const floatx4*>(
          lds + L::PM + (w1_tile<NB>(K, J) - (K + 1)) * 256 + 4 * lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) pr[r] = fmaf(pm[r], xcol[J], pr[r]);
    });
#pragma unroll
    for (int r = 0; r < 4; ++r) pr[r] = reduce_lanes16(pr[r]);  // rows 4q+r of Pm x
    if (m == 0) *reinterpret_cast<floatx4*>(vec + 4 * q) = floatx4{pr[0], pr[1], pr[2], pr[3]};
    wave_lds_order();
    xcol[K] = zcol[K] + vec[m];
    wave_lds_order();
  });
  // a NaN pivot (or overflow) leaves a non-finite solution; a pivot spread beyond
  // kCondMax (a lower bound on cond(A)) is outside what the fp32 solve can hold to the
  // 1e-4 bar: the row is re-solved in fp64 (rescue64_kernel)
  bool fin = true;
#pragma unroll
  for (int c = 0; c < NB; ++c) fin = fin && (xcol[c] - xcol[c] == 0.f);
  // spread over the 16 lanes of a row group (every row group holds the same pivots)
  rmin = fminf(rmin, dpp_f<0xB1>(rmin));
  rmax = fmaxf(rmax, dpp_f<0xB1>(rmax));
  rmin = fminf(rmin, dpp_f<0x4E>(rmin));
  rmax = fmaxf(rmax, dpp_f<0x4E>(rmax));
  rmin = fminf(rmin, dpp_f<0x141>(rmin));
  rmax = fmaxf(rmax, dpp_f<0x141>(rmax));
  rmin = fminf(rmin, dpp_f<0x140>(rmin));
  rmax = fmaxf(rmax, dpp_f<0x140>(rmax));
  return dmin > 0.f && rmin > 0.f && rmax <= cond_max * rmin && __ballot(!fin) == 0;
}

// w1_solve_x, then the solution row written un-permuted: dim d = i * NB + c <->
// block c, index i = lane m; dims in [k, ld) written as zero.
template <int NB, bool SPLIT = kW1SplitSchur<NB>, bool FULL = false>
__device__ __forceinline__ bool w1_solve(floatx4 (&A)[NB * (NB + 1) / 2], float (&bcol)[NB],
                                         float* __restrict__ lds, int k,
                                         float* __restrict__ xrow, int ld,
                                         float cond_max = kCondMax) {
  float xcol[NB];
  const bool ok = w1_solve_x<NB, SPLIT, FULL>(A, bcol, lds, k, xcol, cond_max);
  const int lane = threadIdx.x & 63, m = lane & 15;
  if (lane < 16) {
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      const int d = m * NB + c;
      if constexpr (FULL) xrow[d] = ok ? xcol[c] : 0.f;  // d < k = 16 NB <= ld
      else if (d < ld) xrow[d] = (d < k && ok) ? xcol[c] : 0.f;
    }
  }
  // a caller's ld may exceed k_pad = 16 NB (any ld >= k is allowed): those columns too
  for (int d = 16 * NB + lane; d < ld; d += 64) xrow[d] = 0.f;
  return ok;
}

// ---------------------------------------------------------------------------
// W1 kernels (k in (64, 128], one wavefront per system).  The 36 scaled Gram
// tiles are finished in place, tile by tile (regularisation, implicit YtY from
// a C-layout fp32 table, identity rows for padded dims), so the register file
// holds one copy of the system.  Heavy-row chunk partials are stored as fp32
// (a chunk's sum is fp32 anyway) and summed in fp64 in launch 2, where the YtY
// merge is done in fp64 before the single rounding.
// ---------------------------------------------------------------------------
constexpr int kW1NT = 36;
constexpr int kW1Slot = (kW1NT * 4 + kW1NB + 1) * 64;  // floats per chunk partial
constexpr int kW1YtyC = kW1NT * 4 * 64;               // floats of the C-layout YtY table
// Implicit W1 light rows: the C-layout YtY table is copied into the wave's LDS by
// LDS-DMA when the row starts (36 KB, landing while the Gram accumulates), past the
// Gram's 192-word staging area; the solve's LDS (W1Lds, written only after the table
// has been read) overlaps it.  Read from global at the end instead, the compiler
// spread the 144 loads per lane over ~20 dependent waits — at one wavefront per SIMD,
// each an unhidden L2 round trip.  4 x 37.9 KB per CU (one wave per SIMD).
constexpr int kW1YtyLdsOff = 1024;  // bytes
constexpr int kW1SmemImplicit =
    (kW1YtyLdsOff + 4 * kW1YtyC) > (int)sizeof(float) * W1Lds::SIZE ? (kW1YtyLdsOff + 4 * kW1YtyC)
                                                                    : (int)sizeof(float) * W1Lds::SIZE;
static_assert(kW1YtyC % 256 == 0, "YtY table in 1 KB LDS-DMA pieces");

// Completes the normal equations of one system in place and solves them.  A holds
// the Gram divided by `scale` (the split MFMA's power-of-two scaling, 1 for the
// reduced heavy rows); instead of rescaling 144 registers, the system is solved
// in that scale: (A + (lambda n / scale) I) x = b / scale  (+ YtY / scale for
// implicit, from the C-layout table).  Padded dims (k < 128) become identity
// rows/columns.  bt: per-lane rhs partials (summed over the 4 rating slots here).
template <bool ADD_YTY, int NB = kW1NB, bool SPLIT = kW1SplitSchur<NB>, bool FULL = false>
__device__ __forceinline__ void w1_finish_and_solve(floatx4 (&A)[NB * (NB + 1) / 2],
                                                    float scale, float (&bt)[NB], int64_t n_reg,
                                                    const float* __restrict__ ytyC,
                                                    unsigned char* smem, int k, float reg,
                                                    float* __restrict__ xrow, int ld, int row,
                                                    RescueList rl, float cond_max = kCondMax) {
  constexpr int NT_ = NB * (NB + 1) / 2;
  const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
  // power of two: exact (FULL: from the exponent, not an IEEE division's dozen VALU)
  const float inv = FULL ? ldexpf(1.f, 1 - __builtin_amdgcn_frexp_expf(scale)) : 1.f / scale;
  float bq[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const float v = reduce_rows4(bt[c]) * inv;
    bq[c] = (FULL || m * NB + c < k) ? v : 0.f;
  }
  const float lam = (float)((double)reg * (double)n_reg) * inv;
  if constexpr (ADD_YTY) {
    static_for<NT_>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
#pragma unroll
      for (int r = 0; r < 4; ++r) A[t][r] = fmaf(ytyC[(t * 4 + r) * 64 + lane], inv, A[t][r]);
    });
  }
  if (FULL || k == NB * 16) {  // uniform: no padded dims, lambda on the diagonal only
    static_for<NB>([&](auto cc) {
      constexpr int c = decltype(cc)::value;
      constexpr int t = w1_tile<NB>(c, c);
#pragma unroll
      for (int r = 0; r < 4; ++r) A[t][r] += (4 * q + r == m) ? lam : 0.f;
    });
  } else {
    static_for<NT_>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      constexpr int c1 = FullTiles<NB>::l1(t), c2 = FullTiles<NB>::l2(t);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i, j;
        tile_ij<NB>(c1, c2, r, i, j);
        const bool pad = (i >= k) | (j >= k);
        float v = pad ? 0.f : A[t][r];
        if constexpr (c1 == c2) v = (i == j) ? (pad ? 1.f : v + lam) : v;
        A[t][r] = v;
      }
    });
  }
  const bool ok =
      w1_solve<NB, SPLIT, FULL>(A, bq, reinterpret_cast<float*>(smem), k, xrow, ld, cond_max);
  if (!ok) rescue_append(rl, row);  // re-solved in fp64
}

}  // namespace als
