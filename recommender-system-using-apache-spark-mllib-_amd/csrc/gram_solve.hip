// K2 + K3 (+ K2b) — normal equations and Cholesky solve for one ALS half-sweep.
//
// Replaces, per dst row j (Spark ml/recommendation/ALS.scala, upstream):
//   computeFactors -> NormalEquation.add   (blas.dspr + blas.daxpy, fp64)
//                  -> CholeskySolver.solve (ata += lambda*n on the diagonal,
//                                           LAPACK dppsv "U", fp64, result -> Float)
//   computeYtY (implicit)                  (dspr over all src rows + treeAggregate)
// reached from ALS.train at RecommenderSystem.py:148-149, :163, :218.
//
// MI355X design:
//  * A task is a whole "light" row (<= chunk ratings, default 2048) or one
//    2048-rating chunk of a heavy row; light rows arrive longest-first (LPT).
//    k <= 64: one wavefront per task (gram_solve_kernel<CN>); 64 < k <= 128: one
//    wavefront per task with the whole 128 x 128 system in its registers
//    (gram_solve_w1_kernel, "W1").  One code path per (k range, implicit).
//  * Gram on the f16 matrix cores with fp32-grade products: every operand t is
//    carried as hi = f16_rn(t), lo = f16_rn(t - hi) after a power-of-two scale
//    (largest |t| in [2^14, 2^15), from max |Y| and max |r| computed on the
//    device), and each 16 x 16 tile accumulates hi.hi + hi.lo + lo.hi with three
//    v_mfma_f32_16x16x32_f16 per 32 ratings (~2^-21 relative per product).
//    MFMA K = rating index; lane (q, m) holds ratings 8q..8q+7 of a step and dims
//    m*CN .. m*CN+CN-1, so only the CN(CN+1)/2 upper tiles of the dim-permuted
//    Gram are computed (Spark's packed dspr uses the same symmetry).
//    Explicit: Y is pre-split once per half-sweep into hi|lo words
//    (split_table_kernel) and the rhs runs on the matrix cores; implicit: the
//    fp32 rows are split in registers after the per-rating weight, whose
//    sqrt(alpha |r|) and (1 + alpha |r|) are computed once per rating when the
//    64-rating block is staged in LDS.
//  * Accumulation: fp32 within a task (<= 2048 ratings; test_gpu_configs pins
//    the error at the production chunk), fp64 across a heavy row's chunks
//    (partial slots summed element-wise in a fixed order, deterministic).
//  * Normal equations as CholeskySolver.solve: A_ii += lambda * n (n = #ratings,
//    implicit: #ratings > 0), implicit YtY merged in fp64 before the one
//    rounding to fp32; padded dims get identity rows and zero rhs.
//  * Solve (fp32, same solution as Spark's dppsv): k <= 32 column-per-lane panel
//    LDL^T with the trailing tiles on fp32 MFMA; k in (32, 64] and (64, 128]:
//    block elimination with 16 x 16 diagonal inverses by the sweep operator
//    (VALU, DPP broadcasts) and the Pm / Schur products on the matrix cores —
//    split f16 (fp32-grade) for rank 65-128 implicit light rows and heavy rows,
//    fp32 MFMA for the explicit light rows and rank <= 64 (see w1_solve).
//  * YtY (K2b): 512-row tasks of the same MFMA Gram, fp64 slots, parallel slot
//    sum, fixed order.
#include "als_common.h"
#include "dual_solve.h"
#include "gram_accumulate.h"
#include "panel_solve.h"
#include "partial_slots.h"
#include "rescue64.h"
#include "solve_config.h"
#include "solve_guards.h"
#include "task_order.h"
#include "w1_solve.h"

#include <algorithm>

namespace als {

// Launch-1 task t -> heavy-row chunk or light row: the two lists interleaved
// while both last (memory-bound Gram-only chunks beside VALU-heavy fused
// solves), each in its own LPT order.  (The implicit and W1 launches; the rank
// 33-64 explicit launch spreads the chunks through the light list instead:
// decode_task_merged, task_order.h.)
__device__ __forceinline__ void decode_task(int t, int n_chunks, int n_light, int& chunk,
                                            int& light) {
  const int P = n_chunks < n_light ? n_chunks : n_light;
  chunk = -1;
  light = -1;
  if (t < 2 * P) {
    if (t & 1) light = t >> 1;
    else chunk = t >> 1;
  } else if (n_chunks > P) {
    chunk = t - P;
  } else {
    light = t - P;
  }
}

template <int CN, bool IMPLICIT = false>
struct SmemBytes {
  static constexpr int value =
      (int)sizeof(float) * (IMPLICIT ? IrLds<CN>::SIZE : PanelLds<CN>::SIZE);
};
template <bool IMPLICIT>
struct SmemBytes<8, IMPLICIT> {  // W1: transposition buffer (the Gram's 192-word staging fits in it)
  static constexpr int value = (int)sizeof(float) * W1Lds::SIZE;
};

// LDS of launch 1 (gram_solve_kernel): as SmemBytes, except that the explicit
// rank 33-64 rows are solved by the W1 block elimination, never by the panel solve
// (launch 2, reduce_solve_kernel<4, false>, runs the panel solve and keeps SmemBytes).
// They touch the Gram's staging words (columns | rating words), then W1LdsT<4>.
// At most 10,240 B: 16 one-wave workgroups per CU (four waves per SIMD) fit in 160 KiB.
constexpr int kPreStageWords = 128;
template <int CN, bool IMPLICIT>
struct FusedSmemBytes : SmemBytes<CN, IMPLICIT> {};
template <>
struct FusedSmemBytes<4, false> {
  static constexpr int value =
      (int)sizeof(float) * (W1LdsT<4>::SIZE > kPreStageWords ? W1LdsT<4>::SIZE : kPreStageWords);
  static_assert(value >= (int)sizeof(float) * W1LdsT<4>::SIZE &&
                    value >= (int)sizeof(float) * kPreStageWords && value % 16 == 0,
                "rank 33-64 explicit: Gram staging and W1<4> solve");
  static_assert(value <= 10240, "rank 33-64 explicit: 16 workgroups per CU");
};
// Waves per SIMD the launch-1 kernel is compiled for.  Rank 33-64 explicit: a row is a
// latency chain (gathers, then 64 dependent pivots), covered by rows in flight, so it
// is held to the 128 registers of four waves (one rhs tile, see RhsTiles).
template <int CN, bool IMPLICIT>
constexpr int kFusedWaves = IMPLICIT ? 2 : (CN == 4 ? 4 : 3);
// Rank 33-64 explicit keeps its rhs sums in one accumulator tile.
template <int CN>
constexpr bool kOneRhsTile = CN == 4;

// Launch 1 of a half-sweep: heavy-row chunks (-> fp64 partial slots) and
// whole light rows (Gram + solve fused, A never leaves the CU), interleaved.
// Gram on the split f16 MFMA, fp32 accumulation over a task (<= chunk
// ratings), fp64 across the chunks of a heavy row.  scal[0] = max |Y_src|,
// scal[1] = max |rating| (prep phase).  Explicit: Gram and rhs from the split
// table Ysp (kp words per row, zero row `zero_row`); implicit: from Y, split in
// registers after the per-rating confidence weight.
// (k <= 64 keeps one gather step in flight: two steps need 187 registers, i.e. two
// waves per SIMD instead of three, measured slower on configs[1]: 2.07 -> 2.24 ms/iter.)
// (Four waves per SIMD for explicit k <= 64 with CN rhs tiles spill 49 registers: 2.76 vs
// 2.25 ms/iter; round 5, after the lean sweep, 11 spills: 2.14 vs 2.02 ms/iter,
// profiles/r05/ab_occupancy.jsonl, both at the panel's 12,288 B of LDS, i.e. still
// three waves.  Rank 33-64 now fits four without spills: profiles/r09/occupancy4.md.)
//
// CNP = CN, the rank's 16-dim blocks — or -4 for explicit ranks 33-63.  The explicit
// CN = 4 instantiation proper, gram_solve_kernel<4, false>, is FULL: the host launches it
// at rank 64 only, where k = k_pad = 16 CN is known at compile time.  The user launch of
// the rank-64 iteration is bound by VALU issue (profiles/r09/occupancy4.md section 4), and a
// good part of a light row's VALU instructions outside the Gram loop only masked padded
// dims that a full rank does not have, or copied tiles around the k == k_pad branch; with
// FULL they are not compiled, and the diagonal blocks take the lean sweep
// (profiles/r10/valu_trim.md).  Ranks 33-63 keep the run-time masks: <-4, false>.
constexpr int kCnPadded64 = -4;
template <int CNP, bool IMPLICIT>
__global__ __launch_bounds__(64, (kFusedWaves<(CNP < 0 ? -CNP : CNP), IMPLICIT>)) void gram_solve_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, const int32_t* __restrict__ light_rows,
    const int32_t* __restrict__ chunk_row, const int64_t* __restrict__ chunk_begin,
    const int64_t* __restrict__ chunk_end, int32_t n_chunks, int32_t n_light,
    const float* __restrict__ Y, float* __restrict__ X, int ld, int k_arg, float reg, float alpha,
    const double* __restrict__ yty, float* __restrict__ slots, int32_t* __restrict__ status,
    const float* __restrict__ scal, const uint32_t* __restrict__ Ysp, int32_t kp,
    int32_t zero_row, RescueList rl) {
  constexpr int CN = CNP < 0 ? -CNP : CNP;
  constexpr bool FULL = !IMPLICIT && CNP == 4;
  static_assert(CNP > 0 || (CNP == kCnPadded64 && !IMPLICIT), "-4: explicit ranks 33-63 only");
  __shared__ __attribute__((aligned(16))) unsigned char smem[FusedSmemBytes<CN, IMPLICIT>::value];
  constexpr int NT = Cfg<CN>::NT;
  const int k = FULL ? 16 * CN : k_arg;
  floatx4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  float tot[NT][4], bt[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) bt[c] = 0.f;
  int npos = 0;
  int chunk, light;
  // rank 33-64 explicit: chunks and the longest light rows spread through the light
  // list (task_order.h); the other instantiations were not measured with it
  if constexpr (!IMPLICIT && CN == 4) decode_task_merged(blockIdx.x, n_chunks, n_light, chunk, light);
  else decode_task(blockIdx.x, n_chunks, n_light, chunk, light);
  int64_t pb, pe;
  int row = -1;
  if (chunk >= 0) {
    pb = chunk_begin[chunk];
    pe = chunk_end[chunk];
  } else {
    row = light_rows[light];
    pb = row_ptr[row];
    pe = row_ptr[row + 1];
  }
  float inv2;
  float rmax = 0.f;  // explicit: this lane's max |rating| (split window guard)
  if constexpr (IMPLICIT) {
    const int e = split_exponent(scal[0] * __builtin_sqrtf(alpha * scal[1]));
    inv2 = ldexpf(1.f, -2 * e);
    gram_accumulate_split<CN, true>(col, val, pb, pe, Y, ld, k, alpha, ldexpf(1.f, e), acc, bt,
                                    npos, reinterpret_cast<int*>(smem));
  } else {
    const int ey = split_exponent(scal[0]), er = split_exponent(scal[1]);
    inv2 = ldexpf(1.f, -2 * ey);
    constexpr bool ONE = kOneRhsTile<CN>;
    constexpr int NRT = RhsTiles<FullTiles<CN>, ONE>::N;
    floatx4 accb[NRT];
#pragma unroll
    for (int c = 0; c < NRT; ++c) accb[c] = floatx4{0.f, 0.f, 0.f, 0.f};
    gram_accumulate_pre<FullTiles<CN>, ONE>(col, val, pb, pe, Ysp, (uint32_t)kp, zero_row,
                                            ldexpf(1.f, er), (threadIdx.x & 15) * CN, acc, accb,
                                            reinterpret_cast<int*>(smem), rmax);
    rhs_from_tiles<FullTiles<CN>, ONE>(accb, ldexpf(1.f, -ey - er), bt);
    rmax *= ldexpf(1.f, er);
    if (chunk < 0 && (window_miss(diag_max_lane<CN>(acc), (float)(pe - pb), rmax) ||
                      rank_deficient_illcond<CN>(acc, inv2, pe - pb, k, reg))) {
      rescue_append(rl, row);
      return;
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) tot[t][r] = acc[t][r] * inv2;
  if (chunk >= 0) {
    // explicit: the npos entry carries the chunk's scaled max |rating| (launch 2 takes
    // the max over the chunks for the window guard)
    store_slot<NT, CN>(slots + (int64_t)chunk * Cfg<CN>::SLOT, tot, bt,
                           IMPLICIT ? (float)npos : rmax);
    return;
  }
  __syncthreads();  // staging area is reused by the solve
  const int64_t n_reg = IMPLICIT ? (int64_t)npos : (pe - pb);
  if constexpr (!IMPLICIT && CN == 4) {
    // rank 33-64 explicit: the W1 block elimination on 4 x 4 tiles (swept diagonal
    // inverses + fp32 MFMA), in the Gram's scale
    static_assert((int)sizeof(float) * W1LdsT<4>::SIZE <= FusedSmemBytes<4, false>::value,
                  "W1<4> LDS");
    w1_finish_and_solve<false, 4, false, FULL>(acc, inv2, bt, n_reg, nullptr, smem, k, reg,
                                               X + (int64_t)row * ld, ld, row, rl);
  } else {
    finish_and_solve<CN, IMPLICIT, float>(tot, bt, n_reg, smem, k, reg, yty,
                                          X + (int64_t)row * ld, ld, row, rl,
                                          IrArgs{col, val, Y, pb, pe, alpha});
  }
}

__device__ __forceinline__ void block_absmax_publish(float m, unsigned* __restrict__ out) {
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(out, __float_as_uint(m));  // NaN-free non-negative floats order as uints
  }
}

// max |rating| of a CSR block (ratings val[0, row_ptr[n_rows])) -> *out.
__global__ __launch_bounds__(256) void absmax_csr_kernel(const int64_t* __restrict__ row_ptr,
                                                         int32_t n_rows,
                                                         const float* __restrict__ val,
                                                         unsigned* __restrict__ out) {
  const int64_t n = row_ptr[n_rows];
  float m = 0.f;
  const int64_t n4 = n >> 2;  // val is 16-byte aligned (a CSR value array)
  const float4* v4 = reinterpret_cast<const float4*>(val);
  auto fold = [&](const float4& v) {
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  };
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {  // four independent loads in flight
    const float4 a = v4[i], b = v4[i + stride], c = v4[i + 2 * stride], d = v4[i + 3 * stride];
    fold(a);
    fold(b);
    fold(c);
    fold(d);
  }
  for (; i < n4; i += stride) fold(v4[i]);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = fmaxf(m, fabsf(val[4 * n4 + threadIdx.x]));
  block_absmax_publish(m, out);
}

// max |x| over n floats -> *out (as ordered uint bits; *out zeroed beforehand).
// (zero_word[0..1], when given, are cleared by block 0: the rescue count and its
// finished-block counter for the half-sweep this prep starts, without a memset)
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, int64_t n,
                                                     unsigned* __restrict__ out,
                                                     unsigned* __restrict__ zero_word) {
  if (zero_word != nullptr && blockIdx.x == 0 && threadIdx.x < 2) zero_word[threadIdx.x] = 0u;
  float m = 0.f;
  const int64_t n4 = n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  auto fold = [&](const float4& v) {
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  };
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {  // four independent loads in flight
    const float4 a = x4[i], b = x4[i + stride], c = x4[i + 2 * stride], d = x4[i + 3 * stride];
    fold(a);
    fold(b);
    fold(c);
    fold(d);
  }
  for (; i < n4; i += stride) fold(x4[i]);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = fmaxf(m, fabsf(x[4 * n4 + threadIdx.x]));
  block_absmax_publish(m, out);
}

// Launch 2: heavy rows — sum their chunk slots in a fixed order (fp64), then solve.
template <int CN, bool IMPLICIT>
__global__ __launch_bounds__(64, 2) void reduce_solve_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, const float* __restrict__ Y, float alpha,
    const int32_t* __restrict__ heavy_rows, const int32_t* __restrict__ slot_begin,
    const int32_t* __restrict__ slot_begin2, const float* __restrict__ slots,
    float* __restrict__ X, int ld, int k, float reg, const double* __restrict__ yty,
    int32_t* __restrict__ status, const float* __restrict__ scal,
    RescueList rl) {
  constexpr int NT = Cfg<CN>::NT;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SmemBytes<CN, IMPLICIT>::value];
  const int h = blockIdx.x;
  const int row = heavy_rows[h];
  double a64[NT][4], b64[CN];
  zero_acc<NT, CN, double>(a64, b64);
  int npos = 0;
  // the row's chunk slots were summed into its home slot (heavy_sum_f64_kernel)
  const float* sl =
      slots + (int64_t)slot_range(slot_begin, slot_begin2, h).home() * Cfg<CN>::SLOT;
  add_slot<NT, CN>(sl, a64, b64, npos);
  const int64_t n_reg = IMPLICIT ? (int64_t)npos : (row_ptr[row + 1] - row_ptr[row]);
  if constexpr (!IMPLICIT) {  // split window guard over the whole row
    const float s2 = ldexpf(1.f, 2 * split_exponent(scal[0]));
    float d = 0.f;
    const int lane = threadIdx.x & 63, q = lane >> 4, m = lane & 15;
#pragma unroll
    for (int c = 0; c < CN; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * q + r == m) d = fmaxf(d, (float)a64[tile_index(CN, c, c)][r] * s2);
    if (window_miss(d, (float)n_reg, (float)sl[(NT * 4 + CN) * 64 + lane])) {
      rescue_append(rl, row);
      return;
    }
  }
  finish_and_solve<CN, IMPLICIT, double>(a64, b64, n_reg, smem, k, reg, yty,
                                         X + (int64_t)row * ld, ld, row, rl,
                                         IrArgs{col, val, Y, row_ptr[row], row_ptr[row + 1],
                                                alpha});
}

// ytyC[(t * 4 + r) * 64 + lane] = fp32 YtY entry of register r of upper tile t.
__global__ __launch_bounds__(64) void yty_ctab_kernel(const double* __restrict__ yty,
                                                      float* __restrict__ ytyC) {
  static_for<kW1NT>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    constexpr int c1 = FullTiles<8>::l1(t), c2 = FullTiles<8>::l2(t);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i, j;
      tile_ij<8>(c1, c2, r, i, j);
      const int hi = i > j ? i : j, lo = i > j ? j : i;
      ytyC[(t * 4 + r) * 64 + threadIdx.x] = (float)yty[hi * (hi + 1) / 2 + lo];
    }
  });
}

// Launch 1 (W1): heavy-row chunks (-> fp32 partial slots) and whole light rows
// (Gram + solve fused), as gram_solve_kernel.  ytyC: C-layout YtY (implicit).
template <bool IMPLICIT>
__global__ __launch_bounds__(64, 1) void gram_solve_w1_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, const int32_t* __restrict__ light_rows,
    const int64_t* __restrict__ chunk_begin, const int64_t* __restrict__ chunk_end,
    int32_t n_chunks, int32_t n_light, const float* __restrict__ Y, float* __restrict__ X, int ld,
    int k, float reg, float alpha, const float* __restrict__ ytyC, float* __restrict__ slots,
    int32_t* __restrict__ status, const float* __restrict__ scal, const uint32_t* __restrict__ Ysp,
    int32_t kp, int32_t zero_row, RescueList rl) {
  constexpr int CN = 8, NT = kW1NT;
  __shared__ __attribute__((aligned(16))) unsigned char smem[IMPLICIT ? kW1SmemImplicit
                                                                      : SmemBytes<CN>::value];
  const int lane = threadIdx.x & 63;
  floatx4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bt[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) bt[c] = 0.f;
  int npos = 0;
  int chunk, light;
  decode_task(blockIdx.x, n_chunks, n_light, chunk, light);
  int64_t pb, pe;
  int row = -1;
  if (chunk >= 0) {
    pb = chunk_begin[chunk];
    pe = chunk_end[chunk];
  } else {
    row = light_rows[light];
    pb = row_ptr[row];
    pe = row_ptr[row + 1];
  }
  float inv2;
  float rmax = 0.f;  // explicit: this lane's max |rating| (split window guard)
  float* ytyL = reinterpret_cast<float*>(smem + kW1YtyLdsOff);  // implicit light rows
  if constexpr (IMPLICIT) {
    if (chunk < 0) {  // (uniform) the YtY table lands in LDS while the Gram accumulates
#pragma unroll
      for (int j = 0; j < kW1YtyC / 256; ++j)
        __builtin_amdgcn_global_load_lds(ytyC + 256 * j + 4 * lane, ytyL + 256 * j, 16, 0, 0);
    }
    const int e = split_exponent(scal[0] * __builtin_sqrtf(alpha * scal[1]));
    inv2 = ldexpf(1.f, -2 * e);
    gram_accumulate_split<CN, true>(col, val, pb, pe, Y, ld, k, alpha, ldexpf(1.f, e), acc, bt,
                                    npos, reinterpret_cast<int*>(smem));
  } else {
    const int ey = split_exponent(scal[0]), er = split_exponent(scal[1]);
    inv2 = ldexpf(1.f, -2 * ey);
    floatx4 accb[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) accb[c] = floatx4{0.f, 0.f, 0.f, 0.f};
    // two gather steps in flight
    gram_accumulate_pre2<FullTiles<CN>>(col, val, pb, pe, Ysp, (uint32_t)kp, zero_row,
                                        ldexpf(1.f, er), (threadIdx.x & 15) * CN, acc, accb,
                                        reinterpret_cast<int*>(smem), rmax);
    rhs_from_tiles<FullTiles<CN>>(accb, ldexpf(1.f, -ey - er), bt);
    rmax *= ldexpf(1.f, er);
    if (chunk < 0 && (window_miss(diag_max_lane<CN>(acc), (float)(pe - pb), rmax) ||
                      rank_deficient_illcond<CN>(acc, inv2, pe - pb, k, reg))) {
      rescue_append(rl, row);
      return;
    }
  }
  if (chunk >= 0) {
    float* slot = slots + (int64_t)chunk * kW1Slot;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) slot[(t * 4 + r) * 64 + lane] = acc[t][r] * inv2;
#pragma unroll
    for (int c = 0; c < CN; ++c) slot[(NT * 4 + c) * 64 + lane] = bt[c];
    // explicit: the chunk's scaled max |rating| (launch 2a takes the max over chunks)
    slot[(NT * 4 + CN) * 64 + lane] = IMPLICIT ? (float)npos : rmax;
    return;
  }
  wave_lds_sync();  // the Gram's staging words are reused by the solve (one wave)
  if constexpr (IMPLICIT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the table landed
  const int64_t n_reg = IMPLICIT ? (int64_t)npos : (pe - pb);
  w1_finish_and_solve<IMPLICIT, kW1NB, IMPLICIT>(acc, inv2, bt, n_reg, IMPLICIT ? ytyL : ytyC,
                                               smem, k, reg,
                                               X + (int64_t)row * ld, ld, row, rl,
                                               IMPLICIT ? kCondMaxImplicit : kCondMax);
}

// Launch 2 (W1): heavy rows — fp64 sums of the fp32 chunk partials in a fixed
// order (+ YtY in fp64 for implicit), one rounding, then the solve.  Entries are
// reduced 16 at a time (a memory clobber keeps the groups' slot loops apart, so
// only 16 fp64 sums are live).
// Launch 2b: one wavefront per heavy row solves from its summed slot.
template <bool IMPLICIT>
__global__ __launch_bounds__(64, 1) void reduce_solve_w1_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ heavy_rows,
    const int32_t* __restrict__ slot_begin, const int32_t* __restrict__ slot_begin2,
    const float* __restrict__ slots, float* __restrict__ X, int ld, int k, float reg,
    int32_t* __restrict__ status, const float* __restrict__ scal, RescueList rl) {
  constexpr int CN = 8, NT = kW1NT;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SmemBytes<CN>::value];
  const int lane = threadIdx.x & 63;
  const int h = blockIdx.x;
  const int row = heavy_rows[h];
  const float* sl =
      slots + (int64_t)slot_range(slot_begin, slot_begin2, h).home() * kW1Slot + lane;
  floatx4 A[NT];
  float bt[CN];
#pragma unroll
  for (int e = 0; e < NT * 4; ++e) A[e / 4][e % 4] = sl[e * 64];
#pragma unroll
  for (int c = 0; c < CN; ++c) bt[c] = sl[(NT * 4 + c) * 64];
  const float npos_f = sl[(NT * 4 + CN) * 64];
  const int64_t n_reg = IMPLICIT ? (int64_t)npos_f : (row_ptr[row + 1] - row_ptr[row]);
  if constexpr (!IMPLICIT) {  // split window guard over the whole row (npos_f: max |rating|)
    const float s2 = ldexpf(1.f, 2 * split_exponent(scal[0]));
    if (window_miss(diag_max_lane<CN>(A) * s2, (float)n_reg, npos_f)) {
      rescue_append(rl, row);
      return;
    }
  }
  w1_finish_and_solve<false>(A, 1.f, bt, n_reg, nullptr, smem, k, reg, X + (int64_t)row * ld, ld,
                             row, rl, IMPLICIT ? kCondMaxImplicit : kCondMax);
}

}  // namespace als

// The YtY kernels (after the solve kernels: the order of the kernels in the code object
// is the order of their definitions).
#include "yty.h"

using namespace als;

extern "C" {

int32_t als_k_pad(int32_t k) { return 16 * cn_for_k(k); }

}  // extern "C"

static size_t slot_doubles(int k) {  // partial slot of one heavy-row chunk (solve)
  switch (cn_for_k(k)) {
    case 1: return (Cfg<1>::SLOT + 1) / 2;  // fp32 chunk partials
    case 2: return (Cfg<2>::SLOT + 1) / 2;
    case 4: return (Cfg<4>::SLOT + 1) / 2;
    default: return (size_t)(kW1Slot + 1) / 2;  // W1 stores fp32 partials
  }
}

static size_t yty_slot_doubles(int k) {  // partial slot of one YtY task (fp64 slots)
  switch (cn_for_k(k)) {
    case 1: return Cfg<1>::SLOT;
    case 2: return Cfg<2>::SLOT;
    case 4: return Cfg<4>::SLOT;
    default: return (size_t)kWgSlot;
  }
}

// The solve launches of one als_solve_half call: the call's arguments, its workspace
// pieces and the grids of the phases asked for (0: phase not run).
namespace {
struct SolveCall {
  const int64_t *row_ptr, *chunk_begin, *chunk_end;
  const int32_t *col, *light_rows, *heavy_rows, *heavy_slot_begin, *heavy_slot_begin2, *chunk_row;
  const float *val, *Y_src, *ytyC, *scal;
  const double* yty_packed;
  const uint32_t* Ysp;
  float *X_dst, *slots_f;
  int32_t* status_dev;
  int32_t n_light_primal, n_chunks, chunk_slot0, ld, k, kp, zero_row;
  float reg, alpha;
  RescueList rl;
  unsigned g1, gd, g2;
  bool rescue;
  hipStream_t st;

  // the n x n dual systems of the light rows past n_light_primal
  template <int KP>
  int launch_dual() const {
    gram_solve_dual_kernel<KP><<<gd, 64, 0, st>>>(row_ptr, col, val, light_rows + n_light_primal,
                                                  X_dst, ld, reg, status_dev, scal, Ysp, zero_row,
                                                  rl);
    ALS_LAUNCH_CHECK();
    return ALS_OK;
  }

  template <bool IMP>
  int launch_rescue() const {
    rescue64_kernel<IMP><<<kRescueGrid, kRescueThreads, 0, st>>>(
        row_ptr, col, val, Y_src, ld, k, reg, alpha, yty_packed, X_dst, status_dev, rl);
    ALS_LAUNCH_CHECK();
    return ALS_OK;
  }

  // rank <= 64: launch 1, the dual rows (explicit rank 33-64), launch 2a + 2b, the rescue
  template <int CN, bool IMP>
  int launch() const {
    // explicit rank 33-64: gram_solve_kernel<4, false> is compiled for k == k_pad
    auto* launch1 = (CN == 4 && !IMP && k != kp) ? gram_solve_kernel<(IMP ? CN : kCnPadded64), IMP>
                                                 : gram_solve_kernel<CN, IMP>;
    if (g1)
      launch1<<<g1, 64, 0, st>>>(row_ptr, col, val, light_rows, chunk_row, chunk_begin, chunk_end,
                                 n_chunks, n_light_primal, Y_src, X_dst, ld, k, reg, alpha,
                                 yty_packed, slots_f + (size_t)chunk_slot0 * Cfg<CN>::SLOT,
                                 status_dev, scal, Ysp, kp, zero_row, rl);
    ALS_LAUNCH_CHECK();
    if (gd && CN == 4 && !IMP && launch_dual<64>() != ALS_OK) return ALS_EDEVICE;
    if (g2) {
      heavy_sum_f64_kernel<Cfg<CN>::SLOT, IMP>
          <<<dim3((Cfg<CN>::SLOT + 255) / 256, g2), 256, 0, st>>>(heavy_slot_begin,
                                                                  heavy_slot_begin2, slots_f);
      ALS_LAUNCH_CHECK();
      reduce_solve_kernel<CN, IMP><<<g2, 64, 0, st>>>(
          row_ptr, col, val, Y_src, alpha, heavy_rows, heavy_slot_begin, heavy_slot_begin2,
          slots_f, X_dst, ld, k, reg, yty_packed, status_dev, scal, rl);
    }
    ALS_LAUNCH_CHECK();
    return rescue ? launch_rescue<IMP>() : ALS_OK;
  }

  // rank 65-128 (W1): the same sequence
  template <bool IMP>
  int launch_w1() const {
    if (g1)
      gram_solve_w1_kernel<IMP><<<g1, 64, 0, st>>>(
          row_ptr, col, val, light_rows, chunk_begin, chunk_end, n_chunks, n_light_primal, Y_src,
          X_dst, ld, k, reg, alpha, ytyC, slots_f + (size_t)chunk_slot0 * kW1Slot, status_dev,
          scal, Ysp, kp, zero_row, rl);
    ALS_LAUNCH_CHECK();
    if (gd && launch_dual<128>() != ALS_OK) return ALS_EDEVICE;
    if (g2) {
      heavy_sum_w1_kernel<IMP><<<dim3((kW1Slot / 4 + 255) / 256, g2), 256, 0, st>>>(
          heavy_slot_begin, heavy_slot_begin2, slots_f, yty_packed);
      ALS_LAUNCH_CHECK();
      reduce_solve_w1_kernel<IMP><<<g2, 64, 0, st>>>(row_ptr, heavy_rows, heavy_slot_begin,
                                                     heavy_slot_begin2, slots_f, X_dst, ld, k,
                                                     reg, status_dev, scal, rl);
    }
    ALS_LAUNCH_CHECK();
    return rescue ? launch_rescue<IMP>() : ALS_OK;
  }

  template <bool IMP>
  int launch_rank(int cn) const {
    return cn == 1 ? launch<1, IMP>() : cn == 2 ? launch<2, IMP>()
         : cn == 4 ? launch<4, IMP>() : launch_w1<IMP>();
  }
};
}  // namespace

// YtY: the task partials, their element-wise sum, the reduce of that one slot
// (CN = 8: the workgroup kernels).
template <int CN>
static int launch_yty(const float* Y, int64_t n, int32_t ld, int32_t k, double* slots, int nslots,
                      int64_t slen, double* out, hipStream_t st) {
  double* ssum = slots + (int64_t)nslots * slen;
  if constexpr (CN == 8) yty_partial_wg_kernel<<<nslots, 256, 0, st>>>(Y, n, ld, k, slots);
  else yty_partial_kernel<CN><<<nslots, 64, 0, st>>>(Y, n, ld, k, slots);
  ALS_LAUNCH_CHECK();
  slot_sum_kernel<<<(unsigned)((slen + 63) / 64), 64 * kSlotSumWaves, 0, st>>>(slots, nslots, slen,
                                                                             ssum);
  ALS_LAUNCH_CHECK();
  if constexpr (CN == 8) yty_reduce_wg_kernel<<<1, 256, 0, st>>>(ssum, 1, out);
  else yty_reduce_kernel<CN><<<1, 64, 0, st>>>(ssum, 1, out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

extern "C" {

static size_t ytyc_bytes(int32_t k) {  // C-layout fp32 YtY table of the W1 path
  return cn_for_k(k) == 8 ? align_up(sizeof(float) * kW1YtyC) : 0;
}

static size_t solve_table_bytes(int32_t k, int64_t n_src) {
  return align_up(sizeof(uint32_t) * (size_t)als_k_pad(k) * (size_t)((n_src > 0 ? n_src : 0) + 1));
}

static size_t slot_bytes(int32_t k, int32_t n_chunks) {
  return align_up(sizeof(double) * slot_doubles(k) * (size_t)(n_chunks > 0 ? n_chunks : 0));
}

size_t als_solve_workspace_bytes(int32_t k, int32_t n_chunks, int64_t n_src, int32_t n_rows) {
  // From the front: 256 B of scale words (max |Y_src|, max |rating|, rescue count) |
  // C-layout YtY (W1 implicit) | partial slots of the heavy-row chunks (n_chunks,
  // counted from slot 0: chunk_slot0 + the call's chunks).
  // From the back: the split table ((n_src + 1) x k_pad words, explicit), ending at
  // the workspace's end (256-B aligned; + 256 B of slack for that alignment), and
  // right below it the rescue list (n_rows).  Calls
  // that share one PREP (row chunks of a half-sweep: same Y_src, any n_chunks / n_rows)
  // find the table at the same place, and the two calls of a two-segment half-sweep
  // (different n_src) find the early partial slots at the same place.
  return 256 + ytyc_bytes(k) + slot_bytes(k, n_chunks) +
         align_up(sizeof(int32_t) * (size_t)(n_rows > 0 ? n_rows : 0)) +
         solve_table_bytes(k, n_src) + 256;
}

int als_solve_half(const int64_t* row_ptr, const int32_t* col, const float* val,
                   const int32_t* light_rows, int32_t n_light, int32_t n_light_primal,
                   const int32_t* heavy_rows,
                   const int32_t* heavy_slot_begin, int32_t n_heavy, const int32_t* chunk_row,
                   const int64_t* chunk_begin, const int64_t* chunk_end, int32_t n_chunks,
                   const int32_t* heavy_slot_begin2, int32_t chunk_slot0,
                   const float* Y_src, int64_t n_src, float* X_dst, int32_t ld, int32_t k,
                   float reg, int implicit, float alpha, const double* yty_packed,
                   int32_t* status_dev, void* ws, size_t ws_bytes, int phases, void* stream) {
  ALS_REQUIRE(k >= 1 && k <= kMaxRank, ALS_EUNSUPPORTED, "als_solve_half: rank %d not in [1, %d]",
              k, kMaxRank);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL, "als_solve_half: ld=%d must be >= k and %%4==0",
              ld);
  ALS_REQUIRE(n_light >= 0 && n_heavy >= 0 && n_chunks >= 0, ALS_EINVAL,
              "als_solve_half: negative counts");
  ALS_REQUIRE(n_light_primal >= 0 && n_light_primal <= n_light, ALS_EINVAL,
              "als_solve_half: n_light_primal %d not in [0, n_light=%d]", n_light_primal, n_light);
  ALS_REQUIRE(n_light_primal == n_light || (!implicit && k > 32 && reg > 0.f), ALS_EINVAL,
              "als_solve_half: the dual path (light rows past n_light_primal) is for explicit "
              "feedback at rank 33-128 with regParam > 0 only");
  ALS_REQUIRE(Y_src && X_dst && row_ptr && status_dev, ALS_EINVAL, "als_solve_half: null pointer");
  ALS_REQUIRE(!implicit || yty_packed, ALS_EINVAL, "als_solve_half: implicit needs yty_packed");
  ALS_REQUIRE(reg >= 0.f && alpha >= 0.f, ALS_EINVAL, "als_solve_half: reg/alpha must be >= 0");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(Y_src) & 15) == 0, ALS_EINVAL,
              "als_solve_half: Y_src must be 16-byte aligned");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(val) & 15) == 0, ALS_EINVAL,
              "als_solve_half: val must be 16-byte aligned");
  ALS_REQUIRE(n_src >= 0 && n_src < (int64_t(1) << 31), ALS_EINVAL,
              "als_solve_half: n_src %lld not in [0, 2^31)", (long long)n_src);
  const int32_t n_rows = n_light + n_heavy;
  ALS_REQUIRE(chunk_slot0 >= 0 && (int64_t)chunk_slot0 + n_chunks < (int64_t(1) << 31),
              ALS_EINVAL, "als_solve_half: chunk_slot0 %d out of range", chunk_slot0);
  const int32_t n_slots = chunk_slot0 + n_chunks;  // slot region: [0, n_slots)
  ALS_REQUIRE(ws_bytes >= als_solve_workspace_bytes(k, n_slots, n_src, n_rows), ALS_EWORKSPACE,
              "als_solve_half: workspace %zu < %zu", ws_bytes,
              als_solve_workspace_bytes(k, n_slots, n_src, n_rows));
  ALS_REQUIRE(phases >= 1 && phases <= ALS_PHASE_ALL, ALS_EINVAL,
              "als_solve_half: phases must be in [1, %d]", ALS_PHASE_ALL);
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, ALS_EINVAL,
              "als_solve_half: workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  // scale words (max |Y_src|, max |rating|), the split table, the partial slots
  unsigned* scal_u = static_cast<unsigned*>(ws);
  const float* scal = reinterpret_cast<const float*>(scal_u);
  float* ytyC = reinterpret_cast<float*>(static_cast<char*>(ws) + 256);
  double* slots = reinterpret_cast<double*>(static_cast<char*>(ws) + 256 + ytyc_bytes(k));
  uint32_t* Ysp = reinterpret_cast<uint32_t*>(
      static_cast<char*>(ws) + ((ws_bytes - solve_table_bytes(k, n_src)) & ~(size_t)255));
  // the rescue list right below the split table (not after this call's slots: blocks
  // sharing one workspace with disjoint slot ranges must not see one call's list land
  // on another block's partial slots; the size check keeps it above every slot)
  int32_t* rescue_list = reinterpret_cast<int32_t*>(
      reinterpret_cast<char*>(Ysp) - align_up(sizeof(int32_t) * (size_t)(n_rows > 0 ? n_rows : 0)));
  unsigned* rescue_cnt = scal_u + 2;
  const RescueList rl{rescue_cnt, rescue_list, (unsigned)(n_light + n_heavy)};
  // the rescue list (count at scale word 2, the rescue launch's finished-block counter
  // at word 3) starts empty at each Y prep (cleared by the prep's absmax launch: a fresh
  // workspace holds garbage) and is emptied by the RESCUE launch that consumes it, so the
  // next row chunk of a half-sweep that shares one prep starts empty too
  if ((phases & ALS_PHASE_PREP) && n_src * (int64_t)ld == 0)
    ALS_HIP(hipMemsetAsync(rescue_cnt, 0, 2 * sizeof(unsigned), st));
  const int cn = cn_for_k(k);
  const int kp = als_k_pad(k);
  const int zero_row = (int)n_src;
  if (phases & ALS_PHASE_PREP) {  // Y_src prep: max |Y_src|, split table (explicit) / YtY table (W1 implicit)
    ALS_HIP(hipMemsetAsync(scal_u, 0, sizeof(unsigned), st));
    if (implicit && cn == 8) {
      yty_ctab_kernel<<<1, 64, 0, st>>>(yty_packed, ytyC);
      ALS_LAUNCH_CHECK();
    }
    const int64_t ny = n_src * (int64_t)ld;
    if (ny > 0) {
      // 256 workgroups (one atomic each on the scale word; 1024 serialised there)
      const int gy = (int)std::min<int64_t>(256, (ny / 4 + 255) / 256 + 1);
      absmax_kernel<<<gy, 256, 0, st>>>(Y_src, ny, scal_u, rescue_cnt);
      ALS_LAUNCH_CHECK();
    }
    if (!implicit) {
      const int kp4_shift = __builtin_ctz(kp / 4);
      const int64_t total = (n_src + 1) << kp4_shift;
      const int gt = (int)std::min<int64_t>(4096, (total + 255) / 256);
      split_table_kernel<<<gt, 256, 0, st>>>(Y_src, n_src, ld, k, kp4_shift, scal,
                                             reinterpret_cast<uint4*>(Ysp));
      ALS_LAUNCH_CHECK();
    }
  }
  if (phases & ALS_PHASE_RSCALE) {  // rating scale of this block: max |rating|
    ALS_HIP(hipMemsetAsync(scal_u + 1, 0, sizeof(unsigned), st));
    if (n_light + n_heavy > 0) {
      ALS_REQUIRE(val != nullptr, ALS_EINVAL, "als_solve_half: null val");
      // every row is light or heavy: the block's ratings are val[0, row_ptr[n_light + n_heavy])
      absmax_csr_kernel<<<256, 256, 0, st>>>(row_ptr, n_light + n_heavy, val, scal_u + 1);
      ALS_LAUNCH_CHECK();
    }
  }
  const unsigned g1 = (phases & ALS_PHASE_LAUNCH1) ? (unsigned)(n_chunks + n_light_primal) : 0u;
  const unsigned gd = (phases & ALS_PHASE_DUAL) ? (unsigned)(n_light - n_light_primal) : 0u;
  const unsigned g2 = (phases & ALS_PHASE_LAUNCH2) ? (unsigned)n_heavy : 0u;
  const bool rescue = (phases & ALS_PHASE_RESCUE) && n_rows > 0;
  const SolveCall c{row_ptr, chunk_begin, chunk_end,
                    col, light_rows, heavy_rows, heavy_slot_begin, heavy_slot_begin2, chunk_row,
                    val, Y_src, ytyC, scal,
                    yty_packed, Ysp, X_dst, reinterpret_cast<float*>(slots), status_dev,
                    n_light_primal, n_chunks, chunk_slot0, ld, k, kp, zero_row,
                    reg, alpha, rl, g1, gd, g2, rescue, st};
  return implicit ? c.launch_rank<true>(cn) : c.launch_rank<false>(cn);
}

size_t als_yty_workspace_bytes(int64_t n, int32_t k) {
  const int64_t nslots = n > 0 ? (n + yty_chunk(n) - 1) / yty_chunk(n) : 1;
  // task slots + their element-wise sum
  return align_up(sizeof(double) * yty_slot_doubles(k) * (size_t)(nslots + 1)) + 256;
}

int als_yty(const float* Y, int64_t n, int32_t ld, int32_t k, double* yty_packed_out, void* ws,
            size_t ws_bytes, void* stream) {
  ALS_REQUIRE(k >= 1 && k <= kMaxRank, ALS_EUNSUPPORTED, "als_yty: rank %d not in [1, %d]", k,
              kMaxRank);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL, "als_yty: bad ld");
  ALS_REQUIRE(n >= 0 && yty_packed_out && (n == 0 || Y), ALS_EINVAL, "als_yty: bad args");
  ALS_REQUIRE(n < (int64_t(1) << 31), ALS_EINVAL, "als_yty: n >= 2^31");
  ALS_REQUIRE(ws_bytes >= als_yty_workspace_bytes(n, k), ALS_EWORKSPACE,
              "als_yty: workspace too small");
  hipStream_t st = as_stream(stream);
  double* slots = static_cast<double*>(ws);
  const int nslots = n > 0 ? (int)((n + yty_chunk(n) - 1) / yty_chunk(n)) : 0;
  const int cn = cn_for_k(k);
  if (nslots == 0) {
    const int kp = 16 * cn;
    ALS_HIP(hipMemsetAsync(yty_packed_out, 0, sizeof(double) * kp * (kp + 1) / 2, st));
    return ALS_OK;
  }
  const int64_t slen = (int64_t)yty_slot_doubles(k);
  return cn == 1 ? launch_yty<1>(Y, n, ld, k, slots, nslots, slen, yty_packed_out, st)
       : cn == 2 ? launch_yty<2>(Y, n, ld, k, slots, nslots, slen, yty_packed_out, st)
       : cn == 4 ? launch_yty<4>(Y, n, ld, k, slots, nslots, slen, yty_packed_out, st)
                 : launch_yty<8>(Y, n, ld, k, slots, nslots, slen, yty_packed_out, st);
}

}  // extern "C"
